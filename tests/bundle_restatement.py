"""NumPy restatement of include/amvs_bundle.h, written from the header's text alone: the terms of an observation, the
serial sums per point and the blocked sums per camera, held points and idle cameras, the reduced system with its pair
lists, the dense Cholesky with its ascending forward and descending back solve, the step and the Levenberg-Marquardt
iteration.  What the header takes from amvs_resection.h (the Jacobian rows, the blocked SUM, the quaternion update) is
restated here from that header's text.  Every float64 operation is one NumPy ufunc call (one rounding, nothing fused),
in the header's order.  The device is compared with this bit for bit (tests/test_hip_bundle.py)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resection_restatement import intrinsics  # noqa: E402

BLOCK = 64                # AMVS_BA_BLOCK
MAX_CAMERAS, MAX_POINTS, MAX_OBS, MAX_PAIRS = 256, 1 << 22, 1 << 24, 1 << 25
LAMBDA_MIN, LAMBDA_MAX = 1e-12, 1e12
TRI3 = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
TRI6 = tuple((i, j) for i in range(6) for j in range(i, 6))


def block_sum(terms, member):
    """The header's blocked SUM over list positions: terms (m, ...), member (m,) bool.  Block partials from +0.0 over the
    qualifying members in ascending position, then the partials of all blocks in ascending order from +0.0."""
    terms = np.asarray(terms, np.float64)
    m, shape = len(terms), terms.shape[1:]
    nb = -(-m // BLOCK)
    t = np.zeros((nb * BLOCK,) + shape)
    t[:m] = terms
    mem = np.zeros(nb * BLOCK, bool)
    mem[:m] = member
    t = t.reshape((nb, BLOCK) + shape)
    mem = mem.reshape((nb, BLOCK) + (1,) * len(shape))
    part = np.zeros((nb,) + shape)
    with np.errstate(all="ignore"):
        for j in range(min(BLOCK, m)):                  # (positions past m exist in no block)
            part = np.where(mem[:, j], part + t[:, j], part)
        total = np.zeros(shape)
        for b in range(nb):
            total = total + part[b]
    return total


class Problem:
    """The inputs of a call, promoted and checked as the header says."""

    def __init__(self, cam, pt, uv, K, C, P, fixed=None):
        self.cam = np.asarray(cam, np.int32).reshape(-1)
        self.pt = np.asarray(pt, np.int32).reshape(-1)
        self.uv = np.asarray(uv, np.float32).reshape(-1, 2).astype(np.float64)
        self.N, self.C, self.P = len(self.cam), int(C), int(P)
        self.intr = intrinsics(K)
        key = self.pt.astype(np.int64) * self.C + self.cam
        assert np.all(np.diff(key) > 0), "observations must be strictly ascending in (pt, cam)"
        assert self.cam.min() >= 0 and self.cam.max() < self.C and self.pt.min() >= 0 and self.pt.max() < self.P
        self.fixed = np.arange(self.C) == 0 if fixed is None else np.asarray(fixed).reshape(-1) != 0
        self.slot = np.full(self.C, -1, np.int32)
        self.slot[~self.fixed] = np.arange(int((~self.fixed).sum()))
        self.F = int((~self.fixed).sum())
        self.n = 6 * self.F
        self.lists = [np.flatnonzero(self.cam == c) for c in range(self.C)]          # ascending k
        self.start = np.searchsorted(self.pt, np.arange(self.P + 1)).astype(np.int64)


def terms(q, R, t, X):
    """The per-observation terms under a state: a dict of arrays over k."""
    fx, fy, cx, cy = q.intr
    R = np.asarray(R, np.float64).reshape(-1, 9)[q.cam]
    t = np.asarray(t, np.float64).reshape(-1, 3)[q.cam]
    Xp = np.asarray(X, np.float64).reshape(-1, 3)[q.pt]
    with np.errstate(all="ignore"):
        Xc = [((R[:, 3 * r] * Xp[:, 0] + R[:, 3 * r + 1] * Xp[:, 1]) + R[:, 3 * r + 2] * Xp[:, 2]) + t[:, r] for r in range(3)]
        x0, x1, z = Xc
        active = z > 0.0
        iz = 1.0 / z
        xz, yz = x0 * iz, x1 * iz
        rx, ry = (fx * xz + cx) - q.uv[:, 0], (fy * yz + cy) - q.uv[:, 1]
        ax, ay = fx * iz, fy * iz
        bx, by = -(ax * xz), -(ay * yz)
        zero = np.zeros_like(z)
        Jx = np.stack([bx * x1, ax * z - bx * x0, -(ax * x1), ax, zero, bx], axis=1)
        Jy = np.stack([by * x1 - ay * z, -(by * x0), ay * x0, zero, ay, by], axis=1)
        Px = np.stack([ax * R[:, j] + bx * R[:, 6 + j] for j in range(3)], axis=1)
        Py = np.stack([ay * R[:, 3 + j] + by * R[:, 6 + j] for j in range(3)], axis=1)
        W = Jx[:, :, None] * Px[:, None, :] + Jy[:, :, None] * Py[:, None, :]
    return {"active": active, "rx": rx, "ry": ry, "Jx": Jx, "Jy": Jy, "Px": Px, "Py": Py, "W": W}


def point_sums(q, T):
    """V (P, 6), gp (P, 3), counts (P,): serial over each point's active observations in ascending k."""
    Px, Py, rx, ry, active = T["Px"], T["Py"], T["rx"], T["ry"], T["active"]
    with np.errstate(all="ignore"):
        tv = np.stack([Px[:, i] * Px[:, j] + Py[:, i] * Py[:, j] for i, j in TRI3], axis=1)
        tg = np.stack([Px[:, i] * rx + Py[:, i] * ry for i in range(3)], axis=1)
        V, gp, cnt = np.zeros((q.P, 6)), np.zeros((q.P, 3)), np.zeros(q.P, np.int32)
        length = q.start[1:] - q.start[:-1]
        for j in range(int(length.max())):
            has = np.flatnonzero(length > j)
            k = q.start[has] + j
            a = active[k]
            V[has] = np.where(a[:, None], V[has] + tv[k], V[has])
            gp[has] = np.where(a[:, None], gp[has] + tg[k], gp[has])
            cnt[has] += a
    return V, gp, cnt


def camera_sums(q, T):
    """(C, 29): U (21), gc (6), cost_c, act_c by the blocked SUM over each camera's list."""
    Jx, Jy, rx, ry = T["Jx"], T["Jy"], T["rx"], T["ry"]
    with np.errstate(all="ignore"):
        cols = [Jx[:, i] * Jx[:, j] + Jy[:, i] * Jy[:, j] for i, j in TRI6]
        cols += [Jx[:, i] * rx + Jy[:, i] * ry for i in range(6)]
        cols += [rx * rx + ry * ry, np.ones_like(rx)]
        all_terms = np.stack(cols, axis=1)
    out = np.zeros((q.C, 29))
    for c, lst in enumerate(q.lists):
        if len(lst):
            out[c] = block_sum(all_terms[lst], T["active"][lst])
    return out


def total(sums):
    """(cost, act): the cameras in ascending order from +0.0."""
    cost, act = np.float64(0.0), np.float64(0.0)
    with np.errstate(all="ignore"):
        for c in range(len(sums)):
            cost = cost + sums[c, 27]
            act = act + sums[c, 28]
    return float(cost), float(act)


def cost(q, R, t, X):
    """amvs_ba_cost: (cost, active, err2 (N,))."""
    T = terms(q, R, t, X)
    c, a = total(camera_sums(q, T))
    with np.errstate(all="ignore"):
        err2 = np.where(T["active"], T["rx"] * T["rx"] + T["ry"] * T["ry"], -1.0)
    return c, int(a), err2


def normal(q, R, t, X):
    """amvs_ba_normal: (U (C, 21), gc (C, 6), V (P, 6), gp (P, 3), counts (P,))."""
    T = terms(q, R, t, X)
    s = camera_sums(q, T)
    V, gp, cnt = point_sums(q, T)
    return s[:, :21].copy(), s[:, 21:27].copy(), V, gp, cnt


def point_factors(V, cnt, lam, refine_points):
    """(Lp (P, 3, 3), held (P,)): the Cholesky factor of the damped V' and who is held."""
    P = len(V)
    Vm = np.zeros((P, 3, 3))
    for e, (i, j) in enumerate(TRI3):
        Vm[:, i, j] = V[:, e]
    L = np.zeros((P, 3, 3))
    ok = np.full(P, bool(refine_points)) & (cnt >= 2)
    with np.errstate(all="ignore"):
        for i in range(3):
            Vm[:, i, i] = Vm[:, i, i] + lam * Vm[:, i, i]
        for j in range(3):
            s = Vm[:, j, j].copy()
            for k in range(j):
                s = s - L[:, j, k] * L[:, j, k]
            ok &= (s > 0.0) & (s < np.inf)
            L[:, j, j] = np.sqrt(s)
            for i in range(j + 1, 3):
                v = Vm[:, j, i].copy()
                for k in range(j):
                    v = v - L[:, i, k] * L[:, j, k]
                L[:, i, j] = v / L[:, j, j]
    return L, ~ok


def solve3(L, b):
    """solve3 of the header, vectorised: L (..., 3, 3), b (..., 3)."""
    with np.errstate(all="ignore"):
        y0 = b[..., 0] / L[..., 0, 0]
        y1 = (b[..., 1] - L[..., 1, 0] * y0) / L[..., 1, 1]
        y2 = ((b[..., 2] - L[..., 2, 0] * y0) - L[..., 2, 1] * y1) / L[..., 2, 2]
        x2 = y2 / L[..., 2, 2]
        x1 = (y1 - L[..., 2, 1] * x2) / L[..., 1, 1]
        x0 = ((y0 - L[..., 1, 0] * x1) - L[..., 2, 0] * x2) / L[..., 0, 0]
    return np.stack([x0, x1, x2], axis=-1)


def dot3(a, b):
    with np.errstate(all="ignore"):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def reduced(q, T, sums, V, gp, cnt, lam, refine_points):
    """(S (n, n), rhs (n,), held (P,), Lp): the reduced system under lam."""
    Lp, held = point_factors(V, cnt, lam, refine_points)
    W, active = T["W"], T["active"]
    Y = solve3(Lp[q.pt][:, None, :, :], W)                                   # (N, 6, 3); used only where it qualifies
    n = q.n
    S, rhs = np.zeros((n, n)), np.zeros(n)
    qualifies = active & ~held[q.pt]
    free = [c for c in range(q.C) if q.slot[c] >= 0]
    with np.errstate(all="ignore"):
        for c in free:
            a, lst = int(q.slot[c]), q.lists[c]
            if sums[c, 28] == 0.0:                                           # idle
                S[6 * a:6 * a + 6, 6 * a:6 * a + 6] = np.eye(6)
                continue
            Tkk = dot3(Y[lst][:, :, None, :], W[lst][:, None, :, :])         # (len, 6, 6)
            tg = dot3(Y[lst], gp[q.pt[lst]][:, None, :])                     # (len, 6)
            sub = block_sum(Tkk, qualifies[lst]) if len(lst) else np.zeros((6, 6))
            sg = block_sum(tg, qualifies[lst]) if len(lst) else np.zeros(6)
            for e, (i, j) in enumerate(TRI6):
                u = sums[c, e]
                if i == j:
                    u = u + lam * u
                S[6 * a + i, 6 * a + j] = S[6 * a + j, 6 * a + i] = u - sub[i, j]
            rhs[6 * a:6 * a + 6] = -(sums[c, 21:27]) + sg
        shared = {}                                                         # (c, c') -> the (k, k') of the points both see
        for p in range(q.P):                                                # ascending p, and c < c' as k < k'
            ks = [k for k in range(int(q.start[p]), int(q.start[p + 1])) if q.slot[q.cam[k]] >= 0]
            for i, k in enumerate(ks):
                for k2 in ks[i + 1:]:
                    shared.setdefault((int(q.cam[k]), int(q.cam[k2])), []).append((k, k2))
        for (c, c2), pairs in shared.items():
            k, k2 = np.array(pairs).T
            Tkk = dot3(Y[k][:, :, None, :], W[k2][:, None, :, :])
            blk = 0.0 - block_sum(Tkk, qualifies[k] & active[k2])
            a, b = int(q.slot[c]), int(q.slot[c2])
            S[6 * a:6 * a + 6, 6 * b:6 * b + 6] = blk
            S[6 * b:6 * b + 6, 6 * a:6 * a + 6] = blk.T
    return S, rhs, held, Lp


def schur(q, R, t, X, lam, refine_points=1):
    """amvs_ba_schur: (S, rhs, slot, held)."""
    T = terms(q, R, t, X)
    V, gp, cnt = point_sums(q, T)
    S, rhs, held, _ = reduced(q, T, camera_sums(q, T), V, gp, cnt, lam, refine_points)
    return S, rhs, q.slot.copy(), held


def dense_solve(S, rhs):
    """The dense solve of the header: x, or None for NO STEP.  The loops run by column k, so that each step is one array
    operation: once column k is known, every entry that still has the product with k to subtract subtracts it.  An entry
    thus subtracts its products in ascending k in the factorisation and the forward solve, in descending k in the back
    solve, each product and each difference rounded once: the header's sequence for every entry."""
    n = len(S)
    W = np.array(S, np.float64)                     # entry (i, j), i >= j: S[j][i] minus the products subtracted so far
    L = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for k in range(n):
            s = W[k, k]
            if not (s > 0.0 and s < np.inf):
                return None
            L[k, k] = np.sqrt(s)
            col = W[k + 1:, k] / L[k, k]
            L[k + 1:, k] = col
            W[k + 1:, k + 1:] = W[k + 1:, k + 1:] - col[:, None] * col[None, :]
        y = np.array(rhs, np.float64)
        for k in range(n):
            y[k] = y[k] / L[k, k]
            y[k + 1:] = y[k + 1:] - L[k + 1:, k] * y[k]
        x = y.copy()
        for k in range(n - 1, -1, -1):
            x[k] = x[k] / L[k, k]
            x[:k] = x[:k] - L[k, :k] * x[k]
    return x


def pose_update(dc, R, t):
    """The quaternion update of amvs_resection.h's STEP from "hx = 0.5*om[0]" on: (R' (9,), t' (3,))."""
    d = np.asarray(dc, np.float64)
    Rm, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    with np.errstate(all="ignore"):
        hx, hy, hz = 0.5 * d[0], 0.5 * d[1], 0.5 * d[2]
        n = np.sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz)
        qw, qx, qy, qz = 1.0 / n, hx / n, hy / n, hz / n
        Q = np.array([[1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qz * qw), 2.0 * (qx * qz + qy * qw)],
                      [2.0 * (qx * qy + qz * qw), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qx * qw)],
                      [2.0 * (qx * qz - qy * qw), 2.0 * (qy * qz + qx * qw), 1.0 - 2.0 * (qx * qx + qy * qy)]])
        Rn, tn = np.empty((3, 3)), np.empty(3)
        for r in range(3):
            for c in range(3):
                Rn[r, c] = (Q[r, 0] * Rm[0, c] + Q[r, 1] * Rm[1, c]) + Q[r, 2] * Rm[2, c]
            tn[r] = ((Q[r, 0] * t[0] + Q[r, 1] * t[1]) + Q[r, 2] * t[2]) + d[3 + r]
    return Rn.reshape(9), tn


def form_step(q, R, t, X, lam, refine_points=1, T=None, sums=None):
    """amvs_ba_step: (ok, dc (C, 6), dp (P, 3), R' (C, 9), t' (C, 3), X' (P, 3)); zeros when there is no step."""
    R, t, X = (np.asarray(R, np.float64).reshape(-1, 9), np.asarray(t, np.float64).reshape(-1, 3),
               np.asarray(X, np.float64).reshape(-1, 3))
    T = terms(q, R, t, X) if T is None else T
    sums = camera_sums(q, T) if sums is None else sums
    V, gp, cnt = point_sums(q, T)
    S, rhs, held, Lp = reduced(q, T, sums, V, gp, cnt, lam, refine_points)
    x = dense_solve(S, rhs)
    if x is None:
        return False, np.zeros((q.C, 6)), np.zeros((q.P, 3)), np.zeros((q.C, 9)), np.zeros((q.C, 3)), np.zeros((q.P, 3))
    dc = np.zeros((q.C, 6))
    Rn, tn = R.copy(), t.copy()
    for c in range(q.C):
        if q.slot[c] >= 0:
            dc[c] = x[6 * q.slot[c]:6 * q.slot[c] + 6]
            Rn[c], tn[c] = pose_update(dc[c], R[c], t[c])
    W, active = T["W"], T["active"]
    with np.errstate(all="ignore"):
        b = -gp
        d = dc[q.cam]                                                        # (N, 6)
        wd = W[:, 0, :] * d[:, 0, None]
        for i in range(1, 6):
            wd = wd + W[:, i, :] * d[:, i, None]
        use = active & (q.slot[q.cam] >= 0)
        length = q.start[1:] - q.start[:-1]
        for j in range(int(length.max())):
            has = np.flatnonzero(length > j)
            k = q.start[has] + j
            b[has] = np.where(use[k][:, None], b[has] - wd[k], b[has])
        dp = np.where(held[:, None], 0.0, solve3(Lp, b))
        Xn = np.where(held[:, None], X, X + dp)
    return True, dc, dp, Rn, tn, Xn


def solve(q, R, t, X, refine_points=1, lambda0=1e-3, ftol=1e-10, max_trials=50, trace=None):
    """amvs_ba_solve: (R (C, 9), t (C, 3), X (P, 3), info (6,)).  trace, a list, receives one (what, lambda, cost') per
    trial: what is "kept", "rejected" or "no step"."""
    R, t, X = (np.array(R, np.float64).reshape(-1, 9), np.array(t, np.float64).reshape(-1, 3),
               np.array(X, np.float64).reshape(-1, 3))
    lam, trials, kept = float(lambda0), 0, 0
    T = terms(q, R, t, X)
    sums = camera_sums(q, T)
    cst, act = total(sums)
    first = cst
    while trials < max_trials:
        trials += 1
        ok, _, _, Rn, tn, Xn = form_step(q, R, t, X, lam, refine_points, T, sums)
        if ok:
            Tn = terms(q, Rn, tn, Xn)
            sn = camera_sums(q, Tn)
            cn, an = total(sn)
        if ok and cn <= cst and an >= act:
            if trace is not None:
                trace.append(("kept", lam, cn))
            d, old = cst - cn, cst
            R, t, X, T, sums, cst, act = Rn, tn, Xn, Tn, sn, cn, an
            kept += 1
            lam = max(lam / 10.0, LAMBDA_MIN)
            if d <= ftol * old:
                break
        else:
            if trace is not None:
                trace.append(("rejected" if ok else "no step", lam, cn if ok else None))
            lam = lam * 10.0
            if lam > LAMBDA_MAX:
                break
    return R, t, X, np.array([trials, kept, lam, first, cst, act], np.float64)
