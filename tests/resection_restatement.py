"""NumPy restatement of include/amvs_resection.h, written from the header's text alone: the 6-draw sampler, the 6-point
DLT with its block sums and fixed-sweep Jacobi, the nearest rotation, the inlier test, the Gauss-Newton refit and the
RANSAC loop.  What the header takes from amvs_epipolar.h and amvs_match.h (mix, SUM, the Jacobi rotation) is taken from
tests/epipolar_restatement.py.  Vectorised over hypotheses; every float64 operation is one NumPy ufunc call (one rounding,
nothing fused), in the header's order.  The device is compared with this bit for bit (tests/test_hip_resection.py)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from epipolar_restatement import JACOBI_SWEEPS, block_sum, draw_sum, jacobi, mix  # noqa: E402,F401

BATCH = 1024              # AMVS_PNP_BATCH
BLOCK = 64                # AMVS_PNP_BLOCK
REFINE_STEPS = 10         # AMVS_PNP_REFINE_STEPS
ROOT3 = 1.7320508075688772
N_SUMS = 29


def intrinsics(K):
    K = np.asarray(K, np.float64).reshape(9)
    return float(K[0]), float(K[4]), float(K[2]), float(K[5])


def promote(pts3d, pts2d):
    X = np.asarray(pts3d, np.float32).reshape(-1, 3).astype(np.float64)
    x = np.asarray(pts2d, np.float32).reshape(-1, 2).astype(np.float64)
    return X, x


# ---- sampler ---------------------------------------------------------------------------------------------------------------
def sample(seed, h, m):
    """(len(h), 6) int64: the samples of the hypotheses h, in draw order."""
    h = np.atleast_1d(np.asarray(h)).astype(np.uint64)
    idx = np.empty((len(h), 6), np.int64)
    for k in range(6):
        r = (mix(np.uint64(seed) ^ mix(np.uint64(6) * h + np.uint64(k))) % np.uint64(m - k)).astype(np.int64)
        chosen = np.sort(idx[:, :k], axis=1)
        for i in range(k):
            r = r + (r >= chosen[:, i])
        idx[:, k] = r
    return idx


# ---- hypotheses ------------------------------------------------------------------------------------------------------------
def nearest_rotation(A, b):
    """Steps 6 and 7 on A (H, 3, 3), b (H, 3): (R (H, 3, 3), t (H, 3))."""
    with np.errstate(all="ignore"):
        det = (A[:, 0, 0] * (A[:, 1, 1] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 1])
               - A[:, 0, 1] * (A[:, 1, 0] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 0])) \
            + A[:, 0, 2] * (A[:, 1, 0] * A[:, 2, 1] - A[:, 1, 1] * A[:, 2, 0])
        neg = det < 0.0
        A = np.where(neg[:, None, None], -A, A)
        b = np.where(neg[:, None], -b, b)
        G = np.empty_like(A)
        for i in range(3):
            for j in range(3):
                G[:, i, j] = (A[:, 0, i] * A[:, 0, j] + A[:, 1, i] * A[:, 1, j]) + A[:, 2, i] * A[:, 2, j]
        _, Gd, V = jacobi(G, return_state=True)
        sw = np.sqrt(Gd[:, np.arange(3), np.arange(3)])                      # (H, 3)
        C = np.empty_like(A)
        for r in range(3):
            for k in range(3):
                C[:, r, k] = ((A[:, r, 0] * V[:, 0, k] + A[:, r, 1] * V[:, 1, k]) + A[:, r, 2] * V[:, 2, k]) / sw[:, k]
        R = np.empty_like(A)
        for r in range(3):
            for c in range(3):
                R[:, r, c] = (C[:, r, 0] * V[:, c, 0] + C[:, r, 1] * V[:, c, 1]) + C[:, r, 2] * V[:, c, 2]
        sc = ((sw[:, 0] + sw[:, 1]) + sw[:, 2]) / 3.0
        t = b / sc[:, None]
    return R, t


def hypotheses(pts3d, pts2d, K, seed, first, count, return_state=False):
    """(idx (count, 6) int32, R (count, 9), t (count, 3)): amvs_pnp_hypotheses."""
    X, x = promote(pts3d, pts2d)
    fx, fy, cx, cy = intrinsics(K)
    idx = sample(seed, np.arange(first, first + count), len(X))
    Xs, xs = X[idx], x[idx]                                                  # (H, 6, 3), (H, 6, 2)
    H = len(idx)
    with np.errstate(all="ignore"):
        xn, yn = (xs[:, :, 0] - cx) / fx, (xs[:, :, 1] - cy) / fy
        c = draw_sum(Xs) / 6.0                                               # (H, 3)
        d3 = Xs - c[:, None, :]
        dist = np.sqrt((d3[:, :, 0] * d3[:, :, 0] + d3[:, :, 1] * d3[:, :, 1]) + d3[:, :, 2] * d3[:, :, 2])
        s = ROOT3 / (draw_sum(dist) / 6.0)
        P = np.concatenate([d3 * s[:, None, None], np.ones((H, 6, 1))], axis=2)          # (H, 6, 4)
        gx, gy = -(xn[:, :, None] * P), -(yn[:, :, None] * P)
        M = np.zeros((H, 12, 12))
        PP = draw_sum(P[:, :, :, None] * P[:, :, None, :])
        M[:, 0:4, 0:4] = PP
        M[:, 4:8, 4:8] = PP
        M[:, 0:4, 8:12] = draw_sum(P[:, :, :, None] * gx[:, :, None, :])
        M[:, 4:8, 8:12] = draw_sum(P[:, :, :, None] * gy[:, :, None, :])
        M[:, 8:12, 8:12] = draw_sum(gx[:, :, :, None] * gx[:, :, None, :] + gy[:, :, :, None] * gy[:, :, None, :])
        iu = np.triu_indices(12, 1)
        M[:, iu[1], iu[0]] = M[:, iu[0], iu[1]]
        p, Md, _ = jacobi(M, return_state=True)
        p = p.reshape(H, 3, 4)
        A = p[:, :, :3] * s[:, None, None]
        b = ((p[:, :, 3] - A[:, :, 0] * c[:, None, 0]) - A[:, :, 1] * c[:, None, 1]) - A[:, :, 2] * c[:, None, 2]
    R, t = nearest_rotation(A, b)
    out = (idx.astype(np.int32), R.reshape(H, 9), t)
    return out + (Md,) if return_state else out


# ---- the inlier test -------------------------------------------------------------------------------------------------------
def camera_points(R, t, X):
    """Xc (3 arrays broadcast over poses (H, 1) and points (1, m))."""
    return [((R[:, 3 * r, None] * X[None, :, 0] + R[:, 3 * r + 1, None] * X[None, :, 1]) + R[:, 3 * r + 2, None] * X[None, :, 2])
            + t[:, r, None] for r in range(3)]


def inlier_matrix(R, t, pts3d, pts2d, K, threshold, with_margin=False):
    """(H, m) bool of the poses R (H, 9), t (H, 3); with_margin also the smallest relative distance of ee from t2 z z."""
    R, t = np.asarray(R, np.float64).reshape(-1, 9), np.asarray(t, np.float64).reshape(-1, 3)
    X, x = promote(pts3d, pts2d)
    fx, fy, cx, cy = intrinsics(K)
    t2 = float(threshold) * float(threshold)
    out = np.empty((len(R), len(X)), bool)
    margin = np.inf
    step = max(1, 2_000_000 // max(len(X), 1))
    with np.errstate(all="ignore"):
        cu, cv = (cx - x[:, 0])[None, :], (cy - x[:, 1])[None, :]
        for a in range(0, len(R), step):
            x0, x1, z = camera_points(R[a:a + step], t[a:a + step], X)
            ex = fx * x0 + cu * z
            ey = fy * x1 + cv * z
            ee = ex * ex + ey * ey
            lim = t2 * (z * z)
            out[a:a + step] = (z > 0.0) & (ee <= lim) & (ee < np.inf)
            if with_margin:
                rel = (np.abs(ee - lim) / lim)[z > 0.0]
                rel = rel[np.isfinite(rel)]
                if rel.size:
                    margin = min(margin, float(rel.min()))
    return (out, margin) if with_margin else out


def score(R, t, pts3d, pts2d, K, threshold):
    return inlier_matrix(R, t, pts3d, pts2d, K, threshold).sum(axis=1).astype(np.int32)


def inliers(R, t, pts3d, pts2d, K, threshold):
    return inlier_matrix(np.asarray(R).reshape(1, 9), np.asarray(t).reshape(1, 3), pts3d, pts2d, K, threshold)[0]


# ---- the refit -------------------------------------------------------------------------------------------------------------
def refit_pass(R, t, X, x, intr, member):
    """The 29 SUMs of one pass under (R (9,), t (3,)) over the set `member`."""
    fx, fy, cx, cy = intr
    with np.errstate(all="ignore"):
        x0, x1, z = (v[0] for v in camera_points(R[None], t[None], X))
        front = member & (z > 0.0)
        iz = 1.0 / z
        xz, yz = x0 * iz, x1 * iz
        rx, ry = (fx * xz + cx) - x[:, 0], (fy * yz + cy) - x[:, 1]
        ax, ay = fx * iz, fy * iz
        bx, by = -(ax * xz), -(ay * yz)
        zero = np.zeros_like(z)
        Jx = [bx * x1, ax * z - bx * x0, -(ax * x1), ax, zero, bx]
        Jy = [by * x1 - ay * z, -(by * x0), ay * x0, zero, ay, by]
        terms = [Jx[i] * Jx[j] + Jy[i] * Jy[j] for i in range(6) for j in range(i, 6)]
        terms += [Jx[i] * rx + Jy[i] * ry for i in range(6)]
        terms += [rx * rx + ry * ry, np.ones_like(z)]
        return block_sum(np.stack(terms, axis=1), front)


def gn_step(sums, R, t):
    """The header's STEP: (R', t') or None when a pivot is not positive and finite."""
    H = np.zeros((6, 6))
    e = 0
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = sums[e]
            e += 1
    g = sums[21:27]
    L = np.zeros((6, 6))
    with np.errstate(all="ignore"):
        for j in range(6):
            s = H[j, j]
            for k in range(j):
                s = s - L[j, k] * L[j, k]
            if not (s > 0.0 and s < np.inf):
                return None
            L[j, j] = np.sqrt(s)
            for i in range(j + 1, 6):
                s = H[j, i]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = s / L[j, j]
        y = np.zeros(6)
        for i in range(6):
            s = -g[i]
            for k in range(i):
                s = s - L[i, k] * y[k]
            y[i] = s / L[i, i]
        d = np.zeros(6)
        for i in range(5, -1, -1):
            s = y[i]
            for k in range(i + 1, 6):
                s = s - L[k, i] * d[k]
            d[i] = s / L[i, i]
        hx, hy, hz = 0.5 * d[0], 0.5 * d[1], 0.5 * d[2]
        n = np.sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz)
        qw, qx, qy, qz = 1.0 / n, hx / n, hy / n, hz / n
        Q = np.array([[1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qz * qw), 2.0 * (qx * qz + qy * qw)],
                      [2.0 * (qx * qy + qz * qw), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qx * qw)],
                      [2.0 * (qx * qz - qy * qw), 2.0 * (qy * qz + qx * qw), 1.0 - 2.0 * (qx * qx + qy * qy)]])
        Rm = R.reshape(3, 3)
        Rn, tn = np.empty((3, 3)), np.empty(3)
        for r in range(3):
            for c in range(3):
                Rn[r, c] = (Q[r, 0] * Rm[0, c] + Q[r, 1] * Rm[1, c]) + Q[r, 2] * Rm[2, c]
            tn[r] = ((Q[r, 0] * t[0] + Q[r, 1] * t[1]) + Q[r, 2] * t[2]) + d[3 + r]
    return Rn.reshape(9), tn


def refine(pts3d, pts2d, K, R, t, mask=None, return_costs=False):
    """amvs_pnp_refine: (R (9,), t (3,), steps, cost)."""
    X, x = promote(pts3d, pts2d)
    intr = intrinsics(K)
    member = np.ones(len(X), bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    R, t = np.array(R, np.float64).reshape(9), np.array(t, np.float64).reshape(3)
    sums = refit_pass(R, t, X, x, intr, member)
    steps, costs = 0, [float(sums[27])]
    for _ in range(REFINE_STEPS):
        new = gn_step(sums, R, t)
        if new is None:
            break
        new_sums = refit_pass(new[0], new[1], X, x, intr, member)
        costs.append(float(new_sums[27]))
        if not (new_sums[27] <= sums[27] and new_sums[28] >= sums[28]):
            break
        R, t, sums = new[0], new[1], new_sums
        steps += 1
    out = (R, t, steps, float(sums[27]))
    return out + (costs,) if return_costs else out


# ---- RANSAC ----------------------------------------------------------------------------------------------------------------
def needed(best, m, confidence, max_hypotheses):
    """(N, N came from a logarithm): the header's N after a batch."""
    w = float(best) / float(m)
    w2 = w * w
    p = (w2 * w2) * w2
    if p >= 1.0:
        return 0.0, False
    if 1.0 - p == 1.0:
        return float(max_hypotheses), False
    return float(math.ceil(math.log(1.0 - confidence) / math.log(1.0 - p))), True


class Scored:
    """The hypotheses of one (points, K, seed, threshold) and their counts, computed once per batch and kept: hypothesis
    h is a function of h alone, so every max_hypotheses reads the same batches."""

    def __init__(self, pts3d, pts2d, K, threshold, seed):
        self.args, self.threshold, self.seed, self.batches = (pts3d, pts2d, K), threshold, seed, {}

    def batch(self, first, count):
        if first not in self.batches:
            _, R, t = hypotheses(*self.args, self.seed, first, BATCH)
            self.batches[first] = (R, t, score(R, t, *self.args, self.threshold))
        R, t, counts = self.batches[first]
        return R[:count], t[:count], counts[:count]


def ransac(pts3d, pts2d, K, threshold=8.0, confidence=0.99, max_hypotheses=5000, seed=0, scored=None):
    """amvs_pnp_ransac: (R (9,), t (3,), mask (m,) bool, n_inliers, info [3], trace of (done, N, N from a logarithm) per
    batch, (steps, steps) of the two refits)."""
    m = len(pts3d)
    scored = scored or Scored(pts3d, pts2d, K, threshold, seed)
    done, best, best_h, trace = 0, -1, 0, []
    while True:
        nb = min(BATCH, max_hypotheses - done)
        R, t, counts = scored.batch(done, nb)
        j = int(np.argmax(counts))                      # the first of the largest: the lowest h
        if int(counts[j]) > best:
            best, best_h, best_pose = int(counts[j]), done + j, (R[j].copy(), t[j].copy())
        done += nb
        N, from_log = needed(best, m, confidence, max_hypotheses)
        trace.append((done, N, from_log))
        if done >= N or done == max_hypotheses:
            break
    info = np.array([done, best_h, best], np.int32)
    none = (np.zeros(9), np.zeros(3), np.zeros(m, bool), 0, info, trace, (0, 0))
    if best < 6:
        return none
    S0 = inliers(*best_pose, pts3d, pts2d, K, threshold)
    R1, t1, k1, _ = refine(pts3d, pts2d, K, *best_pose, S0)
    S1 = inliers(R1, t1, pts3d, pts2d, K, threshold)
    if S1.sum() < 6:
        return none
    R2, t2, k2, _ = refine(pts3d, pts2d, K, R1, t1, S1)
    S2 = inliers(R2, t2, pts3d, pts2d, K, threshold)
    if S2.sum() >= S1.sum():
        return R2, t2, S2, int(S2.sum()), info, trace, (k1, k2)
    return R1, t1, S1, int(S1.sum()), info, trace, (k1, k2)
