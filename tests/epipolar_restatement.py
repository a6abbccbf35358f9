"""NumPy restatement of include/amvs_epipolar.h, written from the header's text alone: the sampler, the 8-point fit with
its block sums and fixed-sweep Jacobi, the inlier test, the refit and the RANSAC loop.  Vectorised over hypotheses; every
float64 operation is one NumPy ufunc call (one rounding, nothing fused), in the header's order.  The device is compared
with this bit for bit (tests/test_hip_epipolar.py)."""
import math

import numpy as np

JACOBI_SWEEPS = 10        # include/amvs_match.h AMVS_JACOBI_SWEEPS
BATCH = 1024              # AMVS_FMAT_BATCH
BLOCK = 64                # AMVS_FMAT_BLOCK
ROOT2 = 1.4142135623730951


# ---- sampler ---------------------------------------------------------------------------------------------------------------
def mix(z):
    """splitmix64's finaliser on a uint64 array (array arithmetic wraps modulo 2^64)."""
    z = np.asarray(z, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sample(seed, h, m):
    """(len(h), 8) int64: the samples of the hypotheses h, in draw order."""
    h = np.atleast_1d(np.asarray(h)).astype(np.uint64)
    idx = np.empty((len(h), 8), np.int64)
    for k in range(8):
        r = (mix(np.uint64(seed) ^ mix(np.uint64(8) * h + np.uint64(k))) % np.uint64(m - k)).astype(np.int64)
        chosen = np.sort(idx[:, :k], axis=1)
        for i in range(k):
            r = r + (r >= chosen[:, i])
        idx[:, k] = r
    return idx


# ---- Jacobi ----------------------------------------------------------------------------------------------------------------
def jacobi(M, sweeps=JACOBI_SWEEPS, return_state=False):
    """amvs_match.h step 3 on (H, N, N) symmetric matrices; returns the (H, N) column of the smallest diagonal entry."""
    M = np.array(M, np.float64)
    H, N, _ = M.shape
    V = np.zeros((H, N, N))
    V[:, np.arange(N), np.arange(N)] = 1.0
    with np.errstate(all="ignore"):
        for _sweep in range(sweeps):
            for p in range(N - 1):
                for q in range(p + 1, N):
                    g = M[:, p, q].copy()
                    act = ~(g == 0.0)
                    if not act.any():
                        continue
                    theta = (M[:, q, q] - M[:, p, p]) / (2.0 * g)
                    sgn = np.where(theta < 0.0, -1.0, 1.0)
                    t = np.where(np.abs(theta) > 1e150, 0.5 / theta, sgn / (np.abs(theta) + np.sqrt(theta * theta + 1.0)))
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    tg = t * g
                    M[:, p, p] = np.where(act, M[:, p, p] - tg, M[:, p, p])
                    M[:, q, q] = np.where(act, M[:, q, q] + tg, M[:, q, q])
                    M[:, p, q] = M[:, q, p] = np.where(act, 0.0, g)
                    rows = [r for r in range(N) if r != p and r != q]
                    a2, c2, s2 = act[:, None], c[:, None], s[:, None]
                    x, y = M[:, rows, p].copy(), M[:, rows, q].copy()
                    xp, yq = np.where(a2, c2 * x - s2 * y, x), np.where(a2, s2 * x + c2 * y, y)
                    M[:, rows, p] = xp
                    M[:, p, rows] = xp
                    M[:, rows, q] = yq
                    M[:, q, rows] = yq
                    x, y = V[:, :, p].copy(), V[:, :, q].copy()
                    V[:, :, p] = np.where(a2, c2 * x - s2 * y, x)
                    V[:, :, q] = np.where(a2, s2 * x + c2 * y, y)
        diag = M[:, np.arange(N), np.arange(N)]
        best, at = diag[:, 0].copy(), np.zeros(H, np.int64)
        for k in range(1, N):
            lt = diag[:, k] < best
            best = np.where(lt, diag[:, k], best)
            at = np.where(lt, k, at)
    f = V[np.arange(H), :, at]
    return (f, M, V) if return_state else f


# ---- sums ------------------------------------------------------------------------------------------------------------------
def block_sum(terms, member):
    """The header's SUM over the set `member` (m,) bool of terms (m, ...): block partials, then the partials in order."""
    terms = np.asarray(terms, np.float64)
    m = len(terms)
    nb = -(-m // BLOCK)
    shape = terms.shape[1:]
    t = np.zeros((nb * BLOCK,) + shape)
    t[:m] = terms
    mem = np.zeros(nb * BLOCK, bool)
    mem[:m] = member
    t = t.reshape((nb, BLOCK) + shape)
    mem = mem.reshape((nb, BLOCK) + (1,) * len(shape))
    part = np.zeros((nb,) + shape)
    with np.errstate(all="ignore"):
        for j in range(BLOCK):
            part = np.where(mem[:, j], part + t[:, j], part)
        total = np.zeros(shape)
        for b in range(nb):
            total = total + part[b]
    return total


def draw_sum(terms):
    """SUM over the 8 matches of samples, terms (H, 8, ...): one block in draw order, then the one partial."""
    with np.errstate(all="ignore"):
        part = np.zeros(terms.shape[:1] + terms.shape[2:])
        for k in range(terms.shape[1]):
            part = part + terms[:, k]
        return 0.0 + part


# ---- the fit ---------------------------------------------------------------------------------------------------------------
def rows_of(x1n, y1n, x2n, y2n):
    return np.stack([x2n * x1n, x2n * y1n, x2n, y2n * x1n, y2n * y1n, y2n, x1n, y1n, np.ones_like(x1n)], axis=-1)


def denormalise(f, cx1, cy1, s1, cx2, cy2, s2):
    """Step 6 on f (H, 9) with per-hypothesis (H,) normalisations."""
    with np.errstate(all="ignore"):
        G = np.empty_like(f)
        for r in range(3):
            G[:, 3 * r] = f[:, 3 * r] * s1
            G[:, 3 * r + 1] = f[:, 3 * r + 1] * s1
            G[:, 3 * r + 2] = (f[:, 3 * r + 2] - G[:, 3 * r] * cx1) - G[:, 3 * r + 1] * cy1
        F = np.empty_like(f)
        for c in range(3):
            F[:, c] = s2 * G[:, c]
            F[:, 3 + c] = s2 * G[:, 3 + c]
            F[:, 6 + c] = (G[:, 6 + c] - F[:, c] * cx2) - F[:, 3 + c] * cy2
    return F


def hypotheses(pts1, pts2, seed, first, count, return_state=False):
    """(idx (count, 8) int32, F (count, 9)): amvs_fmat_hypotheses."""
    p1, p2 = np.asarray(pts1, np.float32).astype(np.float64), np.asarray(pts2, np.float32).astype(np.float64)
    m = len(p1)
    idx = sample(seed, np.arange(first, first + count), m)
    x1, y1, x2, y2 = p1[idx, 0], p1[idx, 1], p2[idx, 0], p2[idx, 1]          # (H, 8)
    with np.errstate(all="ignore"):
        cx1, cy1, cx2, cy2 = (draw_sum(v) / 8.0 for v in (x1, y1, x2, y2))
        u1, v1, u2, v2 = x1 - cx1[:, None], y1 - cy1[:, None], x2 - cx2[:, None], y2 - cy2[:, None]
        s1 = ROOT2 / (draw_sum(np.sqrt(u1 * u1 + v1 * v1)) / 8.0)
        s2 = ROOT2 / (draw_sum(np.sqrt(u2 * u2 + v2 * v2)) / 8.0)
        a = rows_of(u1 * s1[:, None], v1 * s1[:, None], u2 * s2[:, None], v2 * s2[:, None])      # (H, 8, 9)
        M = draw_sum(a[:, :, :, None] * a[:, :, None, :])
    out = jacobi(M, return_state=return_state)
    f = out[0] if return_state else out
    F = denormalise(f, cx1, cy1, s1, cx2, cy2, s2)
    if return_state:
        return idx.astype(np.int32), F, out[1]
    return idx.astype(np.int32), F


def finalise(F):
    """Step 7: unit Frobenius norm by the sequential sum, the entry of largest magnitude positive."""
    with np.errstate(all="ignore"):
        q = F[0] * F[0]
        for e in range(1, 9):
            q = q + F[e] * F[e]
        F = F / np.sqrt(q)
        k = 0
        for e in range(1, 9):
            if abs(F[e]) > abs(F[k]):
                k = e
        if F[k] < 0.0:
            F = -F
    return F


def fit(pts1, pts2, mask=None, rank2=True, final=True):
    """amvs_fmat_fit: the refit (steps 1-7) to the matches of `mask` (None: all); F (9,)."""
    p1, p2 = np.asarray(pts1, np.float32).astype(np.float64), np.asarray(pts2, np.float32).astype(np.float64)
    m = len(p1)
    mem = np.ones(m, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    N = float(int(mem.sum()))
    with np.errstate(all="ignore"):
        c = block_sum(np.concatenate([p1, p2], axis=1), mem) / N            # cx1, cy1, cx2, cy2
        u1, v1, u2, v2 = p1[:, 0] - c[0], p1[:, 1] - c[1], p2[:, 0] - c[2], p2[:, 1] - c[3]
        d = block_sum(np.stack([np.sqrt(u1 * u1 + v1 * v1), np.sqrt(u2 * u2 + v2 * v2)], axis=1), mem) / N
        s1, s2 = ROOT2 / d[0], ROOT2 / d[1]
        a = rows_of(u1 * s1, v1 * s1, u2 * s2, v2 * s2)                     # (m, 9)
        M = block_sum(a[:, :, None] * a[:, None, :], mem)
        f = jacobi(M[None])[0]
        if rank2:
            A = np.empty((3, 3))
            for i in range(3):
                for j in range(3):
                    A[i, j] = (f[i] * f[j] + f[3 + i] * f[3 + j]) + f[6 + i] * f[6 + j]
            v = jacobi(A[None])[0]
            f = f.copy()
            for r in range(3):
                w = (f[3 * r] * v[0] + f[3 * r + 1] * v[1]) + f[3 * r + 2] * v[2]
                for k in range(3):
                    f[3 * r + k] = f[3 * r + k] - w * v[k]
        one = np.ones(1)
        F = denormalise(f[None], c[0] * one, c[1] * one, s1 * one, c[2] * one, c[3] * one, s2 * one)[0]
    return finalise(F) if final else F


# ---- the inlier test -------------------------------------------------------------------------------------------------------
def inlier_matrix(F, pts1, pts2, threshold, with_margin=False):
    """(H, m) bool of F (H, 9); with_margin also the smallest relative distance of a decision from its threshold."""
    F = np.asarray(F, np.float64).reshape(-1, 9)
    p1, p2 = np.asarray(pts1, np.float32).astype(np.float64), np.asarray(pts2, np.float32).astype(np.float64)
    x1, y1, x2, y2 = p1[None, :, 0], p1[None, :, 1], p2[None, :, 0], p2[None, :, 1]
    t2 = float(threshold) * float(threshold)
    out = np.empty((len(F), len(p1)), bool)
    margin = np.inf
    step = max(1, 2_000_000 // max(len(p1), 1))
    with np.errstate(all="ignore"):
        for a in range(0, len(F), step):
            f = [F[a:a + step, e, None] for e in range(9)]
            l20, l21, l22 = (f[0] * x1 + f[1] * y1) + f[2], (f[3] * x1 + f[4] * y1) + f[5], (f[6] * x1 + f[7] * y1) + f[8]
            l10, l11 = (f[0] * x2 + f[3] * y2) + f[6], (f[1] * x2 + f[4] * y2) + f[7]
            e = (x2 * l20 + y2 * l21) + l22
            dd = e * e
            n2, n1 = l20 * l20 + l21 * l21, l10 * l10 + l11 * l11
            out[a:a + step] = (n1 > 0.0) & (n2 > 0.0) & (dd <= t2 * n2) & (dd <= t2 * n1) & (dd < np.inf)
            if with_margin:
                for n in (n1, n2):
                    rel = np.abs(dd - t2 * n) / (t2 * n)
                    rel = rel[np.isfinite(rel)]
                    if rel.size:
                        margin = min(margin, float(rel.min()))
    return (out, margin) if with_margin else out


def score(F, pts1, pts2, threshold):
    return inlier_matrix(F, pts1, pts2, threshold).sum(axis=1).astype(np.int32)


def inliers(F, pts1, pts2, threshold):
    return inlier_matrix(np.asarray(F).reshape(1, 9), pts1, pts2, threshold)[0]


# ---- RANSAC ----------------------------------------------------------------------------------------------------------------
def needed(best, m, confidence, max_hypotheses, with_branch=False):
    """The header's N after a batch (a float; may exceed max_hypotheses); with_branch also whether a logarithm gave it."""
    if with_branch:
        w = float(best) / float(m)
        p = ((w * w) * (w * w)) * ((w * w) * (w * w))
        return needed(best, m, confidence, max_hypotheses), not (p >= 1.0 or 1.0 - p == 1.0)
    w = float(best) / float(m)
    p = w * w
    p = p * p
    p = p * p
    if p >= 1.0:
        return 0.0
    if 1.0 - p == 1.0:
        return float(max_hypotheses)
    return float(math.ceil(math.log(1.0 - confidence) / math.log(1.0 - p)))


def ransac(pts1, pts2, threshold=2.0, confidence=0.999, max_hypotheses=4096, seed=0):
    """amvs_fmat_ransac: (F (9,), mask (m,) bool, n_inliers, info [3], trace of (done, N, N came from a logarithm) per
    batch)."""
    m = len(pts1)
    done, best, best_h, trace = 0, -1, 0, []
    while True:
        nb = min(BATCH, max_hypotheses - done)
        _, F = hypotheses(pts1, pts2, seed, done, nb)
        counts = score(F, pts1, pts2, threshold)
        j = int(np.argmax(counts))                      # the first of the largest: the lowest h
        if int(counts[j]) > best:
            best, best_h = int(counts[j]), done + j
        done += nb
        N, from_log = needed(best, m, confidence, max_hypotheses, with_branch=True)
        trace.append((done, N, from_log))
        if done >= N or done == max_hypotheses:
            break
    info = np.array([done, best_h, best], np.int32)
    none = (np.zeros(9), np.zeros(m, bool), 0, info, trace)
    if best < 8:
        return none
    _, Fh = hypotheses(pts1, pts2, seed, best_h, 1)
    S0 = inliers(Fh[0], pts1, pts2, threshold)
    F1 = fit(pts1, pts2, S0)
    S1 = inliers(F1, pts1, pts2, threshold)
    if S1.sum() < 8:
        return none
    F2 = fit(pts1, pts2, S1)
    S2 = inliers(F2, pts1, pts2, threshold)
    if S2.sum() >= S1.sum():
        return F2, S2, int(S2.sum()), info, trace
    return F1, S1, int(S1.sum()), info, trace
