"""The dense-SIFT mode restated in NumPy from the text of include/amvs_match.h alone (no library code is read or called):
exact 2-nearest-neighbour search, the ratio test and the cross check, the pair triangulation operation by operation,
the bounds and the grid voxel de-duplication, the pair list and the chained reconstruction.  NumPy's element-wise float64
+, -, *, / and sqrt round once and are never fused, which is the arithmetic the header prescribes."""
import numpy as np

JACOBI_SWEEPS = 10
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


# ---- descriptors ---------------------------------------------------------------------------------------------------------
def dist2(q, t):
    """[n_q][n_t] int64: the exact squared distances (float64 products of integers below 2^16 summed 128 times: exact)."""
    a, b = np.asarray(q, np.float64), np.asarray(t, np.float64)
    s = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)
    return s.astype(np.int64)


def knn2(q, t, rows_per_step=512):
    """(idx [n_q][2] int32, dist2 [n_q][2] int32): the two train rows smallest under (s, j)."""
    q, t = np.asarray(q), np.asarray(t)
    idx = np.empty((len(q), 2), np.int32)
    d2 = np.empty((len(q), 2), np.int32)
    for r0 in range(0, len(q), rows_per_step):
        s = dist2(q[r0:r0 + rows_per_step], t)
        order = np.argsort(s, axis=1, kind="stable")[:, :2]          # stable: equal s in ascending j
        idx[r0:r0 + rows_per_step] = order
        d2[r0:r0 + rows_per_step] = np.take_along_axis(s, order, 1)
    return idx, d2


def knn2_by_minima(q, t, rows_per_step=256):
    """knn2 for large sets without a sort: np.argmin returns the FIRST minimum, the lowest index among equal s; the
    second entry is the first minimum of what is left.  tests/test_match_cpu.py holds it to knn2."""
    q, t = np.asarray(q), np.asarray(t)
    b = t.astype(np.float64)
    bn = (b * b).sum(1)
    idx = np.empty((len(q), 2), np.int32)
    d2 = np.empty((len(q), 2), np.int32)
    for r0 in range(0, len(q), rows_per_step):
        a = q[r0:r0 + rows_per_step].astype(np.float64)
        s = ((a * a).sum(1)[:, None] + bn[None, :] - 2.0 * (a @ b.T)).astype(np.int64)
        rows = np.arange(len(a))
        for k in range(2):
            j = np.argmin(s, axis=1)
            idx[r0:r0 + rows_per_step, k] = j
            d2[r0:r0 + rows_per_step, k] = s[rows, j]
            s[rows, j] = np.iinfo(np.int64).max
    return idx, d2


def ratio_keep(d2, ratio):
    r = np.float64(np.float32(ratio))
    return d2[:, 0].astype(np.float64) < (r * r) * d2[:, 1].astype(np.float64)


def match(q, t, ratio, cross_check=False):
    """(q_idx, t_idx, dist2) int32 in query order."""
    idx, d2 = knn2(q, t)
    keep = ratio_keep(d2, ratio)
    if cross_check:
        ridx, rd2 = knn2(t, q)
        rkeep = ratio_keep(rd2, ratio)
        j = idx[:, 0]
        keep &= rkeep[j] & (ridx[j, 0] == np.arange(len(q)))
    i = np.nonzero(keep)[0].astype(np.int32)
    return i, idx[i, 0].copy(), d2[i, 0].copy()


# ---- triangulation ---------------------------------------------------------------------------------------------------------
def projection(K, R, t):
    K, R, t = np.asarray(K, np.float64).reshape(3, 3), np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    Rt = np.concatenate([R, t[:, None]], 1)
    P = np.empty((3, 4))
    for r in range(3):
        for c in range(4):
            P[r, c] = (K[r, 0] * Rt[0, c] + K[r, 1] * Rt[1, c]) + K[r, 2] * Rt[2, c]
    C = np.array([-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) for i in range(3)])
    return P, C


def normal_matrix(P1, P2, pts1, pts2):
    """A ([m][4][4]) and M = A^T A ([m][4][4]) of the header's steps 1 and 2."""
    x1, y1 = pts1[:, 0].astype(np.float64), pts1[:, 1].astype(np.float64)
    x2, y2 = pts2[:, 0].astype(np.float64), pts2[:, 1].astype(np.float64)
    m = len(x1)
    A = np.empty((m, 4, 4))
    for c in range(4):
        A[:, 0, c] = x1 * P1[2, c] - P1[0, c]
        A[:, 1, c] = y1 * P1[2, c] - P1[1, c]
        A[:, 2, c] = x2 * P2[2, c] - P2[0, c]
        A[:, 3, c] = y2 * P2[2, c] - P2[1, c]
    M = np.empty((m, 4, 4))
    for i in range(4):
        for j in range(i, 4):
            v = ((A[:, 0, i] * A[:, 0, j] + A[:, 1, i] * A[:, 1, j]) + A[:, 2, i] * A[:, 2, j]) + A[:, 3, i] * A[:, 3, j]
            M[:, i, j] = v
            M[:, j, i] = v
    return A, M


def jacobi_smallest(M, sqrt=np.sqrt):
    """The eigenvector ([m][4]) of the smallest diagonal entry after the header's cyclic Jacobi; M: [m][4][4]."""
    M = M.copy()
    m = len(M)
    V = np.zeros((m, 4, 4))
    for i in range(4):
        V[:, i, i] = 1.0
    with np.errstate(all="ignore"):
        for _ in range(JACOBI_SWEEPS):
            for p, q in PAIRS:
                g = M[:, p, q].copy()
                live = g != 0.0
                gs = np.where(live, g, 1.0)
                theta = (M[:, q, q] - M[:, p, p]) / (2.0 * gs)
                big = np.abs(theta) > 1e150
                th = np.where(big, 1.0, theta)
                t_small = np.where(th < 0.0, -1.0, 1.0) / (np.abs(th) + sqrt(th * th + 1.0))
                t = np.where(big, 0.5 / np.where(big, theta, 1.0), t_small)
                c = 1.0 / sqrt(t * t + 1.0)
                s = t * c
                N = M.copy()
                N[:, p, p] = M[:, p, p] - t * g
                N[:, q, q] = M[:, q, q] + t * g
                N[:, p, q] = 0.0
                N[:, q, p] = 0.0
                for r in range(4):
                    if r in (p, q):
                        continue
                    x, y = M[:, r, p], M[:, r, q]
                    N[:, r, p] = N[:, p, r] = c * x - s * y
                    N[:, r, q] = N[:, q, r] = s * x + c * y
                W = V.copy()
                for r in range(4):
                    x, y = V[:, r, p], V[:, r, q]
                    W[:, r, p] = c * x - s * y
                    W[:, r, q] = s * x + c * y
                M = np.where(live[:, None, None], N, M)
                V = np.where(live[:, None, None], W, V)
        best = M[:, 0, 0].copy()
        v = V[:, :, 0].copy()
        for k in range(1, 4):
            lower = M[:, k, k] < best
            best = np.where(lower, M[:, k, k], best)
            v = np.where(lower[:, None], V[:, :, k], v)
    return v


def triangulate(K, R1, t1, R2, t2, pts1, pts2, depth_min=0.1, depth_max=50.0, cos_min_parallax=None, max_reproj=6.0,
                sqrt=np.sqrt):
    """(X [m][3], keep [m] bool, margins [m]: the smallest relative distance of a decision that was taken to its
    threshold).  The filters apply in order: a candidate's later margins do not count once it is dropped."""
    if cos_min_parallax is None:
        cos_min_parallax = float(np.cos(np.deg2rad(0.3)))
    K = np.asarray(K, np.float64).reshape(3, 3)
    Rs = [np.asarray(R, np.float64).reshape(3, 3) for R in (R1, R2)]
    ts = [np.asarray(t, np.float64).reshape(3) for t in (t1, t2)]
    pts = [np.asarray(p, np.float32).reshape(-1, 2) for p in (pts1, pts2)]
    m = len(pts[0])
    if m == 0:
        return np.empty((0, 3)), np.zeros(0, bool), np.empty(0)
    (P1, C1), (P2, C2) = projection(K, Rs[0], ts[0]), projection(K, Rs[1], ts[1])
    _, M = normal_matrix(P1, P2, pts[0], pts[1])
    v = jacobi_smallest(M, sqrt)
    with np.errstate(all="ignore"):
        X = np.stack([v[:, i] / v[:, 3] for i in range(3)], 1)
        pc = []
        for R, t in zip(Rs, ts):
            pc.append(np.stack([((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r] for r in range(3)], 1))
        z1, z2 = pc[0][:, 2], pc[1][:, 2]
        keep_d = (z1 > depth_min) & (z1 < depth_max) & (z2 > depth_min) & (z2 < depth_max)
        margin = np.minimum.reduce([np.abs(z - lim) / abs(lim) for z in (z1, z2) for lim in (depth_min, depth_max)])
        w1, w2 = X - C1, X - C2
        dot = (w1[:, 0] * w2[:, 0] + w1[:, 1] * w2[:, 1]) + w1[:, 2] * w2[:, 2]
        n1 = sqrt((w1[:, 0] * w1[:, 0] + w1[:, 1] * w1[:, 1]) + w1[:, 2] * w1[:, 2])
        n2 = sqrt((w2[:, 0] * w2[:, 0] + w2[:, 1] * w2[:, 1]) + w2[:, 2] * w2[:, 2])
        cs = dot / (n1 * n2 + 1e-8)
        keep_p = cs < cos_min_parallax
        # the parallax margin is taken on 1 - cos, the quantity that is small at the floor
        margin = np.where(keep_d, np.minimum(margin, np.abs(cs - cos_min_parallax) / (1.0 - cos_min_parallax)), margin)
        errs = []
        for k in range(2):
            h = [(K[r, 0] * pc[k][:, 0] + K[r, 1] * pc[k][:, 1]) + K[r, 2] * pc[k][:, 2] for r in range(3)]
            du = h[0] / h[2] - pts[k][:, 0].astype(np.float64)
            dv = h[1] / h[2] - pts[k][:, 1].astype(np.float64)
            errs.append(sqrt(du * du + dv * dv))
        keep_r = (errs[0] < max_reproj) & (errs[1] < max_reproj)
        m_r = np.minimum(np.abs(errs[0] - max_reproj), np.abs(errs[1] - max_reproj)) / max_reproj
        margin = np.where(keep_d & keep_p, np.minimum(margin, m_r), margin)
    return X, keep_d & keep_p & keep_r, margin


def triangulate_svd(K, R1, t1, R2, t2, pts1, pts2):
    """X by an SVD of A: the yardstick of the normal-matrix route (not the definition)."""
    (P1, _), (P2, _) = projection(K, R1, t1), projection(K, R2, t2)
    A, _ = normal_matrix(P1, P2, np.asarray(pts1, np.float32), np.asarray(pts2, np.float32))
    v = np.linalg.svd(A)[2][:, 3, :]
    return v[:, :3] / v[:, 3:4]


# ---- bounds and the grid ---------------------------------------------------------------------------------------------------
def bounds(points, keep=None):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if keep is not None:
        p = p[np.asarray(keep, bool)]
    return p.min(0), p.max(0)


def voxel_grid(points, colors, origin, voxel_size, keep=None):
    """(points, colors) after the grid de-duplication: the first kept point of every voxel in lexicographic voxel order."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    c = np.asarray(colors).reshape(-1, 3)
    if keep is not None:
        p, c = p[np.asarray(keep, bool)], c[np.asarray(keep, bool)]
    if len(p) == 0:
        return p, c
    iv = np.floor((p - np.asarray(origin, np.float64)) / np.float64(voxel_size)).astype(np.int64)
    _, first = np.unique(iv, axis=0, return_index=True)
    return p[first], c[first]


# ---- the host logic ---------------------------------------------------------------------------------------------------------
def pair_list(n, window):
    """Positions (i, j), i < j, with |i - j| <= window or |i - j| >= n - window."""
    out = []
    for i in range(n):
        for j in range(n):
            if j <= i:
                continue
            if abs(i - j) <= window or abs(i - j) >= n - window:
                out.append((i, j))
    return out


def knn_mean_brute(points, k=20):
    """Mean distance to the k - 1 nearest other points (a CPU stand-in of the pinned device statistic)."""
    p = np.asarray(points, np.float64)
    out = np.empty(len(p))
    for i in range(len(p)):
        d = p - p[i]
        dist = np.sqrt((d * d).sum(1))
        out[i] = np.sort(dist)[1:k].mean()
    return out


def reconstruct(K, features, images, poses, window=20, ratio=0.85, cross_check=False, knn_stat=knn_mean_brute):
    """The chained restatement of reconstruct_from_features: (points [n][3] float64, colors [n][3] uint8).  features[idx]:
    {'descriptors': (n, 128) uint8, 'points': (n, 2) float32}; poses[idx]: (R, t)."""
    keys = sorted(poses.keys())
    pts_all, col_all = [], []
    for i, j in pair_list(len(keys), window):
        a, b = keys[i], keys[j]
        if a not in features or b not in features:
            continue
        da, db = features[a]["descriptors"], features[b]["descriptors"]
        if len(da) < 2 or len(db) < 2:
            continue
        qi, ti, _ = match(da, db, ratio, cross_check)
        if len(qi) < 10:
            continue
        p1, p2 = features[a]["points"][qi], features[b]["points"][ti]
        img = images[a]["image"]
        h, w = img.shape[:2]
        xs = np.clip(p1[:, 0], 0, w - 1).astype(int)
        ys = np.clip(p1[:, 1], 0, h - 1).astype(int)
        rgb = img[ys, xs][:, ::-1]
        X, keep, _ = triangulate(K, poses[a][0], poses[a][1], poses[b][0], poses[b][1], p1, p2)
        pts_all.append(X[keep])
        col_all.append(rgb[keep])
    if not pts_all or sum(len(p) for p in pts_all) == 0:
        return np.empty((0, 3)), np.empty((0, 3), np.uint8)
    points, colors = np.vstack(pts_all), np.vstack(col_all).astype(np.uint8)
    if len(points) < 100:
        return points, colors
    stat = knn_stat(points, 20)
    keep = stat < np.mean(stat) + 2.5 * np.std(stat)
    if not keep.any():
        return points[keep], colors[keep]
    mn, mx = bounds(points, keep)
    voxel = np.linalg.norm(mx - mn) / 1200.0
    return voxel_grid(points, colors, mn, voxel, keep)
