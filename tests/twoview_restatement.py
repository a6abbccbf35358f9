"""include/amvs_twoview.h restated in NumPy from the header's text alone (no library code is read or called): the
decomposition of F into four pose candidates, the cheirality test, count and mask, the relative pose, and the
triangulation with its seven comparisons.  The DLT is that of include/amvs_match.h steps 1 to 4, which
tests/match_restatement.py restates; it is taken from there.  Python floats and NumPy's element-wise float64 + - * / and
sqrt round once and are never fused, which is the arithmetic the header prescribes.  find_best_initial_pair restates
the pipeline of core/geometry.py on top (with tests/epipolar_restatement.py for the fundamental matrix)."""
import numpy as np

import match_restatement as mr

JACOBI_SWEEPS = mr.JACOBI_SWEEPS
POSE_TILE = 32
MAX_MATCHES, MAX_POSES = 1 << 20, 1 << 20
MAX_DEPTH, DEPTH_MIN, DEPTH_BASELINES, MIN_PARALLAX_DEG, MAX_REPROJ = 50.0, 0.01, 200.0, 1.0, 4.0
INF = float("inf")


# ---- the decomposition (scalar Python floats) -----------------------------------------------------------------------------
def div(a, b):
    """a / b in IEEE arithmetic (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def root(a):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(a)))


def jacobi3(G):
    """JACOBI3: (w [3], V [3][3]) of the symmetric G [3][3] (lists of floats)."""
    G = [[float(x) for x in row] for row in G]
    V = [[1.0 if r == c else 0.0 for c in range(3)] for r in range(3)]
    for _ in range(JACOBI_SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            g = G[p][q]
            if g == 0.0:
                continue
            theta = div(G[q][q] - G[p][p], 2.0 * g)
            if abs(theta) > 1e150:
                t = div(0.5, theta)
            else:
                t = div(-1.0 if theta < 0.0 else 1.0, abs(theta) + root(theta * theta + 1.0))
            c = div(1.0, root(t * t + 1.0))
            s = t * c
            G[p][p] = G[p][p] - t * g
            G[q][q] = G[q][q] + t * g
            G[p][q] = G[q][p] = 0.0
            for r in range(3):
                if r in (p, q):
                    continue
                x, y = G[r][p], G[r][q]
                G[r][p] = G[p][r] = c * x - s * y
                G[r][q] = G[q][r] = s * x + c * y
            for r in range(3):
                x, y = V[r][p], V[r][q]
                V[r][p] = c * x - s * y
                V[r][q] = s * x + c * y
    return [G[0][0], G[1][1], G[2][2]], V


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def essential(F, K):
    F = [[float(x) for x in row] for row in np.asarray(F, np.float64).reshape(3, 3)]
    Kf = np.asarray(K, np.float64).reshape(9)
    fx, fy, cx, cy = float(Kf[0]), float(Kf[4]), float(Kf[2]), float(Kf[5])
    T = [[F[r][0] * fx, F[r][1] * fy, (F[r][0] * cx + F[r][1] * cy) + F[r][2]] for r in range(3)]
    return [[fx * T[0][c] for c in range(3)], [fy * T[1][c] for c in range(3)],
            [(cx * T[0][c] + cy * T[1][c]) + T[2][c] for c in range(3)]]


def decompose(F, K):
    """(ok, R (2, 9), t (3,), w (3,)): amvs_twoview_decompose."""
    E = essential(F, K)
    G = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i, 3):
            G[i][j] = G[j][i] = (E[0][i] * E[0][j] + E[1][i] * E[1][j]) + E[2][i] * E[2][j]
    w, V = jacobi3(G)
    k3 = 0
    if w[1] < w[k3]:
        k3 = 1
    if w[2] < w[k3]:
        k3 = 2
    a, b = [k for k in range(3) if k != k3]
    k1, k2 = (b, a) if w[b] > w[a] else (a, b)
    if not (w[k2] > 0.0 and w[k2] < INF):
        return False, np.zeros((2, 9)), np.zeros(3), np.zeros(3)
    v1, v2 = [V[r][k1] for r in range(3)], [V[r][k2] for r in range(3)]
    v3 = cross(v1, v2)
    s1, s2 = root(w[k1]), root(w[k2])
    u1 = [div((E[r][0] * v1[0] + E[r][1] * v1[1]) + E[r][2] * v1[2], s1) for r in range(3)]
    u2 = [div((E[r][0] * v2[0] + E[r][1] * v2[1]) + E[r][2] * v2[2], s2) for r in range(3)]
    u3 = cross(u1, u2)
    Ra = [(u2[r] * v1[c] - u1[r] * v2[c]) + u3[r] * v3[c] for r in range(3) for c in range(3)]
    Rb = [(u1[r] * v2[c] - u2[r] * v1[c]) + u3[r] * v3[c] for r in range(3) for c in range(3)]
    return True, np.array([Ra, Rb]), np.array(u3), np.array([w[k1], w[k2], w[k3]])


def candidates(R2, t):
    """(R (4, 9), t (4, 3)) in the header's order: (Ra, t) (Rb, t) (Ra, -t) (Rb, -t)."""
    R2, t = np.asarray(R2, np.float64).reshape(2, 9), np.asarray(t, np.float64).reshape(3)
    return np.stack([R2[0], R2[1], R2[0], R2[1]]), np.stack([t, t, -t, -t])


# ---- the cheirality test -------------------------------------------------------------------------------------------------
def normalised(pts, K):
    Kf = np.asarray(K, np.float64).reshape(9)
    p = np.asarray(pts, np.float32).reshape(-1, 2).astype(np.float64)
    return np.stack([(p[:, 0] - Kf[2]) / Kf[0], (p[:, 1] - Kf[5]) / Kf[4]], axis=1)


def depths(R, t, pts1, pts2, K):
    """(z1, z2) (m,) of the matches under one pose."""
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    n1, n2 = normalised(pts1, K), normalised(pts2, K)
    P1 = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
    P2 = np.concatenate([R, t[:, None]], axis=1)
    with np.errstate(all="ignore"):
        _, M = mr.normal_matrix(P1, P2, n1, n2)
        v = mr.jacobi_smallest(M)
        Q = [v[:, i] / v[:, 3] for i in range(3)]
        return Q[2], ((R[2, 0] * Q[0] + R[2, 1] * Q[1]) + R[2, 2] * Q[2]) + t[2]


def front(R, t, pts1, pts2, K, max_depth=MAX_DEPTH):
    """(m,) bool: amvs_twoview_front."""
    z1, z2 = depths(R, t, pts1, pts2, K)
    with np.errstate(all="ignore"):
        return (z1 > 0.0) & (z1 < max_depth) & (z2 > 0.0) & (z2 < max_depth)


def front_matrix(R, t, pts1, pts2, K, max_depth=MAX_DEPTH):
    """(n, m) bool of the poses R (n, 9), t (n, 3)."""
    R, t = np.asarray(R, np.float64).reshape(-1, 9), np.asarray(t, np.float64).reshape(-1, 3)
    return np.stack([front(R[j], t[j], pts1, pts2, K, max_depth) for j in range(len(R))])


def score(R, t, pts1, pts2, K, max_depth=MAX_DEPTH):
    return front_matrix(R, t, pts1, pts2, K, max_depth).sum(axis=1).astype(np.int32)


def pose(F, K, pts1, pts2, max_depth=MAX_DEPTH):
    """(R (9,), t (3,), mask (m,) bool, n_front, info (5,) int32): amvs_twoview_pose; all zero without a model."""
    m = len(pts1)
    none = (np.zeros(9), np.zeros(3), np.zeros(m, bool), 0, np.zeros(5, np.int32))
    ok, R2, t, _ = decompose(F, K)
    if not ok:
        return none
    Rc, tc = candidates(R2, t)
    counts = score(Rc, tc, pts1, pts2, K, max_depth)
    best = 0
    for j in range(1, 4):
        if counts[j] > counts[best]:
            best = j
    if counts[best] == 0:
        return none
    mask = front(Rc[best], tc[best], pts1, pts2, K, max_depth)
    return Rc[best], tc[best], mask, int(mask.sum()), np.array([best, *counts], np.int32)


# ---- triangulation ---------------------------------------------------------------------------------------------------------
def triangulate(K, R1, t1, R2, t2, pts1, pts2, depth_min=DEPTH_MIN, depth_max=None, cos_max_parallax=None, max_reproj=MAX_REPROJ,
                with_margin=False):
    """(X (m, 3), valid (m,) bool, cos (m,)): amvs_twoview_triangulate.  depth_max defaults to 200 baselines and
    cos_max_parallax to cos(1 degree), as the Python layer's.  with_margin: also, per candidate, the smallest relative
    distance of one of the seven compared quantities to its threshold (the parallax on 1 - cos)."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    Rs = [np.asarray(R, np.float64).reshape(3, 3) for R in (R1, R2)]
    ts = [np.asarray(t, np.float64).reshape(3) for t in (t1, t2)]
    pts = [np.asarray(p, np.float32).reshape(-1, 2) for p in (pts1, pts2)]
    if depth_max is None:
        depth_max = float(np.linalg.norm(Rs[1].T @ ts[1] - Rs[0].T @ ts[0])) * DEPTH_BASELINES
    if cos_max_parallax is None:
        cos_max_parallax = float(np.cos(np.deg2rad(MIN_PARALLAX_DEG)))
    m = len(pts[0])
    if m == 0:
        out = (np.empty((0, 3)), np.zeros(0, bool), np.empty(0))
        return out + (np.empty(0),) if with_margin else out
    (P1, C1), (P2, C2) = mr.projection(K, Rs[0], ts[0]), mr.projection(K, Rs[1], ts[1])
    sqrt = np.sqrt
    with np.errstate(all="ignore"):
        _, M = mr.normal_matrix(P1, P2, pts[0], pts[1])
        v = mr.jacobi_smallest(M)
        X = np.stack([v[:, i] / v[:, 3] for i in range(3)], 1)
        pc = [np.stack([((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r] for r in range(3)], 1)
              for R, t in zip(Rs, ts)]
        z1, z2 = pc[0][:, 2], pc[1][:, 2]
        w1, w2 = X - C1, X - C2
        dot = (w1[:, 0] * w2[:, 0] + w1[:, 1] * w2[:, 1]) + w1[:, 2] * w2[:, 2]
        n1 = sqrt((w1[:, 0] * w1[:, 0] + w1[:, 1] * w1[:, 1]) + w1[:, 2] * w1[:, 2])
        n2 = sqrt((w2[:, 0] * w2[:, 0] + w2[:, 1] * w2[:, 1]) + w2[:, 2] * w2[:, 2])
        cs = dot / (n1 * n2 + 1e-8)
        e = []
        for k in range(2):
            h = [(K[r, 0] * pc[k][:, 0] + K[r, 1] * pc[k][:, 1]) + K[r, 2] * pc[k][:, 2] for r in range(3)]
            du = h[0] / h[2] - pts[k][:, 0].astype(np.float64)
            dv = h[1] / h[2] - pts[k][:, 1].astype(np.float64)
            e.append(sqrt(du * du + dv * dv))
        valid = ((z1 > depth_min) & (z2 > depth_min) & (z1 <= depth_max) & (z2 <= depth_max) & (cs <= cos_max_parallax)
                 & (e[0] <= max_reproj) & (e[1] <= max_reproj))
        if not with_margin:
            return X, valid, cs
        margin = np.minimum.reduce([np.abs(z1 - depth_min) / abs(depth_min), np.abs(z2 - depth_min) / abs(depth_min),
                                    np.abs(z1 - depth_max) / abs(depth_max), np.abs(z2 - depth_max) / abs(depth_max),
                                    np.abs(cs - cos_max_parallax) / (1.0 - cos_max_parallax),
                                    np.abs(e[0] - max_reproj) / max_reproj, np.abs(e[1] - max_reproj) / max_reproj])
    return X, valid, cs, margin


# ---- the initial pair -------------------------------------------------------------------------------------------------------
def components(pairs):
    adj = {}
    for i, j in pairs:
        adj.setdefault(i, set()).add(j)
        adj.setdefault(j, set()).add(i)
    seen, out = set(), []
    for start in sorted(adj):
        if start in seen:
            continue
        comp, todo = set(), [start]
        while todo:
            node = todo.pop()
            if node not in comp:
                comp.add(node)
                todo.extend(adj[node] - comp)
        seen |= comp
        out.append(sorted(comp))
    return out


def find_best_initial_pair(K, pair_points, ransac, dropped=None):
    """The pipeline of core/geometry.py find_best_initial_pair with ransac(pts1, pts2, threshold, confidence) ->
    (F (9,) or None, mask (m,) bool) for the fundamental matrix; all candidates, best first (an empty list: None).
    dropped: a dict that receives pair -> (the gate that dropped it, the value it saw)."""
    dropped = {} if dropped is None else dropped
    comps = components(pair_points.keys())
    if not comps:
        return []
    largest = set(max(comps, key=len))
    found = []
    for (i, j), (p1, p2) in pair_points.items():
        p1, p2 = np.asarray(p1, np.float32).reshape(-1, 2), np.asarray(p2, np.float32).reshape(-1, 2)
        if i not in largest or j not in largest:
            dropped[(i, j)] = ("component", None)
            continue
        if len(p1) < 50:
            dropped[(i, j)] = ("matches", len(p1))
            continue
        F, mask = ransac(p1, p2, 1.0, 0.999)
        if F is None or mask.sum() < 50:
            dropped[(i, j)] = ("inliers", 0 if F is None else int(mask.sum()))
            continue
        in1, in2 = p1[mask], p2[mask]
        R, t, _, n_front, _ = pose(F, K, in1, in2, MAX_DEPTH)
        if n_front == 0:
            dropped[(i, j)] = ("pose", 0)
            continue
        sample = np.linspace(0, len(in1) - 1, min(50, len(in1)), dtype=int)
        _, valid, cs = triangulate(K, np.eye(3), np.zeros(3), R, t, in1[sample], in2[sample])
        if valid.sum() < 20:
            dropped[(i, j)] = ("valid", int(valid.sum()))
            continue
        parallax = float(np.median(np.degrees(np.arccos(np.clip(cs[valid], -1, 1)))))
        if parallax < 1.5 or parallax > 40:
            dropped[(i, j)] = ("parallax", parallax)
            continue
        ratio = int(valid.sum()) / len(sample)
        s = len(in1) * ratio
        if 3 < parallax < 20:
            s *= 1.5
        found.append({"pair": (i, j), "mask": mask, "R": R.reshape(3, 3), "t": t.reshape(3, 1), "parallax": parallax, "score": s,
                      "pts1": in1, "pts2": in2, "valid_ratio": ratio})
    return sorted(found, key=lambda c: -c["score"])             # sorted is stable: equal scores keep their order
