"""Inputs of the two-view tests (CPU and GPU): a planted pair of views with exact and noisy matches, outliers, the pose
lists of the scoring tests, matches planted either side of the depth limit and at infinity, triangulation candidates
planted either side of every threshold, and the three pairs of the initial-pair test.  Everything is seeded NumPy on
the conventions of tests/resection_inputs.py; nothing here reads the library or the restatement."""
import math

import numpy as np

import resection_inputs as ri

K = ri.K                                  # 1920 x 1080, f = 1500
WIDTH, HEIGHT, FOCAL = ri.WIDTH, ri.HEIGHT, ri.FOCAL
POSE_TILE = 32                            # include/amvs_twoview.h AMVS_TWOVIEW_POSE_TILE
SCORE_M = (1, 8, 63, 64, 65, 1000)
SCORE_N = (1, 4, 33, 65)
TRI_M = (0, 1, 63, 64, 65, 1000)
DEPTH_LIMIT = 10.0                        # the max_depth of the scoring cases, in baselines


def pose_with(axis, deg, centre):
    """(R, t) of a camera turned by `deg` about `axis` whose centre is `centre`."""
    R = ri.rodrigues(axis, deg)
    return R, -(R @ np.asarray(centre, np.float64))


def true_pose():
    """(R, t) of the second camera: 12 degrees about an axis near y, a unit baseline; the first camera is [I | 0]."""
    c = np.array([1.0, 0.05, 0.1])
    return pose_with([0.1, 1.0, 0.05], 12.0, c / np.linalg.norm(c))


def project(R, t, X):
    return ri.project(R, t, X)


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def fundamental(R, t):
    """The exact F of the pair ([I | 0], [R | t]): K^-T [t]x R K^-1, unit Frobenius norm."""
    Ki = np.linalg.inv(K)
    F = Ki.T @ skew(t) @ R @ Ki
    return F / np.linalg.norm(F)


def cloud(m, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-2.0, 2.0, m), rng.uniform(-2.0, 2.0, m), rng.uniform(4.0, 8.0, m)], axis=1)


def scene(m, noise=0.0, outlier_fraction=0.0, seed=1234, pose=None):
    """(X (m, 3), pts1, pts2 (m, 2) float32, planted inlier (m,) bool): a cloud uniform in a 4-unit cube 6 units in front of
    the first camera seen by both; Gaussian noise of `noise` px; round(outlier_fraction * m) matches whose second pixel is
    drawn uniformly in the image."""
    rng = np.random.default_rng(seed + 7)
    R, t = true_pose() if pose is None else pose
    X = cloud(m, seed)
    p1 = project(np.eye(3), np.zeros(3), X) + rng.normal(0.0, noise, (m, 2))
    p2 = project(R, t, X) + rng.normal(0.0, noise, (m, 2))
    n_out = int(round(outlier_fraction * m))
    inlier = np.ones(m, bool)
    out = rng.permutation(m)[:n_out]
    inlier[out] = False
    p2[out] = np.stack([rng.uniform(0.0, WIDTH, n_out), rng.uniform(0.0, HEIGHT, n_out)], axis=1)
    return X, p1.astype(np.float32), p2.astype(np.float32), inlier


# ---- F matrices for the decomposition ------------------------------------------------------------------------------------
def degenerate_fundamentals():
    """name -> F without a model: all zero, rank 1, one NaN entry; and one infinite entry (whatever the text gives)."""
    a, b = np.array([0.3, -0.2, 1.0]), np.array([-0.1, 0.4, 1.0])
    F = fundamental(*true_pose())
    nan, inf = F.copy(), F.copy()
    nan[1, 1] = np.nan
    inf[0, 2] = np.inf
    return {"zero": np.zeros((3, 3)), "rank1": np.outer(a, b) * 1e-6, "nan": nan, "inf": inf}


# ---- scoring ------------------------------------------------------------------------------------------------------------
def sideways_pose():
    """A pose under which the match ((cx, cy), (cx, cy)) is a point at infinity with v[3] == 0 exactly."""
    return np.eye(3), np.array([1.0, 0.0, 0.0])


def depth_limit_point(direction, factor, limit=DEPTH_LIMIT):
    """The point along `direction` (first camera's frame) whose larger depth in the two cameras is factor * limit."""
    R, t = true_pose()
    d = np.asarray(direction, np.float64)
    s1, s2 = factor * limit / d[2], (factor * limit - t[2]) / (R[2] @ d)
    return min(s1, s2) * d


def score_matches(m):
    """(pts1, pts2 (m, 2) float32, planted (m,) bool: in front under true_pose() and nearer than DEPTH_LIMIT).  From m = 8
    on, match 1 is the pair of principal points (in front under true_pose(), whose optical axes pass each other 4.7 units
    ahead; the point at infinity of sideways_pose()), matches 2 and 4 lie 1 % inside the limit and 3 and 5 1 % outside, 2
    and 3 with the larger depth in the first camera, 4 and 5 in the second."""
    X, p1, p2, _ = scene(m, seed=100 + m)
    planted = np.ones(m, bool)
    if m >= 8:
        R, t = true_pose()
        for i, (d, f) in enumerate((([0.25, -0.1, 1.0], 0.99), ([0.25, -0.1, 1.0], 1.01), ([-0.2, 0.1, 1.0], 0.99), ([-0.2, 0.1, 1.0], 1.01))):
            P = depth_limit_point(d, f)[None]
            p1[2 + i], p2[2 + i] = project(np.eye(3), np.zeros(3), P)[0], project(R, t, P)[0]
            planted[2 + i] = f < 1.0
            z1, z2 = P[0, 2], (R @ P[0] + t)[2]
            assert (z1 > z2) == (i < 2) and abs(max(z1, z2) - f * DEPTH_LIMIT) < 1e-9
        p1[1] = p2[1] = (K[0, 2], K[1, 2])                   # the two optical axes: under true_pose() they pass each other in front
        d2 = R[2]                                            # (the second axis in the first camera's frame), C2 its origin
        C2 = -(R.T @ t)
        a, b = np.linalg.solve(np.array([[1.0, -d2[2]], [d2[2], -1.0]]), np.array([C2[2], d2 @ C2]))
        assert 1.0 < a < DEPTH_LIMIT - 1.0 and 1.0 < b < DEPTH_LIMIT - 1.0 and np.linalg.norm(a * np.array([0, 0, 1.0]) - C2 - b * d2) < 0.2
    return p1, p2, planted


def score_poses(candidates_R, candidates_t, n=max(SCORE_N)):
    """(R (n, 9), t (n, 3)): 0 the true pose, 1 .. 3 the zero / NaN / infinite poses, 4 sideways_pose(), 5 .. 8 the four
    candidates handed in (the decomposition of the exact F), the rest the true pose with perturbed entries."""
    rng = np.random.default_rng(n)
    R0, t0 = true_pose()
    R = R0.reshape(1, 9) * (1.0 + 1e-3 * rng.standard_normal((n, 9)))
    t = t0[None] + 1e-2 * rng.standard_normal((n, 3))
    R[0], t[0] = R0.reshape(9), t0
    R[1:4], t[1:4] = R0.reshape(9), t0
    R[1], t[1] = 0.0, 0.0
    R[2, 4] = np.nan
    t[3, 2] = np.inf
    R[4], t[4] = sideways_pose()[0].reshape(9), sideways_pose()[1]
    R[5:9], t[5:9] = np.asarray(candidates_R).reshape(4, 9), np.asarray(candidates_t).reshape(4, 3)
    return R, t


# ---- triangulation candidates either side of every threshold -----------------------------------------------------------
COS_1_DEG = float(np.cos(np.deg2rad(1.0)))
FILTER_DEFAULTS = (0.01, 200.0, COS_1_DEG, 4.0)              # depth_min, depth_max (200 unit baselines), cosine, pixels
FILTER_NEAR = (0.01, 20.0, COS_1_DEG, 4.0)                   # a depth_max that the parallax floor does not shadow


def svd_point_and_errors(R, t, p1, p2):
    """(X, e1, e2) of one match by an SVD of A and plain NumPy: the yardstick the reprojection cases are planted with."""
    P1, P2 = K @ np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1), K @ np.concatenate([R, t[:, None]], axis=1)
    A = np.stack([p1[0] * P1[2] - P1[0], p1[1] * P1[2] - P1[1], p2[0] * P2[2] - P2[0], p2[1] * P2[2] - P2[1]])
    v = np.linalg.svd(A)[2][-1]
    X = v[:3] / v[3]
    e = [np.linalg.norm(project(Rk, tk, X[None])[0] - pk) for Rk, tk, pk in ((np.eye(3), np.zeros(3), p1), (R, t, p2))]
    return X, e[0], e[1]


def reprojection_case(X, view, factor, limit=4.0):
    """(p1, p2) float32 of the point X with its first pixel moved straight up (across the epipolar line) until the larger of
    the two reprojection errors, measured by svd_point_and_errors on the float32 pixels, is factor * limit.  The DLT
    leaves the larger error in the view the point is nearer to; that must be `view` (0 or 1), and the other error must
    stay 2 % under the limit, so that the case turns on the comparison of e_view alone."""
    R, t = true_pose()
    base = [project(np.eye(3), np.zeros(3), X[None])[0], project(R, t, X[None])[0]]

    def errors(delta):
        p = [b.copy() for b in base]
        p[0][1] += delta
        p = [q.astype(np.float32) for q in p]
        _, e1, e2 = svd_point_and_errors(R, t, p[0].astype(np.float64), p[1].astype(np.float64))
        return p, (e1, e2)

    lo, hi = 0.0, 40.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if max(errors(mid)[1]) < factor * limit:
            lo = mid
        else:
            hi = mid
    p, e = errors(hi)
    assert e[view] == max(e) and abs(max(e) - factor * limit) < 1e-3 * limit and e[1 - view] < 0.98 * limit, (view, factor, e)
    return p


def filter_case():
    """(pts1, pts2 (16, 2) float32, expected (16,) bool, thresholds per candidate as indices into (FILTER_DEFAULTS,
    FILTER_NEAR), names): for each of the seven comparisons of amvs_twoview_triangulate a candidate 1 % on the valid side
    and one 1 % on the other side, every other comparison passing clearly; then two plain scene points.  The two depth_max
    comparisons are planted for 20 baselines: at the reference's 200 the parallax floor of 1 degree (57 baselines) has
    dropped the point already."""
    R, t = true_pose()
    C2 = -(R.T @ t)
    rows, names = [], []

    def add(name, X, valid, near=False, pixels=None):
        p = pixels if pixels is not None else (project(np.eye(3), np.zeros(3), X[None])[0], project(R, t, X[None])[0])
        rows.append((np.asarray(p[0], np.float32), np.asarray(p[1], np.float32), valid, int(near)))
        names.append(name)

    for f in (1.01, 0.99):                                   # depth_min: valid above it
        add(f"z1 {f} depth_min", np.array([-4.0, 3.0, f * 0.01]), f > 1.0)
        add(f"z2 {f} depth_min", R.T @ (np.array([4.0, 3.0, f * 0.01]) - t), f > 1.0)
    for f in (0.99, 1.01):                                   # depth_max: valid at or below it
        add(f"z1 {f} depth_max", np.array([6.0, 1.0, f * 20.0]), f < 1.0, near=True)
        add(f"z2 {f} depth_max", R.T @ (np.array([-6.0, 1.0, f * 20.0]) - t), f < 1.0, near=True)
    up = np.cross(C2, [0.0, 1.0, 0.0])
    up = up / np.linalg.norm(up) * np.sign(up[2])            # across the baseline, towards the scene
    for f in (1.01, 0.99):                                   # parallax: valid at 1 degree or more
        d = 0.5 / math.tan(math.radians(f * 1.0) / 2.0)
        add(f"parallax {f} degree", 0.5 * C2 + d * up, f > 1.0)
    for view, X in ((0, np.array([-1.5, 0.3, 4.0])), (1, np.array([2.5, 0.3, 4.0]))):
        for f in (0.99, 1.01):                               # reprojection: valid at or below it
            add(f"e{view + 1} {f} max_reproj", X, f < 1.0, pixels=reprojection_case(X, view, f))
    for X in cloud(2, 5):
        add("plain", X, True)
    p1, p2 = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    return p1, p2, np.array([r[2] for r in rows]), np.array([r[3] for r in rows]), names


def triangulate_candidates(m):
    """(pts1, pts2 (m, 2) float32): noisy scene matches with 30 % outliers; from m = 63 on the first 16 are those of
    filter_case() (their expectations hold under FILTER_DEFAULTS / FILTER_NEAR as filter_case() says)."""
    _, p1, p2, _ = scene(m, noise=0.5, outlier_fraction=0.3, seed=300 + m)
    if m >= 63:
        f1, f2 = filter_case()[:2]
        p1[:16], p2[:16] = f1, f2
    return p1, p2


# ---- the initial pair ---------------------------------------------------------------------------------------------------
def initial_pairs():
    """pair -> (pts1, pts2): (0, 1) has a baseline so short that the median parallax stays under 1.5 degrees, (1, 2) has 40
    matches, (0, 2) is a pair at about 10 degrees of parallax, and (3, 4), good as well, is a component of its own that
    the restriction to the first largest component leaves out.  0.3 px of noise, 10 % outliers."""
    short = pose_with([0.1, 1.0, 0.05], 1.0, [0.13, 0.0, 0.0])
    out = {}
    for pair, m, pose, seed in (((0, 1), 300, short, 1), ((1, 2), 40, None, 2), ((0, 2), 300, None, 3), ((3, 4), 320, None, 4)):
        _, p1, p2, _ = scene(m, noise=0.3, outlier_fraction=0.1, seed=500 + seed, pose=pose)
        out[pair] = (p1, p2)
    return out
