"""Inputs of the resection tests (CPU and GPU): planted scenes with outliers, degenerate samples, scattered sets aimed at
the edges of the 64-correspondence blocks, correspondences planted on the inlier threshold, at zero depth and behind the
camera.  Everything is seeded; nothing here reads the library."""
import math

import numpy as np

BLOCK = 64                               # include/amvs_resection.h AMVS_PNP_BLOCK
BATCH = 1024                             # AMVS_PNP_BATCH
WIDTH, HEIGHT, FOCAL = 1920.0, 1080.0, 1500.0
K = np.array([[FOCAL, 0.0, WIDTH / 2], [0.0, FOCAL, HEIGHT / 2], [0.0, 0.0, 1.0]])


def rodrigues(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = math.radians(deg)
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(th) * Kx + (1.0 - math.cos(th)) * (Kx @ Kx)


def true_pose():
    """(R, t) world-to-camera of every planted scene: 25 degrees about a skew axis, the world origin off the centre."""
    return rodrigues([0.3, 1.0, -0.2], 25.0), np.array([0.4, -0.3, 1.1])


def project(R, t, X):
    Xc = X @ R.T + t
    return Xc[:, :2] / Xc[:, 2:3] * np.array([K[0, 0], K[1, 1]]) + np.array([K[0, 2], K[1, 2]])


def scene(m, outlier_fraction=0.0, noise=0.5, seed=1234):
    """(pts3d (m, 3), pts2d (m, 2) float32, planted inlier (m,) bool): a cloud uniform in a 4-unit cube centred 6 units
    in front of the camera, given in world coordinates under true_pose(); Gaussian noise of `noise` px on every pixel
    coordinate; round(outlier_fraction * m) correspondences whose pixel is drawn uniformly in the image."""
    rng = np.random.default_rng(seed)
    R, t = true_pose()
    Xc = np.stack([rng.uniform(-2.0, 2.0, m), rng.uniform(-2.0, 2.0, m), rng.uniform(4.0, 8.0, m)], axis=1)
    X = ((Xc - t) @ R).astype(np.float32)                       # R^T (Xc - t)
    x = project(R, t, X.astype(np.float64)) + rng.normal(0.0, noise, (m, 2))
    n_out = int(round(outlier_fraction * m))
    inlier = np.ones(m, bool)
    out = rng.permutation(m)[:n_out]
    inlier[out] = False
    x[out] = np.stack([rng.uniform(0.0, WIDTH, n_out), rng.uniform(0.0, HEIGHT, n_out)], axis=1)
    return X, x.astype(np.float32), inlier


# the planted scenes of the issue: name -> (points, outlier fraction, noise)
FAMILY = {"300_30": (300, 0.30, 0.5), "2000_50": (2000, 0.50, 0.5), "40_25": (40, 0.25, 0.5), "12_clean": (12, 0.0, 0.0)}
MAX_HYPOTHESES = (1, 1024, 1025, 4096)


def family_scene(name):
    m, frac, noise = FAMILY[name]
    return scene(m, frac, noise, seed=1234 + m)


def uniform_correspondences(m, seed):
    """m correspondences without any geometry."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (m, 3)) + np.array([0.0, 0.0, 6.0])
    x = rng.uniform(0.0, 1.0, (m, 2)) * np.array([WIDTH, HEIGHT])
    return X.astype(np.float32), x.astype(np.float32)


def rotation_error_deg(R, R_true):
    c = (np.trace(np.asarray(R).reshape(3, 3) @ np.asarray(R_true).T) - 1.0) / 2.0
    return math.degrees(math.acos(min(1.0, max(-1.0, c))))


# ---- degenerate samples (m = 6 or 7: every hypothesis draws (nearly) all rows) ---------------------------------------------
def degenerate_cases():
    X, x, _ = scene(7, 0.0, seed=3)
    same = (np.repeat(X[:1], 6, axis=0), np.repeat(x[:1], 6, axis=0))
    s = np.linspace(0.0, 1.0, 6)[:, None]
    line3 = (np.array([-1.0, 0.5, 5.0]) + s * np.array([2.0, -1.0, 1.5])).astype(np.float32)
    line = (line3, project(*true_pose(), line3.astype(np.float64)).astype(np.float32))
    rng = np.random.default_rng(11)
    plane3 = np.concatenate([rng.uniform(-1.5, 1.5, (7, 2)), np.zeros((7, 1))], axis=1).astype(np.float32)   # world z = 0
    plane = (plane3, project(*true_pose(), plane3.astype(np.float64) + np.array([0.0, 0.0, 5.0])).astype(np.float32))
    dup = (np.concatenate([X[:5], X[:1], X[5:6]]), np.concatenate([x[:5], x[:1], x[5:6]]))
    return {"identical": same, "collinear": line, "coplanar": plane, "repeated": dup}


# ---- sets for the refit ----------------------------------------------------------------------------------------------------
REFINE_SET_SIZES = (6, 63, 64, 65, 129, 4097)


def scattered_set(size, seed=0):
    """(pts3d, pts2d, mask): a noisy scene of m correspondences and a set of `size` members in which block 0 is empty,
    block 1 holds one member, block 2 is full when the size allows and the rest is scattered; m is no multiple of 64."""
    rng = np.random.default_rng(1000 + size + seed)
    n_blocks = max(8, 2 * (-(-size // BLOCK)) + 3)
    m = n_blocks * BLOCK - 17
    X, x, _ = scene(m, 0.0, seed=size)
    mask = np.zeros(m, np.uint8)
    mask[BLOCK + int(rng.integers(0, BLOCK))] = 1
    left = size - 1
    if left >= BLOCK + 8:
        mask[2 * BLOCK:3 * BLOCK] = 1
        left -= BLOCK
    free = np.arange(3 * BLOCK, m)
    mask[rng.choice(free, left, replace=False)] = 1
    assert int(mask.sum()) == size and not mask[:BLOCK].any() and mask[BLOCK:2 * BLOCK].sum() == 1
    return X, x, mask


def start_pose(deg=2.0, shift=0.05):
    """A pose near true_pose(): turned by `deg` and moved by `shift`."""
    R, t = true_pose()
    return rodrigues([1.0, -0.5, 0.7], deg) @ R, t + shift * np.array([1.0, -1.0, 0.5])


# ---- correspondences around the threshold ------------------------------------------------------------------------------------
SCORE_M = (6, 63, 64, 65, 255, 256, 257, 4097)
SCORE_N = (1, 64, 65, 1025)


def threshold_case(m, threshold=2.0, seed=0):
    """(pts3d, pts2d, inside (m,) bool): noise-free correspondences whose pixel is moved off its projection under
    true_pose() by threshold * 0.99 for `inside` and threshold * 1.01 for the others, in a random direction."""
    rng = np.random.default_rng(4000 + m + seed)
    X, _, _ = scene(m, 0.0, noise=0.0, seed=m + 77)
    x = project(*true_pose(), X.astype(np.float64))
    inside = rng.random(m) < 0.5
    ang = rng.uniform(0.0, 2.0 * math.pi, m)
    off = threshold * np.where(inside, 0.99, 1.01)
    x = x + off[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    return X, x.astype(np.float32), inside


def on_threshold_case():
    """(pts3d, pts2d, R, t, K, thr, expected (m,) bool) with ee == thr^2 z^2 EXACTLY in float64: the identity rotation,
    t = 0, fx = fy = 1024, cx = cy = 512 and points with small integer coordinates, so every product below is exact.
    A point (X, Y, Z) projects to 1024 X / Z + 512; the pixel is that moved by exactly 3 or 5 (a 3-4-5 triangle for the
    diagonal ones) and thr = 5: on the threshold (inlier), one pixel step inside, one outside; then the same points at
    z == 0 and behind the camera, which are never inliers."""
    Kt = np.array([[1024.0, 0.0, 512.0], [0.0, 1024.0, 512.0], [0.0, 0.0, 1.0]])
    rows = []
    for Z in (1.0, 2.0, 4.0):
        for X, Y in ((0.0, 0.0), (0.25, -0.125), (-0.5, 0.25)):
            u0, v0 = 1024.0 * X / Z + 512.0, 1024.0 * Y / Z + 512.0
            for du, dv, inl in ((5.0, 0.0, True), (0.0, -5.0, True), (3.0, 4.0, True), (-4.0, 3.0, True),
                                (4.0, 0.0, True), (6.0, 0.0, False), (4.0, 4.0, False), (3.0, 3.0, True)):
                rows.append((X, Y, Z, u0 + du, v0 + dv, inl))
    front = list(rows)
    for X, Y, Z, u, v, _ in front[:8]:
        rows.append((X, Y, 0.0, u, v, False))
        rows.append((X, Y, -Z, u, v, False))
        rows.append((-X, -Y, -Z, u, v, False))          # projects to the same pixel from behind
    a = np.array(rows, np.float64)
    assert np.array_equal(a[:, :5], a[:, :5].astype(np.float32).astype(np.float64))
    return a[:, :3].astype(np.float32), a[:, 3:5].astype(np.float32), np.eye(3), np.zeros(3), Kt, 5.0, a[:, 5] != 0


def special_poses():
    """(R (3, 9), t (3, 3)) that must count no inlier: all zero, one entry NaN, one entry infinite."""
    R0, t0 = true_pose()
    R, t = np.stack([R0.reshape(9)] * 3), np.stack([t0] * 3)
    R[0], t[0] = 0.0, 0.0
    R[1, 4] = np.nan
    t[2, 2] = np.inf
    return R, t
