"""Inputs of the epipolar tests (CPU and GPU): the standard two-view scene with planted outliers, degenerate samples,
scattered inlier sets aimed at the edges of the 64-match blocks, and matches planted on either side of the inlier
threshold.  Everything is seeded; nothing here reads the library."""
import math

import numpy as np

BLOCK = 64                               # include/amvs_epipolar.h AMVS_FMAT_BLOCK
BATCH = 1024                             # AMVS_FMAT_BATCH
WIDTH, HEIGHT, FOCAL = 4000.0, 3000.0, 3000.0
K = np.array([[FOCAL, 0.0, WIDTH / 2], [0.0, FOCAL, HEIGHT / 2], [0.0, 0.0, 1.0]])


def second_view(baseline_deg=10.0, radius=6.0):
    """(R, t) of a camera turned by `baseline_deg` about the point (0, 0, radius) the first one looks at."""
    b = math.radians(baseline_deg)
    R = np.array([[math.cos(b), 0.0, -math.sin(b)], [0.0, 1.0, 0.0], [math.sin(b), 0.0, math.cos(b)]])
    C = np.array([radius * math.sin(b), 0.0, radius - radius * math.cos(b)])
    return R, -R @ C


def project(R, t, X):
    x = (K @ (R @ X.T + t[:, None])).T
    return x[:, :2] / x[:, 2:3]


def scene(m, outlier_fraction=0.0, noise=0.5, seed=1234, baseline_deg=10.0):
    """(pts1, pts2 (m, 2) float32, planted inlier (m,) bool): points at depth 4-8 seen by two views 10 degrees apart,
    Gaussian noise of `noise` px on every coordinate, and round(outlier_fraction * m) matches whose second point is
    drawn uniformly in the image."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1.5, 1.5, m), rng.uniform(-1.0, 1.0, m), rng.uniform(4.0, 8.0, m)], axis=1)
    R2, t2 = second_view(baseline_deg)
    p1 = project(np.eye(3), np.zeros(3), X) + rng.normal(0.0, noise, (m, 2))
    p2 = project(R2, t2, X) + rng.normal(0.0, noise, (m, 2))
    n_out = int(round(outlier_fraction * m))
    inlier = np.ones(m, bool)
    out = rng.permutation(m)[:n_out]
    inlier[out] = False
    p2[out] = np.stack([rng.uniform(0.0, WIDTH, n_out), rng.uniform(0.0, HEIGHT, n_out)], axis=1)
    return p1.astype(np.float32), p2.astype(np.float32), inlier


def true_F(baseline_deg=10.0):
    """The fundamental matrix of the noise-free scene, unit Frobenius norm."""
    R, t = second_view(baseline_deg)
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    return F / np.linalg.norm(F)


def uniform_matches(m, seed):
    """m matches without any geometry: both points uniform in the image."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.0, 1.0, (2, m, 2)) * np.array([WIDTH, HEIGHT])
    return p[0].astype(np.float32), p[1].astype(np.float32)


# the RANSAC scenes of the GPU comparison: name -> (pts1, pts2, threshold); the first two are the CPU suite's table
def ransac_scenes():
    out = {"300_30": scene(300, 0.30)[:2] + (2.0,), "2000_50": scene(2000, 0.50)[:2] + (2.0,),
           "8_clean": scene(8, 0.0, noise=0.0, seed=8)[:2] + (2.0,), "20_12out": scene(20, 12 / 20, seed=20)[:2] + (2.0,),
           "no_model": uniform_matches(30, 30) + (0.01,)}
    p1, p2 = uniform_matches(30, 31)
    out["no_model_identical"] = (np.repeat(p1[:1], 30, axis=0), np.repeat(p2[:1], 30, axis=0), 0.01)
    return out


MAX_HYPOTHESES = (1, 1024, 1025, 4096)


# ---- degenerate samples (m = 8 or 9: every hypothesis draws (nearly) all rows) ---------------------------------------------
def degenerate_cases():
    p1, p2, _ = scene(9, 0.0, seed=3)
    same = (np.repeat(p1[:1], 8, axis=0), np.repeat(p2[:1], 8, axis=0))
    s = np.linspace(0.0, 1.0, 8, dtype=np.float64)[:, None]
    line = ((np.array([100.0, 200.0]) + s * np.array([3000.0, 1500.0])).astype(np.float32),
            (np.array([3500.0, 100.0]) + s * s * np.array([-2500.0, 2500.0])).astype(np.float32))
    dup = (np.concatenate([p1[:4], p1[:4], p1[4:5]]), np.concatenate([p2[:4], p2[:4], p2[4:5]]))
    return {"identical": same, "collinear": line, "duplicated": dup}


# ---- inlier sets for the refit ---------------------------------------------------------------------------------------------
FIT_SET_SIZES = (8, 63, 64, 65, 129, 4097)


def scattered_set(size, seed=0):
    """(pts1, pts2, mask): a clean scene of m matches and a set of `size` members in which block 0 is empty, block 1
    holds one member, block 2 is full when the size allows and the rest is scattered; m is no multiple of 64."""
    rng = np.random.default_rng(1000 + size + seed)
    n_blocks = max(8, 2 * (-(-size // BLOCK)) + 3)
    m = n_blocks * BLOCK - 17
    p1, p2, _ = scene(m, 0.0, seed=size)
    mask = np.zeros(m, np.uint8)
    mask[BLOCK + int(rng.integers(0, BLOCK))] = 1
    left = size - 1
    if left >= BLOCK + 8:
        mask[2 * BLOCK:3 * BLOCK] = 1
        left -= BLOCK
    free = np.arange(3 * BLOCK, m)
    mask[rng.choice(free, left, replace=False)] = 1
    assert int(mask.sum()) == size and not mask[:BLOCK].any() and mask[BLOCK:2 * BLOCK].sum() == 1
    return p1, p2, mask


# ---- matches on either side of the threshold ---------------------------------------------------------------------------------
SCORE_M = (8, 63, 64, 65, 255, 256, 257, 4097)
SCORE_N = (1, 64, 65, 1025)


def threshold_case(m, threshold=2.0, seed=0):
    """(pts1, pts2, inside (m,) bool): noise-free matches whose second point is moved off its epipolar line (under
    true_F) by threshold * (1 - 0.01) for `inside` and threshold * (1 + 0.01) for the others."""
    rng = np.random.default_rng(4000 + m + seed)
    p1, p2, _ = scene(m, 0.0, noise=0.0, seed=m + 77)
    F = true_F()
    x1 = np.concatenate([p1.astype(np.float64), np.ones((m, 1))], axis=1)
    l2 = x1 @ F.T
    nrm = l2[:, :2] / np.linalg.norm(l2[:, :2], axis=1, keepdims=True)
    inside = rng.random(m) < 0.5
    side = np.where(rng.random(m) < 0.5, -1.0, 1.0)
    off = threshold * np.where(inside, 0.99, 1.01) * side
    return p1, (p2.astype(np.float64) + nrm * off[:, None]).astype(np.float32), inside


def special_F():
    """Matrices that must count no inlier: zero, one entry infinite, one entry NaN."""
    F = np.stack([true_F().reshape(9)] * 3)
    F[0] = 0.0
    F[1, 4] = np.inf
    F[2, 8] = np.nan
    return F


# ---- FeatureMatcher end to end ---------------------------------------------------------------------------------------------
def matcher_case():
    """(keypoints1, keypoints2 (600, 2) float32, descriptors1, descriptors2 (600, 128) uint8): two sets of random
    descriptors that share 300 rows; the shared rows' keypoints are the standard scene with 20 % outliers, the others
    are uniform in the image."""
    rng = np.random.default_rng(9)
    d1 = rng.integers(0, 256, (600, 128), dtype=np.uint8)
    d2 = rng.integers(0, 256, (600, 128), dtype=np.uint8)
    rows1, rows2 = rng.permutation(600)[:300], rng.permutation(600)[:300]
    d2[rows2] = d1[rows1]
    s1, s2, _ = scene(300, 0.2, seed=99)
    k1, k2 = uniform_matches(600, 1)[0], uniform_matches(600, 2)[0]
    k1[rows1], k2[rows2] = s1, s2
    return k1, k2, d1, d2
