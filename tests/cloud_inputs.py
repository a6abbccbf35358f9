"""Inputs for the point-cloud tests (a helper module, not a conftest; seeded, no GPU): maps, colours, K_inv, poses and
thresholds aimed at the edges of csrc/amvs_fusion.hip and the resident-cloud path of csrc/amvs_knn.hip.  K_inv is an
argument of the entry points, so it is chosen freely: with K_inv = diag(s, s, 1), the identity pose and depth 1, pixel
(x, y) lands on (fl(x*s), fl(y*s), 1), which gives lattices and coordinates on voxel boundaries.

A MapCase is (name, depth (n, H, W) float32, conf (n, H, W) float32, bgr (n, H, W, 3) uint8, K_inv (3, 3) float64,
poses [(R, t)] float64, threshold): min_views for the fusion entry, min_confidence for the stereo entry.

    fusion_cases(H, W)   selected counts 0, 1, 2, 3, 4, 20, 21, 22, 41, 42 (where the percentile's virtual index is
                         integral, where its fraction crosses 0.5, both parities); two points placed symmetrically
                         (the cut removes both); the 7x7x7 lattice and the same lattice off the origin (ties with the
                         threshold); a skewed K_inv with a rotation about two axes per map; coordinates on voxel
                         boundaries on both sides of zero; voxels of 5 to 50 points in shuffled order
    stereo_cases(H, W)   confidence at, one ulp below and one ulp above the thresholds 2.5 and 0.35 (0.35 is not a
                         float32); depths 0, -0, -1 and the smallest positive normal; maps without a selected pixel in
                         first, middle and last position and everywhere; one pixel per map; the cross-axis key
                         collision; the voxel-boundary and shuffled-voxel clouds
    stride_case(kind)    3 maps of 720 x 1024 = 2 211 840 pixels (the launches are capped at 2 097 152 threads) with
                         about 2000 selected pixels: first and last of the stack, both sides of every map boundary and
                         of flat index 2 097 152; stride_cases(kind) adds 21, 1 and 0 selected pixels at that size
    big_cloud_case()     one 160 x 256 map, every pixel selected: 40 960 points fused, 38 912 after the filter, sample
                         stride 2 in the resident kNN
    take_cases(n), keep_masks(m), knn_cases(k)
"""
import collections
import functools

import numpy as np

F32 = np.float32
SIZES = ((2, 2), (3, 5), (17, 33))
COUNTS = (0, 1, 2, 3, 4, 20, 21, 22, 41, 42)
VOXEL_SIZES = (0.01, 0.02, 0.05, 1.0, 1e-3)
KNN_KS = (8, 10, 16, 20, 32)
STRIDE_SHAPE = (3, 720, 1024)
LAUNCH_CAP = 8192 * 256                     # threads of the largest launch (grid_for in amvs_fusion.hip)
BIG_SHAPE = (160, 256)
EYE = np.eye(3)

MapCase = collections.namedtuple("MapCase", "name depth conf bgr K_inv poses threshold")


def _rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def skew_K_inv():
    """Every entry of the first two rows non-zero and none a power of two."""
    return np.array([[0.0123, -0.0007, -0.31], [0.0009, 0.0119, -0.17], [0.0, 0.0, 1.0]])


def skew_poses(n):
    return [(_rot(0, 0.3 + 0.11 * j) @ _rot(1, -0.2 + 0.07 * j), np.array([0.3 * j - 0.4, 0.1 + 0.05 * j, -0.2 * j]))
            for j in range(n)]


def _colors(rng, n, H, W):
    return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def _case(name, depth, conf, seed, K_inv, poses, threshold):
    depth, conf = np.ascontiguousarray(depth, F32), np.ascontiguousarray(conf, F32)
    n, H, W = depth.shape
    assert conf.shape == depth.shape and len(poses) == n
    assert np.isfinite(depth).all() and np.isfinite(conf).all()
    bgr = _colors(np.random.default_rng(9000 + seed), n, H, W)
    return MapCase(name, depth, conf, bgr, np.asarray(K_inv, np.float64), list(poses), threshold)


def _scattered(rng, n, H, W, m, lo, hi):
    """conf with exactly m pixels at hi (seeded positions), the others at lo."""
    conf = np.full(n * H * W, lo, F32)
    conf[rng.permutation(n * H * W)[:m]] = hi
    return conf.reshape(n, H, W)


def _count_case(kind, H, W, n, m, seed):
    """m selected pixels of n maps under the skewed camera; the unselected ones sit just below the threshold."""
    rng = np.random.default_rng(seed)
    thr = 3.0 if kind == "fuse" else 2.5
    below = np.nextafter(F32(thr), F32(0))
    conf = _scattered(rng, n, H, W, m, below, thr)          # (exactly at the threshold: selected)
    depth = rng.uniform(2.0, 6.0, (n, H, W)).astype(F32)
    return _case(f"{kind} {H}x{W}x{n} m={m}", depth, conf, seed, skew_K_inv(), skew_poses(n), thr)


def _lattice(H, W, shift, seed):
    """7 maps, pixels (0..6, 0..6) selected, depth 1, K_inv = I, pose j = (I, shift - (0, 0, j)): the points
    (x, y, 1 + j) - shift, an integer lattice whose distances to the median tie exactly."""
    conf = np.zeros((7, H, W), F32)
    conf[:, :7, :7] = 4.0
    depth = np.ones((7, H, W), F32)
    poses = [(EYE, np.asarray(shift, np.float64) - np.array([0.0, 0.0, float(j)])) for j in range(7)]
    return _case(f"lattice shift {tuple(shift)}", depth, conf, seed, EYE, poses, 3.0)


def _boundary(kind, H, W, seed):
    """K_inv = diag(0.001, 0.001, 1), depths 10 * (1 .. 300): x = fl(fl(px * 0.001) * d), a double next to a multiple
    of 0.01 whose quotient by 0.01 and product with 100 fall on either side of an integer for some; map 1 is turned
    by pi about z and map 2 by pi about y (exact sign changes), so the coordinates lie on both sides of zero."""
    rng = np.random.default_rng(seed)
    n = 3
    depth = (10.0 * rng.integers(1, 301, (n, H, W))).astype(F32)
    conf = np.full((n, H, W), 4.0, F32)
    poses = [(EYE, np.zeros(3)), (np.diag([-1.0, -1.0, 1.0]), np.zeros(3)), (np.diag([-1.0, 1.0, -1.0]), np.zeros(3))]
    return _case(f"{kind} voxel boundaries {H}x{W}", depth, conf, seed, np.diag([0.001, 0.001, 1.0]), poses,
                 3.0 if kind == "fuse" else 2.5)


def _shuffled_voxels(kind, H, W, seed):
    """1 cm voxels of 5 to 50 points each, met in shuffled order: K_inv = diag(1e-7, 1e-7, 1), so a pixel's x and y
    stay inside the first voxel of every size used and its depth picks the voxel along z; a per-pixel offset inside the
    voxel and the random colours tell the points of a voxel apart."""
    rng = np.random.default_rng(seed)
    n, sizes = 2, []
    while sum(sizes) + 50 <= n * H * W:
        sizes.append(int(rng.integers(5, 51)))
    vox = np.repeat(np.arange(len(sizes)) + 200, sizes)
    rng.shuffle(vox)
    m = len(vox)
    depth = np.ones(n * H * W, F32)
    depth[:m] = ((vox + rng.uniform(0.2, 0.8, m)) * 0.01).astype(F32)
    conf = np.zeros(n * H * W, F32)
    conf[:m] = 4.0
    return _case(f"{kind} shuffled voxels {H}x{W}", depth.reshape(n, H, W), conf.reshape(n, H, W), seed,
                 np.diag([1e-7, 1e-7, 1.0]), [(EYE, np.zeros(3))] * n, 3.0 if kind == "fuse" else 2.5)


def _symmetric_pair(H, W, seed):
    """Two points, (0, 0, 1) and (0.5, 0.25 * (H - 1), 1): the median is their midpoint, both distances are equal,
    and the strict cut removes both."""
    conf = np.zeros((1, H, W), F32)
    conf[0, 0, 0] = conf[0, H - 1, 1] = 3.0
    return _case(f"fuse symmetric pair {H}x{W}", np.ones((1, H, W), F32), conf, seed, np.diag([0.5, 0.25, 1.0]),
                 [(EYE, np.zeros(3))], 3.0)


@functools.lru_cache(maxsize=None)
def fusion_cases(H, W):
    hw = H * W
    out = [_symmetric_pair(H, W, 11)]
    for n in sorted({1, min(4, max(1, -(-42 // hw)))} | ({2} if hw == 4 else set())):
        out += [_count_case("fuse", H, W, n, m, 100 * n + m) for m in COUNTS if m <= n * hw]
    if H >= 7 and W >= 7:
        out += [_lattice(H, W, (0.0, 0.0, 0.0), 21), _lattice(H, W, (10.5, -3.25, 1.0), 22)]
        rng = np.random.default_rng(23)
        out.append(_case(f"fuse skewed {H}x{W}", rng.uniform(2.0, 6.0, (3, H, W)), rng.integers(0, 5, (3, H, W)), 23,
                         skew_K_inv(), skew_poses(3), 3.0))
        out += [_boundary("fuse", H, W, 24), _shuffled_voxels("fuse", H, W, 25)]
    return tuple(out)


def _collision(H, W, seed):
    """Voxel 1.0: map 0's pixel lands on (0.5, 1.5, -0.5), key 0*10^9 + 1*10^6 - 1, map 1's on (0.5, 0.5, 999999.5),
    key 999 999 as well; map 2's on (0.5, 0.5, 0.5).  One selected pixel per map."""
    conf = np.zeros((3, H, W), F32)
    conf[0, 0, 0] = conf[1, H - 1, W - 1] = conf[2, 0, W - 1] = 3.0
    K_inv = np.array([[0.0, 0.0, 0.5]] * 3)
    poses = [(EYE, np.array([0.0, -1.0, 1.0])), (EYE, np.array([0.0, 0.0, -999999.0])), (EYE, np.zeros(3))]
    return _case(f"stereo key collision {H}x{W}", np.ones((3, H, W), F32), conf, seed, K_inv, poses, 2.5)


def _threshold_case(H, W, thr, seed):
    """Confidences at float32(thr) and one ulp to either side, cycling over the pixels; depth positive."""
    t = F32(thr)
    vals = np.array([t, np.nextafter(t, F32(0)), np.nextafter(t, F32(10)), t - F32(1), t + F32(1)], F32)
    rng = np.random.default_rng(seed)
    conf = vals[np.arange(2 * H * W) % 5].reshape(2, H, W)
    return _case(f"stereo threshold {thr} {H}x{W}", rng.uniform(2.0, 6.0, (2, H, W)), conf, seed, skew_K_inv(),
                 skew_poses(2), thr)


def _depth_sign_case(H, W, seed):
    """Every pixel confident; depths cycle over 0, -0, -1, the smallest positive normal and 1.5."""
    vals = np.array([0.0, -0.0, -1.0, np.finfo(F32).tiny, 1.5], F32)
    depth = vals[np.arange(2 * H * W) % 5].reshape(2, H, W)
    return _case(f"stereo depth signs {H}x{W}", depth, np.full((2, H, W), 4.0, F32), seed, skew_K_inv(), skew_poses(2), 2.5)


def _empty_maps_case(H, W, empty, seed):
    """4 maps; those listed in `empty` have no selected pixel (confident pixels with depth 0 among them)."""
    rng = np.random.default_rng(seed)
    conf = rng.integers(1, 5, (4, H, W)).astype(F32)
    depth = rng.uniform(2.0, 6.0, (4, H, W)).astype(F32)
    for j in range(4):
        if j in empty:
            depth[j][conf[j] >= 2.5] = 0.0
        else:
            conf[j, H - 1, W - 1] = 4.0                   # at least one selected pixel
    return _case(f"stereo maps {sorted(empty)} empty {H}x{W}", depth, conf, seed, skew_K_inv(), skew_poses(4), 2.5)


@functools.lru_cache(maxsize=None)
def stereo_cases(H, W):
    out = [_threshold_case(H, W, 2.5, 31), _threshold_case(H, W, 0.35, 32), _depth_sign_case(H, W, 33),
           _empty_maps_case(H, W, {0}, 34), _empty_maps_case(H, W, {1, 2}, 35), _empty_maps_case(H, W, {3}, 36),
           _empty_maps_case(H, W, {0, 1, 2, 3}, 37), _collision(H, W, 38)]
    out += [_count_case("stereo", H, W, 3, m, 300 + m) for m in (1, 2, 3) if m <= 3 * H * W]
    if H >= 7 and W >= 7:
        out += [_boundary("stereo", H, W, 39), _shuffled_voxels("stereo", H, W, 40)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def stride_case(kind, count=2000):
    """The 3 x 720 x 1024 stack with `count` seeded pixels selected plus, for the full case, the pixels at its edges;
    the small counts are subsets of the full selection that keep a pixel beyond the launch cap."""
    n, H, W = STRIDE_SHAPE
    hw, total = H * W, n * H * W
    rng = np.random.default_rng(51)
    must = [LAUNCH_CAP, total - 1, 0, LAUNCH_CAP - 1]
    for j in range(1, n):
        must += [j * hw - 1, j * hw]
    scattered = rng.choice(total, 2000, replace=False)
    sel = np.union1d(scattered, must) if count >= 2000 else np.array((must + list(scattered))[:count], np.int64)
    thr = 3.0 if kind == "fuse" else 2.5
    conf = np.full(total, np.nextafter(F32(thr), F32(0)), F32)
    conf[sel] = thr
    depth = np.ones(total, F32)
    depth[sel] = rng.uniform(2.0, 6.0, len(sel)).astype(F32)
    K_inv = skew_K_inv() * np.array([[0.02], [0.02], [1.0]])        # (keeps a 1024-pixel row within a few units)
    return _case(f"{kind} stride {n}x{H}x{W} m={len(sel)}", depth.reshape(n, H, W), conf.reshape(n, H, W), 51, K_inv,
                 skew_poses(n), thr)


def stride_cases(kind):
    return tuple(stride_case(kind, m) for m in (2000, 21, 1, 0))


@functools.lru_cache(maxsize=None)
def big_cloud_case():
    """A wavy sheet seen by one 160 x 256 map, every pixel selected."""
    H, W = BIG_SHAPE
    rng = np.random.default_rng(61)
    y, x = np.mgrid[0:H, 0:W]
    depth = 4.0 + 0.3 * np.sin(0.05 * x) * np.cos(0.07 * y) + rng.normal(0, 0.003, (H, W))
    return _case(f"sheet {H}x{W}", depth[None], np.full((1, H, W), 4.0, F32), 61, skew_K_inv(), skew_poses(1), 2.5)


def take_cases(n):
    """(name, indices) on a cloud of n >= 1 points."""
    return (("reversed", np.arange(n - 1, -1, -1)), ("every index twice", np.repeat(np.arange(n), 2)),
            ("the last index", np.array([n - 1])), ("no index", np.zeros(0, np.int64)), ("seven times the first", np.zeros(7, np.int64)))


def keep_masks(m):
    one = np.zeros(m, bool)
    one[m // 2:m // 2 + 1] = True
    return (("all zero", np.zeros(m, bool)), ("all one", np.ones(m, bool)), ("a single one", one),
            ("alternating", np.arange(m) % 2 == 0))


@functools.lru_cache(maxsize=None)
def knn_cases(k):
    """(name, points) for one compiled neighbour count."""
    rng = np.random.default_rng(700 + k)
    out = [(f"n={n}", rng.normal(size=(n, 3))) for n in (k, k + 1, 2 * k + 1, 2 * k + 2, 300)]
    out.append(("identical points", np.tile(rng.normal(size=(1, 3)), (2 * k + 2, 1))))
    dup = rng.normal(size=(300, 3))
    dup[rng.permutation(300)[:2 * k]] = dup[0]
    out.append(("2k coincident points", dup))
    out.append(("offset by 1e6", rng.normal(size=(300, 3)) + [0.0, 1e6, 0.0]))
    return tuple((f"k={k} {name}", np.ascontiguousarray(p)) for name, p in out)
