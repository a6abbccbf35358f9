"""The input family of the depth-filter tests (a helper module, not a conftest; seeded, no GPU): the smallest shapes at
which csrc/amvs_depth_filter.hip can go wrong, one input per guard and exact edge of the definition in
include/amvs_depth.h, and a height-field scene of amvs.synthetic with its analytic depths, seeded noise and planted
outliers.

A Case holds stacked maps, the cameras, the neighbour rows and the parameters.  `edges` names the counters of
tests/depth_filter_restatement.py the input was built for: the CPU test holds each such input to reaching them on its own.
No input is larger than 5 maps of 48 x 64, except one of 2 x 260 x 256, which the NumPy twin alone restates: its 66 560
pixels a map exceed the 65 536 pixels one trip of the launch grid covers (at most 256 workgroups of 256 lanes along a map,
FILTER_MAX_BLOCKS_X in csrc/amvs_depth_filter.hip), so every lane of the first 1 024 pixels walks the grid-stride loop twice
and the second trip is ragged.
"""
import os
import sys
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32 = np.float32
INF32 = F32(np.inf)
NAN32 = F32(np.nan)
EYE = np.eye(3)
ZERO = np.zeros(3)
SCENE = (5, 48, 64)
NOISE_SIGMA = 0.002                    # relative, of the seeded noise on the scene's analytic depths
OUTLIER_FRACTION = 0.05


def up(x):
    return np.nextafter(F32(x), INF32)


@dataclass
class Case:
    name: str
    depth: np.ndarray                    # (n, H, W) float32
    conf: np.ndarray
    K: np.ndarray                        # (3, 3) float64
    poses: list                          # [(R, t)] float64
    neighbours: np.ndarray = None        # (n, n_nbr) int32 or None: every other map
    min_confidence: float = 1.0
    max_px: float = 1.0
    max_rel: float = 0.01
    min_consistent: int = 1
    edges: tuple = ()
    big: bool = False                    # restated by the NumPy twin only
    extra: dict = field(default_factory=dict)

    @property
    def shape(self):
        return self.depth.shape[1:]

    @property
    def K_inv(self):
        return np.linalg.inv(self.K)     # (as Engine.depth_filter and the classes compute it)

    @property
    def n_nbr(self):
        return len(self.poses) - 1 if self.neighbours is None else self.neighbours.shape[1]

    def args(self, refine=True, min_consistent=None):
        return (self.depth, self.conf, self.K, self.K_inv, self.poses, self.neighbours, self.min_confidence, self.max_px,
                self.max_rel, self.min_consistent if min_consistent is None else min_consistent, refine)


def pinhole(f, W, H):
    return np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])


def const_maps(values, H, W):
    d = np.stack([np.full((H, W), v, F32) for v in values])
    return d, np.ones_like(d)


def rot_y(deg):
    a = np.radians(deg)
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


# ------------------------------------------------------------------------------------------ the small inputs ---
def tiny_case():
    d, c = const_maps([2.0, 2.0], 2, 2)
    return Case("tiny_2x2", d, c, pinhole(2.0, 2, 2), [(EYE, ZERO)] * 2, edges=("consistent", "cnt_at_min"))


def single_map_case():
    """One map: no neighbours, every count 0, nothing kept."""
    rng = np.random.default_rng(21)
    d = rng.uniform(2.0, 3.0, (1, 4, 6)).astype(F32)
    return Case("single_map", d, np.ones_like(d), pinhole(4.0, 6, 4), [(EYE, ZERO)], edges=("cnt_just_below",))


def depth_tie_case():
    """Identical poses, focal length a power of two, integer principal point: forward and backward projection are exact,
    the reprojected pixel is the pixel itself and Y_2 is the neighbour's depth.  From map 0 (d = 1, max_rel = 0.25) map 1
    (1.25) is exactly on the bound and map 2 (the next float32 above 1.25) just outside it."""
    d, c = const_maps([1.0, 1.25, up(1.25)], 8, 12)
    return Case("depth_ties", d, c, pinhole(8.0, 12, 8), [(EYE, ZERO)] * 3, max_rel=0.25, edges=("depth_tie", "depth_fail", "consistent"))


def order_case():
    """Exact projections again, and depths whose float64 sum depends on the order at the very bit that decides the float32
    rounding of the mean: from map 0, ((1 + (1 + 2^-23)) + 2^-52) + 2^-52 = 2 + 2^-23 (each small term is half a unit in the
    last place and rounds to even), a quarter of which is a float32 tie and rounds to 0.5; last to first the sum is
    2 + 2^-23 + 2^-51 and the mean rounds up to 0.5 + 2^-24.  max_rel = 1 lets depths that small agree."""
    d, c = const_maps([1.0, 1.0 + 2.0 ** -23, 2.0 ** -52, 2.0 ** -52], 8, 12)
    return Case("order_matters", d, c, pinhole(8.0, 12, 8), [(EYE, ZERO)] * 4, max_rel=1.0, min_consistent=3, edges=("consistent",))


def e2_tie_case():
    """f = 64, t = (1, 0, 0), d = 32 against di = 64: the pixel lands 2 columns to the right and comes back 1 column off, so
    e2 == 1 == max_px^2 exactly, in both directions.  The third map is the first once more and agrees exactly."""
    d, c = const_maps([32.0, 64.0, 32.0], 8, 12)
    return Case("e2_tie", d, c, pinhole(64.0, 12, 8), [(EYE, ZERO), (EYE, np.array([1.0, 0.0, 0.0])), (EYE, ZERO)], max_px=1.0,
                max_rel=2.0, edges=("e2_tie", "outside_right", "outside_left", "consistent"))


def e2_fail_case():
    """The same geometry with max_px just below 1: what was a tie fails."""
    case = e2_tie_case()
    case.name, case.max_px, case.edges = "e2_fail", float(np.nextafter(F32(1.0), F32(0.0))), ("e2_fail",)
    return case


def shifted_case():
    """A fronto-parallel plane seen by five cameras shifted left, right, up and down: pixels leave every side of the
    neighbour's image; seeded noise of a few 1e-3 straddles max_rel."""
    rng = np.random.default_rng(22)
    H, W = 10, 14
    d = (4.0 * (1.0 + rng.normal(0.0, 0.006, (5, H, W)))).astype(F32)
    t = [ZERO, np.array([1.0, 0.0, 0.0]), np.array([-1.0, 0.0, 0.0]), np.array([0.0, 0.75, 0.0]), np.array([0.0, -0.75, 0.0])]
    return Case("shifted_views", d, np.ones_like(d), pinhole(16.0, W, H), [(EYE, v) for v in t], min_consistent=2,
                edges=("outside_left", "outside_right", "outside_top", "outside_bottom", "depth_fail", "consistent",
                       "cnt_just_below", "cnt_at_min"))


def special_values_case():
    """NaN, +-inf, negative and zero depths and confidences, in the centre's role and in the neighbour's."""
    rng = np.random.default_rng(23)
    H, W = 12, 16
    d = (3.0 * (1.0 + rng.normal(0.0, 0.002, (3, H, W)))).astype(F32)
    c = np.full_like(d, 2.0)
    bad_d = [NAN32, INF32, -INF32, F32(-3.0), F32(0.0), F32(-0.0), INF32, INF32]
    bad_c = [NAN32, -INF32, F32(0.0), F32(-1.0), F32(1.5), np.nextafter(F32(2.0), F32(0.0))]
    for j in range(3):
        for y in range(H):
            for x in range(W):
                slot = (x + 3 * y + 5 * j) % 19
                if slot < 8:
                    d[j, y, x] = bad_d[slot]
                elif slot < 14:
                    c[j, y, x] = bad_c[slot - 8]
                elif slot == 14:
                    c[j, y, x] = INF32                       # (a confidence of +inf is valid)
    poses = [(EYE, ZERO), (EYE, np.array([0.25, 0.0, 0.0])), (EYE, np.array([0.0, -0.25, 0.0]))]
    return Case("special_values", d, c, pinhole(8.0, W, H), poses, min_confidence=2.0, max_rel=0.02,
                edges=("centre_depth_nonpositive", "centre_depth_nonfinite", "centre_conf_low", "nbr_depth_nonpositive",
                       "nbr_depth_nonfinite", "nbr_conf_low"))


def behind_case():
    """Map 1's camera stands in front of the surface map 0 sees and looks the same way (the surface is behind it); map 2's
    camera looks away from it: Xi_2 <= 0 either way.  Map 3's camera faces camera 0 from beyond the surface and claims
    depths that reach behind camera 0: Y_2 <= 0."""
    H, W = 6, 8
    d, c = const_maps([4.0, 4.0, 4.0, 12.0], H, W)
    facing = rot_y(180.0)
    poses = [(EYE, ZERO), (EYE, np.array([0.0, 0.0, -6.0])), (facing, ZERO), (facing, -facing @ np.array([0.0, 0.0, 8.0]))]
    nbr = np.array([[1, 2, 3], [0, -1, -1], [0, -1, -1], [0, -1, -1]], np.int32)
    return Case("behind_and_away", d, c, pinhole(8.0, W, H), poses, neighbours=nbr, edges=("Xi_behind", "Y_behind"))


def odd_intrinsics_case():
    """A K whose third row is not (0, 0, 1), so that uvw_2 is no longer the camera depth: with a sideways baseline it turns
    negative in front of the camera, on the way out for one pair of maps and on the way back for the other."""
    H, W = 12, 8
    K = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 3.0], [0.25, 0.0, 1.0]])
    d, c = const_maps([3.0, 1.0, 3.0], H, W)
    poses = [(EYE, ZERO), (EYE, np.array([8.0, 0.0, 0.0])), (EYE, np.array([-16.0, 0.0, 0.0]))]
    nbr = np.array([[1, 2], [0, -1], [0, -1]], np.int32)
    return Case("odd_intrinsics", d, c, K, poses, neighbours=nbr, max_px=64.0, max_rel=4.0,
                edges=("uvw_behind", "back_uvw_behind"))


# ------------------------------------------------------------------------------------------------- the scene ---
_SCENE = {}


def scene_maps(shape=SCENE, seed=31):
    """(depth with noise and outliers, conf, K, poses, analytic depth, outlier mask) of make_scene(*shape): relative
    Gaussian noise of NOISE_SIGMA on every pixel, OUTLIER_FRACTION of the pixels moved 5 to 40 % off, and a seeded 3 % with
    a confidence below the threshold."""
    key = (shape, seed)
    if key not in _SCENE:
        from amvs.synthetic import make_scene
        n, H, W = shape
        sc = make_scene(n, H, W, seed=3)
        rng = np.random.default_rng(seed)
        truth = np.stack(sc.depths).astype(np.float64)
        depth = truth * (1.0 + rng.normal(0.0, NOISE_SIGMA, truth.shape))
        outlier = rng.random(truth.shape) < OUTLIER_FRACTION
        off = rng.uniform(0.05, 0.40, truth.shape) * rng.choice([-1.0, 1.0], truth.shape)
        depth = np.where(outlier, truth * (1.0 + off), depth).astype(F32)
        conf = np.where(rng.random(truth.shape) < 0.03, 0.0, 3.0).astype(F32)
        poses = [(sc.poses[i].R.astype(np.float64), sc.poses[i].t.astype(np.float64)) for i in range(n)]
        _SCENE[key] = (depth, conf, sc.camera.K.astype(np.float64), poses, truth, outlier)
    return _SCENE[key]


def scene_case():
    depth, conf, K, poses, truth, outlier = scene_maps()
    return Case("scene_5_views", depth, conf, K, poses, min_confidence=3.0, min_consistent=2,
                edges=("e2_fail", "depth_fail", "consistent", "cnt_just_below", "cnt_at_min", "nbr_conf_low", "centre_conf_low"),
                extra=dict(truth=truth, outlier=outlier))


def ragged_case():
    """The scene with neighbour rows of unequal length, padded with -1 (in front, in the middle and at the end)."""
    depth, conf, K, poses, truth, outlier = scene_maps()
    nbr = np.array([[1, 2, -1, -1], [-1, 0, 2, 3], [4, -1, 0, 1], [-1, -1, -1, 4], [3, 2, 1, 0]], np.int32)
    return Case("scene_ragged_rows", depth, conf, K, poses, neighbours=nbr, min_confidence=3.0, min_consistent=2,
                edges=("consistent", "cnt_just_below", "cnt_at_min"))


def big_case():
    """2 maps of 260 x 256: more pixels than one trip of the launch grid covers (see the module docstring)."""
    rng = np.random.default_rng(24)
    H, W = 260, 256
    d = (6.0 * (1.0 + rng.normal(0.0, 0.005, (2, H, W)))).astype(F32)
    c = np.where(rng.random(d.shape) < 0.05, 0.0, 1.0).astype(F32)
    return Case("big_two_maps", d, c, pinhole(200.0, W, H), [(EYE, ZERO), (EYE, np.array([0.3, -0.2, 0.0]))], big=True,
                edges=("consistent", "depth_fail"))


_FAMILY = None


def family():
    global _FAMILY
    if _FAMILY is None:
        _FAMILY = [tiny_case(), single_map_case(), depth_tie_case(), order_case(), e2_tie_case(), e2_fail_case(), shifted_case(),
                   special_values_case(), behind_case(), odd_intrinsics_case(), scene_case(), ragged_case(), big_case()]
    return _FAMILY


def small_family():
    """What the Python loops restate too."""
    return [c for c in family() if not c.big]


def by_name(name):
    return next(c for c in family() if c.name == name)
