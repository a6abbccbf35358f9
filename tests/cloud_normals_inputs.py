"""The input family of the normal tests (a helper module, not a conftest; seeded, no GPU): the smallest shapes at which
csrc/amvs_cloud_normals.hip can go wrong, one input per guard and exact edge of the definition in include/amvs.h, and the
height-field scenes of amvs.synthetic with a seeded 15 % of the pixels declared invalid.

A Case holds stacked maps, the cameras, the parameters of the fit and -- where it has a cloud -- the points and the
parameters of the cloud step.  `edges` names the counters of tests/cloud_normals_restatement.py the input was built for:
the CPU test holds each such input to reaching them on its own.  No input is larger than 4 maps of 48 x 64, except one of
6 x 96 x 128 (many workgroups, each lane walking the fit kernel's grid-stride loop twice, the second round ragged), which
the NumPy twin restates.
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
FLT_MAX = np.finfo(np.float32).max
EYE = np.eye(3)
ZERO = np.zeros(3)
MASK_FRACTION = 0.15
SCENE_SMALL, SCENE_BIG = (4, 48, 64), (6, 96, 128)


def up(x):
    return np.nextafter(F32(x), INF32)


def down(x):
    return np.nextafter(F32(x), -INF32)


@dataclass
class Case:
    name: str
    depth: np.ndarray                    # (n, H, W) float32
    conf: np.ndarray
    K: np.ndarray                        # (3, 3) float64
    poses: list                          # [(R, t)] float64
    min_confidence: float = 1.0
    radius: int = 2
    jump: float = 0.05
    min_points: int = 3
    points: np.ndarray = None            # (N, 3) float64, or None: the fit alone
    depth_tolerance: float = 0.01
    min_views: int = 1
    edges: tuple = ()
    big: bool = False                    # restated by the NumPy twin only
    extra: dict = field(default_factory=dict)

    @property
    def shape(self):
        return self.depth.shape[1:]

    def fit_args(self):
        return (self.depth, self.conf, self.K, self.poses, self.min_confidence, self.radius, self.jump, self.min_points)

    def cloud_args(self):
        return (self.K, self.poses, self.depth_tolerance, self.min_views)


def pinhole(f, W, H):
    return np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])


def plane_depth(n, H, W, rng, base=4.0, slope=0.02):
    """Depths of slanted planes: inverse depth linear in the pixel, rounded to float32."""
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.empty((n, H, W), F32)
    for j in range(n):
        gx, gy = rng.uniform(-slope, slope, 2) / base
        out[j] = (1.0 / (1.0 / base + gx * (xs - W / 2) + gy * (ys - H / 2))).astype(F32)
    return out


def ones(depth):
    return np.ones_like(depth, dtype=F32)


def backproject(K, pose, u, v, z):
    """World points of the pixels (u, v) at camera depth z (float64 NumPy; exactness is the caller's business)."""
    R, t = pose
    Ki = np.linalg.inv(K)
    ray = np.stack([u, v, np.ones_like(u)], axis=-1) @ Ki.T
    return ((ray * np.asarray(z)[..., None]) - t) @ R


# --------------------------------------------------------------------------------------------- fit inputs ---
def tiny_cases():
    rng = np.random.default_rng(11)
    out = []
    for name, (H, W), r in (("tiny_2x3_r3", (2, 3), 3), ("tiny_3x2_r3", (3, 2), 3), ("row_1x9", (1, 9), 2), ("col_9x1", (9, 1), 2),
                            ("one_pixel", (1, 1), 1)):
        d = plane_depth(3, H, W, rng)
        out.append(Case(name, d, ones(d), pinhole(8.0, W, H), [(EYE, ZERO)] * 3, radius=r,
                        edges=("few_points",) if H * W == 1 else ("det_zero",) if 1 in (H, W) else ("nbr_outside",)))
    return out


def border_cases():
    rng = np.random.default_rng(12)
    out = []
    for r in (1, 2, 3, 4):
        d = plane_depth(2, 6, 7, rng)
        out.append(Case(f"borders_r{r}", d, ones(d), pinhole(6.0, 7, 6), [(EYE, ZERO), (EYE, np.array([0.5, 0.0, 0.0]))], radius=r,
                        edges=("nbr_outside",)))
    return out


def det_zero_case(column=False):
    """One valid row (or column) in the image: every used set is collinear, as in an image of one row -- which a context
    cannot have (amvs_create wants 2 x 2 at least), so this is how the device meets the situation."""
    rng = np.random.default_rng(13)
    d = plane_depth(2, 12, 5, rng) if column else plane_depth(2, 5, 12, rng)
    c = np.zeros_like(d)
    if column:
        c[:, :, 2] = 1.0
    else:
        c[:, 2] = 1.0
    H, W = d.shape[1:]
    return Case("one_valid_column" if column else "one_valid_row", d, c, pinhole(8.0, W, H), [(EYE, ZERO)] * 2, radius=2,
                edges=("det_zero", "nbr_invalid"))


def min_points_case():
    rng = np.random.default_rng(14)
    d = plane_depth(1, 12, 16, rng)
    c = np.zeros_like(d)
    for y in (0, 4, 8):                                       # an L of five pixels: (0,0) (0,1) (0,2) (1,0) (1,1), 4 apart
        for x in (0, 4, 8, 12):
            for dy, dx in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1)):
                c[0, y + dy, x + dx] = 1.0
    return Case("five_pixel_islands", d, c, pinhole(16.0, 16, 12), [(EYE, ZERO)], radius=1, min_points=5,
                edges=("few_points", "n_eq_min_points", "n_eq_min_points_minus_1"))


def jump_case():
    """Power-of-two depths and jump = 0.25: around a centre at 4 the limit is exactly 1; neighbours at 5 and 3 sit on it,
    one float32 ulp beyond they are rejected."""
    rng = np.random.default_rng(15)
    d = np.full((2, 8, 10), 4.0, F32)
    choice = np.array([4.0, 5.0, up(5.0), 3.0, down(3.0), 4.0, 4.0, 4.5], F32)
    pick = rng.integers(0, len(choice), d.shape)
    d = choice[pick]
    return Case("jump_power_of_two", d, ones(d), pinhole(8.0, 10, 8), [(EYE, ZERO)] * 2, radius=1, jump=0.25,
                edges=("jump_equal", "jump_rejected"))


def special_value_case():
    rng = np.random.default_rng(16)
    d = plane_depth(2, 10, 12, rng)
    c = np.full_like(d, 2.0)
    bad_d = np.array([0.0, -0.0, -1.5, np.nan, np.inf, -np.inf, FLT_MAX, np.finfo(F32).tiny, 1e-42], F32)
    bad_c = np.array([np.nan, 2.0, down(2.0), up(2.0), -np.inf, np.inf], F32)
    for j in range(2):
        where = rng.choice(d[j].size, 36, replace=False)
        d[j].reshape(-1)[where[:18]] = np.resize(bad_d, 18)
        c[j].reshape(-1)[where[18:]] = np.resize(bad_c, 18)
    return Case("special_values", d, c, pinhole(8.0, 12, 10), [(EYE, ZERO)] * 2, min_confidence=2.0, radius=2, jump=0.5,
                edges=("centre_invalid", "nbr_invalid"))


def fronto_case():
    """A fronto-parallel plane at a power-of-two depth under a power-of-two focal length: every sum is exact, the normal
    is exactly (0, 0, -1) in the camera frame."""
    d = np.full((1, 7, 9), 4.0, F32)
    return Case("fronto_parallel", d, ones(d), pinhole(64.0, 8, 6), [(EYE, ZERO)], radius=2, extra={"exact_normal": (0.0, 0.0, -1.0)})


def c_guard_case():
    """jump = 1 lets a neighbour 128 times nearer into the fit.  Columns repeat (invalid, invalid, 1, 1, 2^-7): the centre in
    the third column sees nothing to its left, two inverse depths of 1 and one of 128 two pixels to its right, so the fitted
    line is negative at the centre: c <= 0."""
    d = np.tile(np.array([1.0, 1.0, 1.0, 1.0, 2.0 ** -7], F32), (2, 6, 2))
    c = np.tile(np.array([0.0, 0.0, 1.0, 1.0, 1.0], F32), (2, 6, 2))
    return Case("negative_fit_at_centre", d, c, pinhole(8.0, 10, 6), [(EYE, ZERO)] * 2, radius=2, jump=1.0, edges=("c_not_positive",))


def len_bad_case():
    """Intrinsics scaled by 2^520: m * m overflows, len is infinite."""
    rng = np.random.default_rng(17)
    d = plane_depth(1, 5, 6, rng)
    return Case("huge_intrinsics", d, ones(d), pinhole(8.0, 6, 5) * 2.0 ** 520, [(EYE, ZERO)], radius=1, edges=("len_bad",))


# ------------------------------------------------------------------------------------------- cloud inputs ---
PLATE_W, PLATE_H, PLATE_F, PLATE_Z = 16, 12, 64.0, 4.0
FLIP = np.diag([-1.0, 1.0, -1.0])                                  # half a turn about y: a camera looking along -z


def _plate_maps(n):
    d = np.full((n, PLATE_H, PLATE_W), PLATE_Z, F32)
    c = ones(d)
    c[:, 1::3, 1::2] = 0.0                                         # pixels without a normal, next to pixels with one
    return d, c


def _plate_point(u, v, z):
    """The point that view (I, 0) sees at pixel position (u, v), depth z: exact for the values used here."""
    return [(u - PLATE_W / 2) * z / PLATE_F, (v - PLATE_H / 2) * z / PLATE_F, z]


def plate_case():
    """Two cameras side by side in front of the plane z = 4 (exact arithmetic: every normal is (0, 0, -1)); the second is
    shifted by 1/4, which is 4 pixels.  min_views = 2."""
    d, c = _plate_maps(2)
    pts = []
    vs = [float(v) for v in range(-6, 18)]                         # 24 rows of points, 12 of them inside the image
    for v in vs:
        pts.append(_plate_point(-0.5, v, PLATE_Z))                 # u == -0.5: pixel 0
        pts.append(_plate_point(PLATE_W - 0.5, v, PLATE_Z))        # u == W - 0.5: outside
        pts.append(_plate_point(2.5, v, PLATE_Z))                  # ties: floor(u + 0.5) = 3, rint = 2
        pts.append(_plate_point(5.0, v + 0.5, PLATE_Z))            # ties in v
        pts.append(_plate_point(6.0, v, -PLATE_Z))                 # behind both cameras
        pts.append(_plate_point(6.0, v, 0.0))                      # Xc2 == 0
        pts.append(_plate_point(7.0, v, PLATE_Z))                  # a pixel with or without a normal, by row
        pts.append(_plate_point(1.0, v, PLATE_Z))                  # seen by the first camera only (u = -3 in the second)
    for u in range(PLATE_W):
        for z in (4.0625, np.nextafter(4.0625, np.inf), 3.9375, np.nextafter(3.9375, 0.0)):
            pts.append(_plate_point(float(u), 3.0, z))             # |d - z| = 2^-6 d exactly, and one float64 ulp beyond
    poses = [(EYE, ZERO), (EYE, np.array([-0.25, 0.0, 0.0]))]
    return Case("plate_two_views", d, c, pinhole(PLATE_F, PLATE_W, PLATE_H), poses, radius=1, points=np.array(pts),
                depth_tolerance=2.0 ** -6, min_views=2,
                edges=("behind", "xc2_zero", "outside", "u_eq_minus_half", "u_eq_w_minus_half", "pixel_tie", "no_normal_pixel",
                       "depth_rejected", "depth_equal", "few_views", "seen_eq_min_views_minus_1"))


def cancel_case():
    """Two cameras on opposite sides of a plate of no thickness at z = 4, both 4 away on the same axis: a point on the plate
    gets (0, 0, -1) from one and (0, 0, 1) from the other with equal weights, and the sum is exactly zero: L == 0."""
    d, c = _plate_maps(2)
    c[:] = 1.0
    pts = [_plate_point(float(u), float(v), PLATE_Z) for v in range(2, 8) for u in range(3, 13)]
    poses = [(EYE, ZERO), (FLIP, np.array([0.0, 0.0, 2 * PLATE_Z]))]
    return Case("plate_opposite_views", d, c, pinhole(PLATE_F, PLATE_W, PLATE_H), poses, radius=1, points=np.array(pts),
                depth_tolerance=2.0 ** -6, min_views=1, edges=("l_zero",))


def grazing_case():
    """w <= 0.  A normal map faces its own camera, so the pixel's own point always has w > 0; a cloud point in the same
    pixel half a pixel to the side does not where the fitted plane is steep enough.  jump = 1 makes it so: column 0 at depth
    1, column 1 at depth 1/4 (inverse depth 1 + 3 dx), nothing else valid.  At u = -0.4 the plane's inverse depth is
    negative: the point is behind the fitted plane as seen along its ray, and w < 0."""
    H, W = 6, 8
    d = np.ones((1, H, W), F32)
    d[:, :, 1] = 0.25
    c = np.zeros_like(d)
    c[:, :, :2] = 1.0
    K = pinhole(8.0, W, H)
    us = np.array([-0.48, -0.45, -0.42, -0.4, -0.37, 0.2, 0.3, 0.4])
    uu, vv = np.meshgrid(us, np.arange(H, dtype=np.float64), indexing="xy")
    pts = backproject(K, (EYE, ZERO), uu.reshape(-1), vv.reshape(-1), np.ones(uu.size))
    return Case("grazing_plane", d, c, K, [(EYE, ZERO)], radius=1, jump=1.0, points=pts, depth_tolerance=2.0 ** -6,
                edges=("backfacing",))


# ------------------------------------------------------------------------------------- height-field scenes ---
_SCENES = {}


def scene(shape):
    if shape not in _SCENES:
        from amvs.synthetic import make_scene
        _SCENES[shape] = make_scene(*shape)
    return _SCENES[shape]


def surface_normal(X, Y, amp=0.15, fx=1.3, fy=1.7):
    """Unit normal of z = amp sin(fx X) cos(fy Y) toward the cameras (negative z)."""
    hx = amp * fx * np.cos(fx * X) * np.cos(fy * Y)
    hy = -amp * fy * np.sin(fx * X) * np.sin(fy * Y)
    n = np.stack([hx, hy, -np.ones_like(hx)], axis=-1)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def scene_maps(shape, noise=0.0, mask_seed=2024):
    """(depth, conf, K, poses) of the ground-truth depths of make_scene(*shape): a seeded 15 % of the pixels invalid
    (confidence 0), optional relative Gaussian depth noise."""
    sc = scene(shape)
    rng = np.random.default_rng(mask_seed)
    depth = np.stack(sc.depths).astype(F32)
    conf = np.where(rng.random(depth.shape) < MASK_FRACTION, 0.0, 3.0).astype(F32)
    if noise:
        depth = (depth.astype(np.float64) * (1.0 + noise * rng.standard_normal(depth.shape))).astype(F32)
    poses = [(sc.poses[i].R.astype(np.float64), sc.poses[i].t.astype(np.float64)) for i in range(shape[0])]
    return depth, conf, sc.camera.K.astype(np.float64), poses


def scene_truth(shape):
    """(analytic world normals (n, H, W, 3), camera-frame points (n, H, W, 3)) at the ground-truth depths."""
    sc = scene(shape)
    n, H, W = shape
    K = sc.camera.K
    vs, us = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    normals, cam = [], []
    for i in range(n):
        pose = (sc.poses[i].R, sc.poses[i].t)
        Xw = backproject(K, pose, us, vs, sc.depths[i].astype(np.float64))
        normals.append(surface_normal(Xw[..., 0], Xw[..., 1]))
        cam.append(Xw @ pose[0].T + pose[1])
    return np.stack(normals), np.stack(cam)


def scene_case(shape, radius, step, noise=0.0):
    """The scene's maps and a cloud of every `step`-th valid pixel of every view, back-projected in float64."""
    depth, conf, K, poses = scene_maps(shape, noise)
    n, H, W = shape
    pts = []
    for j in range(n):
        flat = np.flatnonzero(conf[j].reshape(-1) >= 3.0)[::step]
        v, u = np.divmod(flat, W)
        pts.append(backproject(K, poses[j], u.astype(np.float64), v.astype(np.float64), depth[j].reshape(-1)[flat].astype(np.float64)))
    name = f"scene_{n}x{H}x{W}_r{radius}" + ("_noisy" if noise else "")
    return Case(name, depth, conf, K, poses, min_confidence=3.0, radius=radius, points=np.concatenate(pts), min_views=2,
                big=shape == SCENE_BIG)


# --------------------------------------------------------------------------------------------- the family ---
_FAMILY = None


def family():
    """Every input, small ones first; built once."""
    global _FAMILY
    if _FAMILY is None:
        _FAMILY = (tiny_cases() + border_cases()
                   + [det_zero_case(), det_zero_case(column=True), min_points_case(), jump_case(), special_value_case(), fronto_case(), c_guard_case(),
                      len_bad_case(), plate_case(), cancel_case(), grazing_case()]
                   + [scene_case(SCENE_SMALL, r, 7) for r in (1, 2, 3)]
                   + [scene_case(SCENE_SMALL, 2, 7, noise=1e-3), scene_case(SCENE_BIG, 2, 5)])
    return _FAMILY


def small_family():
    return [c for c in family() if not c.big]


def device_family():
    """The inputs a context can hold: amvs_create refuses images of one row or one column."""
    return [c for c in family() if min(c.shape) >= 2]


def by_name(name):
    return next(c for c in family() if c.name == name)
