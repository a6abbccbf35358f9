"""The input family of the lens-undistortion tests (a helper module, not a conftest): one member per edge of the
definition in include/amvs_lens.h at which csrc/amvs_undistort.hip can go wrong.  tests/test_undistort_cpu.py asserts on
the restatement that every member reaches the edge it was built for; tests/test_hip_undistort.py compares the device
with the restatement on all of them.  Seeded random BGR content unless stated."""
from dataclasses import dataclass, field

import numpy as np

# the four distortion models of the 48 x 64 members; the second (RADIAL_TANGENTIAL) is the one the other members reuse
BARREL = [-0.3, 0.1, 0.0, 0.0, 0.0]
RADIAL_TANGENTIAL = [0.25, -0.05, 0.01, -0.02, 0.03]
RATIONAL = [0.2, 0.1, 0.001, 0.002, 0.01, 0.1, 0.05, 0.01]
FOUR = [-0.35, 0.12, 0.004, -0.003]
MODELS = (("barrel", BARREL), ("radial_tangential", RADIAL_TANGENTIAL), ("rational", RATIONAL), ("four", FOUR))


def matrix(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], np.float64)


K_48x64 = matrix(50.0, 52.0, 31.5, 23.25)


def content(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@dataclass
class Case:
    name: str
    src: np.ndarray
    K: np.ndarray
    dist: list
    big: bool = False                    # restated by the vectorised form only
    identity: bool = False               # the output is the input and nothing is outside
    has_outside: bool = False            # some pixels are OUTSIDE
    has_partial: bool = False            # some inside pixels have taps outside the image
    extra: dict = field(default_factory=dict)

    @property
    def shape(self):
        return self.src.shape[:2]


def identity_cases():
    out = []
    for n, (h, w) in enumerate(((1, 1), (3, 5), (64, 65))):
        m = max(h, w)
        out.append(Case(f"identity_{h}x{w}", content(h, w, 100 + n), matrix(0.8 * m, 0.83 * m, w / 2.0 + 0.2, h / 2.0 - 0.3),
                        [0.0, 0.0, 0.0, 0.0], identity=True))
    return out


def model_cases():
    src = content(48, 64, 7)
    return [Case(f"model_{name}", src, K_48x64, d, has_outside=name in ("radial_tangential", "rational"),
                 has_partial=name in ("radial_tangential", "rational")) for name, d in MODELS]


def strip_cases():
    return [Case("strip_1x37", content(1, 37, 21), matrix(30.0, 31.0, 18.0, 0.0), RADIAL_TANGENTIAL),
            Case("strip_37x1", content(37, 1, 22), matrix(30.0, 31.0, 0.0, 18.0), RADIAL_TANGENTIAL)]


def tie_cases():
    """K = identity on a 3 x 5 image: pixel (j = 1, i = 0) has x = 1, y = 0, so u * 32 = 32 + 32 k1 exactly."""
    src = content(3, 5, 31)
    return [Case("tie_down_to_32", src, np.eye(3), [1.0 / 64.0, 0.0, 0.0, 0.0, 0.0], extra={"pixel": (1, 0), "u32": 32.5, "fu": 32.0}),
            Case("tie_up_to_34", src, np.eye(3), [3.0 / 64.0, 0.0, 0.0, 0.0, 0.0], extra={"pixel": (1, 0), "u32": 33.5, "fu": 34.0})]


def nonfinite_case():
    """K = identity, k4 = -1 on a 9 x 11 image: den = 1 - r2 is 0 at (j = 1, i = 0) -> fu = inf, and at (j = 0, i = 1)
    x * kr = 0 * inf = NaN."""
    return Case("inf_and_nan", content(9, 11, 41), np.eye(3), [0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0], has_outside=True,
                extra={"inf": (1, 0), "nan": (0, 1)})


def grid_stride_case():
    """2 000 x 1 100 pixels are 32 x 275 = 8 800 tiles of 64 x 4, more than the 8 192 workgroups of the largest launch
    (UNDISTORT_MAX_BLOCKS in csrc/amvs_undistort.hip): the first 608 workgroups walk the grid-stride loop twice."""
    return Case("grid_stride_1100x2000", content(1100, 2000, 51), matrix(1700.0, 1690.0, 1003.3, 548.1),
                [-0.28, 0.09, 0.001, -0.0015, -0.01], big=True)


def small_family():
    return identity_cases() + model_cases() + strip_cases() + tie_cases() + [nonfinite_case()]


def family():
    return small_family() + [grid_stride_case()]


def distorted_view(image, K, dist, iterations=30):
    """What a camera with this lens would have recorded of the scene whose pinhole image (same K) is `image`: every raw
    pixel looks up the pinhole image at the point its ray comes from (the lens model inverted by fixed-point iteration,
    bilinear, edge pixels repeated).  Float arithmetic of no particular order: this makes test content, it is no restatement."""
    img = np.asarray(image, np.float64)
    h, w = img.shape[:2]
    k1, k2, p1, p2, k3, k4, k5, k6 = list(dist) + [0.0] * (8 - len(dist))
    xd, yd = np.meshgrid((np.arange(w) - K[0, 2]) / K[0, 0], (np.arange(h) - K[1, 2]) / K[1, 1])
    x, y = xd.copy(), yd.copy()
    for _ in range(iterations):
        r2 = x * x + y * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        x = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / kr
        y = (yd - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) / kr
    u = np.clip(x * K[0, 0] + K[0, 2], 0, w - 1)
    v = np.clip(y * K[1, 1] + K[1, 2], 0, h - 1)
    u0, v0 = np.minimum(u.astype(int), w - 2), np.minimum(v.astype(int), h - 2)
    a, b = (u - u0)[..., None], (v - v0)[..., None]
    out = (img[v0, u0] * (1 - a) + img[v0, u0 + 1] * a) * (1 - b) + (img[v0 + 1, u0] * (1 - a) + img[v0 + 1, u0 + 1] * a) * b
    return np.rint(out).astype(np.uint8)
