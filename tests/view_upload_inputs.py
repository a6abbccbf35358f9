"""The input family of the view-upload tests (a helper module, not a conftest; seeded, no GPU): the source and context
shapes at which csrc/amvs_prep.hip can go wrong, the image contents that tell its taps, weights and coefficients apart,
and the gray float images that sit on either side of the losslessness switch of pack_pairs_kernel.

A ResizeCase is a (source h x w -> context H x W) pair; `edges` names the counters of tests/view_upload_restatement.py
the pair was chosen for (on the content named after the colon, seeded random bytes otherwise), and the CPU test holds
each pair to reaching them on its own.  No pair is larger than 90 x 130 -> 27 x 39, except one of 1100 x 2200 ->
1025 x 2048, which the vectorised restatement alone restates: its 2 099 200 destination pixels exceed the 2 097 152
threads of the largest grid launch_prep_bgr8 starts (8192 workgroups of 256), so the first 2048 threads of both prep
kernels walk their grid-stride loop twice and the second trip is ragged.

A weight pair can miss 2048 only where 1.f - f rounds, that is for a coordinate in (0, 0.5) of source column 0, and only
if 2048 * f lies within 2^-14 of a half-integer without being one; 2048 * f is a multiple of 1 / (2 n_dst) there, so no
axis of fewer than 8192 destination pixels has such a pair.  2 x 10928 -> 2 x 8195 is the first pair a search over
n_dst >= 8192 finds (a0 + a1 = 2047 at column 0): two rows keep it at 16 390 pixels.

A GrayCase is 3 views of 9 x 11 that are exactly code / 255, one pixel of one view replaced; `lossless` is what the pack
must report for each view.
"""
from dataclasses import dataclass

import numpy as np

F32 = np.float32
GRID_CAP_THREADS = 8192 * 256


@dataclass
class ResizeCase:
    src: tuple                           # (h, w)
    dst: tuple                           # (H, W)
    why: str
    edges: tuple = ()                    # "counter" or "counter:content"
    big: bool = False
    only: tuple = None                   # the contents, where not all of CONTENTS

    @property
    def name(self):
        return f"{self.src[0]}x{self.src[1]}_to_{self.dst[0]}x{self.dst[1]}"

    @property
    def contents(self):
        return self.only or CONTENTS


CONTENTS = ("random", "zeros", "full", "checker", "corners", "blue", "green", "red", "ramp")
BIG_CONTENTS = ("random", "random2", "random3")          # the large shape gets random content only (a cost map needs 3 views)

RESIZE_CASES = (
    ResizeCase((3, 5), (7, 9), "upscale: row offset -1 at the top, clamp at the bottom",
               ("row_ofs_minus1", "row_clamp_bottom", "col_clamp_first", "col_clamp_last", "acc_max:full")),
    ResizeCase((2, 2), (9, 9), "upscale from the smallest source", ("row_ofs_minus1", "row_clamp_bottom", "col_clamp_last")),
    ResizeCase((1, 7), (4, 7), "one source row", ("row_ofs_minus1", "row_clamp_bottom")),
    ResizeCase((7, 1), (7, 4), "one source column: every tap clamped, weight zeroed", ("col_clamp_first", "col_clamp_last")),
    ResizeCase((90, 130), (27, 39), "the shape of test_device_image_preparation_equals_host_restatement"),
    ResizeCase((64, 48), (20, 47), "the two axes scaled differently"),
    ResizeCase((5, 300), (4, 2), "extreme reduction along the rows"),
    ResizeCase((300, 5), (2, 4), "extreme reduction along the columns"),
    ResizeCase((32, 48), (16, 24), "the exact 2x reduction (cv.resize routes it to INTER_AREA: the same bytes)"),
    ResizeCase((33, 48), (11, 16), "the exact 3x reduction"),
    ResizeCase((31, 47), (31, 47), "the copy path"),
    ResizeCase((2, 10928), (2, 8195), "a weight pair that does not sum to 2048 (column 0: 1706 + 341)", ("weights_not_2048",),
               only=("random", "checker", "full")),
    ResizeCase((1100, 2200), (1025, 2048), "above the grid cap: both prep kernels wrap their stride loop", big=True, only=BIG_CONTENTS),
)


def by_name(name):
    return next(c for c in RESIZE_CASES if c.name == name)


def small_cases():
    return [c for c in RESIZE_CASES if not c.big]


def content(kind, h, w):
    """(h, w, 3) uint8 BGR image."""
    img = np.zeros((h, w, 3), np.uint8)
    if kind in ("random", "random2", "random3"):
        seed = 1000 * h + w + 7 * ("random", "random2", "random3").index(kind)
        img = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif kind == "zeros":
        pass
    elif kind == "full":
        img[:] = 255
    elif kind == "checker":                              # period 1: neighbours always differ by the full range
        y, x = np.mgrid[0:h, 0:w]
        img[:] = (((y + x) & 1) * 255).astype(np.uint8)[:, :, None]
    elif kind == "corners":
        for y in (0, h - 1):
            for x in (0, w - 1):
                img[y, x] = 255
    elif kind in ("blue", "green", "red"):               # channel order B, G, R: one gray coefficient each
        img[:, :, ("blue", "green", "red").index(kind)] = np.random.default_rng(h * 31 + w).integers(0, 256, (h, w), dtype=np.uint8)
    elif kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        den = max(h + w - 2, 1)
        img[:, :, 0] = (255 * (y + x) // den).astype(np.uint8)
        img[:, :, 1] = (255 * x // max(w - 1, 1)).astype(np.uint8)
        img[:, :, 2] = (255 - 255 * y // max(h - 1, 1)).astype(np.uint8)
    else:
        raise ValueError(kind)
    return img


def source(case, kind):
    return content(kind, *case.src)


# ------------------------------------------------------------------------------------------ the switch's inputs ---
GRAY_SHAPE = (9, 11)
GRAY_VIEWS = 3


@dataclass
class GrayCase:
    name: str
    grays: list                          # GRAY_VIEWS float32 (9, 11) images, as uploaded
    exact: list                          # the same views before the change: exactly code / 255
    lossless: list                       # per view, what the pack must report
    view: int = -1                       # the changed view (-1: none)
    pixel: tuple = None
    finite: bool = True                  # False: NaN or Inf in a view, the oracle's own result is unspecified

    @property
    def all_lossless(self):
        return all(self.lossless)


def exact_views():
    """Three seeded views of codes 1..254 over 255 (so that one step of a code stays inside (0, 1))."""
    rng = np.random.default_rng(97)
    H, W = GRAY_SHAPE
    base = rng.integers(1, 255, (H, W))
    views = []
    for v in range(GRAY_VIEWS):                          # the same texture shifted, so that the sweeps have something to match
        codes = np.clip(np.roll(base, v, axis=1) + rng.integers(-3, 4, (H, W)), 1, 254)
        views.append(codes.astype(F32) / F32(255.0))
    return views


def _code(g):
    return int(np.rint(g * F32(255.0)))


# (name, value from the pixel's exact value, lossless, finite)
CHANGES = (
    ("ulp_up", lambda g: np.nextafter(g, F32(1.0)), False, True),
    ("ulp_down", lambda g: np.nextafter(g, F32(-1.0)), False, True),
    ("code_plus_0p49", lambda g: F32((_code(g) + 0.49) / 255.0), False, True),
    ("nan", lambda g: F32(np.nan), False, False),
    ("plus_inf", lambda g: F32(np.inf), False, False),
    ("minus_inf", lambda g: F32(-np.inf), False, False),
    ("minus_one_code", lambda g: F32(-1.0) / F32(255.0), False, True),
    ("code_256", lambda g: F32(256.0) / F32(255.0), False, True),
    ("one", lambda g: F32(1.0), True, True),
    ("minus_zero", lambda g: F32(-0.0), True, True),
)
# (view, pixel): the first pixel, the last pixel, and a pixel of the last view
PLACES = ((0, (0, 0)), (1, (GRAY_SHAPE[0] - 1, GRAY_SHAPE[1] - 1)), (GRAY_VIEWS - 1, (4, 6)))


def gray_cases():
    exact = exact_views()
    cases = [GrayCase("control", [g.copy() for g in exact], exact, [True] * GRAY_VIEWS)]
    for name, change, lossless, finite in CHANGES:
        for view, pixel in PLACES:
            grays = [g.copy() for g in exact]
            grays[view][pixel] = change(exact[view][pixel])
            flags = [True] * GRAY_VIEWS
            flags[view] = lossless
            cases.append(GrayCase(f"{name}_v{view}_y{pixel[0]}x{pixel[1]}", grays, exact, flags, view, pixel, finite))
    return cases


def gray_case(name):
    return next(c for c in gray_cases() if c.name == name)
