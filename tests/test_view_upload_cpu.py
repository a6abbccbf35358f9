"""The view-upload stage without a GPU: core/imageprep.py (the package's NumPy path, what the classes use when the images
are prepared on the host) against the independent loops of tests/view_upload_restatement.py, the loops against the
float64 bilinear interpolation they approximate, the input family of tests/view_upload_inputs.py against the edges the
GPU comparison relies on, and the restatement of the 8-bit pack against the flags the family states.
tests/test_hip_view_upload.py compares the device with the same restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import view_upload_inputs as vi  # noqa: E402
import view_upload_restatement as vr  # noqa: E402

_RESTATED = {}


def restated(case, kind):
    """prepare() of one (pair, content) by the loops, computed once."""
    key = (case.name, kind)
    if key not in _RESTATED:
        _RESTATED[key] = vr.prepare(vi.source(case, kind), *case.dst)
    return _RESTATED[key]


def package_prepare(src, H, W):
    """core/imageprep.py's NumPy path for an arbitrary context size (prepare_view derives the size from one scale)."""
    from amvs.core import imageprep
    color = imageprep._resize_linear_u8(np.ascontiguousarray(src), W, H)
    return color, imageprep._bgr_to_gray_u8(color)


@pytest.mark.parametrize("case", vi.small_cases(), ids=lambda c: c.name)
def test_package_numpy_path_equals_the_loops_byte_for_byte(case):
    for kind in case.contents:
        want = restated(case, kind)
        color, codes = package_prepare(vi.source(case, kind), *case.dst)
        assert color.dtype == np.uint8 and np.array_equal(color, want["color"]), f"{case.name} {kind}: colour image"
        assert codes.dtype == np.uint8 and np.array_equal(codes, want["codes"]), f"{case.name} {kind}: gray codes"


@pytest.mark.parametrize("scale", [1.0, 0.5, 0.3])
def test_prepare_view_equals_the_loops(scale, monkeypatch):
    """prepare_view itself on its NumPy path (one scale for both axes, the size int(h * scale) x int(w * scale), float32
    gray)."""
    from amvs.core import imageprep
    monkeypatch.setattr(imageprep, "_cv", None)
    src = vi.content("random", 90, 130)
    got = imageprep.prepare_view(src, scale)
    H, W = int(90 * scale), int(130 * scale)
    want = vr.prepare(src, H, W)
    assert got["shape"] == (H, W) and np.array_equal(got["color"], want["color"])
    assert got["gray"].dtype == np.float32 and np.array_equal(got["gray"].view(np.uint32), want["gray"].view(np.uint32))


def test_vectorised_form_equals_the_loops_on_the_small_family():
    for case in vi.small_cases():
        for kind in ("random", "checker", "full"):
            want = restated(case, kind)
            got = vr.prepare_np(vi.source(case, kind), *case.dst)
            assert np.array_equal(got["color"], want["color"]) and np.array_equal(got["codes"], want["codes"]), case.name
            assert np.array_equal(got["gray"].view(np.uint32), want["gray"].view(np.uint32)), case.name


def test_vectorised_form_spot_checked_on_the_large_shape():
    """The one shape the loops do not restate whole: 1200 seeded pixels and 4 x 64 pixels of the four borders (corners
    included) by the loop form's scalar arithmetic, and the package's NumPy path on every pixel."""
    case = next(c for c in vi.RESIZE_CASES if c.big)
    H, W = case.dst
    assert H * W > vi.GRID_CAP_THREADS and (H - 1) * W <= vi.GRID_CAP_THREADS, "the smallest height above the grid cap"
    src = vi.source(case, "random")
    got = vr.prepare_np(src, H, W)
    rng = np.random.default_rng(11)
    ys, xs = list(rng.integers(0, H, 1200)), list(rng.integers(0, W, 1200))
    for k in range(64):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        if k < 2:
            y, x = (0, 0) if k == 0 else (H - 1, W - 1)
        ys += [0, H - 1, y, H - 1 - y if k < 2 else y]
        xs += [x, W - 1 - x if k < 2 else x, 0, W - 1]
    px = vr.PixelRestater(src, H, W)
    for y, x in zip(ys, xs):
        assert px.color(int(y), int(x)) == [int(v) for v in got["color"][y, x]], (y, x)
        assert px.code(int(y), int(x)) == int(got["codes"][y, x]), (y, x)
    assert {0, H - 1} <= set(int(y) for y in ys) and {0, W - 1} <= set(int(x) for x in xs)
    color, codes = package_prepare(src, H, W)
    assert np.array_equal(color, got["color"]) and np.array_equal(codes, got["codes"])


def test_fixed_point_stays_within_the_derived_bound():
    """The 8-bit chain against true bilinear interpolation in float64 (vr.bilinear64), per channel, in gray codes.

    Derivation (S <= 255 a source byte; x~ the float32 source coordinate of a destination index, (s, f) its floor and
    fraction, exact in float32; wsum = 2049 / 2048 the largest sum of a weight pair):
      coordinates  |x~ - x| <= half a float32 unit of the source size; bilinear interpolation with clamped taps is
                   continuous in each coordinate with slope at most 255, and the column rule (s clamped, f = 0) is that
                   function at the clamped coordinate: 255 * (eps_x + eps_y) to either side.
      weights      a1 = rint(2048 f) is at most 2^-12 from f in units of 2048; a0 = rint(2048 * fl(1 - f)) at most
                   2^-12 + 2^-25 from 1 - f: |D / 2048 - (S0 (1 - f) + S1 f)| <= 255 (2^-11 + 2^-25) = E per axis; the
                   horizontal error passes through the row weights, E * wsum, and the row weights add E: both sides.
      D >> 4       D / 16 less r, 0 <= r <= 15/16, that is 15/2048 codes, times (b0 + b1) / 2048 <= wsum: downwards only.
      >> 16, twice (b (D >> 4)) >> 16 is b (D >> 4) / 65536 less q, 0 <= q < 1, and four units of it are one code:
                   (q0 + q1) / 4 < 0.5, downwards only.
      (+ 2) >> 2   rounds the sum to the nearest code: 0.5 to either side.
    Together  -(0.5 + 0.5 + 15/2048 wsum + E wsum + E + 255 (eps_x + eps_y)) <= result - bilinear
              <= 0.5 + E wsum + E + 255 (eps_x + eps_y):  -1.2566 and +0.7492 before the coordinate term, which is 0.0039
              for the 300-pixel axes here and 0.1245 for the rows of 10928 pixels (vr.bilinear_bounds; the widest is
              -1.3810 .. +0.8736, below the 1.5 codes of a rougher count).
    Measured over the small family and every content: -0.7778 and +0.5933 (2 x 10928 -> 2 x 8195, the checkerboard); on
    the pairs of the issue's table alone -0.7500 and +0.5278 (90 x 130 -> 27 x 39, random bytes)."""
    lo_seen, hi_seen, where = 0.0, 0.0, None
    for case in vi.small_cases():
        lo, hi = vr.bilinear_bounds(*case.src)
        assert -1.5 < lo < -1.25 and 0.74 < hi < 1.0
        for kind in case.contents:
            src = vi.source(case, kind)
            err = restated(case, kind)["color"].astype(np.float64) - vr.bilinear64(src, *case.dst)
            assert lo <= err.min() and err.max() <= hi, f"{case.name} {kind}: {err.min():.4f} .. {err.max():.4f} outside {lo:.4f} .. {hi:.4f}"
            if err.min() < lo_seen or err.max() > hi_seen:
                where = (case.name, kind)
            lo_seen, hi_seen = min(lo_seen, err.min()), max(hi_seen, err.max())
    print(f"measured {lo_seen:.4f} .. {hi_seen:.4f} (last extreme at {where})")
    assert lo_seen < -0.5 and hi_seen >= 0.5, "the family never leaves plain rounding: the truncations are not exercised"


def test_exact_reductions_are_the_box_average_and_the_centre_pixel():
    """Two results known without any table.  At an exact 2x reduction every coordinate is 2 d + 0.5 and all four weights
    are 1024: the chain is (a + b + c + d + 2) >> 2 of the 2 x 2 block, which is also what cv.resize computes there (it
    routes the exact 2x to INTER_AREA).  At an exact 3x reduction every coordinate is 3 d + 1: the centre pixel."""
    two, three = vi.by_name("32x48_to_16x24"), vi.by_name("33x48_to_11x16")
    for kind in two.contents:
        s = vi.source(two, kind).astype(np.int64)
        box = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
        assert np.array_equal(restated(two, kind)["color"], box), kind
        assert np.array_equal(restated(three, kind)["color"], vi.source(three, kind)[1::3, 1::3]), kind


def test_gray_coefficients_and_channel_order():
    """The 15-bit coefficients sum to 2^15 (gray of (v, v, v) is v), and the one-channel contents give each coefficient
    alone: B * 3735, G * 19235, R * 9798, rounded."""
    assert vr.GRAY_B + vr.GRAY_G + vr.GRAY_R == 1 << 15
    case = vi.by_name("31x47_to_31x47")
    for kind, k in (("blue", 3735), ("green", 19235), ("red", 9798)):
        src = vi.source(case, kind)
        ch = src[:, :, ("blue", "green", "red").index(kind)].astype(np.int64)
        assert ch.max() > 200 and np.array_equal(restated(case, kind)["codes"], (ch * k + 16384) >> 15), kind
    for kind in ("zeros", "full", "checker"):
        assert np.array_equal(restated(case, kind)["codes"], vi.source(case, kind)[:, :, 0]), kind


def test_family_reaches_every_listed_edge():
    """What keeps the GPU comparison from silently leaving an edge out, counted on the loops' intermediates: a pair chosen
    for an edge reaches it on its own (on random bytes, or on the content it names), and the family as a whole reaches a
    row offset of -1 with a non-zero weight on it, a clamped first and last column whose fraction was not zero already,
    a weight pair that does not sum to 2048, and a horizontal accumulator at its maximum 255 * 2048."""
    total = dict.fromkeys(vr.COUNTERS, 0)
    for case in vi.small_cases():
        for edge in case.edges:
            counter, _, kind = edge.partition(":")
            own = restated(case, kind or "random")["counters"]
            assert own[counter] >= 1, f"{case.name} was chosen for {edge} and does not reach it"
        for kind in case.contents:
            for k, v in restated(case, kind)["counters"].items():
                total[k] += v
    print(total)
    assert all(v >= 1 for v in total.values()), total
    one_col = restated(vi.by_name("7x1_to_7x4"), "random")["counters"]
    assert one_col["col_clamp_first"] + one_col["col_clamp_last"] == 4, "one source column: every tap clamped"
    assert {c.src for c in vi.RESIZE_CASES} >= {(3, 5), (2, 2), (1, 7), (7, 1), (90, 130), (64, 48), (5, 300), (300, 5), (32, 48),
                                                (33, 48), (31, 47), (1100, 2200)}
    assert min(min(c.dst) for c in vi.RESIZE_CASES) == 2, "the smallest context"
    big = [c for c in vi.RESIZE_CASES if c.big]
    assert len(big) == 1 and big[0].dst[0] * big[0].dst[1] > vi.GRID_CAP_THREADS and big[0].contents == vi.BIG_CONTENTS
    assert any(c.src == c.dst for c in vi.RESIZE_CASES), "the copy path"


@pytest.mark.parametrize("variant", vr.VARIANTS)
def test_family_tells_every_near_miss_from_the_definition(variant):
    """The near misses of the kernel, restated: the first row index or the column taps left unclamped (the tap outside the
    image then reads whatever lies in front of the staging buffer: 0 and 255 stand for it, and both must show), the B and R
    coefficients swapped, and the >> 4 taken after the multiplication by the row weight."""
    differing = set()
    for poison in (0, 255):
        seen = set()
        for case in vi.small_cases():
            if case.src[1] > 4096:
                continue
            for kind in ("random", "ramp"):
                got = vr.prepare(vi.source(case, kind), *case.dst, variant=variant, poison=poison)
                want = restated(case, kind)
                if not (np.array_equal(got["color"], want["color"]) and np.array_equal(got["codes"], want["codes"])):
                    seen.add(case.name)
        differing = seen if poison == 0 else differing & seen
    print(variant, sorted(differing))
    assert differing, f"no input of the family tells {variant} from the definition"


def test_unknown_variant_is_refused():
    with pytest.raises(ValueError):
        vr.resize(vi.content("random", 3, 5), 7, 9, variant="none_such")


# ------------------------------------------------------------------------------------------------------ the pack ---
@pytest.mark.parametrize("case", vi.gray_cases(), ids=lambda c: c.name)
def test_pack_restatement_gives_the_stated_flags(case):
    assert vr.pack_views(case.grays) == case.lossless
    assert vr.pack_views(case.exact) == [True] * vi.GRAY_VIEWS
    if case.view >= 0:
        y, x = case.pixel
        changed = [(v, int(i)) for v in range(vi.GRAY_VIEWS)
                   for i in np.flatnonzero(case.grays[v].view(np.uint32) != case.exact[v].view(np.uint32))]
        assert changed == [(case.view, y * vi.GRAY_SHAPE[1] + x)], "exactly one pixel of one view differs"


def test_gray_family_holds_what_the_switch_needs():
    cases = vi.gray_cases()
    assert len(cases) == 1 + len(vi.CHANGES) * len(vi.PLACES) and cases[0].all_lossless and cases[0].view == -1
    H, W = vi.GRAY_SHAPE
    assert {(c.view, c.pixel) for c in cases[1:]} >= {(0, (0, 0)), (1, (H - 1, W - 1))}
    assert any(c.view == vi.GRAY_VIEWS - 1 for c in cases)
    v = {c.name.split("_v")[0]: c for c in cases[1:] if c.view == 0}          # the changed pixel is (0, 0) of view 0
    g = v["ulp_up"].exact[0][0, 0]
    assert v["ulp_up"].grays[0][0, 0] == np.nextafter(g, np.float32(2)) and v["ulp_down"].grays[0][0, 0] == np.nextafter(g, np.float32(-2))
    code = int(np.rint(g * np.float32(255.0)))
    assert v["code_plus_0p49"].grays[0][0, 0] == np.float32((code + 0.49) / 255.0)
    assert vr.pack(v["code_plus_0p49"].grays[0])[0][0, 0] == code, "rounds back to the same code: only the equality test can tell"
    assert np.signbit(v["minus_zero"].grays[0][0, 0]) and v["minus_zero"].all_lossless and v["one"].all_lossless
    assert sorted(n for n, c in v.items() if not c.finite) == ["minus_inf", "nan", "plus_inf"]
    assert not any(c.all_lossless for n, c in v.items() if n not in ("one", "minus_zero"))
    codes = {n: int(vr.pack(c.grays[0])[0][0, 0]) for n, c in v.items()}
    assert (codes["nan"], codes["plus_inf"], codes["minus_inf"], codes["minus_one_code"], codes["code_256"], codes["one"],
            codes["minus_zero"]) == (0, 255, 0, 0, 255, 255, 0)
