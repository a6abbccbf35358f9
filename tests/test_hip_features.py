"""CLAHE and SIFT on the device against tests/features_restatement.py, bit for bit: the CLAHE output for every input and
parameter set, every Gaussian and difference level of every input through sift_level, the keypoint rows and descriptor
bytes of sift_extract, the resident CLAHE result as the input, the selection through a tie, the descriptors' way into a
slot, repeatability, and the refusals.  No tolerances."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import features_inputs as fi  # noqa: E402
import features_restatement as fr  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = fi.cases()


@pytest.fixture(scope="module")
def eng():
    import amvs
    with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as e:     # the feature stages touch no view of the context
        yield e


def compare_space(eng, shapes, gauss, dog, what):
    assert len(shapes) == len(gauss), f"{what}: {len(shapes)} octaves on the device, {len(gauss)} restated"
    for o in range(len(gauss)):
        assert shapes[o] == gauss[o][0].shape, f"{what}: octave {o} is {shapes[o]}, restated {gauss[o][0].shape}"
        for i in range(fr.GAUSS):
            diff = fr.first_difference(f"{what}: Gaussian, octave {o}, index {i}", eng.sift_level(o, i), gauss[o][i])
            assert diff is None, diff
        for i in range(fr.DOG):
            diff = fr.first_difference(f"{what}: DoG, octave {o}, index {i}", eng.sift_level(o, i, dog=True), dog[o][i])
            assert diff is None, diff


@pytest.mark.parametrize("clip,grid", fi.CLAHE_PARAMS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_clahe_byte_for_byte(eng, case, clip, grid):
    want, _ = fi.restated_clahe(case, clip, grid)
    diff = fr.first_difference(f"CLAHE {clip} {grid} of {case.name}", eng.clahe(case.gray, clip, grid), want)
    assert diff is None, diff


@pytest.mark.parametrize("sigma", fi.SIGMAS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_scale_space_bit_for_bit(eng, case, sigma):
    gauss, dog = fi.restated_space(case, sigma)
    compare_space(eng, eng.sift_scale_space(case.gray, sigma), gauss, dog, f"{case.name}, sigma {sigma}")


def compare_extract(got, want, what):
    (kps, desc), (wk, wd) = got, want
    assert len(kps) == len(wk), f"{what}: {len(kps)} keypoints on the device, {len(wk)} restated"
    names = ("x", "y", "size", "angle", "response", "packed octave / layer")
    diff = fr.first_difference(f"{what}: keypoints (row, column of {names})", kps, wk)
    assert diff is None, diff
    diff = fr.first_difference(f"{what}: descriptors (keypoint, byte)", desc, wd)
    assert diff is None, diff


@pytest.mark.parametrize("params", fi.EXTRACT_PARAMS, ids=str)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_extract_bit_for_bit(eng, case, params):
    wk, wd, _ = fi.restated_extract(case, params)
    got = eng.sift_extract(case.gray, *params)
    assert got[0].shape == (len(wk), 6) and got[0].dtype == np.float32 and got[1].shape == (len(wk), 128) and got[1].dtype == np.uint8
    compare_extract(got, (wk, wd), f"{case.name}, {params}")
    # the scale space it built stays resident, and is the scale space
    gauss, dog = fi.restated_space(case, params[3])
    assert fr.first_difference("resident DoG after extract", eng.sift_level(len(dog) - 1, 2, dog=True), dog[-1][2]) is None


def test_selection_cuts_through_a_tie(eng):
    case = next(c for c in CASES if c.name.startswith("lattice"))
    n = fi.tie_cut(case)
    params = (n,) + fi.EXTRACT_PARAMS[0][1:]
    compare_extract(eng.sift_extract(case.gray, *params), fr.extract(case.gray, *params), f"lattice cut at {n}")


def test_extract_after_clahe_on_the_device(eng):
    case = CASES[2]
    want = fr.extract(fi.restated_clahe(case, 3.0, (8, 8))[0], 0, 0.01, 20.0, 1.4)
    compare_extract(eng.sift_extract(case.gray, 0, 0.01, 20.0, 1.4, clahe=(3.0, (8, 8))), want, "CLAHE, then extract")
    assert len(want[0]) > 0


def test_descriptors_into_a_slot_without_the_host(eng):
    """sift_to_slot, then match_descriptors, equals set_descriptors of the fetched bytes, then the same call."""
    a, b, _ = fi.rotated_pair(n=96)
    _, da = eng.sift_extract(a, 0, 0.03, 15.0, 1.6)
    eng.sift_to_slot(0)
    _, db = eng.sift_extract(b, 0, 0.03, 15.0, 1.6)
    eng.sift_to_slot(1)
    eng.set_descriptors(2, da)
    eng.set_descriptors(3, db)
    for ratio, cross in ((0.8, True), (0.85, False)):
        resident = eng.match_descriptors(0, 1, ratio=ratio, cross_check=cross)
        uploaded = eng.match_descriptors(2, 3, ratio=ratio, cross_check=cross)
        assert len(resident[0]) >= 10 and all(np.array_equal(p, q) for p, q in zip(resident, uploaded))
    eng.sift_extract(CASES[7].gray)                   # no keypoints: an empty slot, as set_descriptors of nothing
    eng.sift_to_slot(4)
    assert eng._desc_rows[4] == 0


def test_grid_stride_kernels_wrap(eng):
    """520 x 520: the upsampling, the halving and the CLAHE interpolation have more elements than one pass of their
    grids takes.  Checked on the CLAHE output, the first image of octave 0 and the first image of octave 1."""
    g = fi.texture(520, 520, 12)
    diff = fr.first_difference("CLAHE 520x520", eng.clahe(g, 2.0, (8, 8)), fr.clahe(g, 2.0, 8, 8))
    assert diff is None, diff
    tp = [fr.taps(s) for s in fr.sigmas(1.6)]
    eng.sift_scale_space(g, 1.6)
    img = fr.blur(fr.upsample(g), tp[0])
    diff = fr.first_difference("Gaussian, octave 0, index 0", eng.sift_level(0, 0), img)
    assert diff is None, diff
    for i in range(1, 4):
        img = fr.blur(img, tp[i])
    diff = fr.first_difference("Gaussian, octave 1, index 0", eng.sift_level(1, 0), np.ascontiguousarray(img[::2, ::2]))
    assert diff is None, diff


def test_largest_radius_beyond_every_side(eng):
    """sigma 4: the last blur has radius 31, on octaves of 48, 24, 12 and 6 pixels."""
    case = next(c for c in CASES if c.name.startswith("texture 24x24"))
    assert (len(fr.taps(fr.sigmas(4.0)[5])) - 1) // 2 == 31
    gauss, dog = fr.scale_space(case.gray, 4.0)
    compare_space(eng, eng.sift_scale_space(case.gray, 4.0), gauss, dog, "24x24, sigma 4")


def test_scale_space_of_the_resident_clahe_result(eng):
    case = CASES[2]
    out = eng.clahe(case.gray, 3.0, (8, 8))
    gauss, dog = fr.scale_space(fi.restated_clahe(case, 3.0, (8, 8))[0], 1.4)
    compare_space(eng, eng.sift_scale_space(None, 1.4), gauss, dog, "resident CLAHE result")
    assert np.array_equal(out, fi.restated_clahe(case, 3.0, (8, 8))[0])


def test_same_image_same_bits_with_another_in_between(eng):
    a, b = CASES[1].gray, CASES[6].gray

    def everything(g):
        shapes = eng.sift_scale_space(g, 1.6)
        return list(eng.sift_extract(g, 0, 0.04, 10.0, 1.6)) + list(eng.sift_extract(g, 5, 0.01, 20.0, 1.4, clahe=(3.0, (8, 8)))) + [eng.sift_level(o, i) for o in range(len(shapes)) for i in range(fr.GAUSS)] + \
               [eng.sift_level(o, i, dog=True) for o in range(len(shapes)) for i in range(fr.DOG)] + [eng.clahe(g, 2.0, (8, 8))]

    first = everything(a)
    everything(b)
    again = everything(a)
    assert len(first) == len(again) and all(np.array_equal(p, q) for p, q in zip(first, again))


def test_refusals_leave_the_context_usable(eng):
    from amvs import _lib
    from amvs.engine import AmvsError
    lib, h = eng._lib, eng._h
    img = np.zeros((16, 16), np.uint8)
    p = img.ctypes.data_as(_lib.u8p)
    big = _lib.FEATURES_MAX_SIDE + 1
    n, hh = C.c_int32(0), C.c_int32(0)
    calls = [
        ("grid below 1", lambda: lib.amvs_clahe_u8(h, p, 16, 16, 2.0, 0, 8, None)),
        ("grid above the maximum", lambda: lib.amvs_clahe_u8(h, p, 16, 16, 2.0, 8, _lib.CLAHE_MAX_GRID + 1, None)),
        ("negative clip", lambda: lib.amvs_clahe_u8(h, p, 16, 16, -1.0, 8, 8, None)),
        ("clip not finite", lambda: lib.amvs_clahe_u8(h, p, 16, 16, float("nan"), 8, 8, None)),
        ("NULL image", lambda: lib.amvs_clahe_u8(h, None, 16, 16, 2.0, 8, 8, None)),
        ("side above the maximum", lambda: lib.amvs_clahe_u8(h, p, 1, big, 2.0, 8, 8, None)),
        ("empty image", lambda: lib.amvs_clahe_u8(h, p, 0, 16, 2.0, 8, 8, None)),
        ("sigma 0", lambda: lib.amvs_sift_scale_space(h, p, 16, 16, 0.0, C.byref(n))),
        ("sigma below the minimum", lambda: lib.amvs_sift_scale_space(h, p, 16, 16, _lib.SIFT_MIN_SIGMA / 2, C.byref(n))),
        ("sigma tiny", lambda: lib.amvs_sift_scale_space(h, p, 16, 16, 1e-160, C.byref(n))),
        ("n_features negative", lambda: lib.amvs_sift_extract(h, p, 16, 16, -1, 0.04, 10.0, 1.6, C.byref(n))),
        ("n_features above the maximum", lambda: lib.amvs_sift_extract(h, p, 16, 16, _lib.SIFT_MAX_FEATURES + 1, 0.04, 10.0, 1.6, C.byref(n))),
        ("contrast threshold not finite", lambda: lib.amvs_sift_extract(h, p, 16, 16, 0, float("nan"), 10.0, 1.6, C.byref(n))),
        ("contrast threshold negative", lambda: lib.amvs_sift_extract(h, p, 16, 16, 0, -0.04, 10.0, 1.6, C.byref(n))),
        ("edge threshold not finite", lambda: lib.amvs_sift_extract(h, p, 16, 16, 0, 0.04, float("inf"), 1.6, C.byref(n))),
        ("edge threshold 0", lambda: lib.amvs_sift_extract(h, p, 16, 16, 0, 0.04, 0.0, 1.6, C.byref(n))),
        ("extract: sigma 0", lambda: lib.amvs_sift_extract(h, p, 16, 16, 0, 0.04, 10.0, 0.0, C.byref(n))),
        ("extract: side above the maximum", lambda: lib.amvs_sift_extract(h, p, 16, big, 0, 0.04, 10.0, 1.6, C.byref(n))),
        ("extract: NULL count", lambda: lib.amvs_sift_extract(h, p, 16, 16, 0, 0.04, 10.0, 1.6, None)),
        ("fetch before any extract", lambda: lib.amvs_sift_fetch(h, None, None, 0)),
        ("to_slot before any extract", lambda: lib.amvs_sift_to_slot(h, 0)),
        ("sigma negative", lambda: lib.amvs_sift_scale_space(h, p, 16, 16, -1.6, C.byref(n))),
        ("sigma not finite", lambda: lib.amvs_sift_scale_space(h, p, 16, 16, float("inf"), C.byref(n))),
        ("sigma above the maximum", lambda: lib.amvs_sift_scale_space(h, p, 16, 16, 4.5, C.byref(n))),
        ("side below the minimum", lambda: lib.amvs_sift_scale_space(h, p, 2, 16, 1.6, C.byref(n))),
        ("side above the maximum", lambda: lib.amvs_sift_scale_space(h, p, big, 16, 1.6, C.byref(n))),
        ("NULL octave count", lambda: lib.amvs_sift_scale_space(h, p, 16, 16, 1.6, None)),
        ("no resident CLAHE result of that size", lambda: lib.amvs_sift_scale_space(h, None, 15, 16, 1.6, C.byref(n))),
    ]
    eng.clahe(img, 2.0, (8, 8))
    shapes = eng.sift_scale_space(img, 1.6)
    calls += [
        ("octave beyond the last", lambda: lib.amvs_sift_fetch_level(h, len(shapes), 0, 0, None, C.byref(hh), None)),
        ("negative octave", lambda: lib.amvs_sift_fetch_level(h, -1, 0, 0, None, C.byref(hh), None)),
        ("seventh Gaussian image", lambda: lib.amvs_sift_fetch_level(h, 0, fr.GAUSS, 0, None, C.byref(hh), None)),
        ("sixth difference image", lambda: lib.amvs_sift_fetch_level(h, 0, fr.DOG, 1, None, C.byref(hh), None)),
    ]
    kps, _ = eng.sift_extract(CASES[0].gray)
    assert lib.amvs_sift_fetch(h, None, None, len(kps) + 1) == -1, "fetch of another count"
    assert lib.amvs_sift_to_slot(h, -1) == -1 and lib.amvs_sift_to_slot(h, _lib.DESC_MAX_SLOTS) == -1, "slot outside the slots"
    shapes = eng.sift_scale_space(img, 1.6)           # (drops the keypoints: the two refusals before an extract hold)
    for what, call in calls:
        assert call() == -1, what
        assert eng._lib.amvs_last_error(h), what
    with pytest.raises(AmvsError):
        eng.clahe(img, 2.0, (0, 8))
    # the resident scale space outlives the refused calls
    assert eng.sift_level(len(shapes) - 1, fr.DOG - 1, dog=True).shape == shapes[-1]
