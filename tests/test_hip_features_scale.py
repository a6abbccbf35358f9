"""SIFT on the device where its launches wrap, retry and sort at scale, and at the ends of the sigma range, against
tests/features_restatement.py bit for bit: the second input family of tests/features_inputs.py, whose conditions
tests/test_features_cpu.py asserts with the restatement alone.  No tolerances, no element left out.

What each test would catch, from the kernel text:
- the wrap inputs: no wrap (the 406 and 548 keypoints of octave 0 that start beyond the first pass are missing: the
  counts differ); a grid stride of gridDim.x * 256 - 1 (every pixel is still visited, pixel 8192 * 256 - 1 twice: the
  520 x 700 input has a blob planted so that a keypoint starts exactly there, and comes out twice; 520 x 520 alone would
  not show this one);
- the candidates input: hits beyond the array's capacity dropped instead of searched again (octaves 0 and 1 fill the
  16 384 places before octave 2 is searched, and every keypoint lies in octaves 2 to 4: none would be left);
- the crowd: the low words taken from the response keys before they are sorted (they are 0 .. n - 1 then: the first n
  keypoints in canonical order are kept, not the strongest), a cut that breaks ties by anything but the canonical
  index, a scratch block of a smaller run reused short;
- the scale space on several tiles: a halo span without its 2 r (the last 2 r places of a tile's staging are never
  written, so the last 2 r columns of every 256-column tile and the last 2 r rows of every 64-row tile are sums over
  stale LDS; on the 48 x 48 octave of the first family's sigma 4 case no lane reads that far, here lanes 194 to 255 do)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import features_inputs as fi  # noqa: E402
import features_restatement as fr  # noqa: E402
from test_hip_features import compare_extract, compare_space  # noqa: E402

pytestmark = pytest.mark.gpu

SCALE = fi.scale_cases()


def new_engine():
    import amvs
    return amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32))     # the feature stages touch no view of the context


@pytest.fixture(scope="module")
def eng():
    with new_engine() as e:
        yield e


def check_extract(eng, case, params):
    """sift_extract of a case against the restatement, and the resident last DoG level after it.  Returns the device's."""
    wk, wd, _ = fi.restated_extract(case, params)
    got = eng.sift_extract(case.gray, *params)
    assert got[0].shape == (len(wk), 6) and got[0].dtype == np.float32 and got[1].shape == (len(wk), 128) and got[1].dtype == np.uint8
    compare_extract(got, (wk, wd), f"{case.name}, {params}")
    gauss, dog = fi.restated_space(case, params[3])
    diff = fr.first_difference("resident DoG after extract", eng.sift_level(len(dog) - 1, 2, dog=True), dog[-1][2])
    assert diff is None, diff
    return got


@pytest.mark.parametrize("name", ["wrap", "wrap, mid-layer"])
def test_extrema_search_wraps(eng, name):
    check_extract(eng, *SCALE[name])


def test_more_candidates_than_the_first_array_holds(eng):
    """The search runs twice; then a crowded image whose candidates fit, then the first again: an array enlarged once
    does not change a later, smaller search."""
    first = check_extract(eng, *SCALE["candidates"])
    check_extract(eng, *SCALE["crowd"])
    again = check_extract(eng, *SCALE["candidates"])
    assert all(np.array_equal(p, q) for p, q in zip(first, again))


def test_thousands_of_keypoints_and_the_cuts_among_them(eng):
    """10 594 keypoints: sorts beyond one block.  Then the 3000 strongest, the cut through a tie, and all again:
    scratch sized by the smaller runs is not reused short."""
    case, params = SCALE["crowd"]
    first = check_extract(eng, case, params)
    assert len(first[0]) > 8192
    check_extract(eng, case, (fi.CUT,) + params[1:])
    check_extract(eng, case, (fi.tie_cut_near(first[0], 6000),) + params[1:])
    again = check_extract(eng, case, params)
    assert all(np.array_equal(p, q) for p, q in zip(first, again))


@pytest.mark.parametrize("name", ["wide", "fine", "busy", "clip"])
def test_extract_at_the_ends_of_sigma(eng, name):
    check_extract(eng, *SCALE[name])


def test_no_keypoints_at_the_smallest_sigma(eng):
    kps, desc = eng.sift_extract(fi.SPACE_CASE.gray, 0, 0.04, 10.0, 0.1)
    assert kps.shape == (0, 6) and kps.dtype == np.float32 and desc.shape == (0, 128) and desc.dtype == np.uint8
    assert len(fi.restated_extract(fi.SPACE_CASE, (0, 0.04, 10.0, 0.1))[0]) == 0


@pytest.mark.parametrize("sigma", fi.SPACE_SIGMAS)
def test_scale_space_on_several_tiles_at_the_ends_of_sigma(eng, sigma):
    gauss, dog = fi.restated_space(fi.SPACE_CASE, sigma)
    compare_space(eng, eng.sift_scale_space(fi.SPACE_CASE.gray, sigma), gauss, dog, f"{fi.SPACE_CASE.name}, sigma {sigma}")


def test_refusal_above_the_feature_limit_leaves_the_context_usable():
    """2048 x 2048 noise under the crowded parameters: the 150 x 150 image gives 0.47 keypoints a pixel, so about 1.9
    million here against AMVS_SIFT_MAX_FEATURES = 1 048 576 (the restatement is far too slow to count them).  Its top
    left quarter is below the limit and is extracted and fetched first."""
    from amvs import _lib
    from amvs.engine import AmvsError
    big = fi.noise(2048, 2048)
    case = fi.cases()[0]
    with new_engine() as eng:
        lib, h = eng._lib, eng._h
        kps, desc = eng.sift_extract(np.ascontiguousarray(big[:1024, :1024]), *fi.BUSY_PARAMS)
        print(f"1024 x 1024: {len(kps)} keypoints")
        assert _lib.SIFT_MAX_FEATURES // 3 < 350000 < len(kps) <= _lib.SIFT_MAX_FEATURES and desc.shape == (len(kps), 128)
        assert (kps[:, 4] * 3 >= np.float32(fi.BUSY_PARAMS[1])).all() and (np.diff(kps[:, 5] % 256) >= 0).all()
        with pytest.raises(AmvsError, match="AMVS_SIFT_MAX_FEATURES"):
            eng.sift_extract(big, *fi.BUSY_PARAMS)
        n = C.c_int32(-7)
        assert lib.amvs_sift_extract(h, big.ctypes.data_as(_lib.u8p), 2048, 2048, 0, *[float(np.float32(v)) for v in fi.BUSY_PARAMS[1:3]],
                                     fi.BUSY_PARAMS[3], C.byref(n)) == -1
        assert lib.amvs_last_error(h) and n.value == -7
        for count in (0, len(kps)):
            assert lib.amvs_sift_fetch(h, None, None, count) == -1 and b"no resident keypoints" in lib.amvs_last_error(h)
        assert lib.amvs_sift_to_slot(h, 0) == -1 and b"no resident keypoints" in lib.amvs_last_error(h)
        with pytest.raises(ValueError):
            eng.sift_to_slot(0)
        level = eng.sift_level(0, 0)
        assert level.shape == (4096, 4096) and np.isfinite(level).all() and 100 < level.mean() < 156
        compare_extract(eng.sift_extract(case.gray, *fi.EXTRACT_PARAMS[0]), fi.restated_extract(case, fi.EXTRACT_PARAMS[0])[:2], "after the refusal")
