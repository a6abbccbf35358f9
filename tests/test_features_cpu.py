"""CLAHE and SIFT without a GPU: the eleventh header against its binding table, the refusals that need no
device, the restatement of tests/features_restatement.py against plain loops and against what a scale space has to be,
the input family of tests/features_inputs.py against the edges the GPU comparison relies on, the float32 functions of
the keypoint stages against NumPy, the restated extractor on a rotated and magnified texture ("it is SIFT"), and the
Python classes' argument handling.
tests/test_hip_features.py compares the device with the same restatement, tests/test_hip_features_scale.py on the second
input family (larger and crowded images, the ends of the sigma range), whose conditions are asserted here."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import features_inputs as fi  # noqa: E402
import features_restatement as fr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fi.cases()


# ------------------------------------------------------------------------------------------- header and table ---
def test_eleventh_header_matches_its_table_and_every_symbol_is_exported():
    from amvs import _lib
    header = open(os.path.join(ROOT, "include", "amvs_features.h")).read()
    declared = set(re.findall(r"^(?:int|const char \*)\s*(amvs_\w+)\(", header, re.M))
    assert declared == set(_lib.FEATURE_SIGNATURES) == {"amvs_clahe_u8", "amvs_sift_scale_space", "amvs_sift_fetch_level",
                                                             "amvs_sift_extract", "amvs_sift_fetch", "amvs_sift_to_slot"}
    others = [f for f in os.listdir(os.path.join(ROOT, "include")) if f != "amvs_features.h"]
    for other in others:
        assert not declared & set(re.findall(r"^(?:int|const char \*)\s*(amvs_\w+)\(", open(os.path.join(ROOT, "include", other)).read(), re.M))
    assert '#include "amvs.h"' in header
    lib = _lib.load()
    for name, (res, args) in _lib.FEATURE_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(args)
    for macro, value in (("AMVS_FEATURES_MAX_SIDE", _lib.FEATURES_MAX_SIDE), ("AMVS_CLAHE_MAX_GRID", _lib.CLAHE_MAX_GRID),
                         ("AMVS_SIFT_MIN_SIDE", _lib.SIFT_MIN_SIDE), ("AMVS_SIFT_MAX_SIGMA", _lib.SIFT_MAX_SIGMA),
                         ("AMVS_SIFT_MAX_RADIUS", _lib.SIFT_MAX_RADIUS), ("AMVS_SIFT_LAYERS", _lib.SIFT_LAYERS),
                         ("AMVS_SIFT_GAUSS", _lib.SIFT_GAUSS), ("AMVS_SIFT_DOG", _lib.SIFT_DOG),
                         ("AMVS_SIFT_MIN_SIGMA", _lib.SIFT_MIN_SIGMA), ("AMVS_SIFT_MAX_FEATURES", _lib.SIFT_MAX_FEATURES)):
        assert float(re.search(r"^#define %s (\S+)$" % macro, header, re.M).group(1)) == value
    assert (fr.LAYERS, fr.GAUSS, fr.DOG) == (_lib.SIFT_LAYERS, _lib.SIFT_GAUSS, _lib.SIFT_DOG)
    from amvs.engine import Engine
    assert callable(Engine.clahe) and callable(Engine.sift_scale_space) and callable(Engine.sift_level)
    assert callable(Engine.sift_extract) and callable(Engine.sift_to_slot)
    makefile = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", makefile, re.M).group(1).split()
    assert {"amvs_clahe.o", "amvs_sift.o", "amvs_sift_keypoints.o", "amvs_capi_features.o"} <= set(objs)
    assert "../../include/amvs_features.h" in makefile


def test_a_null_context_is_refused_first():
    from amvs import _lib
    lib = _lib.load()
    img, n = (C.c_uint8 * 64)(), C.c_int32(0)
    assert lib.amvs_clahe_u8(None, img, 8, 8, 2.0, 8, 8, img) == -1
    assert lib.amvs_clahe_u8(None, None, 0, 0, float("nan"), 0, 0, None) == -1
    assert lib.amvs_sift_scale_space(None, img, 8, 8, 1.6, C.byref(n)) == -1
    assert lib.amvs_sift_scale_space(None, None, 0, 0, -1.0, None) == -1
    assert lib.amvs_sift_fetch_level(None, 0, 0, 0, None, None, None) == -1
    assert lib.amvs_sift_extract(None, img, 8, 8, 0, 0.04, 10.0, 1.6, C.byref(n)) == -1
    assert lib.amvs_sift_extract(None, None, 0, 0, -1, float("nan"), float("inf"), 0.0, None) == -1
    assert lib.amvs_sift_fetch(None, None, None, 0) == -1
    assert lib.amvs_sift_to_slot(None, 0) == -1


def test_engine_refuses_what_is_no_gray_u8_image():
    from amvs.engine import Engine
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            Engine._gray8(bad)
    from amvs import _lib
    from amvs.core.features import FeatureExtractor
    wide = np.zeros((1, _lib.FEATURES_MAX_SIDE + 1), np.uint8)           # a side above the maximum, refused before any context
    bare = object.__new__(Engine)                                        # no context: the refusal comes before one is touched
    for call in (lambda: Engine._gray8(wide), lambda: Engine._gray8(wide.T), lambda: FeatureExtractor().extract(wide),
                 lambda: FeatureExtractor().extract(np.zeros(wide.T.shape + (3,), np.uint8)),
                 lambda: bare.sift_extract(wide), lambda: bare.clahe(wide), lambda: bare.sift_scale_space(wide)):
        with pytest.raises(ValueError, match="AMVS_FEATURES_MAX_SIDE"):
            call()
    assert Engine._gray8(wide[:, :-1]).shape == (1, _lib.FEATURES_MAX_SIDE)


# -------------------------------------------------------------------------------------------- the definition ---
def test_fold_reflects_as_often_as_needed():
    assert fr.fold(np.arange(-5, 8), 3).tolist() == [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]
    assert fr.fold(np.arange(-3, 4), 1).tolist() == [0] * 7
    assert fr.fold(np.array([-1, 0, 5, 6, 7]), 6).tolist() == [1, 0, 5, 4, 3]
    for n in (2, 5, 6):
        i = np.arange(-40, 40)
        f = fr.fold(i, n)
        assert f.min() == 0 and f.max() == n - 1 and np.array_equal(f, fr.fold(-i, n)) and np.array_equal(f, fr.fold(i + 2 * (n - 1), n))


def test_octave_count_is_opencvs_without_a_logarithm():
    for m in range(3, 8193):
        want = int(np.rint(math.log(m) / math.log(2.0) - 2.0)) + 1
        assert fr.octaves(m, m + 3) == fr.octaves(m + 7, m) == want, m
    assert [fr.octaves(m, 100) for m in (24, 45, 46, 64)] == [4, 4, 5, 5]


def test_own_exp_against_numpy():
    """Measured here: the largest relative error of exp64 over -40 .. 0 is below 2.3e-16 (one unit in the last place);
    asserted at twice that."""
    x = -np.concatenate([np.linspace(0.0, 40.0, 200001), np.random.RandomState(0).uniform(0, 40, 100000)])
    got = np.array([fr.exp64(float(v)) for v in x])
    rel = np.abs(got - np.exp(x)) / np.exp(x)
    print(f"exp64: largest relative error {rel.max():.3e}")
    assert rel.max() <= 4.6e-16


@pytest.mark.parametrize("sigma", [1.6, 1.4, 4.0, 0.3])
def test_sigmas_and_taps(sigma):
    s = fr.sigmas(sigma)
    assert len(s) == 6
    total = sigma
    for i in range(1, 6):                   # s_i takes the blur from sigma k^(i-1) to sigma k^i
        assert math.isclose(math.hypot(total, s[i]), sigma * 2.0 ** (i / 3.0), rel_tol=1e-12)
        total = sigma * 2.0 ** (i / 3.0)
    assert math.isclose(s[0], math.sqrt(max(sigma * sigma - 1.0, 0.01)))
    for v in s:
        t = fr.taps(v)
        r = (len(t) - 1) // 2
        assert t.dtype == np.float32 and len(t) % 2 == 1 and r <= 32 and len(t) == (int(np.rint(8 * v + 1)) | 1)
        assert np.array_equal(t, t[::-1]) and abs(float(t.astype(np.float64).sum()) - 1.0) < 1e-6
        want = np.exp(-(np.arange(-r, r + 1) ** 2) / (2 * v * v))
        assert np.allclose(t, want / want.sum(), rtol=1e-6, atol=0)


def test_array_blur_equals_the_loops_bit_for_bit():
    rng = np.random.RandomState(3)
    for shape, s in (((9, 13), 1.2), ((5, 4), 3.0), ((1, 7), 1.0), ((6, 1), 2.0)):
        img = rng.uniform(0, 255, shape).astype(np.float32)
        tap = fr.taps(s)
        assert (len(tap) - 1) // 2 > min(shape) or shape == (9, 13)
        assert np.array_equal(fr.blur(img, tap), fr.blur_loops(img, tap))


def test_the_levels_have_the_sigmas_a_scale_space_must_have():
    """An impulse through the chain of blurs: after the base blur and i incremental ones its variance is
    (sigma k^i)^2 - 1 along both axes (the doubled input is taken to have blur 1), within 2 % (the taps end at 4 sigma)."""
    sigma, n = 1.6, 161
    tp = [fr.taps(s) for s in fr.sigmas(sigma)]
    img = np.zeros((n, n), np.float32)
    img[n // 2, n // 2] = 1.0
    d = (np.arange(n) - n // 2).astype(np.float64)
    for i in range(6):
        img = fr.blur(img, tp[i])
        p = img.astype(np.float64)
        assert abs(p.sum() - 1.0) < 1e-5
        want = (sigma * 2.0 ** (i / 3.0)) ** 2 - 1.0
        for var in ((p.sum(0) * d * d).sum(), (p.sum(1) * d * d).sum()):
            assert abs(var - want) <= 0.02 * want, (i, var, want)


def test_upsampling_is_the_linear_resize():
    g = fi.texture(5, 6, 9)
    u = fr.upsample(g)
    assert u.shape == (10, 12) and u.dtype == np.float32
    assert u[0, 0] == g[0, 0] and u[-1, -1] == g[-1, -1]              # replicated border: 0.75 v + 0.25 v
    ramp = (10 * np.arange(6))[None, :].repeat(5, 0).astype(np.uint8)
    assert np.array_equal(fr.upsample(ramp)[0, 1:-1], 10 * (np.arange(1, 11) / 2.0 - 0.25).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the inputs ---
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_scale_space_of_the_family(case):
    h, w = case.gray.shape
    gauss, dog = fi.restated_space(case, 1.6)
    assert len(gauss) == len(dog) == fr.octaves(h, w)
    hh, ww = 2 * h, 2 * w
    for o in range(len(gauss)):
        assert len(gauss[o]) == 6 and len(dog[o]) == 5
        assert all(a.shape == (hh, ww) and a.dtype == np.float32 for a in gauss[o] + dog[o])
        if o:
            assert np.array_equal(gauss[o][0], gauss[o - 1][3][:2 * hh:2, :2 * ww:2])
        hh, ww = hh // 2, ww // 2
    if case.name.startswith("constant"):
        assert all(np.abs(a - 77.0).max() < 1e-3 for o in gauss for a in o) and all(np.abs(a).max() < 1e-3 for o in dog for a in o)
    else:
        assert max(np.abs(a).max() for a in dog[0]) > 1.0


def test_family_reaches_its_edges():
    by = {c.name.split(" (")[0]: c.gray.shape for c in CASES}
    assert fr.octaves(*by["texture 45x50"]) + 1 == fr.octaves(*by["texture 46x50"]) == 5
    h, w = by["texture 24x24"]
    sides = [2 * h >> o for o in range(fr.octaves(h, w))]
    assert sides[-1] < (len(fr.taps(fr.sigmas(1.6)[5])) - 1) // 2, "no octave narrower than the largest radius"
    assert by["texture 47x61"][0] % 2 and by["texture 47x61"][1] % 2
    assert 2 * by["texture 70x150"][1] > 256 and 2 * by["texture 70x150"][0] > 128          # more than one tile each way
    assert all(s % 8 for s in by["texture 53x37"])


@pytest.mark.parametrize("clip,grid", fi.CLAHE_PARAMS)
def test_clahe_of_the_family(clip, grid):
    seen = {"clipped_tiles": 0, "residual_tiles": 0, "unclipped_tiles": 0}
    for case in CASES:
        out, counters = fi.restated_clahe(case, clip, grid)
        assert out.shape == case.gray.shape and out.dtype == np.uint8
        for k in seen:
            seen[k] += counters[k]
        if case.name.startswith("constant") and fr.clahe_limit(clip, 1 << 20) == 0:
            assert (out == 255).all()         # every pixel at the top of its tile's cumulative sum
    if clip in (2.0, 3.0):
        assert seen["clipped_tiles"] and seen["residual_tiles"]
    if clip == 40.0:
        assert seen["unclipped_tiles"], "no tile under the limit"
    if clip in (0.0, 300.0):
        assert not any(seen.values())


def test_clahe_limit_and_redistribution_by_hand():
    assert fr.clahe_limit(2.0, 48) == 1 and fr.clahe_limit(2.0, 8 * 8 * 64) == 32 and fr.clahe_limit(0.0, 48) == 0
    assert fr.clahe_limit(256.0, 48) == 0 and fr.clahe_limit(255.0, 48) == 47
    # one tile, every pixel 77, area 48, limit 1: excess 47, batch 0, step 256 // 47 = 5: bins 0, 5 .. 230 get one each
    lut, tw, th, counters = fr.clahe_luts(np.full((6, 8), 77, np.uint8), 2.0, 1, 1)
    assert (tw, th) == (8, 6) and counters["residual_tiles"] == 1
    hist = np.zeros(256, np.int64)
    hist[77] = 1
    hist[np.arange(47) * 5] += 1
    want = np.minimum(255, np.rint(np.cumsum(hist).astype(np.float32) * (np.float32(255) / np.float32(48))))
    assert np.array_equal(lut[0, 0], want.astype(np.uint8)) and lut[0, 0, 255] == 255


def test_clahe_flattens_a_skewed_histogram():
    """What CLAHE is for: a dark, low-contrast image comes out with a wider spread of values."""
    g = (fi.texture(64, 64, 11).astype(np.float64) / 255.0 * 40 + 10).astype(np.uint8)
    out = fr.clahe(g, 2.0, 8, 8)
    assert out.std() > 1.5 * g.std() and int(out.max()) - int(out.min()) > int(g.max()) - int(g.min())


# ------------------------------------------------------------------------------- the keypoint stages' functions ---
def test_own_expf_against_numpy():
    """Measured here: the largest relative error of expf over -80 .. 80 is 2.5e-7 (two units in the last place);
    asserted at twice that."""
    x = np.concatenate([np.linspace(-80.0, 80.0, 400001), np.random.RandomState(1).uniform(-12, 2, 200000)]).astype(np.float32)
    rel = np.abs(fr.expf(x).astype(np.float64) / np.exp(x.astype(np.float64)) - 1.0)
    print(f"expf: largest relative error {rel.max():.3e}")
    assert rel.max() <= 5.0e-7
    assert fr.expf(np.float32(-80.5)) == 0 and fr.expf(np.float32(0)) == 1


def test_own_atan2_against_numpy():
    """Measured here: the largest error of atan2deg over the whole circle and over magnitudes from 1e-3 to 400 is
    1.17e-4 degrees (the polynomial's 2e-6 radians); asserted at twice that."""
    rng = np.random.RandomState(2)
    ang = np.concatenate([np.linspace(0, 2 * np.pi, 400001), rng.uniform(0, 2 * np.pi, 200000)])
    mag = np.concatenate([np.ones(400001), 10.0 ** rng.uniform(-3, 2.6, 200000)])
    y, x = (mag * np.sin(ang)).astype(np.float32), (mag * np.cos(ang)).astype(np.float32)
    want = np.degrees(np.arctan2(y.astype(np.float64), x.astype(np.float64))) % 360.0
    err = np.abs(fr.atan2deg(y, x).astype(np.float64) - want)
    err = np.minimum(err, 360.0 - err)
    print(f"atan2deg: largest error {err.max():.3e} degrees")
    assert err.max() <= 2.34e-4
    f = np.float32
    assert [float(fr.atan2deg(f(a), f(b))) for a, b in ((0, 0), (0, 1), (1, 0), (0, -1), (-1, 0))] == [0, 0, 90, 180, 270]


def test_own_sincos_against_numpy():
    """Measured here: the largest error of sincosdeg over 0 .. 360 is 1.92e-7; asserted at twice that."""
    a = np.linspace(0, 360, 72001)[:-1].astype(np.float32)
    got = np.array([fr.sincosdeg(v) for v in a], np.float64)
    err = max(np.abs(got[:, 0] - np.sin(np.radians(a.astype(np.float64)))).max(), np.abs(got[:, 1] - np.cos(np.radians(a.astype(np.float64)))).max())
    print(f"sincosdeg: largest error {err:.3e}")
    assert err <= 3.84e-7


# ------------------------------------------------------------------------------------------- the extractor ---
def test_it_is_sift():
    """A 128 x 128 texture and the same texture rotated by 30 degrees and magnified 1.4 times, both rendered from the
    texture function: ratio test 0.8 and cross check give at least 50 matches, at least 90 % within 3 pixels of the map."""
    import match_restatement as mr
    a, b, to_b = fi.rotated_pair()
    ka, da = fr.extract(a, 0, 0.03, 15.0, 1.6)
    kb, db = fr.extract(b, 0, 0.03, 15.0, 1.6)
    qi, ti, _ = mr.match(da, db, 0.8, cross_check=True)
    err = np.linalg.norm(to_b(ka[qi, :2]) - kb[ti, :2], axis=1)
    print(f"it is SIFT: {len(ka)} and {len(kb)} keypoints, {len(qi)} matches, {(err < 3).mean():.3f} within 3 px")
    assert len(qi) >= 50 and (err < 3).mean() >= 0.9


def test_flat_images_have_no_keypoints():
    for case in CASES:
        if case.name.startswith(("constant", "step edge", "sliver")):
            for params in fi.EXTRACT_PARAMS:
                kps, desc, _ = fi.restated_extract(case, params)
                assert kps.shape == (0, 6) and kps.dtype == np.float32 and desc.shape == (0, 128) and desc.dtype == np.uint8


def test_keypoint_inputs_reach_their_edges():
    by = {c.name.split(" (")[0] + ("/1" if "octave 1" in c.name else ""): c for c in CASES}
    pre = fr.pre_threshold(0.04)
    for name, o in (("planted 44x52", 0), ("planted 44x52/1", 1)):
        dog = fi.restated_space(by[name], 1.6)[1][o]
        h, w = dog[0].shape
        cand = fr.candidates(dog, pre)
        for d in (5, 6):                    # a candidate exactly d pixels from each of the four borders
            assert any(r == d for _, r, c in cand) and any(r == h - 1 - d for _, r, c in cand), (name, d)
            assert any(c == d for _, r, c in cand) and any(c == w - 1 - d for _, r, c in cand), (name, d)
        assert not any(min(r, c, h - 1 - r, w - 1 - c) < 5 for _, r, c in cand)
    assert len(fi.restated_extract(by["planted 44x52/1"], fi.EXTRACT_PARAMS[0])[0]) > 0
    # ties, and n_features cutting through one
    lattice = by["lattice 96x96"]
    kps, desc, _ = fi.restated_extract(lattice, fi.EXTRACT_PARAMS[0])
    n = fi.tie_cut(lattice)
    resp = np.sort(kps[:, 4])[::-1]
    assert 0 < n < len(kps) and resp[n - 1] == resp[n]
    cut, cut_desc = fr.extract(lattice.gray, n, *fi.EXTRACT_PARAMS[0][1:])
    keep = [j for j in range(len(kps)) if kps[j, 4] > resp[n]]
    keep += [j for j in range(len(kps)) if kps[j, 4] == resp[n]][:n - len(keep)]      # of the tie, the first in canonical order
    assert np.array_equal(cut, kps[sorted(keep)]) and np.array_equal(cut_desc, desc[sorted(keep)])
    # two or more orientations on one keypoint
    _, _, stages = fi.restated_extract(by["blob between bars 48x48"], fi.EXTRACT_PARAMS[0])
    per = {}
    for k in stages["oriented"]:
        per[k["key"][:4]] = per.get(k["key"][:4], 0) + 1
    assert max(per.values()) >= 2
    # the canonical order: keys ascend strictly
    keys = [k["key"] for k in stages["oriented"]]
    assert keys == sorted(set(keys))


def test_descriptors_are_what_the_matcher_takes():
    from amvs.core.dense import descriptors_u8
    kps, desc, stages = fi.restated_extract(CASES[0], fi.EXTRACT_PARAMS[0])
    assert len(kps) > 10 and descriptors_u8(desc) is not None and desc.max() <= 255 and desc.max() > 100
    assert (kps[:, 0] >= 0).all() and (kps[:, 0] < CASES[0].gray.shape[1]).all() and (kps[:, 3] >= 0).all() and (kps[:, 3] < 360).all()
    assert (kps[:, 4] * 3 >= np.float32(0.04)).all() and stages["n_candidates"] >= stages["n_refined"] > 0


# ------------------------------------------------------------------------------------------ the second family ---
# The conditions tests/test_hip_features_scale.py relies on, with the restatement alone.  The counts in the docstrings were
# measured with it; the assertions are the conditions, not the counts.
def _oriented(name):
    case, params = fi.scale_cases()[name]
    kps, desc, stages = fi.restated_extract(case, params)
    return case, params, kps, desc, stages


def _orientations_per_keypoint(stages):
    per = {}
    for k in stages["oriented"]:
        per[k["key"][:4]] = per.get(k["key"][:4], 0) + 1
    return per


@pytest.mark.parametrize("name,layers", [("wrap", (3,)), ("wrap, mid-layer", (2, 3))])
def test_wrap_inputs_have_keypoints_beyond_the_first_pass(name, layers):
    """One pass of the extrema search takes 8192 * 256 interior pixels, in (layer, row, column) order.
    520 x 520: octave 0 has 3 * 1030 * 1030 of them; 4446 candidates, 2462 keypoints, 406 of octave 0 from a candidate
    beyond the first pass, all of layer 3: the pass ends at row 1006 of the 1030 of layer 2, and no keypoint starts
    in those last rows (the texture's periods are 14 pixels and more there, layers 1 and 2 are nearly empty).
    520 x 700, with a blob planted on the last pixel of the first pass: the pass ends at row 478 of layer 2; 5968
    candidates, 3304 keypoints, 548 beyond the first pass, 1 of layer 2 and 547 of layer 3, and a keypoint that starts
    at index 8192 * 256 - 1."""
    case, _, kps, _, stages = _oriented(name)
    h, w = 2 * case.gray.shape[0], 2 * case.gray.shape[1]
    assert 3 * (h - 10) * (w - 10) > fi.EXTREMA_PASS > (h - 10) * (w - 10)
    late = [k["cand"][0] for k in stages["oriented"] if k["o"] == 0 and fi.extrema_index(k["cand"], h, w) >= fi.EXTREMA_PASS]
    print(f"{case.name}: {stages['n_candidates']} candidates, {len(kps)} keypoints, {len(late)} beyond the first pass, by layer "
          f"{[late.count(i) for i in (1, 2, 3)]}")
    assert len(late) >= 50 and all(i in late for i in layers)
    if name == "wrap, mid-layer":
        # a stride of gridDim.x * 256 - 1 visits every pixel, and pixel k (stride) a second time: only a keypoint that starts
        # exactly there shows it (as a keypoint too many).  The planted blob's does.
        seam = fi.seam_pixel(*case.gray.shape)
        assert fi.extrema_index(seam, h, w) == fi.EXTREMA_PASS - 1 and seam[0] == 2
        assert any(k["o"] == 0 and k["cand"] == seam for k in stages["oriented"])


def test_candidates_input_overflows_the_first_array():
    """220 x 220 blobs in noise: 24 611 candidates against the 16 384 the first array holds, 9 refined, 27 keypoints.
    By octave the candidates are 13 596, 8 399, 2 140, 420, 53, 3 and 0, and every keypoint lies in octaves 2 to 4.  The
    octaves are searched one after the other on one stream, so the hits of octaves 0 and 1 fill an array of 16 384 before
    any other arrives: a search that dropped what does not fit would lose every keypoint, whatever the atomics' order."""
    case, params, kps, _, stages = _oriented("candidates")
    print(f"{stages['n_candidates']} candidates, {stages['n_refined']} refined, {len(kps)} keypoints")
    assert fr.pre_threshold(params[1]) == 0
    assert stages["n_candidates"] > 16384 and stages["n_candidates"] >= 20000 and len(kps) > 0
    per_octave = [len(fr.candidates(d, fr.pre_threshold(params[1]))) for d in fi.restated_space(case, params[3])[1]]
    first = min(k["o"] for k in stages["oriented"])
    assert sum(per_octave) == stages["n_candidates"] and sum(per_octave[:first]) > 16384


def test_crowd_input_ties_and_its_cuts():
    """150 x 150 noise: 11 130 candidates, 7 724 refined, 10 594 keypoints with 7 707 distinct responses, up to 6
    orientations on one keypoint.  The cut at 3000 falls between two responses; the tie cut is 6008.  Both equal
    the rule by hand: the strictly stronger keypoints, then the first of the tie in canonical order."""
    case, params, kps, desc, stages = _oriented("crowd")
    resp = np.sort(kps[:, 4])[::-1]
    n_tie = fi.tie_cut_near(kps, 6000)
    print(f"{stages['n_candidates']} candidates, {stages['n_refined']} refined, {len(kps)} keypoints, {len(np.unique(resp))} distinct responses, "
          f"tie cut at {n_tie}")
    assert len(kps) > 8192 and len(np.unique(resp)) < len(kps) * 0.8
    assert fi.CUT < n_tie < len(kps) and resp[n_tie - 1] == resp[n_tie]
    keys = [k["key"] for k in stages["oriented"]]
    assert keys == sorted(set(keys))
    for n in (fi.CUT, n_tie):
        cut, cut_desc, _ = fi.restated_extract(case, (n,) + params[1:])
        want, want_desc = fi.cut_by_hand(kps, desc, n)
        assert len(cut) == n and np.array_equal(cut, want) and np.array_equal(cut_desc, want_desc)


def test_sigma_ends_reach_their_windows():
    """70 x 150 texture at sigma 4: 73 candidates, 78 keypoints, orientation radius 20 .. 37, descriptor radius 48 .. 88,
    up to 3 orientations.  60 x 60 noise at sigma 0.3: 77 candidates, 66 keypoints, orientation radius 2 .. 3, up to 4
    orientations (25 to 49 samples a histogram).  150 x 150 noise at sigma 0.5: orientation radius 3 .. 5, up to 6
    orientations.  The 70 x 150 texture at sigma 0.5, an ordinary image under the crowded images' parameters: 38 keypoints,
    orientation radius 3 .. 5, up to 3 orientations.  Radius 2 needs sigma below 0.5: a refined scale is at least
    sigma 2^(0.5 / 3), and rint(4.5 * 0.5 * 1.1225) is 3; so radius 2 is asked of the sigma 0.3 input alone, radius 3 of
    the two at 0.5.  At sigma 0.1 the outer taps are 1e-37 to 1.5e-6, the differences vanish: no candidate."""
    def radii(stages):
        return [int(np.rint(np.float32(4.5) * k["scl"])) for k in stages["oriented"]], [fi.descriptor_radius(k["scl"]) for k in stages["oriented"]]

    _, _, kps, _, stages = _oriented("wide")
    ori, desc = radii(stages)
    print(f"sigma 4: {len(kps)} keypoints, orientation radius {min(ori)} .. {max(ori)}, descriptor radius {min(desc)} .. {max(desc)}")
    assert max(ori) >= 30 and max(desc) >= 64 and (2 * max(ori) + 1) ** 2 > 3600
    for name, reach in (("fine", 2), ("crowd", 3), ("busy", 3)):
        _, _, kps, _, stages = _oriented(name)
        ori, _ = radii(stages)
        most = max(_orientations_per_keypoint(stages).values())
        print(f"{name}: {len(kps)} keypoints, orientation radius {min(ori)} .. {max(ori)}, up to {most} orientations")
        assert len(kps) > 10 and min(ori) <= reach and most >= 3
    kps, desc, stages = fi.restated_extract(fi.SPACE_CASE, (0, 0.04, 10.0, 0.1))
    assert stages["n_candidates"] == 0 and kps.shape == (0, 6) and kps.dtype == np.float32 and desc.shape == (0, 128) and desc.dtype == np.uint8


def test_space_input_spans_tiles_at_both_ends_of_sigma():
    """70 x 300: octave 0 is 140 x 600, three 256-column tiles of the row pass, ten by three 64 x 64 tiles of the column
    pass.  Radii at sigma 4: 16, 13, 16, 20, 25, 31; at sigma 0.5: 1, 2, 2, 3, 3, 4; at sigma 0.1: 1 six times."""
    radii = {s: [(len(fr.taps(v)) - 1) // 2 for v in fr.sigmas(s)] for s in fi.SPACE_SIGMAS}
    print(radii)
    assert radii[4.0][-1] == 31 and max(radii[0.5]) <= 4 and radii[0.1] == [1] * 6
    gauss, dog = fi.restated_space(fi.SPACE_CASE, 4.0)
    h, w = gauss[0][0].shape
    assert w > 512 and h > 128 and len(gauss) == fr.octaves(*fi.SPACE_CASE.gray.shape)
    for s in fi.SPACE_SIGMAS:                              # the levels are images, not a constant: the blur has something to get wrong
        gauss, dog = fi.restated_space(fi.SPACE_CASE, s)
        assert all(a.max() - a.min() > 10 for a in gauss[0])
        top = max(np.abs(a).max() for a in dog[0])
        assert top < 1e-3 if s == 0.1 else top > 0.01        # outer taps of 1e-37 to 1.5e-6: the levels differ in the last place at most


def test_clip_search_and_its_frozen_case():
    """The bounded search of features_inputs.clip_recipes() (360 off-centre blobs of sigma 4 to 8 on 12 side pairs up to
    40 x 40, then 200 textures) finds its first input at recipe 19, in 0.3 s: a dark blob of sigma 7 on 14 x 30, whose
    one keypoint lies in octave 1 (14 x 30, rows + columns 44) with scale 4.84 and descriptor radius 51."""
    found = fi.clip_search(limit=40)
    assert found is not None and found[0] == fi.CLIP_RECIPE and fi.clip_recipes().index(fi.CLIP_RECIPE) < 40
    case, params, kps, _, stages = _oriented("clip")
    assert max(case.gray.shape) <= 40 and 3.0 <= params[3] <= 4.0 and params[1:3] == (0.005, 50.0)
    hits = [k for k in stages["oriented"]
            if int(np.rint(np.float32(3) * k["scl"] * np.float32(1.4142135) * np.float32(2.5))) > sum(dim >> k["o"] for dim in (2 * case.gray.shape[0], 2 * case.gray.shape[1]))]
    print(f"{len(kps)} keypoints, {len(hits)} clipped: {[(k['o'], k['i'], float(k['scl'])) for k in hits]}")
    assert len(hits) >= 1


# ---------------------------------------------------------------------------------------------- the classes ---
def test_feature_extractor_arguments():
    from amvs.core.features import FeatureExtractor, ImageFeatures, SiftFeatures
    import amvs
    assert amvs.FeatureExtractor is FeatureExtractor
    ex = FeatureExtractor()
    assert (ex.n_features, ex.contrast_threshold, ex.edge_threshold, ex.sigma, ex.clahe_clip, ex.clahe_grid) == (10000, 0.03, 15.0, 1.6, 2.0, (8, 8))
    for bad in (dict(n_features=-1), dict(contrast_threshold=float("nan")), dict(contrast_threshold=-0.1), dict(edge_threshold=float("inf")),
                dict(edge_threshold=0), dict(sigma=0), dict(sigma=-1.6), dict(sigma=float("nan")), dict(clahe_grid=(0, 8)),
                dict(clahe_grid=(8, 0)), dict(clahe_clip=float("nan"))):
        with pytest.raises(ValueError):
            FeatureExtractor(**bad)
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4, 4), np.uint8), np.zeros((4,), np.uint8)):
        with pytest.raises(ValueError):
            ex.gray(bad)
    from amvs.core.imageprep import _bgr_to_gray_u8
    bgr = np.random.RandomState(0).randint(0, 256, (5, 7, 3)).astype(np.uint8)
    assert np.array_equal(ex.gray(bgr), _bgr_to_gray_u8(bgr)) and np.array_equal(ex.gray(bgr[:, :, 0]), bgr[:, :, 0])
    f = SiftFeatures(np.zeros((2, 2), np.float32), np.zeros((2, 128), np.uint8), (4, 4), sizes=np.ones(2))
    assert isinstance(f, ImageFeatures) and len(f) == 2 and f.points.shape == (2, 2)
    assert [x.name for x in __import__("dataclasses").fields(ImageFeatures)] == ["keypoints", "descriptors", "image_shape"]


def test_reconstruct_without_cv2_and_without_an_extractor_raises_as_before():
    try:
        import cv2  # noqa: F401
        pytest.skip("cv2 is installed")
    except ImportError:
        pass
    import amvs
    cam = amvs.Camera(K=np.eye(3), dist=np.zeros(5))
    with pytest.raises(RuntimeError, match="reconstruct_from_features"):
        amvs.SfMPipeline(cam).reconstruct("nowhere")
    with pytest.raises(ImportError, match="reconstruct_from_features"):
        amvs.DenseReconstructor(cam).reconstruct([], {})
    with pytest.raises(ValueError, match="at least 2"):
        amvs.SfMPipeline(cam).reconstruct_images([np.zeros((8, 8), np.uint8)])
