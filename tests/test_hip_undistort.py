"""The lens undistortion on the device (csrc/amvs_undistort.hip and its entry points in csrc/amvs_capi.hip, declared in
include/amvs_lens.h) against the restatement of tests/undistort_restatement.py on the input family of
tests/undistort_inputs.py; tests/test_undistort_cpu.py shows on the CPU that the restatement's two forms agree, that the
family reaches every edge and that the definition stays within an analytic bound.  Every comparison is byte for byte."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import undistort_inputs as ui  # noqa: E402
import undistort_restatement as ur  # noqa: E402

pytestmark = pytest.mark.gpu

EYE = np.eye(3)


@pytest.fixture(scope="module")
def amvs_mod():
    import amvs
    return amvs


_RESTATED = {}


def restated(case):
    """(image, n_outside) of the case: the small ones by the loops, the large one by the vectorised form (the CPU test
    holds it to the loops)."""
    if case.name not in _RESTATED:
        _RESTATED[case.name] = (ur.undistort_np if case.big else ur.undistort)(case.src, case.K, case.dist)[:2]
    return _RESTATED[case.name]


def _same_image(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} bytes differ, first at {bad[0]}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def _bits_eq(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    diff = a.view(np.uint32) != b.view(np.uint32)
    assert a.shape == b.shape and not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} elements differ in their bits"


def pinhole(H, W):
    f = 0.8 * max(H, W)
    return np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]], np.float32)


def shift(i):
    return np.array([0.05 * i, 0.0, 0.0])


# ------------------------------------------------------------------------------------------ amvs_undistort_bgr8 ---
@pytest.fixture(scope="module")
def any_engine(amvs_mod):
    """A context of some size: the stand-alone call touches none of its views."""
    with amvs_mod.Engine(8, 8, 1, pinhole(8, 8)) as eng:
        yield eng


@pytest.mark.parametrize("case", ui.family(), ids=lambda c: c.name)
def test_stand_alone_call_equals_the_restatement(any_engine, case):
    want, want_outside = restated(case)
    got, n_outside = any_engine.undistort_bgr8(case.src, case.K, case.dist)
    _same_image(got, want, case.name)
    assert n_outside == want_outside
    if case.identity:
        _same_image(got, case.src, case.name + ": identity")


def test_one_context_reused_across_sizes(amvs_mod):
    """Ascending then descending sizes through one context (the staging blocks are regrown between them): each result
    equals a fresh context's and the restatement."""
    K = pinhole(8, 8)
    cases = sorted((c for c in ui.small_family()), key=lambda c: c.src.size)
    order = cases + cases[-2::-1]
    fresh = {}
    for c in cases:
        with amvs_mod.Engine(8, 8, 1, K) as eng:
            fresh[c.name] = eng.undistort_bgr8(c.src, c.K, c.dist)
            _same_image(fresh[c.name][0], restated(c)[0], f"fresh context, {c.name}")
            assert fresh[c.name][1] == restated(c)[1]
    with amvs_mod.Engine(8, 8, 1, K) as eng:
        for c in order:
            got, n_outside = eng.undistort_bgr8(c.src, c.K, c.dist)
            _same_image(got, fresh[c.name][0], f"reused context, {c.name}")
            assert n_outside == fresh[c.name][1]


# ------------------------------------------------------------------------------- amvs_set_view_bgr8_undistorted ---
@pytest.mark.parametrize("dst", [(24, 32), (48, 64)], ids=["half", "scale1"])
def test_undistorting_upload_equals_the_upload_of_the_restated_image(amvs_mod, dst):
    """The four 48 x 64 models as the views of two contexts: uploaded raw through the undistorting entry point, and
    undistorted by the restatement and uploaded through amvs_set_view_bgr8.  The returned colour images, the window
    statistics of every view and a cost map across three views agree.  At 48 x 64 the resize is a copy."""
    H, W = dst
    K = pinhole(H, W)
    cases = ui.model_cases()
    n = len(cases)
    with amvs_mod.Engine(H, W, n, K) as dev, amvs_mod.Engine(H, W, n, K) as host, amvs_mod.Engine(H, W, n, K) as bare:
        for i, c in enumerate(cases):
            color = dev.set_view_bgr8_undistorted(i, c.src, c.K, c.dist, EYE, shift(i))
            want = host.set_view_bgr8(i, restated(c)[0], EYE, shift(i))
            _same_image(color, want, f"{c.name} -> {H} x {W}: colour image")
            if (H, W) == c.shape:
                _same_image(color, restated(c)[0], f"{c.name}: the copy")
            assert bare.set_view_bgr8_undistorted(i, c.src, c.K, c.dist, EYE, shift(i), want_color=False) is None
        assert dev.sampling_mode() == host.sampling_mode() == bare.sampling_mode() == "u8-pairs"
        for i, c in enumerate(cases):
            mh, vh = host.box_stats(i, 3)
            for eng, name in ((dev, "undistorting upload"), (bare, "undistorting upload without the colour image")):
                m, v = eng.box_stats(i, 3)
                _bits_eq(m, mh, f"{c.name} {name}: mean")
                _bits_eq(v, vh, f"{c.name} {name}: variance")
        d = np.full((H, W), 5.0, np.float32)
        ch = host.eval_cost(0, [1, 2], 5, d)
        assert np.isfinite(ch).any()
        for eng in (dev, bare):
            got = eng.eval_cost(0, [1, 2], 5, d)
            assert np.array_equal(got, ch, equal_nan=True)


def test_existing_entry_point_is_unchanged_after_an_undistorting_upload(amvs_mod):
    H, W = 24, 32
    K = pinhole(H, W)
    c = ui.model_cases()[1]
    other = ui.content(40, 72, 77)
    with amvs_mod.Engine(H, W, 1, K) as fresh:
        want = fresh.set_view_bgr8(0, other, EYE, shift(0))
        want_stats = fresh.box_stats(0, 3)
    with amvs_mod.Engine(H, W, 1, K) as eng:
        eng.set_view_bgr8_undistorted(0, c.src, c.K, c.dist, EYE, shift(0))
        _same_image(eng.set_view_bgr8(0, other, EYE, shift(0)), want, "set_view_bgr8 after the undistorting upload")
        m, v = eng.box_stats(0, 3)
        _bits_eq(m, want_stats[0], "mean")
        _bits_eq(v, want_stats[1], "variance")


# ------------------------------------------------------------------------------------------------------- errors ---
def _bad_lenses():
    """(what, K (9,), dist, n_dist) of every lens the header refuses; None = a NULL pointer."""
    K = np.array([20.0, 0, 2.0, 0, 21.0, 1.0, 0, 0, 1.0])
    d = np.array(ui.RATIONAL)
    out = [("NULL K", None, d, 8), ("NULL dist", K, None, 5)]
    out += [(f"n_dist = {n}", K, d, n) for n in (-1, 0, 3, 6, 7, 9, 14)]
    for bad in (np.nan, np.inf, -np.inf):
        for k in (0, 2, 4, 5, 1, 8):
            Kb = K.copy()
            Kb[k] = bad
            out.append((f"K[{k}] = {bad}", Kb, d, 8))
        for k in (0, 3, 7):
            db = d.copy()
            db[k] = bad
            out.append((f"dist[{k}] = {bad}", K, db, 8))
    for k, v in ((0, 0.0), (0, -20.0), (4, 0.0), (4, -1.0), (1, 1e-9), (3, -1.0), (6, 1e-300), (7, 0.5), (8, 2.0), (8, 0.0)):
        Kb = K.copy()
        Kb[k] = v
        out.append((f"K[{k}] = {v}", Kb, d, 8))
    return out


def test_errors_are_refused_and_leave_the_context_usable(amvs_mod):
    f64p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    H, W = 24, 32
    good = ui.model_cases()[2]
    img = np.ascontiguousarray(ui.content(3, 5, 5))
    out = np.empty_like(img)
    scaled = np.empty((H, W, 3), np.uint8)
    R = np.eye(3, dtype=np.float32)
    t = np.zeros(3, np.float32)
    f32p = C.POINTER(C.c_float)
    n_out = C.c_int64(-7)

    def ptr(a, kind):
        return None if a is None else np.ascontiguousarray(a).ctypes.data_as(kind)

    with amvs_mod.Engine(H, W, 2, pinhole(H, W)) as eng:
        lib, h = eng._lib, eng._h
        want_image = eng.undistort_bgr8(good.src, good.K, good.dist)
        want_view = eng.set_view_bgr8_undistorted(1, good.src, good.K, good.dist, EYE, shift(1))
        want_stats = eng.box_stats(1, 3)

        def still_usable(what):
            assert "" != lib.amvs_last_error(h).decode(), what
            got = eng.undistort_bgr8(good.src, good.K, good.dist)
            assert np.array_equal(got[0], want_image[0]) and got[1] == want_image[1], what
            _same_image(eng.set_view_bgr8_undistorted(1, good.src, good.K, good.dist, EYE, shift(1)), want_view, what)

        Kg, dg = np.ascontiguousarray(good.K.reshape(9)), np.array(ui.RATIONAL)
        calls = []
        for what, K, d, n in _bad_lenses():
            Kc = None if K is None else np.ascontiguousarray(K, np.float64)
            dc = None if d is None else np.ascontiguousarray(d, np.float64)
            calls.append((what, lambda Kc=Kc, dc=dc, n=n: lib.amvs_undistort_bgr8(h, ptr(img, u8p), 3, 5, ptr(Kc, f64p), ptr(dc, f64p), n,
                                                                                  ptr(out, u8p), C.byref(n_out)),
                          lambda Kc=Kc, dc=dc, n=n: lib.amvs_set_view_bgr8_undistorted(h, 0, ptr(img, u8p), 3, 5, ptr(Kc, f64p), ptr(dc, f64p),
                                                                                       n, ptr(R, f32p), ptr(t, f32p), ptr(scaled, u8p))))
        for hh, ww in ((0, 5), (3, 0), (-1, 5), (3, -2), ((1 << 24) + 1, 1), (1, (1 << 24) + 1)):
            calls.append((f"size {hh} x {ww}",
                          lambda hh=hh, ww=ww: lib.amvs_undistort_bgr8(h, ptr(img, u8p), hh, ww, ptr(Kg, f64p), ptr(dg, f64p), 8,
                                                                       ptr(out, u8p), None),
                          lambda hh=hh, ww=ww: lib.amvs_set_view_bgr8_undistorted(h, 0, ptr(img, u8p), hh, ww, ptr(Kg, f64p), ptr(dg, f64p), 8,
                                                                                  ptr(R, f32p), ptr(t, f32p), None)))
        calls.append(("NULL image", lambda: lib.amvs_undistort_bgr8(h, None, 3, 5, ptr(Kg, f64p), ptr(dg, f64p), 8, ptr(out, u8p), None),
                      lambda: lib.amvs_set_view_bgr8_undistorted(h, 0, None, 3, 5, ptr(Kg, f64p), ptr(dg, f64p), 8, ptr(R, f32p), ptr(t, f32p), None)))
        calls.append(("NULL output / pose", lambda: lib.amvs_undistort_bgr8(h, ptr(img, u8p), 3, 5, ptr(Kg, f64p), ptr(dg, f64p), 8, None, None),
                      lambda: lib.amvs_set_view_bgr8_undistorted(h, 0, ptr(img, u8p), 3, 5, ptr(Kg, f64p), ptr(dg, f64p), 8, None, ptr(t, f32p), None)))
        calls.append(("view out of range", None,
                      lambda: lib.amvs_set_view_bgr8_undistorted(h, 2, ptr(img, u8p), 3, 5, ptr(Kg, f64p), ptr(dg, f64p), 8, ptr(R, f32p), ptr(t, f32p), None)))
        for what, alone, upload in calls:
            for fn in (alone, upload):
                if fn is None:
                    continue
                assert fn() == -1, what
                with pytest.raises(amvs_mod.AmvsError):
                    eng._chk(fn())
            still_usable(what)
        assert n_out.value == -7, "a refused call wrote its count"
        # through the Engine methods: what Python can express raises AmvsError, the unknown model ValueError
        Kb = good.K.copy()
        Kb[0, 1] = 0.25
        with pytest.raises(amvs_mod.AmvsError, match="K must be"):
            eng.undistort_bgr8(good.src, Kb, good.dist)
        with pytest.raises(amvs_mod.AmvsError, match="positive"):
            eng.set_view_bgr8_undistorted(0, good.src, np.diag([0.0, 1.0, 1.0]), good.dist, EYE, shift(0))
        with pytest.raises(ValueError, match="thin-prism"):
            eng.undistort_bgr8(good.src, good.K, ui.RATIONAL + [0.1])
        still_usable("Engine methods")
        m, v = eng.box_stats(1, 3)
        _bits_eq(m, want_stats[0], "mean of the view uploaded before the errors")
        _bits_eq(v, want_stats[1], "variance of the view uploaded before the errors")


# --------------------------------------------------------------------------------------------------- end to end ---
@pytest.fixture(scope="module")
def lens_scene():
    """5 views of 96 x 128 for scale 0.5 as a camera with the radial + tangential model records them (the synthetic pinhole
    renders put through the lens), and every raw image undistorted by the restatement with both lenses the class test
    uses: ({"images", "poses"}, cameras, restated images)."""
    import amvs
    from amvs.engine import lens_coefficients
    from amvs.synthetic import make_scene
    sc = make_scene(5, 96, 128, seed=3)
    cams = {name: amvs.Camera(K=sc.camera.K.copy(), dist=np.asarray(d, np.float64))
            for name, d in (("first", ui.RADIAL_TANGENTIAL), ("second", ui.BARREL))}
    raw = [{"image": ui.distorted_view(c, sc.camera.K, ui.RADIAL_TANGENTIAL)} for c in sc.colors]
    restated_images = {name: [{"image": ur.undistort_np(r["image"], cam.K, lens_coefficients(cam.dist))[0]} for r in raw]
                       for name, cam in cams.items()}
    # the restated first lens brings the pinhole render back (within the two interpolations) wherever it has a source
    back, pin = restated_images["first"][2]["image"].astype(int), sc.colors[2].astype(int)
    seen = back.any(axis=2)
    assert seen.mean() > 0.8 and np.abs(back - pin)[seen].mean() < 0.6 * np.abs(raw[2]["image"].astype(int) - pin).mean()
    return {"images": raw, "poses": dict(sc.poses)}, cams, restated_images


def _same_cloud(got, want, what):
    assert len(got) == len(want) == 2
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), f"{what}: points"
    assert np.array_equal(got[1], want[1]), f"{what}: colours"


def _classes():
    from amvs.core.dense_stereo import DenseStereoReconstructor
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    return (("patchmatch", lambda cam, **kw: PatchMatchMVS(cam, scale=0.5, patch_size=7, num_iterations=3, num_samples=4, min_views=2,
                                                          seed=5, device=0, **kw)),
            ("stereo", lambda cam, **kw: DenseStereoReconstructor(cam, scale=0.5, num_depths=32, min_views=2, device=0, **kw)))


@pytest.mark.parametrize("which", [0, 1], ids=["patchmatch", "stereo"])
def test_reconstruct_from_raw_images_equals_reconstruct_from_restated_ones(amvs_mod, lens_scene, capsys, which):
    sc, cams, restated_images = lens_scene
    name, make = _classes()[which]
    images, poses = sc["images"], sc["poses"]
    on = make(cams["first"], undistort=True)
    got = on.reconstruct(images, poses)
    want = make(cams["first"], device_prep=True).reconstruct(restated_images["first"], poses)
    _same_cloud(got, want, f"{name}: undistort=True on the raw images against undistort=False on the restated ones")
    assert len(got[0]) > 0
    raw = make(cams["first"], device_prep=True).reconstruct(images, poses)
    assert raw[0].shape != got[0].shape or not np.array_equal(raw[0], got[0]), "the undistortion changed nothing"
    # another lens on the same instance: the views are uploaded again
    on.camera = cams["second"]
    again = on.reconstruct(images, poses)
    assert again[0].shape != got[0].shape or not np.array_equal(again[0], got[0])
    _same_cloud(again, make(cams["second"], undistort=True).reconstruct(images, poses), f"{name}: second lens against a fresh instance")
    _same_cloud(again, make(cams["second"], device_prep=True).reconstruct(restated_images["second"], poses), f"{name}: second lens, restated")
    capsys.readouterr()
    print(f"{name}: {len(got[0])} points from the raw images undistorted on the device, {len(raw[0])} without the undistortion, "
          f"{len(again[0])} with the second lens")
