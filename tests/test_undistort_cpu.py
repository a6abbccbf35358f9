"""The lens undistortion without a GPU: the restatement of tests/undistort_restatement.py against itself (loops against
the NumPy twin), the input family of tests/undistort_inputs.py against the edges the GPU comparison relies on, the
accuracy of the definition against an analytic ramp, and the host-only pieces of the feature (the third header and its
binding table, the coefficient handling, the undistort switch of the two classes with a fake engine).
tests/test_hip_undistort.py compares the device with the same restatement."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import undistort_inputs as ui  # noqa: E402
import undistort_restatement as ur  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_RESTATED = {}


def restated(case):
    """(image, n_outside, counters) of the case by the twin, computed once."""
    if case.name not in _RESTATED:
        _RESTATED[case.name] = ur.undistort_np(case.src, case.K, case.dist)
    return _RESTATED[case.name]


# ------------------------------------------------------------------------------------------- the restatement ---
@pytest.mark.parametrize("case", ui.small_family(), ids=lambda c: c.name)
def test_loops_and_twin_agree_byte_for_byte(case):
    want = restated(case)
    got = ur.undistort(case.src, case.K, case.dist)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]


@pytest.mark.parametrize("case", ui.small_family(), ids=lambda c: c.name)
def test_family_reaches_its_edges(case):
    out, n_outside, counters = restated(case)
    h, w = case.shape
    assert out.shape == (h, w, 3) and out.dtype == np.uint8
    if case.identity:
        assert np.array_equal(out, case.src) and n_outside == 0 and counters["fractional"] == 0
    else:
        assert counters["fractional"] > 0, "no pixel interpolates"
    assert (n_outside > 0) == case.has_outside or case.name.startswith(("strip", "tie"))
    if case.has_partial:
        assert counters["partial"] > 0
    if case.has_outside:
        fu, fv = ur.source_coordinates_np(h, w, *ur.lens(case.K, case.dist))
        with np.errstate(invalid="ignore"):
            outside = ~((fu >= -32.0) & (fu < 32.0 * w) & (fv >= -32.0) & (fv < 32.0 * h))
        assert outside.sum() == n_outside and not out[outside].any(), "an OUTSIDE pixel is not zero"


def test_the_recorded_counts_of_the_four_models():
    """What the definition's prototype recorded at 48 x 64 (the issue's table): 351 pixels (11 %) OUTSIDE and 177 with some
    taps outside for the second model, 145 (5 %) and 197 for the rational one, none for the barrel model."""
    got = {c.name: restated(c) for c in ui.model_cases()}
    assert (got["model_barrel"][1], got["model_barrel"][2]["partial"]) == (0, 0)
    assert (got["model_radial_tangential"][1], got["model_radial_tangential"][2]["partial"]) == (351, 177)
    assert (got["model_rational"][1], got["model_rational"][2]["partial"]) == (145, 197)
    assert got["model_four"][2]["fractional"] > 2000


def test_rounding_ties_go_to_even():
    for case in ui.tie_cases():
        j, i = case.extra["pixel"]
        cam, d = ur.lens(case.K, case.dist)
        fx, fy, cx, cy = cam
        # the map up to u * 32, restated once more for this one pixel (x = 1, y = 0)
        x = (j - cx) / fx
        r2 = x * x
        u32 = (fx * (x * (1.0 + ((d[4] * r2 + d[1]) * r2 + d[0]) * r2)) + cx) * 32.0
        assert u32 == case.extra["u32"] and u32 - np.floor(u32) == 0.5
        fu, fv = ur.source_coordinates(j, i, cam, d)
        assert (fu, fv) == (case.extra["fu"], 0.0)
        out = restated(case)[0]
        sx, ax = int(fu) >> 5, int(fu) & 31
        want = (case.src[0, sx].astype(int) * (32 - ax) * 32 + case.src[0, sx + 1].astype(int) * ax * 32 + 512) >> 10
        assert np.array_equal(out[i, j], want)
    # half-up would send 32.5 to 33 and truncation 33.5 to 33: the content tells 33 from both results
    src = ui.tie_cases()[0].src
    down, up = (restated(c)[0] for c in ui.tie_cases())
    at_33 = (src[0, 1].astype(int) * 31 * 32 + src[0, 2].astype(int) * 32 + 512) >> 10
    assert np.array_equal(down[0, 1], src[0, 1]), "32.5 -> 32: the source pixel itself"
    assert not np.array_equal(down[0, 1], at_33) and not np.array_equal(up[0, 1], at_33)


def test_infinity_and_nan_are_outside():
    case = ui.nonfinite_case()
    cam, d = ur.lens(case.K, case.dist)
    fu, _ = ur.source_coordinates(*case.extra["inf"], cam, d)
    assert np.isinf(fu)
    fu, _ = ur.source_coordinates(*case.extra["nan"], cam, d)
    assert np.isnan(fu)
    out, n_outside, _ = restated(case)
    for j, i in (case.extra["inf"], case.extra["nan"]):
        assert not out[i, j].any()
    assert n_outside >= 2 and np.array_equal(out[0, 0], case.src[0, 0])


def test_grid_stride_case_is_larger_than_the_largest_launch():
    case = ui.grid_stride_case()
    h, w = case.shape
    source = open(os.path.join(_package_dir(), "csrc", "amvs_undistort.hip")).read()
    cap = int(re.search(r"UNDISTORT_MAX_BLOCKS = (\d+);", source).group(1))
    tw, th = (int(v) for v in re.search(r"TILE_W = (\d+), TILE_H = (\d+);", source).groups())
    assert ((w + tw - 1) // tw) * ((h + th - 1) // th) > cap
    out, n_outside, counters = restated(case)
    assert n_outside == 0 and counters["fractional"] > 0.9 * h * w


def _package_dir():
    from amvs import _lib
    return os.path.dirname(os.path.abspath(_lib.__file__))


# --------------------------------------------------------------------------------------------------- accuracy ---
@pytest.mark.parametrize("name,dist", ui.MODELS)
def test_restatement_stays_within_the_analytic_bound_on_a_ramp(name, dist):
    """Source: the ramp a u + b v + c rounded to 8 bits.  Bilinear interpolation is exact on a ramp, so against the ramp at
    the true distorted point the result is off by at most 0.5 (source rounding; the interpolation is a convex combination)
    + 0.5 (output rounding) + (|a| + |b|) / 64 (the fractions are quantised to 1/32 pixel, so each coordinate is off by
    at most 1/64).  The distorted point is computed independently: in np.longdouble, the polynomials expanded."""
    h, w = 48, 64
    a, b, c = 2.3, -1.7, 90.0
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    src = np.rint(a * jj + b * ii + c)
    assert src.min() >= 0 and src.max() <= 255
    src = np.repeat(src.astype(np.uint8)[..., None], 3, axis=2)
    out, _, _ = ur.undistort_np(src, ui.K_48x64, dist)
    L = np.longdouble
    k1, k2, p1, p2, k3, k4, k5, k6 = (L(v) for v in list(dist) + [0.0] * (8 - len(dist)))
    fx, fy, cx, cy = (L(ui.K_48x64[r, s]) for r, s in ((0, 0), (1, 1), (0, 2), (1, 2)))
    x, y = (jj.astype(L) - cx) / fx, (ii.astype(L) - cy) / fy
    r2 = x * x + y * y
    kr = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    u = fx * (x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) + cx
    v = fy * (y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) + cy
    # every tap inside: the quantised point is at most 1/64 from (u, v), so a margin of one pixel is more than enough
    full = (u >= 1) & (u <= w - 2) & (v >= 1) & (v <= h - 2)
    assert full.sum() > 0.5 * h * w
    err = np.abs(out[..., 0].astype(L) - (a * u + b * v + c))[full]
    bound = 1 + (abs(a) + abs(b)) / 64
    print(f"{name}: largest error {float(err.max()):.4f} codes over {int(full.sum())} pixels, bound {bound:.4f}")
    assert err.max() <= bound
    assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])


# --------------------------------------------------------------------------------- symbols and coefficients ---
def test_third_header_matches_its_table_and_every_symbol_is_exported():
    from amvs import _lib
    header = open(os.path.join(ROOT, "include", "amvs_lens.h")).read()
    declared = set(re.findall(r"^(?:int|const char \*)\s*(amvs_\w+)\(", header, re.M))
    assert declared == set(_lib.LENS_SIGNATURES) == {"amvs_undistort_bgr8", "amvs_set_view_bgr8_undistorted"}
    assert not declared & set(_lib.SIGNATURES) and not declared & set(_lib.DEPTH_SIGNATURES)
    for other in ("amvs.h", "amvs_depth.h"):
        assert not declared & set(re.findall(r"\b(amvs_\w+)\(", open(os.path.join(ROOT, "include", other)).read()))
    assert '#include "amvs.h"' in header
    lib = _lib.load()
    for name, (res, args) in _lib.LENS_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(args)
    from amvs.engine import Engine
    assert callable(Engine.undistort_bgr8) and callable(Engine.set_view_bgr8_undistorted)


def test_parameter_errors_need_no_device():
    """A NULL context is refused before anything else happens, whatever the other arguments."""
    from amvs import _lib
    lib = _lib.load()
    K = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    d = (C.c_double * 8)()
    img = (C.c_uint8 * 3)()
    f = (C.c_float * 9)()
    assert lib.amvs_undistort_bgr8(None, img, 1, 1, K, d, 5, img, None) == -1
    assert lib.amvs_undistort_bgr8(None, None, 0, 0, None, None, 7, None, None) == -1
    assert lib.amvs_set_view_bgr8_undistorted(None, 0, img, 1, 1, K, d, 5, f, f, None) == -1


def test_coefficients_are_trimmed_and_unknown_models_refused():
    from amvs.engine import lens_coefficients
    assert lens_coefficients(np.zeros(5)).tolist() == [0.0] * 4
    assert lens_coefficients([0.1, 0.0]).tolist() == [0.1, 0.0, 0.0, 0.0]
    assert lens_coefficients([0.1, 0.2, 0.0, 0.0, 0.0]).tolist() == [0.1, 0.2, 0.0, 0.0]
    assert lens_coefficients(ui.RADIAL_TANGENTIAL).tolist() == ui.RADIAL_TANGENTIAL
    assert lens_coefficients(ui.RATIONAL + [0.0] * 6).tolist() == ui.RATIONAL
    assert lens_coefficients(ui.RADIAL_TANGENTIAL + [0.0, 0.0, 0.0]).tolist() == ui.RADIAL_TANGENTIAL
    assert lens_coefficients([0, 0, 0, 0, 0, 0, 0.5]).tolist() == [0, 0, 0, 0, 0, 0, 0.5, 0]
    assert lens_coefficients(np.zeros((1, 14))).dtype == np.float64
    with pytest.raises(ValueError, match="thin-prism"):
        lens_coefficients(ui.RATIONAL + [1e-4])
    with pytest.raises(ValueError, match="thin-prism"):
        lens_coefficients([0.0] * 13 + [0.01])


# ---------------------------------------------------------------------------- the switch of the two classes ---
class _Fake:
    """Engine stand-in (as tests/test_distributed.py does it): records every upload call in `log`."""
    log = None

    def __init__(self, H, W, n, K, device=0, mode="exact"):
        self.H, self.W = H, W

    def reusable_for(self, *a, **k):
        return False

    def set_view_bgr8(self, slot, img, R, t, want_color=True):
        self.log.append(("bgr8", slot, img, R, t, want_color))
        return np.zeros((self.H, self.W, 3), np.uint8) if want_color else None

    def set_view_bgr8_undistorted(self, slot, img, K_src, dist, R, t, want_color=True):
        self.log.append(("undistorted", slot, img, np.array(K_src), np.array(dist), R, t, want_color))
        return np.full((self.H, self.W, 3), 7, np.uint8) if want_color else None

    def close(self):
        pass


def _owners(dist, **kw):
    import amvs
    K = np.array([[80.0, 0, 16.0], [0, 81.0, 12.0], [0, 0, 1.0]])
    cam = amvs.Camera(K=K, dist=np.asarray(dist, np.float64))
    return (lambda **more: amvs.PatchMatchMVS(cam, scale=0.5, patch_size=7, device=0, **kw, **more),
            lambda **more: amvs.DenseStereoReconstructor(cam, scale=0.5, device=0, **kw, **more))


def _scene():
    import amvs
    images = [{"image": np.full((24, 32, 3), 10 + i, np.uint8)} for i in range(3)]
    poses = {i: amvs.CameraPose(R=np.eye(3), t=np.array([0.1 * i, 0.0, 0.0])) for i in range(3)}
    return images, poses


def test_undistort_refuses_the_host_path_and_unknown_models(capsys):
    for make in _owners(ui.RADIAL_TANGENTIAL):
        with pytest.raises(ValueError, match="device_prep=False"):
            make(undistort=True, device_prep=False)
        assert make(undistort=True).device_prep is True and make(undistort=True, device_prep=True).device_prep is True
        assert make().undistort is False
    for make in _owners(ui.RATIONAL + [0.002]):
        with pytest.raises(ValueError, match="thin-prism"):
            make(undistort=True)
        make()                                                   # (the coefficient is not looked at without the switch)
    capsys.readouterr()


def test_switch_off_is_todays_call_and_todays_key(monkeypatch, capsys):
    from amvs import engine as engine_mod
    images, poses = _scene()
    for scale in (0.5, 1.0):
        for make in _owners(ui.RADIAL_TANGENTIAL):
            fake = type("Fake", (_Fake,), {"log": []})
            monkeypatch.setattr(engine_mod, "Engine", fake)
            obj = make(device_prep=True)
            obj.scale = scale
            prepared = obj._prepare_images_device(images, [0, 1, 2], poses)
            H, W = int(24 * scale), int(32 * scale)
            assert [(u[0], u[1], u[5]) for u in fake.log] == [("bgr8", s, scale != 1.0) for s in range(3)]
            for s, u in enumerate(fake.log):
                assert len(u) == 6 and u[2] is images[s]["image"] and u[3] is poses[s].R and u[4] is poses[s].t
            pose_print = b"".join(np.asarray(poses[i].R, np.float64).tobytes() + np.asarray(poses[i].t, np.float64).tobytes() for i in range(3))
            assert obj._engine_key == ((0, 1, 2), (H, W), pose_print, obj.K_scaled.tobytes(), 0)
            assert all((prepared[i]["color"] is images[i]["image"]) == (scale == 1.0) for i in range(3))
    capsys.readouterr()


def test_switch_on_uploads_with_the_lens_and_keys_on_it(monkeypatch, capsys):
    import amvs
    from amvs import engine as engine_mod
    images, poses = _scene()
    for n, make in enumerate(_owners(ui.RADIAL_TANGENTIAL + [0.0] * 3)):
        for scale in (0.5, 1.0):
            fake = type("Fake", (_Fake,), {"log": []})
            monkeypatch.setattr(engine_mod, "Engine", fake)
            obj = make(undistort=True)
            obj.scale = scale
            prepared = obj._prepare_images_device(images, [0, 1, 2], poses)
            assert [(u[0], u[1], u[7]) for u in fake.log] == [("undistorted", s, True) for s in range(3)]
            for s, u in enumerate(fake.log):
                assert u[2] is images[s]["image"] and np.array_equal(u[3], obj.camera.K) and u[3].dtype == np.float64
                assert u[4].tolist() == ui.RADIAL_TANGENTIAL and u[5] is poses[s].R and u[6] is poses[s].t
            assert all((prepared[i]["color"] == 7).all() for i in range(3)), "the colour image is the undistorted one at every scale"
            key = obj._engine_key
            assert len(key) == 7 and key[5] == obj.camera.K.tobytes() and key[6] == np.asarray(ui.RADIAL_TANGENTIAL).tobytes()
            # another lens on the same instance: the key changes with dist and with K
            obj.camera = amvs.Camera(K=obj.camera.K.copy(), dist=np.asarray(ui.BARREL))
            obj._prepare_images_device(images, [0, 1, 2], poses)
            assert obj._engine_key != key and obj._engine_key[:5] == key[:5] and fake.log[-1][4].tolist() == ui.BARREL[:4]
            key2 = obj._engine_key
            K2 = obj.camera.K.copy()
            K2[0, 2] += 0.5
            obj.camera = amvs.Camera(K=K2, dist=np.asarray(ui.BARREL))
            assert obj._make_engine_key(prepared, poses, [0, 1, 2]) != key2
    capsys.readouterr()
