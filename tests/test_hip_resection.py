"""Camera resection on the device (csrc/amvs_pnp.hip behind include/amvs_resection.h) against the restatement of
tests/resection_restatement.py on the inputs of tests/resection_inputs.py: samples and hypotheses, inlier counts and
masks, the refit, the whole RANSAC, register_view, and the parameter errors behind a valid context.  Every comparison is
bit for bit and leaves no element out; where the header lets a NaN appear, NaN-ness and the bits of the other entries
are compared.  tests/test_resection_cpu.py shows on the CPU that the restatement does what it should."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resection_inputs as ri  # noqa: E402
import resection_restatement as rr  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 1234
K = ri.K


@pytest.fixture(scope="module")
def eng():
    import amvs
    with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as e:
        yield e


def same_bits(a, b):
    """Equal as bit patterns, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


# ------------------------------------------------------------------------------------------------- hypotheses ---
COUNTS, FIRSTS = (1, 64, 65), (0, 1000)
_HYP = {}


def restated_hypotheses(key, X, x):
    """Hypotheses 0 .. 1064 of a case, once: hypothesis h is a function of h, so every (first, count) is a slice."""
    if key not in _HYP:
        _HYP[key] = rr.hypotheses(X, x, K, SEED, 0, max(FIRSTS) + max(COUNTS))
    return _HYP[key]


def check_hypotheses(eng, key, X, x):
    ridx, rR, rt = restated_hypotheses(key, X, x)
    for first in FIRSTS:
        for count in COUNTS:
            idx, R, t = eng.pnp_hypotheses(X, x, K, seed=SEED, first=first, count=count)
            assert idx.shape == (count, 6) and idx.dtype == np.int32 and R.shape == (count, 3, 3) and t.shape == (count, 3)
            assert np.array_equal(idx, ridx[first:first + count]), (key, first, count)
            assert same_bits(R.reshape(count, 9), rR[first:first + count]), (key, first, count)
            assert same_bits(t, rt[first:first + count]), (key, first, count)
    return rR, rt


@pytest.mark.parametrize("m", [6, 7, 63, 64, 65, 1000])
def test_hypotheses_bit_for_bit(eng, m):
    X, x, _ = ri.scene(m, 0.25 if m >= 63 else 0.0, seed=m)
    rR, rt = check_hypotheses(eng, m, X, x)
    assert np.isfinite(rR).all() and np.isfinite(rt).all()


@pytest.mark.parametrize("name", ["identical", "collinear", "coplanar", "repeated"])
def test_hypotheses_of_degenerate_samples(eng, name):
    X, x = ri.degenerate_cases()[name]
    rR, rt = check_hypotheses(eng, name, X, x)
    if name == "identical":
        assert np.isnan(rR).all()                       # d == 0: no scale, and no inlier below
        assert not eng.pnp_score(rR[:3], rt[:3], X, x, K).any()


# ------------------------------------------------------------------------------------------ scoring and inliers ---
_SCORE = {}


def score_case(m):
    """The correspondences on either side of the threshold, max(SCORE_N) poses around the true one (the first is the true
    pose, three of them are the zero / NaN / inf ones), the restated inlier matrix and its smallest margin; once per m."""
    if m not in _SCORE:
        X, x, inside = ri.threshold_case(m)
        rng = np.random.default_rng(m)
        R0, t0 = ri.true_pose()
        n = max(ri.SCORE_N)
        R = R0.reshape(1, 9) * (1.0 + 1e-5 * rng.standard_normal((n, 9)))
        t = t0[None] + 1e-4 * rng.standard_normal((n, 3))
        R[0], t[0] = R0.reshape(9), t0
        R[5:8], t[5:8] = ri.special_poses()
        inl, margin = rr.inlier_matrix(R, t, X, x, K, 2.0, with_margin=True)
        _SCORE[m] = (X, x, inside, R, t, inl, margin)
    return _SCORE[m]


@pytest.mark.parametrize("m", ri.SCORE_M)
def test_score_and_inliers_bit_for_bit(eng, m):
    X, x, inside, R, t, inl, margin = score_case(m)
    print(f"m = {m}: smallest relative margin of a decision to its threshold {margin:.3e}")
    assert margin > 1e-9
    assert np.array_equal(inl[0], inside)                    # planted 1 % inside / outside: decided as planted
    assert not inl[5:8].any()                                # zero, NaN and inf poses keep nothing
    for n in ri.SCORE_N:
        counts = eng.pnp_score(R[:n], t[:n], X, x, K, threshold=2.0)
        assert counts.dtype == np.int32 and np.array_equal(counts, inl[:n].sum(axis=1)), (m, n)
    assert not eng.pnp_score(*ri.special_poses(), X, x, K, threshold=2.0).any()
    for j in (0, 1, 5, 6, 7, 64):
        assert np.array_equal(eng.pnp_inliers(R[j], t[j], X, x, K, threshold=2.0), inl[j]), (m, j)


def test_on_the_threshold_at_zero_depth_and_behind_the_camera(eng):
    X, x, R, t, Kt, thr, expected = ri.on_threshold_case()
    assert np.array_equal(rr.inliers(R, t, X, x, Kt, thr), expected)
    assert np.array_equal(eng.pnp_inliers(R, t, X, x, Kt, threshold=thr), expected)
    assert eng.pnp_score(R, t, X, x, Kt, threshold=thr).tolist() == [int(expected.sum())]


# -------------------------------------------------------------------------------------------------------- refit ---
def check_refine(eng, X, x, R0, t0, mask):
    rR, rt, rsteps, rcost, costs = rr.refine(X, x, K, R0, t0, mask, return_costs=True)
    R, t, steps, cost = eng.pnp_refine(X, x, K, R0, t0, mask)
    assert steps == rsteps and same_bits(R.reshape(9), rR) and same_bits(t, rt) and same_bits([cost], [rcost])
    return R, t, steps, costs


@pytest.mark.parametrize("size", ri.REFINE_SET_SIZES)
def test_refine_bit_for_bit_on_scattered_sets(eng, size):
    X, x, mask = ri.scattered_set(size)
    R, t, steps, _ = check_refine(eng, X, x, *ri.start_pose(), mask)
    assert steps >= 1 and np.isfinite(R).all() and ri.rotation_error_deg(R, ri.true_pose()[0]) < 2.0


def test_refine_without_a_mask_is_the_refit_to_all(eng):
    X, x, _ = ri.scene(1000, 0.0, seed=5)
    R0, t0 = ri.start_pose()
    R, t, steps, _ = check_refine(eng, X, x, R0, t0, None)
    R1, t1, steps1, cost1 = eng.pnp_refine(X, x, K, R0, t0, np.ones(1000, bool))
    assert same_bits(R, R1) and same_bits(t, t1) and steps == steps1
    from amvs._lib import AmvsError
    few = np.zeros(1000, bool)
    few[:5] = True
    with pytest.raises(AmvsError):
        eng.pnp_refine(X, x, K, R0, t0, few)


def test_refine_undoes_a_rejected_step_and_stops_on_a_bad_pivot(eng):
    X, x, _ = ri.scene(200, 0.0, seed=21)
    R, t, steps, costs = check_refine(eng, X, x, *ri.start_pose(deg=60.0, shift=1.5), None)
    assert len(costs) == steps + 2 and not costs[-1] <= costs[steps]         # the restatement saw a pass it undid
    R0, t0 = ri.true_pose()
    same = (np.repeat(X[:1], 6, axis=0), np.repeat(x[:1], 6, axis=0))
    R, t, steps, _ = check_refine(eng, *same, R0, t0, None)
    assert steps == 0 and np.array_equal(R, R0) and np.array_equal(t, t0)


# ------------------------------------------------------------------------------------------------------- RANSAC ---
_SCORED, _RANSAC = {}, {}


def restated_ransac(name, max_hyp, seed=SEED, threshold=2.0, confidence=0.99):
    key = (name, max_hyp, seed, threshold)
    if key not in _RANSAC:
        X, x, _ = ri.family_scene(name)
        scored = _SCORED.setdefault((name, seed, threshold), rr.Scored(X, x, K, threshold, seed))
        _RANSAC[key] = rr.ransac(X, x, K, threshold, confidence, max_hyp, seed, scored=scored)
    return _RANSAC[key]


def check_ransac(eng, X, x, restated, max_hyp, seed=SEED, threshold=2.0):
    rR, rt, rmask, rn, rinfo = restated[:5]
    R, t, mask, info = eng.pnp_ransac(X, x, K, threshold=threshold, confidence=0.99, max_hypotheses=max_hyp, seed=seed)
    assert [info["hypotheses"], info["best_hypothesis"], info["best_count"]] == rinfo.tolist(), max_hyp
    assert info["n_inliers"] == rn and np.array_equal(mask, rmask)
    if rn == 0:
        assert R is None and t is None and not mask.any()
    else:
        assert same_bits(R.reshape(9), rR) and same_bits(t, rt)
        assert np.array_equal(eng.pnp_inliers(R, t, X, x, K, threshold=threshold), mask)
    return R, t, mask, info


@pytest.mark.parametrize("max_hyp", ri.MAX_HYPOTHESES)
@pytest.mark.parametrize("name", list(ri.FAMILY))
def test_ransac_bit_for_bit(eng, name, max_hyp):
    X, x, _ = ri.family_scene(name)
    R, t, mask, info = check_ransac(eng, X, x, restated_ransac(name, max_hyp), max_hyp)
    if max_hyp >= 1024:
        assert R is not None and np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12


def test_ransac_without_a_model(eng):
    X, x = ri.uniform_correspondences(64, 5)
    restated = rr.ransac(X, x, K, 2.0, 0.99, 1025, SEED)
    assert restated[3] == 0 and restated[4][0] == 1025
    R, t, mask, info = check_ransac(eng, X, x, restated, 1025)
    assert R is None and info["n_inliers"] == 0


def test_ransac_repeats_itself_and_follows_the_seed(eng):
    X, x, _ = ri.family_scene("2000_50")
    a = eng.pnp_ransac(X, x, K, threshold=2.0, max_hypotheses=4096, seed=SEED)
    b = eng.pnp_ransac(X, x, K, threshold=2.0, max_hypotheses=4096, seed=SEED)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    other = check_ransac(eng, X, x, restated_ransac("2000_50", 4096, seed=SEED + 1), 4096, seed=SEED + 1)
    assert other[3]["best_hypothesis"] != a[3]["best_hypothesis"]


# -------------------------------------------------------------------------------------------- register_view ---
def test_register_view_end_to_end(eng):
    from amvs.core import refine_pose, register_view
    from amvs.core.camera import Camera, CameraPose
    X, x, planted = ri.family_scene("300_30")
    pose, mask = register_view(Camera(K), X, x, engine=eng)
    rR, rt, rmask = rr.ransac(X, x, K, 8.0, 0.99, 5000, 0)[:3]
    assert isinstance(pose, CameraPose) and same_bits(pose.R.reshape(9), rR) and same_bits(pose.t, rt)
    assert np.array_equal(mask, rmask) and mask.sum() >= planted.sum()
    assert register_view(Camera(K), X, x, engine=eng, min_inliers=int(mask.sum()) + 1) is None
    again = refine_pose(Camera(K), pose, X, x, mask, engine=eng)
    assert same_bits(again.R.reshape(9), rr.refine(X, x, K, rR, rt, rmask)[0])


# ----------------------------------------------------------------------------- parameter errors behind a context ---
def test_every_documented_parameter_error_is_refused(eng):
    """AMVS_EINVAL (-1) for each error include/amvs_resection.h lists, through the raw entry points on a live context."""
    lib, h = eng._lib, eng._h
    f64, f32 = C.POINTER(C.c_double), C.POINTER(C.c_float)
    X, x, _ = ri.scene(8, 0.0, seed=1)
    p3, p2 = X.ctypes.data_as(f32), x.ctypes.data_as(f32)
    R0, t0 = ri.true_pose()
    Rd, td = np.ascontiguousarray(R0).ctypes.data_as(f64), np.ascontiguousarray(t0).ctypes.data_as(f64)
    Ro, to = (C.c_double * 9)(), (C.c_double * 3)()
    idx, info, mask = (C.c_int32 * 6)(), (C.c_int32 * 3)(), (C.c_uint8 * 8)()
    n64, steps, cost = C.c_int64(0), C.c_int32(0), C.c_double(0.0)

    def Kp(**change):
        Kc = K.copy().reshape(9)
        for k, v in change.items():
            Kc[int(k[1:])] = v
        return Kc.ctypes.data_as(f64), Kc                    # (the array is kept alive by the tuple)

    good, good_kept = Kp()

    def ransac(m=8, K_=good, thr=2.0, conf=0.99, hyp=1, a3=p3, a2=p2, R_=Ro):
        return lib.amvs_pnp_ransac(h, a3, a2, m, K_, thr, conf, hyp, 0, R_, to, mask, C.byref(n64), info)

    assert ransac() == 0                                     # the call every case below spoils in one place
    bad_K = [Kp(k0=0.0), Kp(k0=-1.0), Kp(k0=np.inf), Kp(k0=np.nan), Kp(k4=0.0), Kp(k4=np.nan), Kp(k2=np.inf), Kp(k5=np.nan),
             Kp(k1=0.5)]
    for ptr, keep in bad_K:
        assert ransac(K_=ptr) == -1, keep
        assert lib.amvs_pnp_hypotheses(h, p3, p2, 8, ptr, 0, 0, 1, idx, Ro, to) == -1
        assert lib.amvs_pnp_score(h, Rd, td, 1, p3, p2, 8, ptr, 2.0, info) == -1
        assert lib.amvs_pnp_inliers(h, Rd, td, p3, p2, 8, ptr, 2.0, mask, C.byref(n64)) == -1
        assert lib.amvs_pnp_refine(h, p3, p2, 8, ptr, Rd, td, None, Ro, to, C.byref(steps), C.byref(cost), C.byref(n64)) == -1
    for m in (5, 0, -1, (1 << 20) + 1):
        assert ransac(m=m) == -1 and lib.amvs_pnp_hypotheses(h, p3, p2, m, good, 0, 0, 1, idx, Ro, to) == -1
    assert ransac(a3=None) == -1 and ransac(a2=None) == -1 and ransac(K_=None) == -1 and ransac(R_=None) == -1
    for thr in (0.0, -2.0, np.inf, np.nan):
        assert ransac(thr=thr) == -1
        assert lib.amvs_pnp_score(h, Rd, td, 1, p3, p2, 8, good, thr, info) == -1
        assert lib.amvs_pnp_inliers(h, Rd, td, p3, p2, 8, good, thr, mask, C.byref(n64)) == -1
    for conf in (0.0, 1.0, -0.5, 1.5, np.nan):
        assert ransac(conf=conf) == -1
    for hyp in (0, -1, (1 << 20) + 1):
        assert ransac(hyp=hyp) == -1
        assert lib.amvs_pnp_hypotheses(h, p3, p2, 8, good, 0, 0, hyp, idx, Ro, to) == -1
        assert lib.amvs_pnp_score(h, Rd, td, hyp, p3, p2, 8, good, 2.0, info) == -1
    assert lib.amvs_pnp_hypotheses(h, p3, p2, 8, good, 0, -1, 1, idx, Ro, to) == -1                  # first < 0
    assert lib.amvs_pnp_hypotheses(h, p3, p2, 8, good, 0, 0, 1, None, Ro, to) == -1
    assert lib.amvs_pnp_score(h, None, td, 1, p3, p2, 8, good, 2.0, info) == -1
    assert lib.amvs_pnp_inliers(h, Rd, td, p3, p2, 8, good, 2.0, None, C.byref(n64)) == -1
    five = (C.c_uint8 * 8)(1, 1, 1, 1, 1, 0, 0, 0)
    assert lib.amvs_pnp_refine(h, p3, p2, 8, good, Rd, td, five, Ro, to, C.byref(steps), C.byref(cost), C.byref(n64)) == -1
    assert lib.amvs_pnp_refine(h, p3, p2, 8, good, None, td, None, Ro, to, C.byref(steps), C.byref(cost), C.byref(n64)) == -1
    assert ransac() == 0                                     # and the context still serves
