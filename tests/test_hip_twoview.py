"""The first two views on the device (csrc/amvs_twoview.hip behind include/amvs_twoview.h) against the restatement of
tests/twoview_restatement.py on the inputs of tests/twoview_inputs.py: the decomposition of F, the cheirality counts and
masks, the relative pose, the triangulation, find_best_initial_pair end to end, and the parameter errors behind a valid
context.  Every comparison is bit for bit and leaves no element out; where the header lets a NaN appear, NaN-ness and the
bits of the other entries are compared.  tests/test_twoview_cpu.py shows on the CPU that the restatement does what it
should."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_restatement as er  # noqa: E402
import twoview_inputs as ti  # noqa: E402
import twoview_restatement as tr  # noqa: E402

pytestmark = pytest.mark.gpu
K = ti.K
I3, Z3 = np.eye(3), np.zeros(3)
f64p, f32p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint8)


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


def ptr(a, kind=f64p):
    return a.ctypes.data_as(kind)


# ------------------------------------------------------------------------------------------ the decomposition ---
def raw_decompose(eng, F):
    """(ok, R (2, 9), t, w) straight from the entry point, so that the zeros of `no model` are seen too."""
    F9, K9 = np.ascontiguousarray(F, np.float64).reshape(9), np.ascontiguousarray(K).reshape(9)
    R, t, w, ok = np.full((2, 9), 7.0), np.full(3, 7.0), np.full(3, 7.0), C.c_int32(7)
    assert eng._lib.amvs_twoview_decompose(eng._h, ptr(F9), ptr(K9), ptr(R), ptr(t), ptr(w), C.byref(ok)) == 0
    return ok.value, R, t, w


def fundamentals():
    R, t = ti.true_pose()
    _, p1, p2, _ = ti.scene(200, noise=0.5, seed=77)
    out = {"exact": ti.fundamental(R, t), "noisy": er.fit(p1, p2).reshape(3, 3), "scaled": 1e-9 * ti.fundamental(R, t)}
    out.update(ti.degenerate_fundamentals())
    return out


@pytest.mark.parametrize("name", ["exact", "noisy", "scaled", "zero", "rank1", "nan", "inf"])
def test_decompose_bit_for_bit(eng, name):
    F = fundamentals()[name]
    rok, rR, rt, rw = tr.decompose(F, K)
    ok, R, t, w = raw_decompose(eng, F)
    assert ok == int(rok) and same_bits(R, rR) and same_bits(t, rt) and same_bits(w, rw), name
    assert bool(ok) == (name in ("exact", "noisy", "scaled")) or name == "inf"
    got = eng.twoview_decompose(F, K)
    if not ok:
        assert got is None and not R.any() and not t.any() and not w.any()
    else:
        assert got[0].shape == (2, 3, 3) and same_bits(got[0].reshape(2, 9), rR) and same_bits(got[1], rt) and same_bits(got[2], rw)


# ------------------------------------------------------------------------------------------ scoring and masks ---
_SCORE = {}


def score_case(m):
    """The matches of ti.score_matches(m), max(SCORE_N) poses (ti.score_poses around the candidates of the exact F) and the
    restated matrices at the limit of the case and without a limit; once per m."""
    if m not in _SCORE:
        p1, p2, planted = ti.score_matches(m)
        ok, R2, tt, _ = tr.decompose(ti.fundamental(*ti.true_pose()), K)
        R, t = ti.score_poses(*tr.candidates(R2, tt))
        _SCORE[m] = (p1, p2, planted, R, t, tr.front_matrix(R, t, p1, p2, K, ti.DEPTH_LIMIT),
                     tr.front_matrix(R[:9], t[:9], p1, p2, K, float("inf")))
    return _SCORE[m]


@pytest.mark.parametrize("m", ti.SCORE_M)
def test_score_and_front_bit_for_bit(eng, m):
    p1, p2, planted, R, t, inl, unlimited = score_case(m)
    assert np.array_equal(inl[0], planted)                    # 1 % inside / outside the limit: decided as planted
    assert not inl[1:4].any()                                 # the zero, NaN and infinite poses count nothing
    assert len(R) > ti.POSE_TILE * 2 and 33 in ti.SCORE_N and 65 in ti.SCORE_N       # both sides of the tile boundary, twice
    for n in ti.SCORE_N:
        counts = eng.twoview_score(R[:n], t[:n], p1, p2, K, max_depth=ti.DEPTH_LIMIT)
        assert counts.dtype == np.int32 and np.array_equal(counts, inl[:n].sum(axis=1)), (m, n)
    assert not eng.twoview_score(R[1:4], t[1:4], p1, p2, K, max_depth=float("inf")).any()
    assert np.array_equal(eng.twoview_score(R[:9], t[:9], p1, p2, K, max_depth=float("inf")), unlimited.sum(axis=1))
    for j in (0, 1, 2, 3, 4, 5, 6, 7, 8, 31, 32, 64):
        mask = eng.twoview_front(R[j], t[j], p1, p2, K, max_depth=ti.DEPTH_LIMIT)
        assert mask.dtype == bool and np.array_equal(mask, inl[j]), (m, j)
    assert np.array_equal(eng.twoview_front(R[4], t[4], p1, p2, K, max_depth=float("inf")), unlimited[4])
    if m >= 8:
        assert not unlimited[4][1] and unlimited[0][[3, 5]].all()            # the point at infinity; outside only the limit
        # matches in front of one camera only: the twisted candidates put every scene point behind one camera
        z = [tr.depths(R[j], t[j], p1[6:], p2[6:], K) for j in range(5, 9)]
        assert any(((z1 > 0) != (z2 > 0)).all() for z1, z2 in z) and sum(int(inl[j][6:].all()) for j in range(5, 9)) == 1


def test_score_with_the_default_limit(eng):
    p1, p2, planted, R, t, _, _ = score_case(1000)
    assert np.array_equal(eng.twoview_score(R[:9], t[:9], p1, p2, K), tr.score(R[:9], t[:9], p1, p2, K, 50.0))


# ---------------------------------------------------------------------------------------------------- the pose ---
def check_pose(eng, F, p1, p2, max_depth=50.0):
    rR, rt, rmask, rn, rinfo = tr.pose(F, K, p1, p2, max_depth)
    R, t, mask, info = eng.twoview_pose(F, K, p1, p2, max_depth=max_depth)
    assert [info["best"], *info["counts"]] == rinfo.tolist() and info["n_front"] == rn and np.array_equal(mask, rmask)
    if rn == 0:
        assert R is None and t is None and not mask.any()
    else:
        assert same_bits(R.reshape(9), rR) and same_bits(t, rt)
        assert np.abs(R.T @ R - I3).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12 and abs(np.linalg.norm(t) - 1.0) < 1e-12
        assert np.array_equal(eng.twoview_front(R, t, p1, p2, K, max_depth=max_depth), mask)
    return R, t, mask, info


def test_pose_on_the_clean_scene(eng):
    R0, t0 = ti.true_pose()
    _, p1, p2, _ = ti.scene(200)
    R, t, mask, info = check_pose(eng, ti.fundamental(R0, t0), p1, p2)
    assert mask.all() and sorted(info["counts"].tolist()) == [0, 0, 0, 200]
    assert np.abs(R - R0).max() < 1e-9 and np.abs(t - t0).max() < 1e-9


def test_pose_with_outliers_and_a_fitted_F(eng):
    R0, t0 = ti.true_pose()
    _, p1, p2, planted = ti.scene(300, noise=0.5, outlier_fraction=0.3, seed=8)
    R, t, mask, info = check_pose(eng, ti.fundamental(R0, t0), p1, p2)
    assert info["n_front"] == max(info["counts"]) and mask[planted].all() and np.abs(R - R0).max() < 1e-9
    F = er.fit(p1, p2, planted)
    R, t, mask, info = check_pose(eng, F, p1, p2, max_depth=ti.DEPTH_LIMIT)
    assert ti.ri.rotation_error_deg(R, R0) < 0.5 and mask[planted].all()


def test_pose_without_a_model(eng):
    _, p1, p2, _ = ti.scene(65)
    for name in ("zero", "rank1", "nan"):
        R, t, mask, info = check_pose(eng, ti.degenerate_fundamentals()[name], p1, p2)
        assert R is None and info["n_front"] == 0 and not info["counts"].any()
    # a model none of whose candidates puts a match in front: the principal points under a sideways translation
    centre = np.array([[K[0, 2], K[1, 2]]], np.float32)
    F = np.linalg.inv(K).T @ ti.skew(np.array([1.0, 0.0, 0.0])) @ np.linalg.inv(K)
    assert tr.decompose(F, K)[0]
    R, t, mask, info = check_pose(eng, F, centre, centre)
    assert R is None and not info["counts"].any()


# ----------------------------------------------------------------------------------------------- triangulation ---
def raw_triangulate(eng, R2, t2, p1, p2, thresholds):
    m = len(p1)
    a = [np.ascontiguousarray(x, np.float64).reshape(-1) for x in (K, I3, Z3, R2, t2)]
    X, valid, cs, n = np.full((m, 3), 7.0), np.full(m, 7, np.uint8), np.full(m, 7.0), C.c_int64(-1)
    rc = eng._lib.amvs_twoview_triangulate(eng._h, *[ptr(x) for x in a], ptr(p1, f32p) if m else None, ptr(p2, f32p) if m else None, m,
                                           *[float(x) for x in thresholds], ptr(X) if m else None, ptr(valid, u8p) if m else None,
                                           ptr(cs) if m else None, C.byref(n))
    assert rc == 0
    return X, valid, cs, n.value


@pytest.mark.parametrize("m", ti.TRI_M)
def test_triangulate_bit_for_bit(eng, m):
    R, t = ti.true_pose()
    p1, p2 = ti.triangulate_candidates(m)
    for which, thresholds in enumerate((ti.FILTER_DEFAULTS, ti.FILTER_NEAR)):
        rX, rvalid, rcs = tr.triangulate(K, I3, Z3, R, t, p1, p2, *thresholds)
        X, valid, cs, n = raw_triangulate(eng, R, t, p1, p2, thresholds)
        assert same_bits(X, rX) and np.array_equal(valid, rvalid.astype(np.uint8)) and same_bits(cs, rcs) and n == rvalid.sum(), (m, which)
        if m >= 63:                                            # the planted candidates on either side of all seven comparisons
            _, _, expected, near, names = ti.filter_case()
            rows = np.flatnonzero(near == which)
            assert np.array_equal(valid[rows] != 0, expected[rows]), [names[r] for r in rows]
            assert 0 < n < m
    eX, evalid, ecs = eng.twoview_triangulate(K, I3, Z3, R, t, p1, p2)                  # the defaults: 200 baselines, 1 degree, 4 px
    rX, rvalid, rcs = tr.triangulate(K, I3, Z3, R, t, p1, p2)
    assert eX.shape == (m, 3) and evalid.dtype == bool and same_bits(eX, rX) and np.array_equal(evalid, rvalid) and same_bits(ecs, rcs)


def test_triangulate_between_two_general_poses_and_of_bad_candidates(eng):
    """Neither camera at the origin, so P_1 and C_1 are not trivial; a NaN and an infinite pixel are never valid."""
    R2, t2 = ti.true_pose()
    R1, t1 = ti.pose_with([1.0, -0.3, 0.2], 7.0, [-0.3, 0.1, -0.2])
    Xw = ti.cloud(200, 21)
    rng = np.random.default_rng(2)
    p1 = (ti.project(R1, t1, Xw) + rng.normal(0.0, 0.5, (200, 2))).astype(np.float32)
    p2 = (ti.project(R2, t2, Xw) + rng.normal(0.0, 0.5, (200, 2))).astype(np.float32)
    p1[3, 0], p2[5, 1], p1[7] = np.nan, np.inf, p2[7]
    rX, rvalid, rcs = tr.triangulate(K, R1, t1, R2, t2, p1, p2)
    X, valid, cs = eng.twoview_triangulate(K, R1, t1, R2, t2, p1, p2)
    assert same_bits(X, rX) and np.array_equal(valid, rvalid) and same_bits(cs, rcs)
    assert not valid[3] and not valid[5] and valid.sum() > 150 and np.isnan(X[3]).all()
    from amvs.core import triangulate_points
    from amvs.core.camera import Camera, CameraPose
    gX, gvalid, gcs = triangulate_points(Camera(K), CameraPose(R1, t1), CameraPose(R2, t2.reshape(3, 1)), p1, p2, return_cos=True, engine=eng)
    assert same_bits(gX, rX) and np.array_equal(gvalid, rvalid) and same_bits(gcs, rcs)


# ------------------------------------------------------------------------------------------- the initial pair ---
def restated_ransac(p1, p2, threshold, confidence):
    F, mask, n, _, trace = er.ransac(p1, p2, threshold, confidence)
    # (the device takes log from the C library: no stop of these inputs is decided within 2 of a batch boundary)
    assert all(not from_log or min(abs(N - k) for k in (1024, 2048, 3072, 4096)) >= 2 for _, N, from_log in trace)
    return (F if n >= 8 else None), mask


def test_find_best_initial_pair_end_to_end(eng):
    from amvs.core import decompose_essential, compute_essential_matrix, find_best_initial_pair, relative_pose
    from amvs.core.camera import Camera
    pairs = ti.initial_pairs()
    dropped = {}
    restated = tr.find_best_initial_pair(K, pairs, restated_ransac, dropped)
    assert [c["pair"] for c in restated] == [(0, 2)]
    assert dropped[(0, 1)][0] == "parallax" and dropped[(0, 1)][1] < 1.5 and dropped[(1, 2)] == ("matches", 40)
    assert dropped[(3, 4)] == ("component", None)
    print(f"(0, 1): median parallax {dropped[(0, 1)][1]:.3f} degrees; (0, 2): {restated[0]['parallax']:.3f} degrees, score {restated[0]['score']}")
    best = find_best_initial_pair(Camera(K), pairs, engine=eng)
    want = restated[0]
    assert set(best) == set(want) and best["pair"] == (0, 2)
    assert np.array_equal(best["mask"], want["mask"]) and best["mask"].dtype == bool and best["mask"].shape == (300,)
    assert same_bits(best["R"], want["R"]) and same_bits(best["t"], want["t"]) and best["t"].shape == (3, 1)
    assert same_bits([best["parallax"], best["score"], best["valid_ratio"]], [want["parallax"], want["score"], want["valid_ratio"]])
    assert np.array_equal(best["pts1"], want["pts1"]) and np.array_equal(best["pts2"], want["pts2"])
    assert 3.0 < best["parallax"] < 20.0 and ti.ri.rotation_error_deg(best["R"], ti.true_pose()[0]) < 0.5
    # alone, the short pair and the small pair give nothing
    assert find_best_initial_pair(Camera(K), {k: pairs[k] for k in ((0, 1), (1, 2))}, engine=eng) is None
    # decompose_essential goes through K^-T E K^-1: the pose of the clean scene again, to rounding
    R0, t0 = ti.true_pose()
    _, p1, p2, _ = ti.scene(200)
    F = ti.fundamental(R0, t0)
    R, t, mask = decompose_essential(compute_essential_matrix(Camera(K), F), Camera(K), p1, p2, engine=eng)
    pose, mask2 = relative_pose(Camera(K), F, p1, p2, engine=eng)
    assert np.abs(R - R0).max() < 1e-9 and np.abs(t.ravel() - t0).max() < 1e-9 and mask.all() and t.shape == (3, 1)
    assert np.abs(pose.R - R).max() < 1e-12 and mask2.all()
    with pytest.raises(ValueError):
        decompose_essential(np.zeros((3, 3)), Camera(K), p1, p2, engine=eng)


# ----------------------------------------------------------------------------- parameter errors behind a context ---
def test_every_documented_parameter_error_is_refused(eng):
    """AMVS_EINVAL (-1) for each error include/amvs_twoview.h lists, through the raw entry points on a live context."""
    lib, h = eng._lib, eng._h
    _, x1, x2, _ = ti.scene(8, seed=1)
    a1, a2 = ptr(x1, f32p), ptr(x2, f32p)
    R0, t0 = ti.true_pose()
    R0, F0 = np.ascontiguousarray(R0), np.ascontiguousarray(ti.fundamental(R0, t0))
    Rd, td, Fd = ptr(R0), ptr(t0), ptr(F0)
    Id, Zd = ptr(I3), ptr(Z3)
    R2, Ro, to, wo = (C.c_double * 18)(), (C.c_double * 9)(), (C.c_double * 3)(), (C.c_double * 3)()
    X, cs, valid, mask = (C.c_double * 24)(), (C.c_double * 8)(), (C.c_uint8 * 8)(), (C.c_uint8 * 8)()
    counts, info, ok, n64 = (C.c_int32 * 4)(), (C.c_int32 * 5)(), C.c_int32(0), C.c_int64(0)

    def Kp(**change):
        Kc = K.copy().reshape(9)
        for k, v in change.items():
            Kc[int(k[1:])] = v
        return Kc.ctypes.data_as(f64p), Kc                   # (the array is kept alive by the tuple)

    good, good_kept = Kp()

    def decompose(F_=Fd, K_=good, R_=R2, t_=to, w_=wo, ok_=C.byref(ok)):
        return lib.amvs_twoview_decompose(h, F_, K_, R_, t_, w_, ok_)

    def score(R_=Rd, t_=td, n=1, p1=a1, p2=a2, m=8, K_=good, depth=50.0, out=counts):
        return lib.amvs_twoview_score(h, R_, t_, n, p1, p2, m, K_, depth, out)

    def front(R_=Rd, t_=td, p1=a1, p2=a2, m=8, K_=good, depth=50.0, out=mask, cnt=C.byref(n64)):
        return lib.amvs_twoview_front(h, R_, t_, p1, p2, m, K_, depth, out, cnt)

    def pose(F_=Fd, K_=good, p1=a1, p2=a2, m=8, depth=50.0, R_=Ro, t_=to, out=mask, cnt=C.byref(n64), info_=info):
        return lib.amvs_twoview_pose(h, F_, K_, p1, p2, m, depth, R_, t_, out, cnt, info_)

    def tri(K_=good, R1=Id, t1=Zd, R2_=Rd, t2=td, p1=a1, p2=a2, m=8, thr=(0.01, 200.0, 0.9998, 4.0), X_=X, v_=valid, c_=cs, cnt=C.byref(n64)):
        return lib.amvs_twoview_triangulate(h, K_, R1, t1, R2_, t2, p1, p2, m, *thr, X_, v_, c_, cnt)

    calls = (decompose, score, front, pose, tri)
    assert [f() for f in calls] == [0] * 5                   # the calls every case below spoils in one place
    for bad, keep in [Kp(k0=0.0), Kp(k0=-1.0), Kp(k0=np.inf), Kp(k0=np.nan), Kp(k4=0.0), Kp(k4=np.nan), Kp(k2=np.inf), Kp(k5=np.nan),
                      Kp(k1=0.5)]:
        assert [f(K_=bad) for f in calls] == [-1] * 5, keep
    assert [f(K_=None) for f in calls] == [-1] * 5
    for m in (0, -1, (1 << 20) + 1):
        assert score(m=m) == -1 and front(m=m) == -1 and pose(m=m) == -1
    assert tri(m=-1) == -1 and tri(m=(1 << 20) + 1) == -1
    assert tri(m=0) == 0 and tri(m=0, p1=None, p2=None, X_=None, v_=None, c_=None) == 0 and n64.value == 0       # m = 0 is no error
    for f in (score, front, pose, tri):
        assert f(p1=None) == -1 and f(p2=None) == -1
    for depth in (0.0, -1.0, np.nan, -np.inf):
        assert score(depth=depth) == -1 and front(depth=depth) == -1 and pose(depth=depth) == -1
    assert score(depth=np.inf) == 0 and front(depth=np.inf) == 0 and pose(depth=np.inf) == 0
    for n in (0, -1, (1 << 20) + 1):
        assert score(n=n) == -1
    assert score(R_=None) == -1 and score(t_=None) == -1 and score(out=None) == -1
    assert front(R_=None) == -1 and front(t_=None) == -1 and front(out=None) == -1 and front(cnt=None) == -1
    assert pose(F_=None) == -1 and pose(R_=None) == -1 and pose(t_=None) == -1 and pose(out=None) == -1 and pose(cnt=None) == -1
    assert pose(info_=None) == -1
    assert decompose(F_=None) == -1 and decompose(R_=None) == -1 and decompose(t_=None) == -1 and decompose(w_=None) == -1
    assert decompose(ok_=None) == -1
    assert tri(R1=None) == -1 and tri(t1=None) == -1 and tri(R2_=None) == -1 and tri(t2=None) == -1 and tri(cnt=None) == -1
    assert tri(X_=None) == -1 and tri(v_=None) == -1 and tri(c_=None) == -1
    for k in range(4):
        thr = [0.01, 200.0, 0.9998, 4.0]
        thr[k] = np.nan
        assert tri(thr=thr) == -1
    assert tri(thr=(-np.inf, np.inf, 2.0, np.inf)) == 0      # infinite thresholds are values, not errors
    assert [f() for f in calls] == [0] * 5                   # and the context still serves
