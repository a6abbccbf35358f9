"""Bundle adjustment on the device (csrc/amvs_bundle.hip behind include/amvs_bundle.h) against the restatement of
tests/bundle_restatement.py on the scenes of tests/bundle_inputs.py: the cost, the normal sums, the reduced system, one
step and the whole iteration, core/bundle.py, and the parameter errors behind a valid context.  Every comparison is bit
for bit and leaves no element out; a NaN matches a NaN.  tests/test_bundle_cpu.py shows on the CPU that the restatement
does what it should."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_inputs as bi  # noqa: E402
import bundle_restatement as br  # noqa: E402

pytestmark = pytest.mark.gpu
K = bi.K
PANEL = 32                       # the columns of a Cholesky panel of csrc/amvs_bundle.hip (NB)


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


def problem(sc, fixed=None):
    return br.Problem(sc["cam"], sc["pt"], sc["uv"], K, sc["C"], sc["P"], fixed)


def obs(sc):
    return sc["cam"], sc["pt"], sc["uv"], K


# ---- what is compared ----------------------------------------------------------------------------------------------------------
def check_cost_and_normal(eng, sc, R, t, X, fixed=None):
    q = problem(sc, fixed)
    rc, ra, rerr = br.cost(q, R, t, X)
    c, a, err = eng.ba_cost(R, t, X, *obs(sc))
    assert same_bits([c], [rc]) and a == ra and same_bits(err, rerr)
    rU, rgc, rV, rgp, rcnt = br.normal(q, R, t, X)
    U, gc, V, gp, cnt = eng.ba_normal(R, t, X, *obs(sc), fixed=fixed)
    assert same_bits(U, rU) and same_bits(gc, rgc) and same_bits(V, rV) and same_bits(gp, rgp)
    assert cnt.dtype == np.int32 and np.array_equal(cnt, rcnt)
    return rcnt, rerr


def check_schur(eng, sc, R, t, X, lam, fixed=None, refine_points=True):
    q = problem(sc, fixed)
    rS, rrhs, rslot, rheld = br.schur(q, R, t, X, lam, refine_points)
    S, rhs, slot, held = eng.ba_schur(R, t, X, *obs(sc), lam, fixed=fixed, refine_points=refine_points)
    assert S.shape == (q.n, q.n) and np.array_equal(slot, rslot) and np.array_equal(held, rheld)
    assert same_bits(S, rS) and same_bits(rhs, rrhs)
    assert same_bits(S, S.T)
    return rS, rheld


def check_step(eng, sc, R, t, X, lam, fixed=None, refine_points=True):
    q = problem(sc, fixed)
    rok, rdc, rdp, rR, rt, rX = br.form_step(q, R, t, X, lam, refine_points)
    ok, dc, dp, Rn, tn, Xn = eng.ba_step(R, t, X, *obs(sc), lam, fixed=fixed, refine_points=refine_points)
    assert ok == rok
    assert same_bits(dc, rdc) and same_bits(dp, rdp)
    assert same_bits(Rn.reshape(-1, 9), rR) and same_bits(tn, rt) and same_bits(Xn, rX)
    if not rok:
        for a in (dc, dp, Rn, tn, Xn):
            assert not a.any() and not np.signbit(a).any()                  # the zeros of "no step" are +0.0
    return rok, rdc, rdp


def check_solve(eng, sc, R, t, X, fixed=None, refine_points=True, **kw):
    q = problem(sc, fixed)
    trace = []
    rR, rt, rX, rinfo = br.solve(q, R, t, X, refine_points, trace=trace, **kw)
    Rn, tn, Xn, info = eng.ba_solve(R, t, X, *obs(sc), fixed=fixed, refine_points=refine_points, **kw)
    got = [info["trials"], info["kept"], info["lambda"], info["first_cost"], info["cost"], info["active"]]
    assert same_bits(got, rinfo), (got, rinfo)
    assert same_bits(Rn.reshape(-1, 9), rR) and same_bits(tn, rt) and same_bits(Xn, rX)
    return rinfo, trace, (Rn, tn, Xn)


# ---- the scene of list lengths and point kinds ---------------------------------------------------------------------------------
_LISTS = {}


def lists_case(name):
    """(scene, R, t, X, fixed) of a configuration of the lists scene, started 0.3 pixels of noise and a small step off."""
    if "scene" not in _LISTS:
        _LISTS["scene"] = bi.lists_scene()
    sc = _LISTS["scene"]
    fixed = {"null": None, "two": bi.fixed_mask(8, 0, 7), "middle": bi.fixed_mask(8, 3), "all but one": bi.fixed_mask(8, 0, 1, 2, 3, 5, 6, 7),
             "idle": None}[name]
    R, t, X = bi.perturbed(sc, np.zeros(8, bool), rot=0.002, trans=0.005, pts=0.005, seed=3)
    X[130], X[131] = sc["X"][130], sc["X"][131]                             # (the two points placed behind a camera stay there)
    if name == "idle":
        Ri, ti = bi.with_idle(sc, 2)
        R[2], t[2] = Ri[2], ti[2]
    return sc, R, t, X, fixed


def test_the_lists_scene_has_the_lengths_it_is_for():
    sc = bi.lists_scene()
    q = problem(sc)
    assert [len(q.lists[c]) for c in range(1, 6)] == [1, 63, 64, 65, 129]
    shared = {(a, b): int(np.count_nonzero(np.isin(sc["pt"][q.lists[a]], sc["pt"][q.lists[b]]))) for a in range(1, 8) for b in range(a + 1, 8)}
    assert shared[(1, 6)] == 0 and shared[(2, 6)] == 0 and shared[(1, 2)] == 1 and shared[(3, 4)] == 64 and shared[(4, 5)] == 65
    assert shared[(2, 3)] == 63


@pytest.mark.parametrize("name", ["null", "idle"])
def test_cost_and_normal_sums_bit_for_bit(eng, name):
    sc, R, t, X, fixed = lists_case(name)
    cnt, err2 = check_cost_and_normal(eng, sc, R, t, X, fixed)
    assert cnt[129] == 1 and cnt[130] == 0 and cnt[131] == 1               # one observation; all behind; one active, one not
    assert (err2 < 0).sum() == (3 if name == "null" else 3 + 63) and err2[err2 >= 0].max() < 400.0


@pytest.mark.parametrize("lam", [1e-3, 1e6])
@pytest.mark.parametrize("name", ["null", "two", "middle", "all but one", "idle"])
def test_schur_and_step_bit_for_bit(eng, name, lam):
    sc, R, t, X, fixed = lists_case(name)
    S, held = check_schur(eng, sc, R, t, X, lam, fixed)
    assert held[129] and held[130] and held[131] and held.sum() == 3
    q = problem(sc, fixed)
    if name == "idle":
        a = 6 * q.slot[2]
        assert np.array_equal(S[a:a + 6, a:a + 6], np.eye(6)) and not S[a:a + 6, :a].any() and not S[a:a + 6, a + 6:].any()
    if name == "null":
        a, b = 6 * q.slot[1], 6 * q.slot[6]                                 # cameras 1 and 6 share no point
        assert not S[a:a + 6, b:b + 6].any() and not np.signbit(S[a:a + 6, b:b + 6]).any()
    ok, dc, dp = check_step(eng, sc, R, t, X, lam, fixed)
    assert ok and np.isfinite(dc).all() and np.isfinite(dp).all()
    if name == "two":
        assert not held[132] and dp[132].any()                              # seen by fixed cameras only: it still moves
    assert not dc[q.fixed].any() and not dp[held].any()


def test_no_damping_with_the_gauge_fixed(eng):
    """lambda = 0 and two fixed cameras; the camera with one observation is fixed too, or S would be singular."""
    sc, R, t, X, _ = lists_case("two")
    fixed = bi.fixed_mask(8, 0, 1, 7)
    check_schur(eng, sc, R, t, X, 0.0, fixed)
    ok, _, _ = check_step(eng, sc, R, t, X, 0.0, fixed)
    assert ok


def test_motion_only_mode_holds_every_point(eng):
    sc, R, t, X, fixed = lists_case("two")
    _, held = check_schur(eng, sc, R, t, X, 1e-3, fixed, refine_points=False)
    assert held.all()
    ok, dc, dp = check_step(eng, sc, R, t, X, 1e-3, fixed, refine_points=False)
    assert ok and not dp.any() and dc[1:7].any(axis=1).all()


def test_no_step_returns_zeros(eng):
    """Without damping the camera that sees one point has a singular block (found on the CPU: the restatement reports
    NO STEP); so does a state with an infinite point, whose sums are NaN."""
    sc, R, t, X, fixed = lists_case("null")
    ok, _, _ = check_step(eng, sc, R, t, X, 0.0, fixed)
    assert not ok
    Xi = X.copy()
    Xi[5, 0] = np.inf
    check_schur(eng, sc, R, t, Xi, 1e-3, fixed)
    ok, _, _ = check_step(eng, sc, R, t, Xi, 1e-3, fixed)
    assert not ok
    info, trace, _ = check_solve(eng, sc, R, t, Xi, fixed, max_trials=20)
    assert info[1] == 0 and info[2] > br.LAMBDA_MAX and all(w[0] == "no step" for w in trace) and np.isnan(info[4])


# ---- the number of free cameras ------------------------------------------------------------------------------------------------
# n = 6 F: 6 (one free camera of two), 36 (just above one panel of the Cholesky), 42 and 66 (no multiple of a wave; 66 is just
# above two panels)
@pytest.mark.parametrize("C,fixed", [(2, None), (7, None), (8, None), (12, None), (9, (4,)), (9, (0, 1, 2, 3, 5, 6, 7, 8))])
def test_camera_counts(eng, C, fixed):
    sc = bi.scene(C, 60, seed=C, noise=0.5, mean_track=3)
    fx = None if fixed is None else bi.fixed_mask(C, *fixed)
    q = problem(sc, fx)
    assert q.n in (6, 36, 42, 66, 48) and (C != 7 or q.n == PANEL + 4)
    R, t, X = bi.perturbed(sc, q.fixed, seed=C)
    check_cost_and_normal(eng, sc, R, t, X, fx)
    check_schur(eng, sc, R, t, X, 1e-3, fx)
    ok, _, _ = check_step(eng, sc, R, t, X, 1e-3, fx)
    assert ok
    info, _, _ = check_solve(eng, sc, R, t, X, fx, max_trials=8)
    assert info[1] >= 2 and info[4] < info[3]


# n = 300: the rows below a panel need two workgroups of 256 lanes (n - 32 > 256) and the update a grid of 9 x 9 tiles.
# n = 1 062: the loops of the one-workgroup triangular solves pass their stride of 1 024, the rows need four workgroups.
@pytest.mark.parametrize("C", [51, 178])
def test_large_systems(eng, C):
    sc = bi.scene(C, 3 * C, seed=C, noise=0.5, mean_track=4)
    q = problem(sc)
    assert q.n == 6 * (C - 1) and q.n in (300, 1062)
    R, t, X = bi.perturbed(sc, q.fixed, rot=0.002, trans=0.005, pts=0.005, seed=C)
    ok, dc, _ = check_step(eng, sc, R, t, X, 1e-3)                      # (S and rhs are inside: the step is their solution)
    assert ok and dc[1:].any(axis=1).all()
    if C == 51:
        check_schur(eng, sc, R, t, X, 1e-3)
        info, _, _ = check_solve(eng, sc, R, t, X, max_trials=3)
        assert info[1] >= 2 and info[4] < info[3]


# ---- the iteration -------------------------------------------------------------------------------------------------------------
_SOLVE = {}


def solve_scene():
    """12 cameras, 700 points, 2 852 observations."""
    if not _SOLVE:
        for name, noise in (("noise-free", 0.0), ("noisy", 0.5)):
            _SOLVE[name] = bi.scene(12, 700, seed=3, noise=noise, mean_track=4)
        _SOLVE["outliers"], _SOLVE["at"] = bi.with_outliers(_SOLVE["noisy"])
    return _SOLVE


@pytest.mark.parametrize("name", ["noise-free", "noisy", "outliers"])
def test_solve_end_to_end(eng, name):
    sc = solve_scene()[name]
    assert sc["C"] <= 12 and len(sc["cam"]) <= 3000
    fixed = bi.fixed_mask(12, 0, 11)
    R, t, X = bi.perturbed(sc, fixed != 0)
    info, trace, (Rn, tn, Xn) = check_solve(eng, sc, R, t, X, fixed)
    assert info[1] >= 3 and info[4] < (0.2 if name == "outliers" else 0.01) * info[3]     # (the two outliers keep 13 % of the cost)
    if name == "noise-free":
        assert np.abs(Rn.reshape(-1, 9) - sc["R"]).max() < 1e-5 and np.abs(Xn - sc["X"]).max() < 1e-4
    if name == "outliers":
        _, _, err2 = eng.ba_cost(Rn, tn, Xn, *obs(sc))
        assert set(np.argsort(err2)[-2:]) == set(solve_scene()["at"])       # what a caller filters by


def test_solve_motion_only(eng):
    sc = solve_scene()["noisy"]
    fixed = bi.fixed_mask(12, 0)
    R, t, _ = bi.perturbed(sc, fixed != 0)
    info, _, (_, _, Xn) = check_solve(eng, sc, R, t, sc["X"], fixed, refine_points=False)
    assert same_bits(Xn, sc["X"]) and info[1] >= 2 and info[4] < 0.01 * info[3]


def test_a_step_that_is_not_kept_raises_lambda_and_goes_on(eng):
    """With ftol = 0 the iteration does not stop at convergence: steps there raise the cost by rounding, are not kept, and
    lambda goes up until a step is kept again or lambda passes its maximum."""
    sc = bi.scene(6, 80, seed=1, noise=0.5)
    fixed = bi.fixed_mask(6, 0, 1)
    R, t, X = bi.perturbed(sc, fixed != 0)
    info, trace, _ = check_solve(eng, sc, R, t, X, fixed, ftol=0.0, max_trials=30)
    what = [w[0] for w in trace]
    first = what.index("rejected")
    assert first < len(what) - 1 and info[0] > info[1] >= 3


# ---- core/bundle.py ------------------------------------------------------------------------------------------------------------
def test_bundle_adjust_sorts_reports_and_refuses_duplicates(eng):
    from amvs.core import bundle_adjust, reprojection_errors
    from amvs.core.camera import CameraPose

    class Camera:
        K = bi.K

    sc = bi.scene(5, 50, seed=9, noise=0.5)
    views, ids = [3, 10, 11, 20, 42], [100 + 7 * p for p in range(50)]     # names that are no indices
    R, t, X = bi.perturbed(sc, np.arange(5) == 0)
    poses = {v: CameraPose(R[i].reshape(3, 3), t[i]) for i, v in enumerate(views)}
    points = {p: X[i] for i, p in enumerate(ids)}
    rows = np.array([(views[c], ids[p], u, v) for c, p, (u, v) in zip(sc["cam"], sc["pt"], sc["uv"].astype(np.float64))])
    new_poses, new_points, report = bundle_adjust(Camera, poses, points, rows, engine=eng)
    Rn, tn, Xn, info = eng.ba_solve(R, t, X, *obs(sc))
    for i, v in enumerate(views):
        assert same_bits(new_poses[v].R, Rn[i]) and same_bits(new_poses[v].t, tn[i])
    assert same_bits(np.array([new_points[p] for p in ids]), Xn)
    assert {k: report[k] for k in info} == info
    _, _, e0 = br.cost(problem(sc), R, t, X)
    _, _, e1 = br.cost(problem(sc), Rn.reshape(-1, 9), tn, Xn)
    assert report["mean_error_before"] == float(np.sqrt(e0).mean()) and report["mean_error_after"] == float(np.sqrt(e1).mean())
    assert report["mean_error_after"] < 1.0 < report["mean_error_before"]
    shuffle = np.random.default_rng(0).permutation(len(rows))
    again_poses, again_points, again = bundle_adjust(Camera, poses, points, rows[shuffle], engine=eng)
    assert again == report and all(same_bits(again_points[p], new_points[p]) for p in ids)
    assert all(same_bits(again_poses[v].R, new_poses[v].R) and same_bits(again_poses[v].t, new_poses[v].t) for v in views)
    errs = reprojection_errors(Camera, poses, points, rows[shuffle], engine=eng)
    assert same_bits(errs, np.sqrt(e0)[shuffle])
    # an array of points and fixed view names
    arr_poses, arr_points, _ = bundle_adjust(Camera, poses, X, np.column_stack([rows[:, 0], sc["pt"], rows[:, 2:]]), fixed=[3, 42],
                                             engine=eng)
    Rf, tf, Xf, _ = eng.ba_solve(R, t, X, *obs(sc), fixed=bi.fixed_mask(5, 0, 4))
    assert same_bits(arr_points, Xf) and same_bits(arr_poses[42].R, R[4].reshape(3, 3)) and same_bits(arr_poses[11].t, tf[2])
    with pytest.raises(ValueError):
        bundle_adjust(Camera, poses, points, np.concatenate([rows, rows[7:8]]), engine=eng)
    with pytest.raises(ValueError):
        bundle_adjust(Camera, poses, points, rows, fixed=[4], engine=eng)


# ---- the parameter errors ------------------------------------------------------------------------------------------------------
def test_every_parameter_error_is_einval_and_leaves_the_outputs_untouched(eng):
    from amvs import _lib
    lib = eng._lib
    sc = bi.scene(3, 8, seed=4)
    N, Cn, P = len(sc["cam"]), 3, 8
    f64p, i32p, f32p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    base = {"R": sc["R"].copy(), "t": sc["t"].copy(), "X": sc["X"].copy(), "cam": sc["cam"].copy(), "pt": sc["pt"].copy(),
            "uv": sc["uv"].copy(), "K": K.reshape(9).copy(), "fixed": bi.fixed_mask(3, 1)}
    SENTINEL = 7.0

    def ptr(a):
        if a is None:
            return None
        kind = {np.dtype(np.float64): f64p, np.dtype(np.int32): i32p, np.dtype(np.float32): f32p, np.dtype(np.uint8): u8p,
                np.dtype(np.int64): C.POINTER(C.c_int64)}[a.dtype]
        return a.ctypes.data_as(kind)

    def call(name, arrays, dims=(Cn, P, N), scalars=None, null_out=None):
        """rc and whether every output still holds the sentinel."""
        a = arrays
        Cc, Pp, Nn = dims
        head = [eng._h, ptr(a["R"]), ptr(a["t"]), Cc, ptr(a["X"]), Pp, ptr(a["cam"]), ptr(a["pt"]), ptr(a["uv"]), Nn, ptr(a["K"])]
        n = 6 * 2
        outs = {"amvs_ba_cost": [np.full(1, SENTINEL), np.full(1, 7, np.int64), np.full(N, SENTINEL)],
                "amvs_ba_normal": [np.full((Cn, 21), SENTINEL), np.full((Cn, 6), SENTINEL), np.full((P, 6), SENTINEL), np.full((P, 3), SENTINEL),
                                   np.full(P, 7, np.int32)],
                "amvs_ba_schur": [np.full((n, n), SENTINEL), np.full(n, SENTINEL), np.full(Cn, 7, np.int32), np.full(P, 7, np.uint8)],
                "amvs_ba_step": [np.full(1, 7, np.int32), np.full((Cn, 6), SENTINEL), np.full((P, 3), SENTINEL), np.full((Cn, 9), SENTINEL),
                                 np.full((Cn, 3), SENTINEL), np.full((P, 3), SENTINEL)],
                "amvs_ba_solve": [np.full((Cn, 9), SENTINEL), np.full((Cn, 3), SENTINEL), np.full((P, 3), SENTINEL), np.full(6, SENTINEL)]}[name]
        s = {"lam": 1e-3, "ftol": 1e-10, "max_trials": 5}
        s.update(scalars or {})
        mid = {"amvs_ba_cost": [], "amvs_ba_normal": [ptr(a["fixed"])], "amvs_ba_schur": [ptr(a["fixed"]), 1, s["lam"]],
               "amvs_ba_step": [ptr(a["fixed"]), 1, s["lam"]],
               "amvs_ba_solve": [ptr(a["fixed"]), 1, s["lam"], s["ftol"], s["max_trials"]]}[name]
        po = [ptr(o) for o in outs]
        if null_out is not None:
            po[null_out] = None
        rc = getattr(lib, name)(*head, *mid, *po)
        return rc, all((o == 7).all() for o in outs)

    names = list(_lib.BA_SIGNATURES)
    assert len(names) == 5
    for name in names:
        rc, untouched = call(name, base)
        assert rc == 0 and not untouched, name                              # the valid call works and writes
        bad = []
        for key in ("R", "t", "X", "cam", "pt", "uv", "K"):
            bad.append(({**base, key: None}, {}))
        for at, v in ((0, 0.0), (0, -1.0), (0, np.inf), (4, np.nan), (2, np.inf), (5, np.nan), (1, 0.5)):
            Kb = base["K"].copy()
            Kb[at] = v
            bad.append(({**base, "K": Kb}, {}))
        for dims in ((0, P, N), (_lib.BA_MAX_CAMERAS + 1, P, N), (Cn, 0, N), (Cn, _lib.BA_MAX_POINTS + 1, N), (Cn, P, 0), (Cn, P, -1),
                     (Cn, P, _lib.BA_MAX_OBS + 1), (2, P, N), (Cn, 7, N)):      # (the last two: an index out of range)
            bad.append((base, {"dims": dims}))
        for key, at, v in (("cam", 2, -1), ("cam", 2, Cn), ("pt", 2, -1), ("pt", N - 1, P)):
            arr = base[key].copy()
            arr[at] = v
            bad.append(({**base, key: arr}, {}))
        swapped = base["cam"].copy()
        swapped[[0, 1]] = swapped[[1, 0]]                                   # point 0 is seen by every camera: descending
        bad.append(({**base, "cam": swapped}, {}))
        twice = base["cam"].copy()
        twice[1] = twice[0]
        bad.append(({**base, "cam": twice}, {}))
        down = base["pt"].copy()
        down[-1] = 0
        bad.append(({**base, "pt": down}, {}))
        if name != "amvs_ba_cost":
            bad.append(({**base, "fixed": np.ones(3, np.uint8)}, {}))       # no free camera
        if name in ("amvs_ba_schur", "amvs_ba_step", "amvs_ba_solve"):
            for v in (-1e-9, np.inf, np.nan):
                bad.append((base, {"scalars": {"lam": v}}))
        if name == "amvs_ba_solve":
            for v in (-1e-9, np.inf, np.nan):
                bad.append((base, {"scalars": {"ftol": v}}))
            bad.append((base, {"scalars": {"max_trials": 0}}))
        n_out = {"amvs_ba_cost": 3, "amvs_ba_normal": 5, "amvs_ba_schur": 4, "amvs_ba_step": 6, "amvs_ba_solve": 4}[name]
        for i in range(n_out):
            bad.append((base, {"null_out": i}))
        for arrays, kw in bad:
            rc, untouched = call(name, arrays, **kw)
            assert rc == -1 and untouched, (name, kw, [k for k in arrays if arrays[k] is not base[k]])
    # more than AMVS_BA_MAX_PAIRS pairs: 1 030 points seen by each of 255 free cameras have 32 640 pairs each
    Cb, Pb = 256, 1030
    big = {"R": np.zeros((Cb, 9)), "t": np.zeros((Cb, 3)), "X": np.zeros((Pb, 3)), "cam": np.tile(np.arange(Cb, dtype=np.int32), Pb),
           "pt": np.repeat(np.arange(Pb, dtype=np.int32), Cb), "uv": np.zeros((Cb * Pb, 2), np.float32), "K": base["K"], "fixed": None}
    assert Pb * 255 * 256 // 2 > _lib.BA_MAX_PAIRS >= (Pb - 2) * 255 * 256 // 2
    out = [np.full((Cb, 9), SENTINEL), np.full((Cb, 3), SENTINEL), np.full((Pb, 3), SENTINEL), np.full(6, SENTINEL)]
    rc = lib.amvs_ba_solve(eng._h, ptr(big["R"]), ptr(big["t"]), Cb, ptr(big["X"]), Pb, ptr(big["cam"]), ptr(big["pt"]), ptr(big["uv"]),
                           Cb * Pb, ptr(big["K"]), None, 1, 1e-3, 1e-10, 1, *[ptr(o) for o in out])
    assert rc == -1 and all((o == 7).all() for o in out) and b"AMVS_BA_MAX_PAIRS" in lib.amvs_last_error(eng._h)
    # fixed = NULL with one camera: camera 0 is fixed and nothing is free; the cost needs no free camera
    one = {**base, "cam": np.zeros(2, np.int32), "pt": np.arange(2, dtype=np.int32), "fixed": None}
    assert call("amvs_ba_cost", one, dims=(1, P, 2))[0] == 0
    assert call("amvs_ba_normal", one, dims=(1, P, 2)) == (-1, True)
    assert b"free camera" in lib.amvs_last_error(eng._h)
