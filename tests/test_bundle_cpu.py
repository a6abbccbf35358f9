"""The bundle adjustment without a GPU: the ninth header against its binding table, the refusal of a NULL context, and
the restatement of tests/bundle_restatement.py against independent yardsticks -- central finite differences of its own
projection, numpy.linalg.solve on the full damped normal equations, the planted scene, scipy.optimize.least_squares, and
the refit of tests/resection_restatement.py.  tests/test_hip_bundle.py compares the device with the same restatement.

Where a bound is "about ten times the measured value", the measured value stands next to it; ten times leaves room for
another platform's libm and BLAS and still catches a wrong term, which shows in the first digits.

A context needs a device, so the parameter errors behind a valid context are checked in tests/test_hip_bundle.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_inputs as bi  # noqa: E402
import bundle_restatement as br  # noqa: E402
import resection_restatement as rr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_METHODS = ("ba_cost", "ba_normal", "ba_schur", "ba_step", "ba_solve")
DECL = r"^(?:int|const char \*)\s*(amvs_\w+)\("
K = bi.K


def problem(sc, fixed=None):
    return br.Problem(sc["cam"], sc["pt"], sc["uv"], K, sc["C"], sc["P"], fixed)


# ----------------------------------------------------------------------------------------- header and table ---
def test_ninth_header_matches_its_table_and_every_symbol_is_exported():
    from amvs import _lib
    header = open(os.path.join(ROOT, "include", "amvs_bundle.h")).read()
    declared = set(re.findall(DECL, header, re.M))
    assert declared == set(_lib.BA_SIGNATURES) and len(declared) == 5
    assert declared == {"amvs_ba_cost", "amvs_ba_normal", "amvs_ba_schur", "amvs_ba_step", "amvs_ba_solve"}
    others = (_lib.SIGNATURES, _lib.DEPTH_SIGNATURES, _lib.LENS_SIGNATURES, _lib.MATCH_SIGNATURES, _lib.EPIPOLAR_SIGNATURES,
              _lib.PNP_SIGNATURES, _lib.TWOVIEW_SIGNATURES, _lib.STEP_SIGNATURES)
    assert len(others) == 8 and len(_lib.SIGNATURES) == 92
    for table in others:
        assert not declared & set(table)
    for other in ("amvs.h", "amvs_depth.h", "amvs_lens.h", "amvs_match.h", "amvs_epipolar.h", "amvs_resection.h", "amvs_twoview.h",
                  "amvs_step.h"):
        assert not declared & set(re.findall(DECL, open(os.path.join(ROOT, "include", other)).read(), re.M))
    lib = _lib.load()
    for name, (res, args) in _lib.BA_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(args), name
    from amvs.engine import Engine
    for m in ENGINE_METHODS:
        assert callable(getattr(Engine, m)), m
    for name, values in (("AMVS_BA_BLOCK", (br.BLOCK, _lib.BA_BLOCK, 64)), ("AMVS_BA_MAX_CAMERAS", (br.MAX_CAMERAS, _lib.BA_MAX_CAMERAS, 256)),
                         ("AMVS_BA_MAX_POINTS", (br.MAX_POINTS, _lib.BA_MAX_POINTS, 1 << 22)),
                         ("AMVS_BA_MAX_OBS", (br.MAX_OBS, _lib.BA_MAX_OBS, 1 << 24)),
                         ("AMVS_BA_MAX_PAIRS", (br.MAX_PAIRS, _lib.BA_MAX_PAIRS, 1 << 25)),
                         ("AMVS_BA_LAMBDA_MIN", (br.LAMBDA_MIN, _lib.BA_LAMBDA_MIN, 1e-12)),
                         ("AMVS_BA_LAMBDA_MAX", (br.LAMBDA_MAX, _lib.BA_LAMBDA_MAX, 1e12))):
        text = re.search(r"#define %s\s+(.+)" % name, header).group(1).strip()
        defined = float(eval(text, {"__builtins__": {}}))                    # "64", "(1 << 22)" or "1e-12"
        assert all(defined == v for v in values), name
    makefile = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", makefile, re.M).group(1).split()
    assert {"amvs_bundle.o", "amvs_capi_bundle.o"} <= set(objs)
    assert "../../include/amvs_bundle.h" in re.search(r"^%\.o:(.*)$", makefile, re.M).group(1)
    assert "UNPINNED" in header
    from amvs import core
    assert callable(core.bundle_adjust) and callable(core.reprojection_errors)


def test_a_null_context_is_refused_by_every_entry_point_without_a_device():
    from amvs import _lib
    lib = _lib.load()
    d = (C.c_double * 64)()
    i4, f4, u4, n64 = (C.c_int32 * 4)(), (C.c_float * 4)(), (C.c_uint8 * 4)(), C.c_int64(0)
    Kc = (C.c_double * 9)(*K.reshape(9))
    head = (None, d, d, 2, d, 1, i4, i4, f4, 2, Kc)
    calls = {
        "amvs_ba_cost": head + (d, C.byref(n64), d),
        "amvs_ba_normal": head + (u4, d, d, d, d, i4),
        "amvs_ba_schur": head + (u4, 1, 1e-3, d, d, i4, u4),
        "amvs_ba_step": head + (u4, 1, 1e-3, i4, d, d, d, d, d),
        "amvs_ba_solve": head + (u4, 1, 1e-3, 1e-10, 5, d, d, d, d),
    }
    assert set(calls) == set(_lib.BA_SIGNATURES)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1, name
    assert lib.amvs_ba_solve(None, None, None, -3, None, 0, None, None, None, 0, None, None, 1, float("nan"), -1.0, 0, None, None, None,
                             None) == -1                                    # whatever the rest


# ------------------------------------------------------------------------------------------- the Jacobians ---
def residual_vector(q, R, t, X):
    T = br.terms(q, R, t, X)
    return T["rx"], T["ry"]


def test_jacobians_agree_with_central_differences_of_the_projection():
    """Jx, Jy against the perturbation Xc <- Xc + om x Xc + dt of the camera, Px, Py against a moved point.
    Measured: the largest difference relative to the largest entry of the row is 4.5e-10 (h = 1e-6: the truncation of a
    central difference, h^2 times the third derivative, and the rounding 1e-16 / h of a residual of a few
    pixels); asserted 5e-9."""
    sc = bi.scene(4, 30, seed=2, noise=0.5)
    q = problem(sc)
    R, t, X = bi.perturbed(sc, np.zeros(4, bool))
    T = br.terms(q, R, t, X)
    assert T["active"].all()
    h, worst = 1e-6, 0.0
    for i in range(6):
        def moved(s):
            d = np.zeros(6)
            d[i] = s * h
            om, dt = d[:3], d[3:]
            A = np.eye(3) + np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
            Rn = np.array([(A @ R[c].reshape(3, 3)).reshape(9) for c in range(4)])
            tn = np.array([A @ t[c] + dt for c in range(4)])
            return residual_vector(q, Rn, tn, X)
        (xp, yp), (xm, ym) = moved(1.0), moved(-1.0)
        for J, fd in ((T["Jx"][:, i], (xp - xm) / (2 * h)), (T["Jy"][:, i], (yp - ym) / (2 * h))):
            scale = np.maximum(np.abs(T["Jx"]).max(axis=1), np.abs(T["Jy"]).max(axis=1))
            worst = max(worst, float((np.abs(J - fd) / scale).max()))
    for j in range(3):
        Xp, Xm = X.copy(), X.copy()
        Xp[:, j] += h
        Xm[:, j] -= h
        (xp, yp), (xm, ym) = residual_vector(q, R, t, Xp), residual_vector(q, R, t, Xm)
        for J, fd in ((T["Px"][:, j], (xp - xm) / (2 * h)), (T["Py"][:, j], (yp - ym) / (2 * h))):
            scale = np.maximum(np.abs(T["Px"]).max(axis=1), np.abs(T["Py"]).max(axis=1))
            worst = max(worst, float((np.abs(J - fd) / scale).max()))
    print(f"Jacobians against central differences: largest relative difference {worst:.3e}")
    assert worst < 5e-9
    assert np.array_equal(T["W"], T["Jx"][:, :, None] * T["Px"][:, None, :] + T["Jy"][:, :, None] * T["Py"][:, None, :])


# ---------------------------------------------------------------------------------------------- one step ---
def dense_step(q, T, lam):
    """(dc (C, 6), dp (P, 3)) from numpy.linalg.solve on the full damped normal equations."""
    nc = q.n
    J = np.zeros((2 * q.N, nc + 3 * q.P))
    for k in range(q.N):
        a, p = q.slot[q.cam[k]], q.pt[k]
        if a >= 0:
            J[2 * k, 6 * a:6 * a + 6], J[2 * k + 1, 6 * a:6 * a + 6] = T["Jx"][k], T["Jy"][k]
        J[2 * k, nc + 3 * p:nc + 3 * p + 3], J[2 * k + 1, nc + 3 * p:nc + 3 * p + 3] = T["Px"][k], T["Py"][k]
    r = np.stack([T["rx"], T["ry"]], axis=1).reshape(-1)
    H = J.T @ J
    H[np.diag_indices_from(H)] *= 1.0 + lam
    d = np.linalg.solve(H, -(J.T @ r))
    dc = np.zeros((q.C, 6))
    for c in range(q.C):
        if q.slot[c] >= 0:
            dc[c] = d[6 * q.slot[c]:6 * q.slot[c] + 6]
    return dc, d[nc:].reshape(-1, 3)


@pytest.mark.parametrize("lam", [1e-3, 1.0])
def test_one_step_agrees_with_the_full_normal_equations(lam):
    """The Schur complement, the two Cholesky factorisations and the back-substitution against one dense solve of the
    (6 F + 3 P)-square system.  Measured: the largest difference relative to the largest entry of the step is 7.0e-14 at
    lambda = 1e-3 (the rounding unit times the condition number of the damped system with one camera fixed) and 1.7e-15
    at lambda = 1; asserted 7e-13 and 2e-14."""
    sc = bi.scene(5, 40, seed=7, noise=0.5)
    q = problem(sc)
    R, t, X = bi.perturbed(sc, q.fixed)
    T = br.terms(q, R, t, X)
    ok, dc, dp, _, _, _ = br.form_step(q, R, t, X, lam)
    S, rhs, _, held = br.schur(q, R, t, X, lam)
    assert ok and T["active"].all() and not held.any()
    rdc, rdp = dense_step(q, T, lam)
    worst = max(np.abs(dc - rdc).max() / np.abs(rdc).max(), np.abs(dp - rdp).max() / np.abs(rdp).max())
    print(f"lambda = {lam}: one step against numpy.linalg.solve, largest relative difference {worst:.3e}")
    assert worst < (7e-13 if lam == 1e-3 else 2e-14)
    assert np.array_equal(S, S.T)


# ------------------------------------------------------------------------------------------ the iteration ---
def test_solve_returns_the_planted_scene_without_noise():
    """Two cameras fixed at the truth (gauge and scale), the others and the points perturbed, exact pixels rounded to
    float32.  Measured: 4.2e-8 in R, 3.9e-8 in t, 7.1e-7 in X (the float32 rounding of the pixels, 3e-5 px, seen from
    6 units away at f = 1500); asserted 4e-7, 4e-7, 7e-6."""
    sc = bi.scene(6, 80, seed=1)
    fixed = bi.fixed_mask(6, 0, 5)
    q = problem(sc, fixed)
    R, t, X = bi.perturbed(sc, fixed != 0)
    Rn, tn, Xn, info = br.solve(q, R, t, X, max_trials=50)
    dR, dt, dX = np.abs(Rn - sc["R"]).max(), np.abs(tn - sc["t"]).max(), np.abs(Xn - sc["X"]).max()
    print(f"noise-free: |dR| {dR:.3e} |dt| {dt:.3e} |dX| {dX:.3e}; cost {info[3]:.3e} -> {info[4]:.3e}, {int(info[1])} steps kept of {int(info[0])}")
    assert dR < 4e-7 and dt < 4e-7 and dX < 7e-6
    assert info[4] < 1e-6 < info[3] and np.array_equal(Rn[[0, 5]], sc["R"][[0, 5]]) and np.array_equal(tn[[0, 5]], sc["t"][[0, 5]])
    for c in range(6):
        Rm = Rn[c].reshape(3, 3)
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-12


def test_final_cost_agrees_with_scipy_least_squares():
    """The same parameters (the left perturbation of each free camera about the start, the points), the same residuals.
    Measured: the two final costs differ by 5.9e-14 relative (both run until the cost stops falling, ftol = 1e-14);
    asserted 6e-13."""
    scipy_optimize = pytest.importorskip("scipy.optimize")
    sc = bi.scene(4, 30, seed=1, noise=0.5)
    fixed = bi.fixed_mask(4, 0, 3)
    q = problem(sc, fixed)
    R, t, X = bi.perturbed(sc, fixed != 0)
    _, _, _, info = br.solve(q, R, t, X, ftol=1e-14, max_trials=50)
    free = np.flatnonzero(~q.fixed)

    def residuals(x):
        Rn, tn = R.copy(), t.copy()
        for a, c in enumerate(free):
            Rn[c], tn[c] = br.pose_update(x[6 * a:6 * a + 6], R[c], t[c])
        return np.concatenate(residual_vector(q, Rn, tn, X + x[6 * len(free):].reshape(-1, 3)))

    out = scipy_optimize.least_squares(residuals, np.zeros(6 * len(free) + 3 * q.P), method="trf", x_scale=1.0, ftol=1e-14, xtol=1e-14,
                                       gtol=1e-14)
    rel = abs(2.0 * out.cost - info[4]) / info[4]
    print(f"noisy: final cost {info[4]:.9e} against scipy's {2.0 * out.cost:.9e}: relative difference {rel:.3e}")
    assert rel < 6e-13 and info[4] < 0.01 * info[3]


# ------------------------------------------------------------------------------------------ motion only ---
def test_motion_only_of_one_camera_is_the_resections_refit_step():
    """One free camera, every point held, lambda = 0: the sums are those of the resection's refit pass bit for bit, the
    reduced system is (U, -gc) itself, and the step solves what the resection's STEP solves.  The two back solves
    subtract in opposite orders (include/amvs_bundle.h says why), so the poses need only agree to rounding: an entry of
    the step, at most 0.1 here, changes by a few rounding units (1.1e-16) times the condition number of the factor,
    below 1e3 for this camera, so 1e-12 bounds it with room.  Measured: 0.0 (on this input the five subtractions of
    every entry round alike in both orders)."""
    sc = bi.scene(1, 70, seed=3, noise=0.5)
    sc["X"] = sc["X"].astype(np.float32).astype(np.float64)                 # (the resection takes float32 points)
    q = problem(sc, np.zeros(1, np.uint8))
    assert q.F == 1 and np.array_equal(q.pt, np.arange(70))
    R, t, _ = bi.perturbed(sc, np.zeros(1, bool))
    X = sc["X"]
    sums = rr.refit_pass(R[0], t[0], X, q.uv, q.intr, np.ones(70, bool))
    U, gc, _, _, _ = br.normal(q, R, t, X)
    cost, act, _ = br.cost(q, R, t, X)
    assert np.array_equal(U[0], sums[:21]) and np.array_equal(gc[0], sums[21:27]) and cost == sums[27] and act == sums[28] == 70
    S, rhs, _, held = br.schur(q, R, t, X, 0.0, refine_points=0)
    assert held.all() and np.array_equal(S[np.triu_indices(6)], sums[:21]) and np.array_equal(rhs, -sums[21:27])
    ok, _, dp, Rn, tn, Xn = br.form_step(q, R, t, X, 0.0, refine_points=0)
    Rr, tr = rr.gn_step(sums, R[0], t[0])
    worst = max(np.abs(Rn[0] - Rr).max(), np.abs(tn[0] - tr).max())
    print(f"motion only against the resection's step: largest difference {worst:.3e}")
    assert ok and worst < 1e-12 and not dp.any() and np.array_equal(Xn, X)
    # and the iteration is the resection's refit: the same pose to rounding after its steps
    Rs, ts, _, info = br.solve(q, R, t, X, refine_points=0, lambda0=0.0, ftol=0.0, max_trials=rr.REFINE_STEPS)
    Rf, tf, steps, cf = rr.refine(X.astype(np.float32), sc["uv"], K, R[0], t[0])
    assert abs(info[4] - cf) <= 1e-9 * cf and np.abs(Rs[0] - Rf).max() < 1e-9 and np.abs(ts[0] - tf).max() < 1e-9
