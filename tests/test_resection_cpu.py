"""Camera resection without a GPU: the seventh header against its binding table, the refusal of a NULL context, the
restatement of tests/resection_restatement.py against independent yardsticks (a sampler loop in Python integers,
numpy.linalg.svd for the DLT null vector and the nearest rotation, numpy.linalg.solve for the normal equations, the
planted poses and inliers), the stopping rule on the scenes the GPU comparison uses, and the host logic of
core/registration.py with a fake engine.  tests/test_hip_resection.py compares the device with the same restatement.

A context needs a device, so the parameter errors behind a valid context are checked in tests/test_hip_resection.py."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resection_inputs as ri  # noqa: E402
import resection_restatement as rr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_METHODS = ("pnp_hypotheses", "pnp_score", "pnp_inliers", "pnp_refine", "pnp_ransac")
DECL = r"^(?:int|const char \*)\s*(amvs_\w+)\("
SEED = 1234


# ----------------------------------------------------------------------------------------- header and table ---
def test_seventh_header_matches_its_table_and_every_symbol_is_exported():
    from amvs import _lib
    header = open(os.path.join(ROOT, "include", "amvs_resection.h")).read()
    declared = set(re.findall(DECL, header, re.M))
    assert declared == set(_lib.PNP_SIGNATURES) and len(declared) == 5
    for table in (_lib.SIGNATURES, _lib.DEPTH_SIGNATURES, _lib.LENS_SIGNATURES, _lib.MATCH_SIGNATURES, _lib.EPIPOLAR_SIGNATURES,
                  _lib.STEP_SIGNATURES):
        assert not declared & set(table)
    for other in ("amvs.h", "amvs_depth.h", "amvs_lens.h", "amvs_match.h", "amvs_epipolar.h", "amvs_step.h"):
        assert not declared & set(re.findall(DECL, open(os.path.join(ROOT, "include", other)).read(), re.M))
    lib = _lib.load()
    for name, (res, args) in _lib.PNP_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(args), name
    from amvs.engine import Engine
    for m in ENGINE_METHODS:
        assert callable(getattr(Engine, m)), m
    for name, value in (("AMVS_PNP_BATCH", rr.BATCH), ("AMVS_PNP_BLOCK", rr.BLOCK), ("AMVS_PNP_BATCH", ri.BATCH),
                        ("AMVS_PNP_BLOCK", ri.BLOCK), ("AMVS_PNP_BATCH", _lib.PNP_BATCH), ("AMVS_PNP_BLOCK", _lib.PNP_BLOCK),
                        ("AMVS_PNP_REFINE_STEPS", rr.REFINE_STEPS), ("AMVS_PNP_REFINE_STEPS", _lib.PNP_REFINE_STEPS),
                        ("AMVS_PNP_MAX_POINTS", 1 << 20), ("AMVS_PNP_MAX_HYP", 1 << 20), ("AMVS_PNP_MAX_POINTS", _lib.PNP_MAX_POINTS),
                        ("AMVS_PNP_MAX_HYP", _lib.PNP_MAX_HYP)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, header).group(1)) == value
    assert repr(rr.ROOT3) in header and rr.ROOT3 == math.sqrt(3.0)
    match_h = open(os.path.join(ROOT, "include", "amvs_match.h")).read()
    assert int(re.search(r"#define AMVS_JACOBI_SWEEPS\s+(\d+)", match_h).group(1)) == rr.JACOBI_SWEEPS
    makefile = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", makefile, re.M).group(1).split()
    assert {"amvs_pnp.o", "amvs_capi_pnp.o"} <= set(objs)
    assert "../../include/amvs_resection.h" in re.search(r"^%\.o:(.*)$", makefile, re.M).group(1)
    assert "UNPINNED" in header and "PLANAR" in header


def test_a_null_context_is_refused_by_every_entry_point_without_a_device():
    from amvs import _lib
    lib = _lib.load()
    d9, d3, f18, f12, u8 = (C.c_double * 9)(), (C.c_double * 3)(), (C.c_float * 18)(), (C.c_float * 12)(), (C.c_uint8 * 6)()
    K = (C.c_double * 9)(*ri.K.reshape(9))
    i6, i3, n64, steps, cost = (C.c_int32 * 6)(), (C.c_int32 * 3)(), C.c_int64(0), C.c_int32(0), C.c_double(0.0)
    calls = {
        "amvs_pnp_hypotheses": (None, f18, f12, 6, K, 0, 0, 1, i6, d9, d3),
        "amvs_pnp_score": (None, d9, d3, 1, f18, f12, 6, K, 8.0, i3),
        "amvs_pnp_inliers": (None, d9, d3, f18, f12, 6, K, 8.0, u8, C.byref(n64)),
        "amvs_pnp_refine": (None, f18, f12, 6, K, d9, d3, None, d9, d3, C.byref(steps), C.byref(cost), C.byref(n64)),
        "amvs_pnp_ransac": (None, f18, f12, 6, K, 8.0, 0.99, 1, 0, d9, d3, u8, C.byref(n64), i3),
    }
    assert set(calls) == set(_lib.PNP_SIGNATURES)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1, name
    assert lib.amvs_pnp_ransac(None, None, None, -3, None, -1.0, 7.0, 0, 0, None, None, None, None, None) == -1   # whatever the rest


# ----------------------------------------------------------------------------------------------- the sampler ---
MASK = (1 << 64) - 1


def mix_int(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def sample_loop(seed, h, m):
    """The header's sampler for one hypothesis, in Python integers."""
    chosen = []
    for k in range(6):
        r = mix_int(seed ^ mix_int(6 * h + k)) % (m - k)
        for c in sorted(chosen):
            if r >= c:
                r += 1
        chosen.append(r)
    return chosen


@pytest.mark.parametrize("m", [6, 7, 64, 1000, 1 << 20])
def test_sampler_draws_6_distinct_indices_and_is_the_loop(m):
    seed = 0xDEADBEEFCAFEF00D
    idx = rr.sample(seed, np.arange(4096), m)
    assert idx.shape == (4096, 6) and idx.min() >= 0 and idx.max() < m
    assert (np.diff(np.sort(idx, axis=1), axis=1) > 0).all()
    assert idx.tolist() == [sample_loop(seed, h, m) for h in range(4096)]
    if m == 6:
        assert (np.sort(idx, axis=1) == np.arange(6)).all()
    else:
        assert len(np.unique(idx[:, 0])) > 1 and len(np.unique(np.sort(idx, axis=1), axis=0)) > (1 if m == 7 else 1000)
    assert np.array_equal(rr.sample(seed, np.arange(1000, 1010), m), idx[1000:1010])       # a function of h alone


# -------------------------------------------------------------------------- hypotheses against the SVD route ---
def pose_svd(X, x):
    """6-point DLT and the nearest rotation, both by numpy.linalg.svd, with the Hartley scaling of the 3D points."""
    X, x = X.astype(np.float64), x.astype(np.float64)
    xn = (x - ri.K[:2, 2]) / np.array([ri.K[0, 0], ri.K[1, 1]])
    c = X.mean(axis=0)
    s = math.sqrt(3.0) / np.linalg.norm(X - c, axis=1).mean()
    P = np.concatenate([(X - c) * s, np.ones((len(X), 1))], axis=1)
    Z = np.zeros_like(P)
    rows = np.concatenate([np.concatenate([P, Z, -xn[:, :1] * P], axis=1), np.concatenate([Z, P, -xn[:, 1:] * P], axis=1)])
    p = np.linalg.svd(rows)[2][-1].reshape(3, 4)
    A, b = p[:, :3] * s, p[:, 3] - (p[:, :3] * s) @ c
    if np.linalg.det(A) < 0:
        A, b = -A, -b
    U, S, Vt = np.linalg.svd(A)
    return U @ Vt, b / S.mean()


@pytest.mark.parametrize("name", list(ri.FAMILY))
def test_hypotheses_agree_with_the_svd_route_and_are_rotations(name):
    X, x, planted = ri.family_scene(name)
    idx, R, t, M = rr.hypotheses(X, x, ri.K, SEED, 0, 1024, return_state=True)
    diag = np.abs(M[:, np.arange(12), np.arange(12)]).max(axis=1)
    off = np.abs(M - M * np.eye(12)).max(axis=(1, 2))
    clean = np.flatnonzero(planted[idx].all(axis=1))[:32]                # samples without a planted outlier: well posed
    dR, dt = 0.0, 0.0
    for j in clean:
        Rs, ts = pose_svd(X[idx[j]], x[idx[j]])
        dR, dt = max(dR, np.abs(R[j].reshape(3, 3) - Rs).max()), max(dt, np.abs(t[j] - ts).max())
    Rm = R.reshape(-1, 3, 3)
    orth_all = np.abs(np.einsum("hki,hkj->hij", Rm, Rm) - np.eye(3)).max(axis=(1, 2))
    det_all = np.abs(np.linalg.det(Rm) - 1.0)
    orth, det = orth_all[clean].max(), det_all[clean].max()
    print(f"{name}: 1024 hypotheses, largest off-diagonal entry after {rr.JACOBI_SWEEPS} sweeps relative to the largest diagonal "
          f"entry {(off / diag).max():.3e}; {len(clean)} outlier-free samples against the SVD route: largest difference in R "
          f"{dR:.3e}, in t {dt:.3e}, |R^T R - I| <= {orth:.3e}, |det R - 1| <= {det:.3e}; over all 1024 (samples with planted "
          f"outliers included, whose A can be close to singular) |R^T R - I| <= {orth_all.max():.3e}, |det R - 1| <= {det_all.max():.3e}")
    assert len(clean) >= 8 and np.isfinite(R).all() and np.isfinite(t).all()
    assert (off < 1e-30 * diag).all()
    assert orth < 1e-12 and det < 1e-12                # (A^T A squares the conditioning of A: a near-singular A loses more)
    # No bit comparison: the SVD of the 12 x 12 system and Jacobi on its normal matrix differ by about the rounding unit
    # over the relative gap between the two smallest eigenvalues of that matrix.  With 0.5 px of noise on f = 1500 the
    # smallest is some 1e-7 of the largest and the next one far above it, so ten digits are expected (the differences are
    # printed and recorded in DESIGN.md section 14); three are asserted, which a wrong row or sign cannot pass.
    assert dR < 1e-3 and dt < 1e-2


# ------------------------------------------------------------------------------ the refit against linalg.solve ---
def gauss_newton_reference(X, x, R, t, iterations=10):
    """Gauss-Newton on the same left perturbation with numpy.linalg.solve and a Rodrigues update."""
    X, x = X.astype(np.float64), x.astype(np.float64)
    fx, fy, cx, cy = ri.K[0, 0], ri.K[1, 1], ri.K[0, 2], ri.K[1, 2]
    for _ in range(iterations):
        Xc = X @ R.T + t
        z = Xc[:, 2]
        r = np.concatenate([fx * Xc[:, 0] / z + cx - x[:, 0], fy * Xc[:, 1] / z + cy - x[:, 1]])
        zero = np.zeros_like(z)
        dx = np.stack([fx / z, zero, -fx * Xc[:, 0] / z ** 2], axis=1)
        dy = np.stack([zero, fy / z, -fy * Xc[:, 1] / z ** 2], axis=1)
        skew = np.zeros((len(X), 3, 3))
        skew[:, 0, 1], skew[:, 0, 2], skew[:, 1, 0] = Xc[:, 2], -Xc[:, 1], -Xc[:, 2]
        skew[:, 1, 2], skew[:, 2, 0], skew[:, 2, 1] = Xc[:, 0], Xc[:, 1], -Xc[:, 0]
        J = np.concatenate([np.concatenate([np.einsum("ni,nij->nj", d, skew), d], axis=1) for d in (dx, dy)])
        step = np.linalg.solve(J.T @ J, -J.T @ r)
        ang = np.linalg.norm(step[:3])
        Q = ri.rodrigues(step[:3], math.degrees(ang)) if ang > 0 else np.eye(3)
        R, t = Q @ R, Q @ t + step[3:]
    Xc = X @ R.T + t
    cost = ((fx * Xc[:, 0] / Xc[:, 2] + cx - x[:, 0]) ** 2 + (fy * Xc[:, 1] / Xc[:, 2] + cy - x[:, 1]) ** 2).sum()
    return R, t, cost


@pytest.mark.parametrize("name", list(ri.FAMILY))
def test_refit_agrees_with_gauss_newton_by_linalg_solve(name):
    X, x, planted = ri.family_scene(name)
    R0, t0 = ri.start_pose()
    R, t, steps, cost, costs = rr.refine(X, x, ri.K, R0, t0, planted, return_costs=True)
    Rr, tr, cost_r = gauss_newton_reference(X[planted], x[planted], R0, t0)
    Rm = R.reshape(3, 3)
    print(f"{name}: refit of {planted.sum()} planted inliers from 2 degrees / 0.09 units off: {steps} steps, cost {costs[0]:.4e} -> "
          f"{cost:.6e} (linalg.solve route {cost_r:.6e}); difference in R {np.abs(Rm - Rr).max():.3e}, in t {np.abs(t - tr).max():.3e}; "
          f"|R^T R - I| = {np.abs(Rm.T @ Rm - np.eye(3)).max():.3e}")
    assert 1 <= steps <= rr.REFINE_STEPS and cost <= costs[0]
    assert all(b <= a for a, b in zip(costs[:steps], costs[1:steps + 1]))
    assert np.abs(Rm - Rr).max() < 1e-8 and np.abs(t - tr).max() < 1e-7 and abs(cost - cost_r) <= 1e-9 * max(cost_r, 1.0)
    assert np.abs(Rm.T @ Rm - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rm) - 1.0) < 1e-12


def test_refit_undoes_a_step_that_raises_the_cost_and_stops_on_a_bad_pivot():
    X, x, _ = ri.scene(200, 0.0, seed=21)
    R0, t0 = ri.start_pose(deg=60.0, shift=1.5)
    R, t, steps, cost, costs = rr.refine(X, x, ri.K, R0, t0, return_costs=True)
    print(f"far start (60 degrees, 2.25 units): {steps} steps kept, costs seen {['%.3e' % c for c in costs]}")
    assert len(costs) == steps + 2 and not costs[-1] <= costs[steps] and steps < rr.REFINE_STEPS     # the last pass was undone
    assert cost == costs[steps]
    same = (np.repeat(X[:1], 6, axis=0), np.repeat(x[:1], 6, axis=0))
    Rs, ts, k, _ = rr.refine(*same, ri.K, *ri.true_pose())
    assert k == 0 and np.array_equal(Rs, ri.true_pose()[0].reshape(9)) and np.array_equal(ts, ri.true_pose()[1])


def test_block_sum_of_a_pass_is_the_header_s_order():
    X, x, _ = ri.scene(200, 0.0, seed=2)
    rng = np.random.default_rng(1)
    mem = rng.random(200) < 0.5
    mem[64:128] = False
    R, t = ri.start_pose()
    sums = rr.refit_pass(R.reshape(9), t, *rr.promote(X, x), rr.intrinsics(ri.K), mem)
    fx, fy, cx, cy = rr.intrinsics(ri.K)
    total, count = 0.0, 0.0
    for b in range(4):
        part = 0.0
        for i in range(64 * b, min(64 * b + 64, 200)):
            if mem[i]:
                Xi = X[i].astype(np.float64)
                Xc = [((R[r, 0] * Xi[0] + R[r, 1] * Xi[1]) + R[r, 2] * Xi[2]) + t[r] for r in range(3)]
                iz = 1.0 / Xc[2]
                rx, ry = (fx * (Xc[0] * iz) + cx) - float(x[i, 0]), (fy * (Xc[1] * iz) + cy) - float(x[i, 1])
                part = part + (rx * rx + ry * ry)
                count += 1.0
        total = total + part
    assert sums.shape == (rr.N_SUMS,) and sums[27] == total and sums[28] == count == mem.sum()


# ------------------------------------------------------------------------------------------ the inlier test ---
@pytest.mark.parametrize("m", ri.SCORE_M)
def test_threshold_case_is_decided_as_planted_with_a_margin(m):
    X, x, inside = ri.threshold_case(m)
    R, t = ri.true_pose()
    Rs, ts = ri.special_poses()
    inl, margin = rr.inlier_matrix(np.concatenate([R.reshape(1, 9), Rs]), np.concatenate([t[None], ts]), X, x, ri.K, 2.0,
                                   with_margin=True)
    assert np.array_equal(inl[0], inside) and not inl[1:].any() and margin > 1e-9
    assert m < 63 or (inside.any() and not inside.all())


def test_correspondences_exactly_on_the_threshold_are_inliers_and_none_behind_the_camera():
    X, x, R, t, K, thr, expected = ri.on_threshold_case()
    got = rr.inliers(R, t, X, x, K, thr)
    assert np.array_equal(got, expected) and expected.sum() == 54 and (~expected).sum() == 18 + 24
    # exactly on it: ee == thr^2 z^2 in float64, so the smallest relative margin is zero
    assert rr.inlier_matrix(R.reshape(1, 9), t[None], X, x, K, thr, with_margin=True)[1] == 0.0


# ------------------------------------------------------------------------------------------ the whole RANSAC ---
_SCORED, _RUN = {}, {}


def run(name, max_hyp=4096, threshold=2.0, seed=SEED):
    key = (name, max_hyp, threshold, seed)
    if key not in _RUN:
        X, x, _ = ri.family_scene(name)
        scored = _SCORED.setdefault((name, threshold, seed), rr.Scored(X, x, ri.K, threshold, seed))
        _RUN[key] = rr.ransac(X, x, ri.K, threshold, 0.99, max_hyp, seed, scored=scored)
    return _RUN[key]


@pytest.mark.parametrize("threshold", [8.0, 2.0])
@pytest.mark.parametrize("name", list(ri.FAMILY))
def test_restatement_recovers_the_planted_pose(name, threshold):
    X, x, planted = ri.family_scene(name)
    R, t, mask, n, info, _, steps = run(name, 4096, threshold)
    R_true, t_true = ri.true_pose()
    Rm = R.reshape(3, 3)
    rot, bound = ri.rotation_error_deg(Rm, R_true), math.degrees(math.atan(threshold / ri.FOCAL))
    kept, false = (mask & planted).sum() / planted.sum(), int((mask & ~planted).sum())
    print(f"{name} at threshold {threshold}: best hypothesis {info[1]} of {info[0]} keeps {info[2]}; after the refits ({steps[0]} and "
          f"{steps[1]} steps) {100 * kept:.1f} % of the planted inliers, {false} planted outliers; rotation error {rot:.5f} degrees "
          f"(bound {bound:.4f}), translation error {np.linalg.norm(t - t_true):.3e}")
    assert n == mask.sum() and n >= 6
    assert rot < bound                                                       # the angle one threshold-pixel subtends
    assert np.abs(Rm.T @ Rm - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rm) - 1.0) < 1e-12
    assert np.array_equal(mask, rr.inliers(R, t, X, x, ri.K, threshold))
    if threshold == 2.0:
        assert false == 0


def test_no_model_on_random_correspondences_and_below_six():
    X, x = ri.uniform_correspondences(64, 5)
    R, t, mask, n, info, _, _ = rr.ransac(X, x, ri.K, 2.0, 0.99, 1025, SEED)
    print(f"64 random correspondences: best count {info[2]}, {n} inliers")
    assert n == 0 and not mask.any() and not R.any() and not t.any() and info[0] == 1025
    same = (np.repeat(X[:1], 30, axis=0), np.repeat(x[:1], 30, axis=0))
    R, t, mask, n, info, _, _ = rr.ransac(*same, ri.K, 2.0, 0.99, 1025, SEED)
    assert info.tolist() == [1025, 0, 0] and n == 0                          # every hypothesis is NaN and counts 0


def test_stopping_rule_values():
    assert rr.needed(10, 10, 0.99, 4096) == (0.0, False)                     # p >= 1
    assert rr.needed(0, 10, 0.99, 4096) == (4096.0, False)                   # 1 - p == 1
    assert rr.needed(1, 1000, 0.99, 77) == (77.0, False)                     # p = 1e-18 vanishes beside 1
    assert rr.needed(5, 10, 0.99, 4096) == (float(np.ceil(np.log(0.01) / np.log(1.0 - 0.5 ** 6))), True)


@pytest.mark.parametrize("name", list(ri.FAMILY))
def test_no_gpu_scene_decides_its_stop_within_2_of_a_batch_boundary(name):
    """The device takes log from the C library, the restatement from Python's: an N that a last-place difference could
    move across a comparison with `done` would make the two stop differently.  No scene comes near."""
    for max_hyp in ri.MAX_HYPOTHESES:
        for seed in (SEED, SEED + 1) if (name, max_hyp) == ("2000_50", 4096) else (SEED,):     # (the seeds the GPU tests use)
            trace = run(name, max_hyp, 2.0, seed)[5]
            marks = sorted(set(range(rr.BATCH, max_hyp + 1, rr.BATCH)) | {max_hyp})
            for done, N, from_log in trace:
                assert done in marks
                if from_log:
                    assert min(abs(N - k) for k in marks) >= 2, (name, max_hyp, seed, done, N)
    X, x, _ = ri.family_scene("300_30")                                       # register_view's call in the GPU suite
    trace = rr.ransac(X, x, ri.K, 8.0, 0.99, 5000, 0)[5]
    assert all(not from_log or min(abs(N - k) for k in (1024, 2048, 3072, 4096, 5000)) >= 2 for _, N, from_log in trace)


# ----------------------------------------------------------------------------------------------- host logic ---
class FakeEngine:
    """Stands in for the engine: a fixed pose, a mask that keeps every third correspondence."""

    def __init__(self, model=True):
        self.model, self.calls = model, []

    def pnp_ransac(self, points3d, points2d, K, threshold=8.0, confidence=0.99, max_hypotheses=5000, seed=0):
        self.calls.append(("ransac", points3d, points2d, np.array(K), threshold, confidence, max_hypotheses, seed))
        m = len(points3d)
        if not self.model:
            return None, None, np.zeros(m, bool), {}
        return np.eye(3), np.array([1.0, 2.0, 3.0]), np.arange(m) % 3 == 0, {}

    def pnp_refine(self, points3d, points2d, K, R, t, mask=None):
        self.calls.append(("refine", points3d, points2d, np.array(K), np.array(R), np.array(t), mask))
        return 2.0 * np.eye(3), np.array(t) + 1.0, 3, 0.5


def test_registration_host_logic():
    from amvs.core import refine_pose, register_view, registration
    from amvs.core.camera import Camera, CameraPose
    cam = Camera(ri.K)
    X = np.arange(90, dtype=np.float64).reshape(30, 3)
    x = [[float(i), float(2 * i)] for i in range(30)]                        # a list of lists: converted
    fake = FakeEngine()
    pose, mask = register_view(cam, X, x, engine=fake)
    assert isinstance(pose, CameraPose) and np.array_equal(pose.R, np.eye(3)) and pose.t.tolist() == [1.0, 2.0, 3.0]
    assert mask.dtype == bool and np.array_equal(mask, np.arange(30) % 3 == 0)
    call = fake.calls[0]
    assert call[0] == "ransac" and call[1].dtype == np.float32 and call[1].shape == (30, 3) and call[2].dtype == np.float32
    assert call[2].shape == (30, 2) and np.array_equal(call[3], ri.K) and call[4:] == (8.0, 0.99, 5000, 0)
    assert register_view(cam, X, x, threshold=3, engine=fake) is not None and fake.calls[-1][4] == 3.0
    # the None paths: fewer than 6 correspondences (the engine is not asked), no model, fewer than min_inliers
    n_calls = len(fake.calls)
    assert register_view(cam, X[:5], x[:5], engine=fake) is None and len(fake.calls) == n_calls
    assert register_view(cam, X, x, engine=FakeEngine(model=False)) is None
    assert register_view(cam, X, x, min_inliers=11, engine=fake) is None and register_view(cam, X, x, min_inliers=10, engine=fake)
    with pytest.raises(ValueError):
        register_view(cam, X, x[:29], engine=fake)
    # refine_pose: the pose goes in as it is, a column t is flattened, the mask is passed on
    keep = np.arange(30) % 2 == 0
    out = refine_pose(cam, CameraPose(np.eye(3), np.array([[0.5], [0.25], [4.0]])), X, x, keep, engine=fake)
    call = fake.calls[-1]
    assert call[0] == "refine" and call[5].tolist() == [0.5, 0.25, 4.0] and call[6] is keep and np.array_equal(call[4], np.eye(3))
    assert isinstance(out, CameraPose) and np.array_equal(out.R, 2.0 * np.eye(3)) and out.t.tolist() == [1.5, 1.25, 5.0]
    assert refine_pose(cam, out, X, x, engine=fake) and fake.calls[-1][6] is None
    # the module keeps the engine it creates: one per device, handed out again
    made = []

    class Recorded(FakeEngine):
        def __init__(self, *a, **kw):
            super().__init__()
            made.append((a, kw))

    import amvs.engine
    real, kept = amvs.engine.Engine, dict(registration._engines)
    amvs.engine.Engine = Recorded
    registration._engines.clear()
    try:
        assert register_view(cam, X, x) is not None and register_view(cam, X, x, device=0) is not None
        assert refine_pose(cam, out, X, x) is not None
        assert len(made) == 1 and made[0][1] == {"device": 0} and len(registration._engines[0].calls) == 3
        register_view(cam, X, x, device=1)
        assert len(made) == 2 and made[1][1] == {"device": 1}
    finally:
        amvs.engine.Engine = real
        registration._engines.clear()
        registration._engines.update(kept)
