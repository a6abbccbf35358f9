"""The start of a reconstruction from two views without a GPU: the eighth header against its binding table, the refusal of
a NULL context, the restatement of tests/twoview_restatement.py against independent yardsticks (the planted pose,
numpy.linalg.svd for the decomposition and the DLT, the planted points and planted threshold cases), and the host logic
of core/geometry.py with a fake engine.  tests/test_hip_twoview.py compares the device with the same restatement.

A context needs a device, so the parameter errors behind a valid context are checked in tests/test_hip_twoview.py."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_restatement as er  # noqa: E402
import match_restatement as mr  # noqa: E402
import twoview_inputs as ti  # noqa: E402
import twoview_restatement as tr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_METHODS = ("twoview_decompose", "twoview_score", "twoview_front", "twoview_pose", "twoview_triangulate")
DECL = r"^(?:int|const char \*)\s*(amvs_\w+)\("
I3, Z3 = np.eye(3), np.zeros(3)


# ----------------------------------------------------------------------------------------- header and table ---
def test_eighth_header_matches_its_table_and_every_symbol_is_exported():
    from amvs import _lib
    header = open(os.path.join(ROOT, "include", "amvs_twoview.h")).read()
    declared = set(re.findall(DECL, header, re.M))
    assert declared == set(_lib.TWOVIEW_SIGNATURES) and len(declared) == 5
    assert declared == {"amvs_twoview_decompose", "amvs_twoview_score", "amvs_twoview_front", "amvs_twoview_pose",
                        "amvs_twoview_triangulate"}
    for table in (_lib.SIGNATURES, _lib.DEPTH_SIGNATURES, _lib.LENS_SIGNATURES, _lib.MATCH_SIGNATURES, _lib.EPIPOLAR_SIGNATURES,
                  _lib.PNP_SIGNATURES, _lib.STEP_SIGNATURES):
        assert not declared & set(table)
    for other in ("amvs.h", "amvs_depth.h", "amvs_lens.h", "amvs_match.h", "amvs_epipolar.h", "amvs_resection.h", "amvs_step.h"):
        assert not declared & set(re.findall(DECL, open(os.path.join(ROOT, "include", other)).read(), re.M))
    lib = _lib.load()
    for name, (res, args) in _lib.TWOVIEW_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(args), name
    from amvs.engine import Engine
    for m in ENGINE_METHODS:
        assert callable(getattr(Engine, m)), m
    for name, values in (("AMVS_TWOVIEW_MAX_MATCHES", (tr.MAX_MATCHES, _lib.TWOVIEW_MAX_MATCHES, 1 << 20)),
                         ("AMVS_TWOVIEW_MAX_POSES", (tr.MAX_POSES, _lib.TWOVIEW_MAX_POSES, 1 << 20)),
                         ("AMVS_TWOVIEW_POSE_TILE", (tr.POSE_TILE, _lib.TWOVIEW_POSE_TILE, ti.POSE_TILE)),
                         ("AMVS_TWOVIEW_MAX_DEPTH", (tr.MAX_DEPTH, _lib.TWOVIEW_MAX_DEPTH, 50.0)),
                         ("AMVS_TWOVIEW_DEPTH_MIN", (tr.DEPTH_MIN, _lib.TWOVIEW_DEPTH_MIN, 0.01)),
                         ("AMVS_TWOVIEW_DEPTH_BASELINES", (tr.DEPTH_BASELINES, _lib.TWOVIEW_DEPTH_BASELINES, 200.0)),
                         ("AMVS_TWOVIEW_MIN_PARALLAX_DEG", (tr.MIN_PARALLAX_DEG, _lib.TWOVIEW_MIN_PARALLAX_DEG, 1.0)),
                         ("AMVS_TWOVIEW_MAX_REPROJ", (tr.MAX_REPROJ, _lib.TWOVIEW_MAX_REPROJ, 4.0))):
        defined = float(re.search(r"#define %s\s+([\d.]+)" % name, header).group(1))
        assert all(defined == v for v in values), name
    from amvs.core import geometry
    assert (geometry.MAX_DEPTH, geometry.DEPTH_MIN, geometry.DEPTH_BASELINES, geometry.MIN_PARALLAX_DEG, geometry.MAX_REPROJ) == \
        (tr.MAX_DEPTH, tr.DEPTH_MIN, tr.DEPTH_BASELINES, tr.MIN_PARALLAX_DEG, tr.MAX_REPROJ)
    match_h = open(os.path.join(ROOT, "include", "amvs_match.h")).read()
    assert int(re.search(r"#define AMVS_JACOBI_SWEEPS\s+(\d+)", match_h).group(1)) == tr.JACOBI_SWEEPS
    makefile = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", makefile, re.M).group(1).split()
    assert {"amvs_twoview.o", "amvs_capi_twoview.o"} <= set(objs)
    assert "../../include/amvs_twoview.h" in re.search(r"^%\.o:(.*)$", makefile, re.M).group(1)
    assert "UNPINNED" in header


def test_a_null_context_is_refused_by_every_entry_point_without_a_device():
    from amvs import _lib
    lib = _lib.load()
    d18, d9, d3, f2, u8 = (C.c_double * 18)(), (C.c_double * 9)(), (C.c_double * 3)(), (C.c_float * 2)(), (C.c_uint8 * 1)()
    K = (C.c_double * 9)(*ti.K.reshape(9))
    i1, i5, n64, one = C.c_int32(0), (C.c_int32 * 5)(), C.c_int64(0), (C.c_double * 1)()
    calls = {
        "amvs_twoview_decompose": (None, d9, K, d18, d3, d3, C.byref(i1)),
        "amvs_twoview_score": (None, d9, d3, 1, f2, f2, 1, K, 50.0, i5),
        "amvs_twoview_front": (None, d9, d3, f2, f2, 1, K, 50.0, u8, C.byref(n64)),
        "amvs_twoview_pose": (None, d9, K, f2, f2, 1, 50.0, d9, d3, u8, C.byref(n64), i5),
        "amvs_twoview_triangulate": (None, K, d9, d3, d9, d3, f2, f2, 1, 0.01, 200.0, 0.99, 4.0, d3, u8, one, C.byref(n64)),
    }
    assert set(calls) == set(_lib.TWOVIEW_SIGNATURES)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1, name
    assert lib.amvs_twoview_pose(None, None, None, None, None, -3, float("nan"), None, None, None, None, None) == -1   # whatever the rest


# ------------------------------------------------------------------------------------------ the decomposition ---
def nearest_candidate(R, t, Rs, ts):
    """Largest entry difference of (R, t) to the nearest of the poses (Rs[j], ts[j])."""
    d = [max(np.abs(R - Rj).max(), np.abs(t - tj).max()) for Rj, tj in zip(Rs, ts)]
    return min(d)


def test_decomposition_of_the_exact_F_holds_the_planted_pose():
    R, t = ti.true_pose()
    ok, R2, tt, w = tr.decompose(ti.fundamental(R, t), ti.K)
    assert ok
    Rc, tc = tr.candidates(R2, tt)
    dR = min(np.abs(Rc[j].reshape(3, 3) - R).max() for j in range(4))
    dt = min(np.abs(tc[j] - t).max() for j in range(4))
    both = [j for j in range(4) if np.abs(Rc[j].reshape(3, 3) - R).max() < 1e-9 and np.abs(tc[j] - t).max() < 1e-9]
    print(f"exact F: nearest candidate differs from the planted pose by {dR:.3e} in R and {dt:.3e} in the unit t; w = {w}")
    assert dR < 1e-9 and dt < 1e-9 and len(both) == 1
    for Rm in R2.reshape(2, 3, 3):
        assert np.abs(Rm.T @ Rm - I3).max() < 1e-12 and abs(np.linalg.det(Rm) - 1.0) < 1e-12
    assert abs(np.linalg.norm(tt) - 1.0) < 1e-12
    assert w[0] >= w[1] > 0.0 and abs(w[2]) < 1e-12 * w[0] and abs(w[0] - w[1]) < 1e-9 * w[0]


def opencv_construction(E):
    """The four candidates as cv.decomposeEssentialMat forms them, with numpy.linalg.svd."""
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
    return [R1, R2, R1, R2], [t, t, -t, -t]


def test_decomposition_of_a_noisy_F_is_the_svd_s():
    _, p1, p2, _ = ti.scene(200, noise=0.5, seed=77)
    F = er.fit(p1, p2)                                        # refitted to points carrying 0.5 px of noise: rank 2, not exact
    ok, R2, tt, w = tr.decompose(F, ti.K)
    assert ok
    E = np.array(tr.essential(F, ti.K))                      # both routes decompose this one matrix
    Rs, ts = opencv_construction(E)
    Rc, tc = tr.candidates(R2, tt)
    worst = max(nearest_candidate(Rc[j].reshape(3, 3), tc[j], Rs, ts) for j in range(4))
    back = max(nearest_candidate(Rs[j], ts[j], Rc.reshape(4, 3, 3), tc) for j in range(4))
    sv = np.linalg.svd(E, compute_uv=False)
    print(f"noisy F: the four candidates against numpy.linalg.svd in OpenCV's construction: {worst:.3e} (and back {back:.3e}); "
          f"singular values of E {sv}, sqrt(w) {np.sqrt(np.abs(w))}")
    assert worst < 1e-9 and back < 1e-9
    assert sv[0] - sv[1] > 1e-4 * sv[0]                      # (the two singular values do differ: the case is not the exact one)
    R, t = ti.true_pose()
    assert min(ri_err(Rc[j].reshape(3, 3), R) for j in range(4)) < 0.5          # and it is near the planted pose, in degrees


def ri_err(R, R_true):
    return ti.ri.rotation_error_deg(R, R_true)


@pytest.mark.parametrize("name", ["zero", "rank1", "nan"])
def test_no_model_without_two_positive_singular_values(name):
    ok, R2, t, w = tr.decompose(ti.degenerate_fundamentals()[name], ti.K)
    assert not ok and not R2.any() and not t.any() and not w.any()


def test_the_vote_picks_the_planted_candidate_alone():
    R, t = ti.true_pose()
    _, p1, p2, _ = ti.scene(200)
    F = ti.fundamental(R, t)
    ok, R2, tt, _ = tr.decompose(F, ti.K)
    Rc, tc = tr.candidates(R2, tt)
    counts = tr.score(Rc, tc, p1, p2, ti.K)
    true = [j for j in range(4) if np.abs(Rc[j].reshape(3, 3) - R).max() < 1e-9 and np.abs(tc[j] - t).max() < 1e-9]
    print(f"clean scene, 200 matches: counts of the four candidates {counts.tolist()}, the planted one is {true}")
    assert len(true) == 1 and counts[true[0]] == 200 and counts.sum() == 200
    Rp, tp, mask, n, info = tr.pose(F, ti.K, p1, p2)
    assert info.tolist() == [true[0], *counts] and n == 200 and mask.all()
    assert np.array_equal(Rp, Rc[true[0]]) and np.array_equal(tp, tc[true[0]])
    # the other three put every point behind one camera or both
    for j in range(4):
        z1, z2 = tr.depths(Rc[j], tc[j], p1, p2, ti.K)
        assert j == true[0] or ((z1 < 0) | (z2 < 0)).all()
    assert any(((tr.depths(Rc[j], tc[j], p1, p2, ti.K)[0] > 0) != (tr.depths(Rc[j], tc[j], p1, p2, ti.K)[1] > 0)).all() for j in range(4))
    none = tr.pose(np.zeros((3, 3)), ti.K, p1, p2)
    assert not none[0].any() and not none[1].any() and not none[2].any() and none[3] == 0 and not none[4].any()


@pytest.mark.parametrize("m", ti.SCORE_M)
def test_depth_limit_and_special_poses(m):
    p1, p2, planted = ti.score_matches(m)
    R, t = ti.true_pose()
    assert np.array_equal(tr.front(R, t, p1, p2, ti.K, ti.DEPTH_LIMIT), planted)
    ok, R2, tt, _ = tr.decompose(ti.fundamental(R, t), ti.K)
    Rs, ts = ti.score_poses(*tr.candidates(R2, tt))
    inl = tr.front_matrix(Rs[:9], ts[:9], p1, p2, ti.K, ti.DEPTH_LIMIT)
    assert not inl[1:4].any()                                 # the zero, NaN and infinite poses count nothing
    if m >= 8:
        assert planted[[2, 4]].all() and not planted[[3, 5]].any()
        z1, _ = tr.depths(*ti.sideways_pose(), p1, p2, ti.K)
        assert np.isinf(z1[1]) and not tr.front(*ti.sideways_pose(), p1, p2, ti.K, float("inf"))[1]     # the point at infinity
        assert tr.front(R, t, p1, p2, ti.K, float("inf"))[[3, 5]].all()


# ---------------------------------------------------------------------------------------------- triangulation ---
PARALLAX_SCALE = (0.3 / 1.0) ** 2
SVD_BOUND = 5e-12 * PARALLAX_SCALE


def test_dlt_stays_close_to_the_svd_of_A():
    """include/amvs_match.h gives 5e-12 relative in X at ITS parallax floor of 0.3 degrees.  The eigenvector of A^T A is
    off by the rounding unit times the square of A's condition number, and that number grows as one over the parallax
    angle, so at this header's floor of 1 degree the figure scales by (0.3 / 1)^2: 4.5e-13.  Candidates at or above the
    floor are held to it: the noisy scene (about 10 degrees) and points 50 to 57 baselines away (1.0 to 1.2 degrees)."""
    R, t = ti.true_pose()
    _, p1, p2, _ = ti.scene(1000, noise=0.5, seed=9)
    rng = np.random.default_rng(3)
    far = np.stack([rng.uniform(-15.0, 15.0, 1000), rng.uniform(-10.0, 10.0, 1000), rng.uniform(50.0, 57.0, 1000)], axis=1)
    q1 = (ti.project(I3, Z3, far) + rng.normal(0.0, 0.5, (1000, 2))).astype(np.float32)
    q2 = (ti.project(R, t, far) + rng.normal(0.0, 0.5, (1000, 2))).astype(np.float32)
    for name, a, b in (("scene", p1, p2), ("at the floor", q1, q2)):
        X, _, cs = tr.triangulate(ti.K, I3, Z3, R, t, a, b)
        Xs = mr.triangulate_svd(ti.K, I3, Z3, R, t, a, b)
        rel = np.linalg.norm(X - Xs, axis=1) / np.linalg.norm(Xs, axis=1)
        above = cs <= ti.COS_1_DEG
        print(f"{name}: Jacobi on A^T A against the SVD of A, largest relative difference in X {rel[above].max():.3e} over the "
              f"{above.sum()} candidates at 1 degree or more ({rel.max():.3e} over all 1000); bound {SVD_BOUND:.2e}")
        assert above.sum() >= 300 and rel[above].max() < SVD_BOUND


def test_noise_free_matches_give_the_planted_points():
    R, t = ti.true_pose()
    Xp, p1, p2, _ = ti.scene(500, seed=11)
    X, valid, cs = tr.triangulate(ti.K, I3, Z3, R, t, p1, p2)
    err = np.abs(X - Xp).max()
    # float32 pixels: half an ulp at 2048 is 6e-5 px, a depth of 8 over a unit baseline turns that into 8^2 / 1500 * 6e-5
    print(f"noise-free scene: largest difference to the planted points {err:.3e}")
    assert valid.all() and err < 1e-4
    ang = np.degrees(np.arccos(cs))
    C2 = -(R.T @ t)
    planted = np.degrees(np.arccos(np.einsum("ij,ij->i", Xp, Xp - C2) / np.linalg.norm(Xp, axis=1) / np.linalg.norm(Xp - C2, axis=1)))
    assert np.abs(ang - planted).max() < 1e-3


def test_every_filter_decides_its_planted_candidates_with_a_margin():
    R, t = ti.true_pose()
    p1, p2, expected, near, names = ti.filter_case()
    smallest = np.inf
    seen = set()
    for which, thresholds in enumerate((ti.FILTER_DEFAULTS, ti.FILTER_NEAR)):
        X, valid, cs, margin = tr.triangulate(ti.K, I3, Z3, R, t, p1, p2, *thresholds, with_margin=True)
        rows = np.flatnonzero(near == which)
        for r in rows:
            assert bool(valid[r]) == bool(expected[r]), (names[r], X[r])
            seen.add(names[r])
        planted = [r for r in rows if names[r] != "plain"]
        assert all(0.005 < margin[r] < 0.025 for r in planted), margin[planted]        # 1 % (2 % on 1 - cos) off its threshold
        smallest = min(smallest, margin[rows].min())
    print(f"16 candidates, 14 planted 1 % either side of the seven comparisons: smallest relative margin of a decision {smallest:.3e}")
    assert smallest > 1e-9 and len(seen) == 15                # 7 comparisons x 2 sides and the plain ones
    # a NaN candidate is never valid (the reference's negative phrasing lets it through)
    bad = p1.copy()
    bad[0, 0] = np.nan
    assert not tr.triangulate(ti.K, I3, Z3, R, t, bad, p2)[1][0]
    # the defaults are the reference's: 200 baselines and cos(1 degree)
    a = tr.triangulate(ti.K, I3, Z3, R, t, p1, p2)
    b = tr.triangulate(ti.K, I3, Z3, R, t, p1, p2, *ti.FILTER_DEFAULTS)
    assert np.array_equal(a[1], b[1]) and abs(np.linalg.norm(R.T @ t) - 1.0) < 1e-15
    assert tr.triangulate(ti.K, I3, Z3, R, t, p1[:0], p2[:0])[0].shape == (0, 3)


# ------------------------------------------------------------------------------------------------- host logic ---
class FakeEngine:
    """Stands in for the engine.  A pair's script is found by the first coordinate of its first match: n_inliers (the
    first ones), n_valid (the first ones of the sample), the parallax angle every valid point reports, and whether F or
    the pose is missing."""

    def __init__(self, scripts):
        self.scripts, self.calls = scripts, []

    def script(self, pts1):
        return self.scripts[int(round(float(pts1[0, 0])))]

    def fundamental_ransac(self, pts1, pts2, threshold=2.0, confidence=0.999, max_hypotheses=4096, seed=0):
        self.calls.append(("ransac", pts1, pts2, threshold, confidence, max_hypotheses, seed))
        s = self.script(pts1)
        mask = np.arange(len(pts1)) < s["n_inliers"]
        return (None if s.get("no_F") else np.full((3, 3), float(pts1[0, 0]))), mask, {}

    def twoview_pose(self, F, K, pts1, pts2, max_depth=50.0):
        self.calls.append(("pose", np.array(F), np.array(K), pts1, pts2, max_depth))
        s = self.script(pts1)
        if s.get("no_pose"):
            return None, None, np.zeros(len(pts1), bool), {}
        return 2.0 * np.eye(3), np.array([1.0, 0.0, 0.0]), np.arange(len(pts1)) % 2 == 0, {}

    def twoview_triangulate(self, K, R1, t1, R2, t2, pts1, pts2, depth_min=0.01, depth_max=None, cos_max_parallax=None, max_reproj=4.0):
        self.calls.append(("triangulate", np.array(K), np.array(R1), np.array(t1), np.array(R2), np.array(t2), pts1, pts2, depth_min,
                           depth_max, cos_max_parallax, max_reproj))
        s = self.script(pts1)
        m = len(pts1)
        valid = np.arange(m) < s["n_valid"]
        cs = np.where(valid, math.cos(math.radians(s["angle"])), 1.0)
        return np.arange(3.0 * m).reshape(m, 3), valid, cs


def pair(ident, m):
    """m matches that carry their script's number in the first coordinate."""
    p1 = np.stack([np.full(m, float(ident)), np.arange(m, dtype=np.float64)], axis=1)
    return p1, p1 + 1.0


def test_find_best_initial_pair_host_logic():
    from amvs.core import find_best_initial_pair, geometry
    from amvs.core.camera import Camera
    cam = Camera(ti.K)
    good = {"n_inliers": 100, "n_valid": 50, "angle": 10.0}
    scripts = {
        1: dict(good, n_inliers=80),                          # score 80 * 1.0 * 1.5 = 120
        2: dict(good, n_inliers=120, n_valid=25, angle=25.0),  # 120 * 0.5, no bonus: 60
        3: dict(good, n_inliers=300),                          # the best by far, but in the second component
        4: dict(good),                                         # 49 matches: never reaches the engine
        5: dict(good, n_inliers=49),                           # 49 inliers
        6: dict(good, n_valid=19),
        7: dict(good, angle=1.49), 8: dict(good, angle=40.01),
        9: dict(good, no_F=True), 10: dict(good, no_pose=True),
        11: dict(good, n_inliers=60, n_valid=20, angle=1.51),  # 60 * 0.4 = 24, inside the window, no bonus
        12: dict(good, n_inliers=50, angle=39.99),             # 50, no bonus
    }
    pairs = {(0, 1): pair(1, 150), (1, 2): pair(2, 150), (7, 8): pair(3, 400), (8, 9): pair(3, 400), (0, 2): pair(4, 49),
             (0, 3): pair(5, 150), (1, 3): pair(6, 150), (2, 3): pair(7, 150), (0, 4): pair(8, 150), (1, 4): pair(9, 150),
             (2, 4): pair(10, 150), (3, 4): pair(11, 150), (0, 5): pair(12, 50)}
    fake = FakeEngine(scripts)
    best = find_best_initial_pair(cam, pairs, engine=fake)
    assert best["pair"] == (0, 1) and best["score"] == 120.0 and best["valid_ratio"] == 1.0
    assert set(best) == {"pair", "mask", "R", "t", "parallax", "score", "pts1", "pts2", "valid_ratio"}
    assert best["mask"].dtype == bool and best["mask"].shape == (150,) and best["mask"].sum() == 80
    assert best["pts1"].shape == (80, 2) and best["pts1"].dtype == np.float32 and np.array_equal(best["pts2"], best["pts1"] + 1.0)
    assert np.array_equal(best["R"], 2.0 * np.eye(3)) and best["t"].shape == (3, 1) and best["t"].ravel().tolist() == [1.0, 0.0, 0.0]
    assert abs(best["parallax"] - 10.0) < 1e-9
    # the second component (views 7, 8, 9) and the pair under 50 matches never reach the engine
    first = [int(c[1][0, 0]) for c in fake.calls if c[0] == "ransac"]
    assert first == [1, 2, 5, 6, 7, 8, 9, 10, 11, 12]
    assert all(c[3:5] == (1.0, 0.999) for c in fake.calls if c[0] == "ransac")
    assert [int(c[3][0, 0]) for c in fake.calls if c[0] == "pose"] == [1, 2, 6, 7, 8, 10, 11, 12]      # 5 and 9 stop before it
    tri = [c for c in fake.calls if c[0] == "triangulate"]
    assert [int(c[6][0, 0]) for c in tri] == [1, 2, 6, 7, 8, 11, 12]
    # the sample: linspace over the inliers, at most 50; the first camera is [I | 0]; the reference's thresholds
    for c, n_in in zip(tri, (80, 120, 100, 100, 100, 60, 50)):
        idx = np.linspace(0, n_in - 1, min(50, n_in), dtype=int)
        assert np.array_equal(c[6][:, 1], idx.astype(np.float32)) and len(c[6]) == 50
        assert np.array_equal(c[2], np.eye(3)) and not c[3].any() and np.array_equal(c[4], 2.0 * np.eye(3))
        assert c[8] == 0.01 and c[9] == 200.0 * 2.0 and c[10] == float(np.cos(np.deg2rad(1.0))) and c[11] == 4.0   # |C2| = |R^T t| = 2
    # the gates and the window, one candidate at a time
    def only(ident, m=150):
        return find_best_initial_pair(cam, {(0, 1): pair(ident, m)}, engine=FakeEngine(scripts))
    for ident in (4, 5, 6, 7, 8, 9, 10):
        assert only(ident, 49 if ident == 4 else 150) is None
    assert only(11)["score"] == 60 * (20 / 50) and only(12, 50)["score"] == 50.0
    scripts[13], scripts[14] = dict(good, n_inliers=50, n_valid=20), dict(good, n_inliers=50, angle=2.99)
    scripts[15], scripts[16] = dict(good, n_inliers=50, angle=3.01), dict(good, n_inliers=50, angle=19.99)
    scripts[17] = dict(good, n_inliers=50, angle=20.01)
    assert only(13, 50)["score"] == 50 * 0.4 * 1.5 and only(14)["score"] == 50.0 and only(15)["score"] == 75.0
    assert only(16)["score"] == 75.0 and only(17)["score"] == 50.0
    # equal scores: the first in the order of pair_points wins, whichever that is
    scripts[18] = dict(scripts[1])
    for order in (((0, 1), 18, (1, 2), 1), ((1, 2), 1, (0, 1), 18)):
        got = find_best_initial_pair(cam, {order[0]: pair(order[1], 150), order[2]: pair(order[3], 150)}, engine=FakeEngine(scripts))
        assert got["pair"] == order[0]
    assert find_best_initial_pair(cam, {}, engine=fake) is None
    # of two components of the same size the first is taken (the one with the smallest view)
    assert find_best_initial_pair(cam, {(5, 6): pair(3, 150), (0, 1): pair(11, 150)}, engine=FakeEngine(scripts))["pair"] == (0, 1)
    assert geometry._components([(3, 4), (0, 2), (2, 1), (9, 3)]) == [[0, 1, 2], [3, 4, 9]]


def test_geometry_host_logic():
    from amvs.core import (compute_essential_matrix, compute_reprojection_error, decompose_essential, relative_pose,
                           triangulate_points)
    from amvs.core.camera import Camera, CameraPose
    cam = Camera(ti.K)
    R, t = ti.true_pose()
    F = ti.fundamental(R, t)
    E = compute_essential_matrix(cam, F)
    assert np.array_equal(E, ti.K.T @ F @ ti.K)
    fake = FakeEngine({1: {}, 2: {"no_pose": True}, 3: {"n_valid": 2, "angle": 5.0}})
    p1, p2 = pair(1, 30)
    Rd, td, mask = decompose_essential(E, cam, p1.tolist(), p2, engine=fake)              # a list of lists: converted
    assert np.array_equal(Rd, 2.0 * np.eye(3)) and td.shape == (3, 1) and mask.dtype == bool and mask.shape == (30,)
    call = fake.calls[-1]
    assert call[0] == "pose" and call[3].dtype == np.float32 and call[3].shape == (30, 2) and call[5] == 50.0
    assert np.abs(call[1] - F).max() < 1e-12 * np.abs(F).max()                             # K^-T E K^-1 is F again
    with pytest.raises(ValueError):
        decompose_essential(E, cam, *pair(2, 30), engine=fake)
    assert relative_pose(cam, F, *pair(2, 30), engine=fake) is None
    assert relative_pose(cam, F, p1[:0], p2[:0], engine=fake) is None
    pose, mask = relative_pose(cam, F, p1, p2, max_depth=7, engine=fake)
    assert isinstance(pose, CameraPose) and fake.calls[-1][5] == 7.0 and np.array_equal(fake.calls[-1][1], F)
    with pytest.raises(ValueError):
        relative_pose(cam, F, p1, p2[:29], engine=fake)
    # triangulate_points: the reference's empty-input return, a column t flattened, the defaults from the baseline
    n_calls = len(fake.calls)
    X, valid = triangulate_points(cam, CameraPose.identity(), CameraPose(R, t), [], [], engine=fake)
    assert X.shape == (0,) and valid.shape == (0,) and valid.dtype == bool and len(fake.calls) == n_calls
    assert len(triangulate_points(cam, CameraPose.identity(), CameraPose(R, t), [], [], return_cos=True, engine=fake)) == 3
    X, valid, cs = triangulate_points(cam, CameraPose.identity(), CameraPose(R, t.reshape(3, 1)), *pair(3, 5), return_cos=True, engine=fake)
    call = fake.calls[-1]
    assert X.shape == (5, 3) and valid.tolist() == [True, True, False, False, False] and cs.shape == (5,)
    assert call[5].shape == (3,) and np.array_equal(call[5], t) and call[8:] == (0.01, 200.0 * float(np.linalg.norm(R.T @ t)),
                                                                                  float(np.cos(np.deg2rad(1.0))), 4.0)
    assert len(triangulate_points(cam, CameraPose.identity(), CameraPose(R, t), *pair(3, 5), engine=fake)) == 2
    # compute_reprojection_error: NumPy
    Xp, q1, q2, _ = ti.scene(20, seed=4)
    e = compute_reprojection_error(cam, CameraPose(R, t), Xp, q2.astype(np.float64) + np.array([3.0, 4.0]))
    assert e.shape == (20,) and np.abs(e - 5.0).max() < 1e-3
