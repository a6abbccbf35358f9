"""The fundamental-matrix RANSAC without a GPU: the fifth header against its binding table, the refusal of a NULL context,
the restatement of tests/epipolar_restatement.py against independent yardsticks (a loop in Python integers, an SVD, the
planted inliers), the stopping rule on the scenes the GPU comparison uses, and the host logic of core/features.py with
a fake engine.  tests/test_hip_epipolar.py compares the device with the same restatement."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_inputs as ei  # noqa: E402
import epipolar_restatement as er  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_METHODS = ("fmat_hypotheses", "fmat_score", "fmat_inliers", "fmat_fit", "fundamental_ransac")
DECL = r"^(?:int|const char \*)\s*(amvs_\w+)\("


# ----------------------------------------------------------------------------------------- header and table ---
def test_fifth_header_matches_its_table_and_every_symbol_is_exported():
    from amvs import _lib
    header = open(os.path.join(ROOT, "include", "amvs_epipolar.h")).read()
    declared = set(re.findall(DECL, header, re.M))
    assert declared == set(_lib.EPIPOLAR_SIGNATURES) and len(declared) == 5
    for table in (_lib.SIGNATURES, _lib.DEPTH_SIGNATURES, _lib.LENS_SIGNATURES, _lib.MATCH_SIGNATURES):
        assert not declared & set(table)
    for other in ("amvs.h", "amvs_depth.h", "amvs_lens.h", "amvs_match.h"):
        assert not declared & set(re.findall(DECL, open(os.path.join(ROOT, "include", other)).read(), re.M))
    lib = _lib.load()
    for name, (res, args) in _lib.EPIPOLAR_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(args), name
    from amvs.engine import Engine
    for m in ENGINE_METHODS:
        assert callable(getattr(Engine, m)), m
    for name, value in (("AMVS_FMAT_BATCH", er.BATCH), ("AMVS_FMAT_BLOCK", er.BLOCK), ("AMVS_FMAT_BATCH", ei.BATCH),
                        ("AMVS_FMAT_BLOCK", ei.BLOCK), ("AMVS_FMAT_BATCH", _lib.FMAT_BATCH), ("AMVS_FMAT_BLOCK", _lib.FMAT_BLOCK),
                        ("AMVS_FMAT_MAX_MATCHES", 1 << 20), ("AMVS_FMAT_MAX_HYP", 1 << 20)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, header).group(1)) == value
    match_h = open(os.path.join(ROOT, "include", "amvs_match.h")).read()
    assert int(re.search(r"#define AMVS_JACOBI_SWEEPS\s+(\d+)", match_h).group(1)) == er.JACOBI_SWEEPS
    makefile = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", makefile, re.M).group(1).split()
    assert {"amvs_fmat.o", "amvs_capi_fmat.o"} <= set(objs)
    assert "../../include/amvs_epipolar.h" in re.search(r"^%\.o:(.*)$", makefile, re.M).group(1)
    assert "UNPINNED" in header


def test_a_null_context_is_refused_by_every_entry_point_without_a_device():
    from amvs import _lib
    lib = _lib.load()
    d9, f16, u8 = (C.c_double * 9)(), (C.c_float * 16)(), (C.c_uint8 * 8)()
    i8, i3, n64 = (C.c_int32 * 8)(), (C.c_int32 * 3)(), C.c_int64(0)
    calls = {
        "amvs_fmat_hypotheses": (None, f16, f16, 8, 0, 0, 1, i8, d9),
        "amvs_fmat_score": (None, d9, 1, f16, f16, 8, 2.0, i3),
        "amvs_fmat_inliers": (None, d9, f16, f16, 8, 2.0, u8, C.byref(n64)),
        "amvs_fmat_fit": (None, f16, f16, None, 8, d9, C.byref(n64)),
        "amvs_fmat_ransac": (None, f16, f16, 8, 2.0, 0.999, 1, 0, d9, u8, C.byref(n64), i3),
    }
    assert set(calls) == set(_lib.EPIPOLAR_SIGNATURES)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1, name
    assert lib.amvs_fmat_ransac(None, None, None, -3, -1.0, 7.0, 0, 0, None, None, None, None) == -1   # whatever the rest


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
    for k in range(8):
        r = mix_int(seed ^ mix_int(8 * h + k)) % (m - k)
        for c in sorted(chosen):
            if r >= c:
                r += 1
        chosen.append(r)
    return chosen


@pytest.mark.parametrize("m", [8, 9, 64, 1000, 1 << 20])
def test_sampler_draws_8_distinct_indices_and_is_the_loop(m):
    seed = 0xDEADBEEFCAFEF00D
    idx = er.sample(seed, np.arange(4096), m)
    assert idx.shape == (4096, 8) and idx.min() >= 0 and idx.max() < m
    assert (np.diff(np.sort(idx, axis=1), axis=1) > 0).all()
    assert idx.tolist() == [sample_loop(seed, h, m) for h in range(4096)]
    if m == 8:
        assert (np.sort(idx, axis=1) == np.arange(8)).all()
    else:
        assert len(np.unique(idx[:, 0])) > 1 and len(np.unique(np.sort(idx, axis=1), axis=0)) > (1 if m == 9 else 1000)
    assert np.array_equal(er.sample(seed, np.arange(1000, 1010), m), idx[1000:1010])       # a function of h alone


# ------------------------------------------------------------------------------------------------- the fit ---
# the scene family of the fit's yardsticks: (matches, outlier fraction)
FAMILY = [(300, 0.30), (2000, 0.50), (64, 0.25), (9, 0.0)]


def hartley(p):
    c = p.mean(axis=0)
    s = np.sqrt(2.0) / np.linalg.norm(p - c, axis=1).mean()
    return np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]])


def fit_svd(p1, p2):
    """Normalised 8-point and rank 2, both by numpy.linalg.svd; unit norm, the header's sign."""
    p1, p2 = p1.astype(np.float64), p2.astype(np.float64)
    T1, T2 = hartley(p1), hartley(p2)
    h1 = np.concatenate([p1, np.ones((len(p1), 1))], axis=1) @ T1.T
    h2 = np.concatenate([p2, np.ones((len(p2), 1))], axis=1) @ T2.T
    A = (h2[:, :, None] * h1[:, None, :]).reshape(-1, 9)
    Fn = np.linalg.svd(A)[2][-1].reshape(3, 3)
    U, S, Vt = np.linalg.svd(Fn)
    Fn = U @ np.diag([S[0], S[1], 0.0]) @ Vt
    F = (T2.T @ Fn @ T1).reshape(9)
    F = F / np.linalg.norm(F)
    return -F if F[np.argmax(np.abs(F))] < 0 else F


@pytest.mark.parametrize("m,frac", FAMILY)
def test_fit_agrees_with_the_svd_route_and_has_rank_2(m, frac):
    p1, p2, inl = ei.scene(m, frac)
    F = er.fit(p1, p2, inl)
    diff = np.abs(F - fit_svd(p1[inl], p2[inl])).max()
    det = abs(np.linalg.det(F.reshape(3, 3)))
    print(f"{m} matches, {inl.sum()} in the set: Jacobi on the normal matrix against the SVD route, largest difference in the "
          f"unit-norm F {diff:.3e}; |det F| = {det:.3e}")
    assert diff < 1e-9 and det < 1e-20
    assert abs(np.linalg.norm(F) - 1.0) < 1e-15 and F[np.argmax(np.abs(F))] > 0


@pytest.mark.parametrize("m,frac", FAMILY)
def test_fixed_sweeps_leave_no_off_diagonal_residual(m, frac):
    p1, p2, _ = ei.scene(m, frac)
    _, F, M = er.hypotheses(p1, p2, 1234, 0, 1024, return_state=True)
    diag = np.abs(M[:, np.arange(9), np.arange(9)]).max(axis=1)
    off = np.abs(M - M * np.eye(9)).max(axis=(1, 2))
    print(f"{m} matches: largest off-diagonal entry after {er.JACOBI_SWEEPS} sweeps, relative to the largest diagonal entry, "
          f"{(off / diag).max():.3e} over 1024 hypotheses")
    assert np.isfinite(F).all() and (off < 1e-30 * diag).all()


def test_block_sum_is_the_header_s_order():
    rng = np.random.default_rng(1)
    t = rng.standard_normal(200) * 10.0 ** rng.integers(-8, 8, 200)
    mem = rng.random(200) < 0.5
    mem[64:128] = False                                   # an empty block
    total = 0.0
    for b in range(4):
        part = 0.0
        for i in range(64 * b, min(64 * b + 64, 200)):
            if mem[i]:
                part = part + t[i]
        total = total + part
    assert er.block_sum(t, mem) == total


@pytest.mark.parametrize("m", ei.SCORE_M)
def test_threshold_case_is_decided_as_planted_with_a_margin(m):
    p1, p2, inside = ei.threshold_case(m)
    inl, margin = er.inlier_matrix(np.concatenate([ei.true_F().reshape(1, 9), ei.special_F()]), p1, p2, 2.0, with_margin=True)
    assert np.array_equal(inl[0], inside) and not inl[1:].any() and margin > 1e-9
    assert m < 63 or (inside.any() and not inside.all())


# ------------------------------------------------------------------------------------------ the whole RANSAC ---
_RUN = {}


def run(name, max_hyp=4096, seed=1234):
    if (name, max_hyp, seed) not in _RUN:
        p1, p2, thr = ei.ransac_scenes()[name]
        _RUN[name, max_hyp, seed] = er.ransac(p1, p2, thr, 0.999, max_hyp, seed)
    return _RUN[name, max_hyp, seed]


@pytest.mark.parametrize("name,m,frac", [("300_30", 300, 0.30), ("2000_50", 2000, 0.50)])
def test_restatement_recovers_the_planted_inliers(name, m, frac):
    _, _, planted = ei.scene(m, frac)
    F, mask, n, info, _ = run(name)
    kept = (mask & planted).sum() / planted.sum()
    false = (mask & ~planted).sum() / mask.sum()
    print(f"{m} matches, {100 * frac:.0f} % outliers: best hypothesis {info[1]} of {info[0]} keeps {info[2]}; after the refits "
          f"{100 * kept:.1f} % of the planted inliers, {100 * false:.2f} % of the kept are planted outliers")
    assert n == mask.sum() and kept >= 0.95 and false <= 0.02
    assert np.array_equal(mask, er.inliers(F, *ei.ransac_scenes()[name][:2], 2.0))


def test_an_all_inlier_scene_stops_after_one_batch():
    p1, p2, _ = ei.scene(500, 0.0, seed=4)
    F, mask, n, info, trace = er.ransac(p1, p2, 2.0, 0.999, 4096, 1234)
    assert info[0] == er.BATCH and len(trace) == 1 and n >= 0.95 * 500


def test_8_inliers_of_400_run_to_max_hypotheses():
    p1, p2, _ = ei.scene(400, 392 / 400, seed=5)
    for max_hyp in (1025, 4096):
        _, _, _, info, trace = er.ransac(p1, p2, 2.0, 0.999, max_hyp, 1234)
        assert info[0] == max_hyp and len(trace) == -(-max_hyp // er.BATCH) and info[2] < 40


def test_stopping_rule_values():
    assert er.needed(10, 10, 0.999, 4096) == 0.0                       # p >= 1
    assert er.needed(0, 10, 0.999, 4096) == 4096.0                     # 1 - p == 1
    assert er.needed(1, 1000, 0.999, 77) == 77.0                       # p = 1e-24 vanishes beside 1
    assert er.needed(5, 10, 0.999, 4096) == float(np.ceil(np.log(0.001) / np.log(1.0 - 0.5 ** 8)))


@pytest.mark.parametrize("name", list(ei.ransac_scenes()))
def test_no_gpu_scene_decides_its_stop_within_2_of_a_batch_boundary(name):
    """The device takes log from the C library, the restatement from Python's: an N that a last-place difference could
    move across a comparison with `done` would make the two stop differently.  No scene comes near."""
    for max_hyp in ei.MAX_HYPOTHESES:
        for seed in (1234, 1235) if (name, max_hyp) == ("2000_50", 4096) else (1234,):     # (the seeds the GPU tests use)
            trace = run(name, max_hyp, seed)[4]
            marks = sorted(set(range(er.BATCH, max_hyp + 1, er.BATCH)) | {max_hyp})
            for done, N, from_log in trace:
                assert done in marks
                if from_log:
                    assert min(abs(N - k) for k in marks) >= 2, (name, max_hyp, seed, done, N)


def test_the_end_to_end_scene_has_the_same_margin_and_a_model():
    import match_restatement as mr
    k1, k2, d1, d2 = ei.matcher_case()
    qi, ti, _ = mr.match(d1, d2, 0.8, cross_check=True)
    assert len(qi) >= 300
    F, mask, n, info, trace = er.ransac(k1[qi], k2[ti], 2.0, 0.999, 4096, 0)
    assert n >= 200
    marks = list(range(er.BATCH, 4097, er.BATCH))
    assert all(not from_log or min(abs(N - k) for k in marks) >= 2 for _, N, from_log in trace)


# ----------------------------------------------------------------------------------------------- host logic ---
class FakeEngine:
    """Stands in for the engine: fixed symmetric matches, a mask that keeps every third one."""

    def __init__(self, n_matches, model=True):
        self.n, self.model, self.calls = n_matches, model, []

    def set_descriptors(self, slot, d):
        self.calls.append(("set", slot, d.shape, d.dtype))

    def match_descriptors(self, q, t, ratio=0.85, cross_check=False):
        self.calls.append(("match", q, t, ratio, cross_check))
        i = np.arange(self.n, dtype=np.int32)
        return i, (i * 7) % 50, (i * i).astype(np.int32)

    def fundamental_ransac(self, pts1, pts2, threshold=2.0, confidence=0.999, max_hypotheses=4096, seed=0):
        self.calls.append(("ransac", np.array(pts1), np.array(pts2), threshold, confidence))
        mask = np.arange(self.n) % 3 == 0
        if not self.model:
            return None, np.zeros(self.n, bool), {}
        return np.eye(3), mask, {}


def features(n, offset):
    from amvs.core.features import ImageFeatures
    pts = np.arange(2 * n, dtype=np.float32).reshape(n, 2) + offset
    return ImageFeatures(pts, np.full((n, 128), 3, np.uint8), (100, 100))


def test_feature_matcher_host_logic():
    from amvs.core.features import FeatureMatch, FeatureMatcher, ImageFeatures
    f1, f2 = features(50, 0.0), features(50, 1000.0)
    fake = FakeEngine(30)
    fm = FeatureMatcher(ratio_threshold=0.75, engine=fake)
    raw = fm.match(f1, f2)
    assert [c[0] for c in fake.calls] == ["set", "set", "match"] and fake.calls[2] == ("match", 0, 1, 0.75, True)
    assert raw == [FeatureMatch(i, (i * 7) % 50, float(np.float32(np.sqrt(float(i * i))))) for i in range(30)]
    matches, F = fm.match_pair_geometric(f1, f2)
    assert np.array_equal(F, np.eye(3)) and matches == [raw[i] for i in range(0, 30, 3)]
    call = fake.calls[-1]
    assert call[0] == "ransac" and call[3:] == (2.0, 0.999)
    assert np.array_equal(call[1], f1.points[np.arange(30)]) and np.array_equal(call[2], f2.points[(np.arange(30) * 7) % 50])
    # below min_matches: no RANSAC at all
    n_calls = len(fake.calls)
    assert fm.match_pair_geometric(f1, f2, min_matches=31) == ([], None)
    assert [c[0] for c in fake.calls[n_calls:]] == ["set", "set", "match"]
    # no model
    assert FeatureMatcher(engine=FakeEngine(30, model=False)).match_pair_geometric(f1, f2) == ([], None)
    # fewer than two descriptors: nothing to match, the engine is not asked
    lone = FakeEngine(30)
    assert FeatureMatcher(engine=lone).match(features(1, 0.0), f2) == [] and not lone.calls
    # keypoints with .pt, and the descriptor check of core/dense.py
    class KP:
        def __init__(self, x, y):
            self.pt = (x, y)
    kp = ImageFeatures([KP(1.5, 2.0), KP(3.0, 4.25)], np.zeros((2, 128), np.uint8), (10, 10))
    assert kp.points.dtype == np.float32 and kp.points.tolist() == [[1.5, 2.0], [3.0, 4.25]] and len(kp) == 2
    bad = ImageFeatures(f1.keypoints, np.full((50, 128), 0.5, np.float32), (100, 100))
    with pytest.raises(ValueError, match="RootSIFT"):
        FeatureMatcher(engine=FakeEngine(30)).match(bad, f2)
    assert FeatureMatcher()._engine is None                            # created on first use
