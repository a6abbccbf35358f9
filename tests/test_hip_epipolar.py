"""The fundamental-matrix RANSAC on the device (csrc/amvs_fmat.hip behind include/amvs_epipolar.h) against the
restatement of tests/epipolar_restatement.py on the inputs of tests/epipolar_inputs.py: samples and hypotheses, inlier
counts and masks, the refit, the whole RANSAC and FeatureMatcher.match_pair_geometric.  Every comparison is bit for bit
and leaves no element out; where the header lets a NaN appear, NaN-ness and the bits of the finite entries are compared.
tests/test_epipolar_cpu.py shows on the CPU that the restatement does what it should."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_inputs as ei  # noqa: E402
import epipolar_restatement as er  # noqa: E402
import match_restatement as mr  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 1234


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
COUNTS, FIRSTS = (1, 63, 64, 65, 1025), (0, 1000)
_HYP = {}


def restated_hypotheses(key, p1, p2):
    """Hypotheses 0 .. 2024 of a case, once: hypothesis h is a function of h, so every (first, count) is a slice."""
    if key not in _HYP:
        _HYP[key] = er.hypotheses(p1, p2, SEED, 0, max(FIRSTS) + max(COUNTS))
    return _HYP[key]


def check_hypotheses(eng, key, p1, p2):
    ridx, rF = restated_hypotheses(key, p1, p2)
    for first in FIRSTS:
        for count in COUNTS:
            idx, F = eng.fmat_hypotheses(p1, p2, seed=SEED, first=first, count=count)
            assert idx.shape == (count, 8) and idx.dtype == np.int32 and F.shape == (count, 3, 3)
            assert np.array_equal(idx, ridx[first:first + count]), (key, first, count)
            assert same_bits(F.reshape(count, 9), rF[first:first + count]), (key, first, count)
    return rF


@pytest.mark.parametrize("m", [8, 9, 63, 64, 65, 1000])
def test_hypotheses_bit_for_bit(eng, m):
    p1, p2, _ = ei.scene(m, 0.25 if m >= 63 else 0.0, seed=m)
    rF = check_hypotheses(eng, m, p1, p2)
    assert np.isfinite(rF).all()


@pytest.mark.parametrize("name", ["identical", "collinear", "duplicated"])
def test_hypotheses_of_degenerate_samples(eng, name):
    p1, p2 = ei.degenerate_cases()[name]
    rF = check_hypotheses(eng, name, p1, p2)
    if name == "identical":
        assert np.isnan(rF).all()                       # d == 0: no scale, and no inlier below
        assert not eng.fmat_score(rF[:3], p1, p2).any()


# ------------------------------------------------------------------------------------------ scoring and inliers ---
_SCORE = {}


def score_case(m):
    """The matches on either side of the threshold, max(SCORE_N) matrices around the true one (the first is the true F,
    three of them are the zero / inf / NaN ones), the restated inlier matrix and its smallest margin; once per m."""
    if m not in _SCORE:
        p1, p2, inside = ei.threshold_case(m)
        rng = np.random.default_rng(m)
        F = ei.true_F().reshape(1, 9) * (1.0 + 2e-4 * rng.standard_normal((max(ei.SCORE_N), 9)))
        F[0] = ei.true_F().reshape(9)
        F[5:8] = ei.special_F()
        inl, margin = er.inlier_matrix(F, p1, p2, 2.0, with_margin=True)
        _SCORE[m] = (p1, p2, inside, F, inl, margin)
    return _SCORE[m]


@pytest.mark.parametrize("m", ei.SCORE_M)
def test_score_and_inliers_bit_for_bit(eng, m):
    p1, p2, inside, F, inl, margin = score_case(m)
    print(f"m = {m}: smallest relative margin of a decision to its threshold {margin:.3e}")
    assert margin > 1e-9
    assert np.array_equal(inl[0], inside)                    # planted 1 % inside / outside: decided as planted
    assert not inl[5:8].any()                                # zero, inf and NaN matrices keep nothing
    for n in ei.SCORE_N:
        counts = eng.fmat_score(F[:n], p1, p2, threshold=2.0)
        assert counts.dtype == np.int32 and np.array_equal(counts, inl[:n].sum(axis=1)), (m, n)
    assert not eng.fmat_score(ei.special_F(), p1, p2, threshold=2.0).any()
    for j in (0, 1, 5, 6, 7, 64):
        assert np.array_equal(eng.fmat_inliers(F[j], p1, p2, threshold=2.0), inl[j]), (m, j)


# -------------------------------------------------------------------------------------------------------- refit ---
@pytest.mark.parametrize("size", ei.FIT_SET_SIZES)
def test_fit_bit_for_bit_on_scattered_sets(eng, size):
    p1, p2, mask = ei.scattered_set(size)
    F = eng.fmat_fit(p1, p2, mask)
    assert same_bits(F.reshape(9), er.fit(p1, p2, mask)) and np.isfinite(F).all()


def test_fit_without_a_mask_is_the_fit_to_all(eng):
    p1, p2, _ = ei.scene(1000, 0.0, seed=5)
    F = eng.fmat_fit(p1, p2)
    assert same_bits(F.reshape(9), er.fit(p1, p2)) and same_bits(F, eng.fmat_fit(p1, p2, np.ones(1000, bool)))
    from amvs._lib import AmvsError
    few = np.zeros(1000, bool)
    few[:7] = True
    with pytest.raises(AmvsError):
        eng.fmat_fit(p1, p2, few)


# ------------------------------------------------------------------------------------------------------- RANSAC ---
_RANSAC = {}


def restated_ransac(name, max_hyp, seed=SEED):
    key = (name, max_hyp, seed)
    if key not in _RANSAC:
        p1, p2, thr = ei.ransac_scenes()[name]
        _RANSAC[key] = er.ransac(p1, p2, thr, 0.999, max_hyp, seed)
    return _RANSAC[key]


def check_ransac(eng, name, max_hyp, seed=SEED):
    p1, p2, thr = ei.ransac_scenes()[name]
    rF, rmask, rn, rinfo, _ = restated_ransac(name, max_hyp, seed)
    F, mask, info = eng.fundamental_ransac(p1, p2, threshold=thr, confidence=0.999, max_hypotheses=max_hyp, seed=seed)
    assert [info["hypotheses"], info["best_hypothesis"], info["best_count"]] == rinfo.tolist(), (name, max_hyp)
    assert info["n_inliers"] == rn and np.array_equal(mask, rmask)
    if rn == 0:
        assert F is None and not mask.any()
    else:
        assert same_bits(F.reshape(9), rF) and np.array_equal(eng.fmat_inliers(F, p1, p2, threshold=thr), mask)
    return F, mask, info


@pytest.mark.parametrize("max_hyp", ei.MAX_HYPOTHESES)
@pytest.mark.parametrize("name", ["300_30", "2000_50", "8_clean", "20_12out"])
def test_ransac_bit_for_bit(eng, name, max_hyp):
    check_ransac(eng, name, max_hyp)


def test_ransac_without_a_model(eng):
    """30 uniformly random matches at threshold 0.01 have no model.  An 8-point hypothesis that is not forced to rank 2
    passes through its own sample, so the best count of such a scene is 8 (9 when a ninth match happens to fit), never
    below: the no-model answer comes from the refit keeping fewer than 8.  The branch best < 8 is reached by matches
    that are all one point (every hypothesis is NaN and counts 0)."""
    for max_hyp in (1024, 4096):
        rinfo = restated_ransac("no_model", max_hyp)[3]
        assert 8 <= rinfo[2] <= 9 and restated_ransac("no_model", max_hyp)[2] == 0
        F, mask, info = check_ransac(eng, "no_model", max_hyp)
        assert F is None and info["n_inliers"] == 0
    rinfo = restated_ransac("no_model_identical", 1025)[3]
    assert rinfo.tolist() == [1025, 0, 0]                            # the restatement's best count is below 8
    F, mask, info = check_ransac(eng, "no_model_identical", 1025)
    assert F is None and info["best_count"] == 0


def test_ransac_repeats_itself_and_follows_the_seed(eng):
    p1, p2, thr = ei.ransac_scenes()["2000_50"]
    a = eng.fundamental_ransac(p1, p2, seed=SEED)
    b = eng.fundamental_ransac(p1, p2, seed=SEED)
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    other = check_ransac(eng, "2000_50", 4096, seed=SEED + 1)
    assert other[2]["best_hypothesis"] != a[2]["best_hypothesis"]


# ------------------------------------------------------------------------------------------------ FeatureMatcher ---
def test_match_pair_geometric_end_to_end(eng):
    from amvs.core.features import FeatureMatcher, ImageFeatures
    k1, k2, d1, d2 = ei.matcher_case()
    f1, f2 = ImageFeatures(k1, d1, (3000, 4000)), ImageFeatures(k2, d2, (3000, 4000))
    matcher = FeatureMatcher(ratio_threshold=0.8, engine=eng)
    matches, F = matcher.match_pair_geometric(f1, f2)
    qi, ti, s = mr.match(d1, d2, 0.8, cross_check=True)
    assert len(qi) >= 300
    rF, rmask, rn, _, _ = er.ransac(k1[qi], k2[ti], 2.0, 0.999, 4096, 0)
    assert rn >= 200 and same_bits(F.reshape(9), rF)
    assert [(m.idx1, m.idx2) for m in matches] == list(zip(qi[rmask].tolist(), ti[rmask].tolist()))
    assert np.array_equal(np.float32([m.distance for m in matches]), np.sqrt(s[rmask].astype(np.float64)).astype(np.float32))
    assert matcher.match_pair_geometric(f1, f2, min_matches=len(qi) + 1) == ([], None)
