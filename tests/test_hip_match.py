"""The descriptor matcher on the device (csrc/amvs_match.hip behind include/amvs_match.h) against the restatement of
tests/match_restatement.py on the inputs of tests/match_inputs.py: indices and squared distances of the 2-nearest-
neighbour search, and the compacted triples of the ratio test with and without the cross check.  Every comparison is
bit for bit and leaves no element out.  tests/test_match_cpu.py shows on the CPU that the restatement is the definition
and that the inputs reach the edges they name."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_inputs as mi  # noqa: E402
import match_restatement as mr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import amvs
    with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as e:
        yield e


def check_knn2(eng, q, t, slots=(0, 1)):
    eng.set_descriptors(slots[0], q)
    eng.set_descriptors(slots[1], t)
    idx, d2 = eng.knn2(*slots)
    ri, rd = mr.knn2(q, t)
    assert idx.dtype == np.int32 and d2.dtype == np.int32
    assert np.array_equal(idx, ri) and np.array_equal(d2, rd)
    return idx, d2


@pytest.mark.parametrize("shape", mi.KNN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_knn2_bit_for_bit_at_the_edges_of_the_launch_shape(eng, shape):
    check_knn2(eng, *mi.knn_shape_case(*shape))


def test_best_and_second_best_in_different_splits(eng):
    q, t, planted = mi.split_case()
    assert mi.splits(len(q), len(t)) >= 3
    idx, _ = check_knn2(eng, q, t)
    assert np.array_equal(idx, planted)


def test_far_rows_are_not_beaten_by_padding(eng):
    idx, d2 = check_knn2(eng, *mi.far_case())
    assert idx.tolist() == [[0, 1]] and d2.tolist() == [[8323200, 8323200]]


def test_identical_rows_have_distance_zero(eng):
    idx, d2 = check_knn2(eng, *mi.identical_case())
    assert idx[:, 0].tolist() == [3, 40, 69, 0] and not d2[:, 0].any()


def test_duplicates_go_to_the_lowest_index_then_the_next(eng):
    q, t, rows = mi.duplicate_case()
    idx, d2 = check_knn2(eng, q, t)
    assert idx.tolist() == [rows[:2]] * 3 and (d2[:, 0] == d2[:, 1]).all()


def test_a_slot_set_again_with_fewer_rows_forgets_the_old_ones(eng):
    rng = np.random.default_rng(8)
    q = mi.random_desc(rng, 50)
    big, small = mi.random_desc(rng, 1000), mi.random_desc(rng, 40)
    big[40:] = np.repeat(q[:48], 20, axis=0)                      # rows that would win if they stayed readable
    check_knn2(eng, q, big, slots=(2, 3))
    idx, _ = check_knn2(eng, q, small, slots=(2, 3))
    assert idx.max() < 40
    idx, _ = check_knn2(eng, small, q, slots=(3, 2))             # and as the query set
    assert len(idx) == 40


def test_full_comparison_4096_by_5003(eng):
    check_knn2(eng, *mi.full_case(), slots=(4, 5))


def test_workgroups_that_walk_more_than_one_chunk(eng):
    """4096 x 66 100: two chunks a workgroup and a last share of one (tests/test_match_cpu.py asserts the shape and what is
    planted across the chunk boundaries); every index and distance, and the ratio test on top."""
    q, t, planted = mi.multi_chunk_case()
    assert mi.chunks_per_split(len(q), len(t)) == 2
    eng.set_descriptors(12, q)
    eng.set_descriptors(13, t)
    idx, d2 = eng.knn2(12, 13)
    ri, rd = mr.knn2_by_minima(q, t)
    assert np.array_equal(idx, ri) and np.array_equal(d2, rd)
    assert np.array_equal(idx[:600], planted)
    got = eng.match_descriptors(12, 13, 0.85)
    keep = mr.ratio_keep(rd, 0.85)
    want = np.nonzero(keep)[0]
    assert len(want) >= 300
    assert np.array_equal(got[0], want) and np.array_equal(got[1], ri[want, 0]) and np.array_equal(got[2], rd[want, 0])


@pytest.mark.parametrize("ratio", [0.85, 0.8])
@pytest.mark.parametrize("cross_check", [False, True])
def test_ratio_test_and_cross_check_give_the_same_triples_in_the_same_order(eng, ratio, cross_check):
    q, t = mi.ratio_case()
    eng.set_descriptors(6, q)
    eng.set_descriptors(7, t)
    got = eng.match_descriptors(6, 7, ratio, cross_check)
    want = mr.match(q, t, ratio, cross_check)
    assert len(want[0]) > 50
    for g, w in zip(got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w)


def test_ratio_test_on_the_full_set(eng):
    q, t = mi.full_case()
    eng.set_descriptors(4, q)
    eng.set_descriptors(5, t)
    for cross_check in (False, True):
        got = eng.match_descriptors(4, 5, 0.85, cross_check)
        want = mr.match(q, t, 0.85, cross_check)
        assert len(want[0]) >= 400
        for g, w in zip(got, want):
            assert np.array_equal(g, w)


def test_parameter_errors(eng):
    import amvs
    rng = np.random.default_rng(1)
    eng.set_descriptors(8, mi.random_desc(rng, 5))
    eng.set_descriptors(9, mi.random_desc(rng, 1))
    eng.set_descriptors(10, np.empty((0, 128), np.uint8))
    with pytest.raises(amvs.AmvsError):
        eng.knn2(8, 9)                                             # fewer than 2 train rows
    with pytest.raises(amvs.AmvsError):
        eng.set_descriptors(11, np.zeros((4, 64), np.uint8))       # d != 128
    with pytest.raises(amvs.AmvsError):
        eng.match_descriptors(9, 8, 0.85, cross_check=True)        # the reverse search has 1 train row
    with pytest.raises(amvs.AmvsError):
        eng.match_descriptors(8, 8, float("nan"))
    idx, d2 = eng.knn2(10, 8)                                      # no query: nothing to write
    assert idx.shape == (0, 2) and d2.shape == (0, 2)
    assert all(len(a) == 0 for a in eng.match_descriptors(10, 8))
