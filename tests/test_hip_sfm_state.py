"""The resident track state (include/amvs_sfm.h) on the device against tests/sfm_state_restatement.py: every script of
tests/sfm_state_inputs.py is played on both and EVERY step's result compared -- integers exactly, points and pixels bit for
bit.  The scripts' sizes are the smallest at which the kernels can go wrong: a dozen keypoints for the rules, B - 1 .. 2 B + 1
rows and keypoints for the launch edges (B = AMVS_SFM_BLOCK lanes a workgroup), B + 40 rows for the id order across a
workgroup boundary.  What the hand-built states must give is asserted for the restatement in tests/test_sfm_state_cpu.py;
here the device only has to agree with it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sfm_state_inputs as si  # noqa: E402
import sfm_state_restatement as sr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import amvs
    with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as e:
        yield e


class Device:
    """The Engine's sfm_* methods under the names of the restatement's State."""

    def __init__(self, eng, kps, pairs):
        self.eng = eng
        eng.sfm_begin(kps, pairs)

    def register(self, view, R, t, kp=(), pid=(), mask=None):
        return self.eng.sfm_register(view, R, t, kp, pid, mask)

    def scores(self):
        return self.eng.sfm_scores()

    def correspondences(self, view):
        return self.eng.sfm_correspondences(view)

    def triangulate(self, view, K):
        return self.eng.sfm_triangulate(view, K)

    def counts(self):
        return self.eng.sfm_counts()

    def observations(self):
        return self.eng.sfm_observations()

    def points(self):
        return self.eng.sfm_points()

    def set_points(self, X, alive):
        return self.eng.sfm_set_points(X, alive)

    def set_pose(self, view, R, t):
        return self.eng.sfm_set_pose(view, R, t)

    def drop(self, cam, pt, min_obs=2):
        return self.eng.sfm_drop(cam, pt, min_obs)


def refusals():
    from amvs._lib import AmvsError
    return (AmvsError,)


def agree(eng, kps, pairs, script):
    """Plays the script on both; returns the restatement's log."""
    want = si.play(sr.State(kps, pairs), script, (sr.Refused,))
    got = si.play(Device(eng, kps, pairs), script, refusals())
    assert si.first_difference(want, got) is None
    return want


def assert_no_index_violation():
    from amvs import _lib
    assert _lib.index_check(reset=False)[0] == 0


@pytest.mark.parametrize("variant", si.RULES_VARIANTS)
def test_scores_and_correspondences_rules(eng, variant):
    agree(eng, *si.rules_case(variant))
    assert_no_index_violation()


@pytest.mark.parametrize("N", [si.B - 1, si.B, si.B + 1, 2 * si.B + 1])
def test_launch_edges_of_the_row_and_keypoint_kernels(eng, N):
    kps, pairs, script = si.edges_case(N)
    log = agree(eng, kps, pairs, script)
    corr = [r for name, r in log if name == "correspondences"]
    assert len(corr[0][0]) > N // 4 and len(corr[1][0]) > N // 8           # the case does exercise the rules
    assert_no_index_violation()


@pytest.mark.parametrize("variant", si.TRIANGULATE_VARIANTS)
def test_triangulate(eng, variant):
    agree(eng, *si.triangulate_case(variant))
    assert_no_index_violation()


def test_observations_and_drop(eng):
    agree(eng, *si.drop_case())
    assert_no_index_violation()


def test_register_refusals_leave_the_state_alone(eng):
    kps, pairs, script, refused, after = si.register_refusals()
    dev, state = Device(eng, kps, pairs), sr.State(kps, pairs)
    assert si.first_difference(si.play(state, script + si.QUERIES, (sr.Refused,)), si.play(dev, script + si.QUERIES, refusals())) is None
    before = si.play(dev, si.QUERIES, refusals())
    assert [r for _, r in si.play(dev, refused, refusals())] == ["refused"] * len(refused)
    assert si.first_difference(before, si.play(dev, si.QUERIES, refusals())) is None
    assert si.first_difference(si.play(state, after, (sr.Refused,)), si.play(dev, after, refusals())) is None


def test_other_refusals(eng):
    from amvs._lib import AmvsError
    kps, pairs, script = si.drop_case()
    dev = Device(eng, kps, pairs)
    si.play(dev, script[:3], refusals())
    R, t = np.eye(3), np.zeros(3)
    for call in (lambda: eng.sfm_correspondences(0), lambda: eng.sfm_correspondences(3), lambda: eng.sfm_triangulate(2, si.K),
                 lambda: eng.sfm_triangulate(0, np.zeros((3, 3))), lambda: eng.sfm_triangulate(0, si.K, depth_min=float("nan")),
                 lambda: eng.sfm_set_pose(2, R, t), lambda: eng.sfm_drop([3], [0]), lambda: eng.sfm_drop([0], [10]),
                 lambda: eng.sfm_drop([0], [0], min_obs=-1), lambda: eng.sfm_set_points(np.zeros((9, 3)), np.ones(9))):
        with pytest.raises(AmvsError):
            call()
    X, alive = eng.sfm_points()
    alive[2] = False
    eng.sfm_set_points(X, alive)
    with pytest.raises(AmvsError):
        eng.sfm_set_points(X, np.ones(10, bool))                            # a dead point cannot come back
    bad = {"order": [((0, 2), [[0, 0]]), ((0, 1), [[0, 0]])], "ij": [((1, 1), [[0, 0]])], "range": [((0, 1), [[0, 10]])],
           "twice_i": [((0, 1), [[1, 0], [1, 2]])], "twice_j": [((0, 1), [[0, 2], [1, 2]])]}
    for name, p in bad.items():
        with pytest.raises(AmvsError):
            eng._chk(_begin_unsorted(eng, kps, p))
    assert eng.sfm_counts() == (10, 9, 18)                                 # a refused begin leaves the state alone


def _begin_unsorted(eng, kps, pairs):
    """amvs_sfm_begin with the pairs in the order given (Engine.sfm_begin sorts them)."""
    import ctypes as C
    n_kp = np.array([len(k) for k in kps], np.int32)
    kp = np.ascontiguousarray(np.concatenate(kps), np.float32)
    views = np.array([p for p, _ in pairs], np.int32).reshape(-1, 2)
    rows = np.concatenate([np.array(r, np.int32).reshape(-1, 2) for _, r in pairs])
    start = np.zeros(len(pairs) + 1, np.int32)
    start[1:] = np.cumsum([len(r) for _, r in pairs])
    i32p = C.POINTER(C.c_int32)
    return eng._lib.amvs_sfm_begin(eng._h, len(kps), n_kp.ctypes.data_as(i32p), kp.ctypes.data_as(C.POINTER(C.c_float)), len(pairs),
                                   views.ctypes.data_as(i32p), start.ctypes.data_as(i32p), rows.ctypes.data_as(i32p))


@pytest.mark.parametrize("seed", range(20))
def test_random_states_agree_at_every_step(eng, seed):
    agree(eng, *si.random_case(seed))
    assert_no_index_violation()


def test_begin_twice_leaves_nothing_of_the_first_state(eng):
    big = si.edges_case(si.B + 1)
    small = si.rules_case("full")
    agree(eng, *big)
    agree(eng, *small)                                                     # fewer views, keypoints, rows and points than before
    dev = Device(eng, small[0], small[1])
    assert dev.counts() == (0, 0, 0) and dev.scores().tolist() == [0, 0, 0, 0] and len(dev.observations()[0]) == 0


def test_two_contexts_side_by_side(eng):
    import amvs
    a, b = si.random_case(3), si.random_case(4)
    with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as other:
        da, db = Device(eng, a[0], a[1]), Device(other, b[0], b[1])
        log_a, log_b = [], []
        for n in range(max(len(a[2]), len(b[2]))):                          # interleaved, step by step
            log_a += si.play(da, a[2][n:n + 1], refusals())
            log_b += si.play(db, b[2][n:n + 1], refusals())
    assert si.first_difference(si.play(sr.State(a[0], a[1]), a[2], (sr.Refused,)), log_a) is None
    assert si.first_difference(si.play(sr.State(b[0], b[1]), b[2], (sr.Refused,)), log_b) is None
