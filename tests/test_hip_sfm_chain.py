"""The sparse-reconstruction stages chained on the device -- fundamental-matrix RANSAC, the initial pair, triangulation,
registration, bundle adjustment, through the public layer and one context -- against the same chain over the
restatements of the headers, on the planted scenes of tests/sfm_chain_inputs.py.  The bookkeeping between the stages is
that of tests/sfm_chain.py for both, so every difference is the device's: a stage given what only another stage
produces (poses far from the per-stage inputs, triangulated points rounded to float32, the rows one mask selects, the
zeros of `no model`), or scratch that one stage released and the next was handed.  Every comparison is bit for bit and
leaves nothing out.  tests/test_sfm_chain_cpu.py shows on the CPU that the restatement chain finds the planted scene.

The restatement chain of a scene is computed once per process (6 to 9 s each); the device's share of every test is well
under a second."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_restatement as er  # noqa: E402
import sfm_chain as ch  # noqa: E402
import sfm_chain_inputs as ci  # noqa: E402
import twoview_restatement as tr  # noqa: E402
from test_hip_bundle import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
K = ci.K
BATCH_ENDS = (1024, 2048, 3072, 4096, 5000)
_DEVICE = {}


@pytest.fixture(scope="module")
def eng():
    import amvs
    with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as e:
        yield e


def restated(name):
    """The restatement's record; the device takes log from the C library, so no stop of a RANSAC of the chain may be
    decided within 2 of the end of a batch."""
    sc, rec, ops, _ = ch.restated(name)
    assert all(min(abs(N - k) for k in BATCH_ENDS) >= 2 for _, N in ops.log_decided)
    return sc, rec


def on_the_shared_context(eng, name):
    """The device's record of a scene on the module's context, run once: the first use of `eng` by this module is the
    clean scene's chain when the tests run in order."""
    if name not in _DEVICE:
        _DEVICE[name] = ch.run(ci.scene(name), ch.DeviceOps(K, engine=eng))
    return _DEVICE[name]


@pytest.mark.parametrize("name", ci.NAMES)
def test_every_boundary_bit_for_bit(eng, name):
    sc, want = restated(name)
    got = on_the_shared_context(eng, name)
    where = ch.first_difference(got, want, same=same_bits)
    assert where is None, f"{name}: the device's chain first differs from the restatement's at {where}"
    assert got["registered"] == want["registered"] and len(got["bundles"]) == 2 and len(got["registered"]) == (7 if name == "edges" else 6)
    assert got["initial"]["winner"]["pair"] == got["initial"]["candidates"][0]["pair"] == tuple(got["registered"][:2])
    if name == "edges":
        pairs = [c["pair"] for c in got["initial"]["candidates"]]
        at = pairs.index((4, 6))                                           # equal scores keep the order of pair_points
        assert pairs[at + 1] == (5, 6) and got["initial"]["candidates"][at]["score"] == got["initial"]["candidates"][at + 1]["score"]
        assert not got["pairs"][(2, 7)]["model"] and got["registrations"][-1]["view"] == 7
        both = [t for t in got["triangulations"] if t["pair"] == (2, 6)]
        assert len(both) == 1 and not both[0]["valid"].any()


def test_one_context_or_one_for_every_call(eng):
    """Scratch that a stage releases into the context's cache is handed to the next one; with a context of its own every
    call starts from fresh blocks.  The records are the same."""
    want = on_the_shared_context(eng, "noisy")
    got = ch.run(ci.scene("noisy"), ch.DeviceOps(K, fresh=True))
    where = ch.first_difference(got, want, same=same_bits)
    assert where is None, f"a context for every call first differs from the shared one at {where}"


def test_twice_on_one_context():
    import amvs
    with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as e:
        ops = ch.DeviceOps(K, engine=e)
        first = ch.run(ci.scene("noisy"), ops)
        between = ch.run(ci.scene("clean"), ops)
        third = ch.run(ci.scene("noisy"), ops)
    where = ch.first_difference(third, first, same=same_bits)
    assert where is None, f"the second run of the noisy scene on one context first differs from the first at {where}"
    assert ch.first_difference(between, restated("clean")[1], same=same_bits) is None
    assert ch.first_difference(first, restated("noisy")[1], same=same_bits) is None


def test_no_model_crosses_the_boundary(eng):
    """60 matches, all false: the fundamental-matrix RANSAC has no model, the zeros it writes for that have no pose, and
    the pair is no initial pair; every step as the restatement's."""
    from amvs.core import find_best_initial_pair, relative_pose
    from amvs.core.camera import Camera
    p1, p2 = ci.false_pair()
    assert len(p1) == 60
    rF, rmask, rn, rinfo, trace = er.ransac(p1, p2, ch.F_THRESHOLD, ch.F_CONFIDENCE, ch.F_HYPOTHESES, ch.SEED)
    assert all(not from_log or min(abs(N - k) for k in BATCH_ENDS) >= 2 for _, N, from_log in trace)
    assert rn == 0 and rinfo[2] >= 8 and not rF.any()      # a hypothesis kept 8 matches, its refit fewer: no model
    F, mask, info = eng.fundamental_ransac(p1, p2, threshold=ch.F_THRESHOLD, confidence=ch.F_CONFIDENCE, max_hypotheses=ch.F_HYPOTHESES,
                                           seed=ch.SEED)
    assert [info["hypotheses"], info["best_hypothesis"], info["best_count"], info["n_inliers"]] == [*rinfo.tolist(), rn]
    assert np.array_equal(mask, rmask) and (F is None) == (rn < 8) and (F is None or same_bits(F.reshape(9), rF))
    # what the entry point itself writes, over a sentinel
    f32p, f64p, u8p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    raw, rawmask, k, rawinfo = np.full(9, 7.0), np.full(60, 7, np.uint8), C.c_int64(-1), np.full(3, 7, np.int32)
    rc = eng._lib.amvs_fmat_ransac(eng._h, p1.ctypes.data_as(f32p), p2.ctypes.data_as(f32p), 60, ch.F_THRESHOLD, ch.F_CONFIDENCE,
                                   ch.F_HYPOTHESES, ch.SEED, raw.ctypes.data_as(f64p), rawmask.ctypes.data_as(u8p), C.byref(k),
                                   rawinfo.ctypes.data_as(i32p))
    assert rc == 0 and k.value == rn and same_bits(raw, rF) and np.array_equal(rawmask != 0, rmask) and np.array_equal(rawinfo, rinfo)
    if rn < 8:
        assert not raw.any() and not np.signbit(raw).any() and not rawmask.any()       # the zeros of `no model` are +0.0
    # ... handed to the next stage
    zeros = np.zeros((3, 3))
    for handed in (raw.reshape(3, 3), zeros):
        wR, wt, wmask, wn, winfo = tr.pose(handed, K, p1, p2)
        R, t, front, pinfo = eng.twoview_pose(handed, K, p1, p2)
        assert [pinfo["best"], *pinfo["counts"]] == winfo.tolist() and pinfo["n_front"] == wn and np.array_equal(front, wmask)
        assert (R is None) == (wn == 0) and (R is None or (same_bits(R.reshape(9), wR) and same_bits(t, wt)))
        got = relative_pose(Camera(K), handed, p1, p2, engine=eng)
        assert (got is None) == (wn == 0)
    assert tr.pose(zeros, K, p1, p2)[3] == 0 and relative_pose(Camera(K), zeros, p1, p2, engine=eng) is None
    # ... and through the layer that chains the two itself
    dropped = {}

    def ransac(a, b, threshold, confidence):
        got = er.ransac(a, b, threshold, confidence, ch.F_HYPOTHESES, ch.SEED)
        return (got[0] if got[2] >= 8 else None), got[1]

    assert tr.find_best_initial_pair(K, {(0, 3): (p1, p2)}, ransac, dropped) == [] and dropped[(0, 3)] == ("inliers", rn if rn >= 8 else 0)
    assert find_best_initial_pair(Camera(K), {(0, 3): (p1, p2)}, engine=eng) is None
