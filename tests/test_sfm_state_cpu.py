"""The track state of include/amvs_sfm.h without a GPU: the tenth header against its binding table, the refusal of a NULL
context, and the restatement of tests/sfm_state_restatement.py against the properties the header promises -- on the
hand-built states, whose expected lists are written out here, and on the seeded random states of tests/sfm_state_inputs.py.
tests/test_hip_sfm_state.py compares the device with the same restatement on the same scripts.

A context needs a device, so the parameter errors behind a valid context are checked in tests/test_hip_sfm_state.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sfm_state_inputs as si  # noqa: E402
import sfm_state_restatement as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_METHODS = ("sfm_begin", "sfm_register", "sfm_scores", "sfm_correspondences", "sfm_triangulate", "sfm_counts", "sfm_observations",
                  "sfm_points", "sfm_set_points", "sfm_set_pose", "sfm_drop")
DECL = r"^(?:int|const char \*)\s*(amvs_\w+)\("
NAMES = {"amvs_sfm_begin", "amvs_sfm_register", "amvs_sfm_scores", "amvs_sfm_correspondences", "amvs_sfm_triangulate", "amvs_sfm_counts",
         "amvs_sfm_observations", "amvs_sfm_points_get", "amvs_sfm_points_set", "amvs_sfm_pose_set", "amvs_sfm_drop"}


def played(case):
    kps, pairs, script = case[:3]
    state = sr.State(kps, pairs)
    return state, dict_of(si.play(state, script, (sr.Refused,)))


def dict_of(log):
    """name -> the list of its results, in order"""
    out = {}
    for name, res in log:
        out.setdefault(name, []).append(res)
    return out


# ----------------------------------------------------------------------------------------- header and table ---
def test_tenth_header_matches_its_table_and_every_symbol_is_exported():
    from amvs import _lib
    header = open(os.path.join(ROOT, "include", "amvs_sfm.h")).read()
    declared = set(re.findall(DECL, header, re.M))
    assert declared == set(_lib.SFM_SIGNATURES) == NAMES and len(declared) == 11
    others = (_lib.SIGNATURES, _lib.DEPTH_SIGNATURES, _lib.LENS_SIGNATURES, _lib.MATCH_SIGNATURES, _lib.EPIPOLAR_SIGNATURES,
              _lib.PNP_SIGNATURES, _lib.TWOVIEW_SIGNATURES, _lib.BA_SIGNATURES, _lib.STEP_SIGNATURES)
    assert len(others) == 9 and len(_lib.SIGNATURES) == 92
    for table in others:
        assert not declared & set(table)
    for other in ("amvs.h", "amvs_depth.h", "amvs_lens.h", "amvs_match.h", "amvs_epipolar.h", "amvs_resection.h", "amvs_twoview.h",
                  "amvs_bundle.h", "amvs_step.h"):
        assert not declared & set(re.findall(DECL, open(os.path.join(ROOT, "include", other)).read(), re.M))
    lib = _lib.load()
    for name, (res, args) in _lib.SFM_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(args), name
    from amvs.engine import Engine
    for m in ENGINE_METHODS:
        assert callable(getattr(Engine, m)), m
    names = {"AMVS_BA_MAX_POINTS": _lib.BA_MAX_POINTS}
    for name, values in (("AMVS_SFM_BLOCK", (sr.BLOCK, si.B, _lib.SFM_BLOCK, 256)), ("AMVS_SFM_MAX_VIEWS", (sr.MAX_VIEWS, _lib.SFM_MAX_VIEWS, 4096)),
                         ("AMVS_SFM_MAX_KEYPOINTS", (sr.MAX_KEYPOINTS, _lib.SFM_MAX_KEYPOINTS, 1 << 28)),
                         ("AMVS_SFM_MAX_ROWS", (sr.MAX_ROWS, _lib.SFM_MAX_ROWS, 1 << 28)),
                         ("AMVS_SFM_MAX_POINTS", (sr.MAX_POINTS, _lib.SFM_MAX_POINTS, _lib.BA_MAX_POINTS)),
                         ("AMVS_SFM_MIN_SCORE", (sr.MIN_SCORE, _lib.SFM_MIN_SCORE, 12)), ("AMVS_SFM_MIN_OBS", (sr.MIN_OBS, _lib.SFM_MIN_OBS, 2))):
        text = re.search(r"#define %s\s+(.+)" % name, header).group(1).strip()
        defined = eval(text, {"__builtins__": {}}, names)                   # "256", "(1 << 28)" or "AMVS_BA_MAX_POINTS"
        assert all(defined == v for v in values), name
    makefile = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", makefile, re.M).group(1).split()
    assert {"amvs_sfm.o", "amvs_capi_sfm.o"} <= set(objs)
    assert "../../include/amvs_sfm.h" in re.search(r"^%\.o:(.*)$", makefile, re.M).group(1)
    assert "UNPINNED" in header


def test_a_null_context_is_refused_by_every_entry_point_without_a_device():
    from amvs import _lib
    lib = _lib.load()
    d, f4 = (C.c_double * 16)(), (C.c_float * 8)()
    i4, u4, n64 = (C.c_int32 * 8)(), (C.c_uint8 * 8)(), C.c_int64(0)
    calls = {
        "amvs_sfm_begin": (None, 1, i4, f4, 0, i4, i4, i4),
        "amvs_sfm_register": (None, 0, d, d, i4, i4, u4, 0, C.byref(n64)),
        "amvs_sfm_scores": (None, i4),
        "amvs_sfm_correspondences": (None, 0, i4, i4, f4, f4, C.byref(n64)),
        "amvs_sfm_triangulate": (None, 0, d, 0.01, 200.0, 0.99, 4.0, C.byref(n64), i4),
        "amvs_sfm_counts": (None, C.byref(n64), C.byref(n64), C.byref(n64)),
        "amvs_sfm_observations": (None, i4, i4, f4, 4, C.byref(n64)),
        "amvs_sfm_points_get": (None, d, u4, 4),
        "amvs_sfm_points_set": (None, d, u4, 0),
        "amvs_sfm_pose_set": (None, 0, d, d),
        "amvs_sfm_drop": (None, i4, i4, 0, 2, C.byref(n64), C.byref(n64)),
    }
    assert set(calls) == set(_lib.SFM_SIGNATURES)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1, name
    assert lib.amvs_sfm_begin(None, -5, None, None, -1, None, None, None) == -1          # whatever the rest


# ------------------------------------------------------------------------------------ the hand-built states ---
def test_rules_of_scores_and_correspondences_on_the_hand_built_state():
    state, out = played(si.rules_case("full"))
    assert out["triangulate"][0][0] == 12                                  # exact projections: every row of (0, 1) a point
    assert np.array_equal(out["observations"][0][1], np.repeat(np.arange(12), 2))       # id == row number
    kp, pid, X, x = out["correspondences"][0]
    assert kp.tolist() == [0, 1, 6, 7] and pid.tolist() == [5, 3, 2, 8]
    assert X.dtype == np.float32 and si.same_bits(X, np.array(state.X)[pid].astype(np.float32))
    assert si.same_bits(x, state.kp[3][kp])
    assert out["correspondences"][1] == "refused"                          # view 2 is registered
    assert out["scores"][1].tolist() == [-1, -1, -1, 6]
    assert out["counts"][1] == (12, 11, 24 + 3 - 2)                       # point 6 took its two observations with it


def test_rules_variants():
    _, two = played(si.rules_case("two"))
    assert two["scores"][1].tolist() == [-1, -1, 0, 5]                     # only views 0 and 1: keypoint 7 of view 3 has no candidate
    assert two["correspondences"][0][0].tolist() == [0, 1, 6] and two["correspondences"][1][0].tolist() == []
    _, empty = played(si.rules_case("empty_view"))
    assert empty["scores"][1].tolist() == [-1, -1, -1, 0] and len(empty["correspondences"][0][0]) == 0
    _, none = played(si.rules_case("no_rows"))
    assert none["counts"][0] == (0, 0, 0) and none["scores"][0].tolist() == [-1, -1, 0, 0] and none["register"][2] == "refused"
    _, allr = played(si.rules_case("all_registered"))
    assert allr["scores"][-1].tolist() == [-1, -1, -1, -1] and allr["correspondences"][-1] == "refused"


def test_triangulation_order_and_the_pair_that_must_skip():
    state, out = played(si.triangulate_case("plain"))
    n_new, per = out["triangulate"][1]
    assert per.tolist() == [6, 4, 0] and n_new == 10                       # (0, 2): tracks 6 .. 11, not the one behind; (1, 2): 12 .. 15 only
    assert state.owner[2][6:16] == list(range(6, 16)) and state.owner[2][16] == -1 and state.owner[0][16] == -1
    assert state.owner[1][6:12] == [-1] * 6                                # pair (1, 2) skipped the keypoints pair (0, 2) had used
    _, same = played(si.triangulate_case("same_pose"))
    assert same["triangulate"][1][1][1] == 0                               # zero baseline: nothing valid with view 1
    state, edge = played(si.triangulate_case("boundary"))
    made = edge["triangulate"][0][0]
    rows = state.pairs[0][1]
    right = [n for n in range(len(rows)) if rows[n, 0] == rows[n, 1]]
    assert made >= len(right) and min(right) < si.B - 1 and max(right) > si.B          # valid rows on both sides of the boundary
    assert [state.owner[0][n] for n in right] == sorted(state.owner[0][n] for n in right)   # ids ascend with the rank


def test_drop_frees_a_keypoint_for_a_later_triangulation():
    state, out = played(si.drop_case())
    assert out["counts"][1] == (10, 9, 20 + 5 - 2)      # point 9 died with its two observations
    assert out["drop"][0] == (2, 1)                     # (1, 7) named twice counts once, (0, 9) is no observation; point 7 dies
    assert out["counts"][2] == (10, 8, 23 - 2 - 1)      # ... and takes its observation in view 0 along
    cam, pt, uv = out["observations"][3]
    assert out["triangulate"][1][0] == 1 and cam[pt == 10].tolist() == [0, 2] and si.same_bits(uv[pt == 10][0], state.kp[0][7])
    assert out["counts"][3] == (11, 9, 22)
    assert out["drop"][1] == (0, 5) and out["counts"][4] == (11, 4, 12)      # min_obs = 3: only the points view 2 observes too stay


def test_register_refusals_leave_the_state_alone():
    kps, pairs, script, refused, after = si.register_refusals()
    state = sr.State(kps, pairs)
    si.play(state, script, (sr.Refused,))
    before = si.play(state, si.QUERIES, (sr.Refused,))
    assert [r for _, r in si.play(state, refused, (sr.Refused,))] == ["refused"] * len(refused)
    assert si.first_difference(before, si.play(state, si.QUERIES, (sr.Refused,))) is None
    log = si.play(state, after, (sr.Refused,))
    assert log[0][1] == 2                               # of the three rows the mask keeps, point 4 is dead


@pytest.mark.parametrize("bad", ["order", "ij", "range", "twice_i", "twice_j"])
def test_begin_refusals_of_the_restatement(bad):
    kps = [np.zeros((3, 2), np.float32)] * 3
    pairs = {"order": [((0, 2), [[0, 0]]), ((0, 1), [[0, 0]])], "ij": [((1, 1), [[0, 0]])], "range": [((0, 1), [[0, 3]])],
             "twice_i": [((0, 1), [[1, 0], [1, 2]])], "twice_j": [((0, 1), [[0, 2], [1, 2]])]}[bad]
    with pytest.raises(sr.Refused):
        sr.State(kps, pairs)


# ------------------------------------------------------------------------------------------ random states ---
def check_invariants(state):
    for v in range(state.V):
        owned = [p for p in state.owner[v] if p >= 0]
        assert state.registered[v] or not owned                            # (I1)
        assert all(state.alive[p] for p in owned)                          # (I2)
        assert len(set(owned)) == len(owned)                               # (I3)


@pytest.mark.parametrize("seed", range(20))
def test_properties_of_the_restatement_on_random_states(seed):
    kps, pairs, script = si.random_case(seed)
    state = sr.State(kps, pairs)
    made = 0
    for step in script:
        (name, res), = si.play(state, [step], (sr.Refused,))
        assert not isinstance(res, str), name                              # nothing is refused
        check_invariants(state)
        if name == "observations":
            cam, pt, uv = res
            key = pt.astype(np.int64) * state.V + cam
            assert (np.diff(key) > 0).all() and len(cam) == state.counts()[2]
        if name == "correspondences":
            kp, pid = res[0], res[1]
            assert len(set(kp.tolist())) == len(kp) and len(set(pid.tolist())) == len(pid) and (np.diff(kp) > 0).all()
        if name == "drop_random":
            left = np.bincount(state.observations()[1], minlength=state.n_points())
            assert all(left[p] >= 2 for p in range(state.n_points()) if state.alive[p])
            assert all(left[p] == 0 for p in range(state.n_points()) if not state.alive[p])
        if name == "triangulate":
            made += res[0]
    assert made == state.n_points() and made >= 15                         # the scenes do make points (noise 0.5 px, bound 4 px)


# ------------------------------------------------------------------------------- the pipeline over the restatement ---
# measured on the restatement pipeline (tests/sfm_pipeline_restatement.py): (largest rotation error in degrees, largest
# centre error in baselines, largest point error in baselines, final RMS reprojection error in pixels); asserted: ten times
# each, the convention of tests/test_sfm_chain_cpu.py, whose numbers for the chain (noisy: 0.117, 0.0146, 0.0345, 0.771) are
# of the same size: this pipeline adjusts the same observations and drops none.
PIPELINE_MEASURED = {"clean": (1.02e-6, 1.87e-7, 5.93e-7, 2.27e-5),
                     "noisy": (0.0683, 0.0112, 0.0229, 0.564),
                     "edges": (0.0683, 0.0114, 0.0249, 0.569)}
PIPELINE_REGISTERED = {"clean": [1, 2, 4, 3, 5, 0], "noisy": [1, 2, 4, 3, 5, 0], "edges": [1, 2, 6, 4, 5, 3, 0]}


@pytest.mark.parametrize("name", ["clean", "noisy", "edges"])
def test_the_restatement_pipeline_finds_the_planted_scene(name):
    """Measured: rotation 1.02e-6 degrees (clean), 0.0683 (noisy), 0.0683 (edges); centre 1.87e-7, 0.0112, 0.0114 baselines;
    point 5.93e-7, 0.0229, 0.0249 baselines (medians 1.6e-7, 0.0124, 0.0125); RMS 2.27e-5, 0.564, 0.569 px; compared points
    160, 141, 147 of the 160 planted.  Asserted: ten times each, at least 120 points.  View 7 of `edges` has five keypoints:
    its score never reaches 12, it is never tried and is not among the failed."""
    import sfm_chain as ch
    import sfm_pipeline_restatement as pr
    sc, matches, rec, ops = pr.restated(name)
    e = ch.truth_errors(sc, dict(rec, observations=rec["aside"]["observations"]))
    print(f"{name}: rotation {e['rotation']:.3g} degrees, centre {e['centre']:.3g}, point {e['point']:.3g} (median {e['point_median']:.3g}) "
          f"baselines, rms {e['rms']:.3g} px, {len(e['compared'])} points compared")
    rot, cen, pnt, rms = PIPELINE_MEASURED[name]
    assert e["rotation"] < 10.0 * rot and e["centre"] < 10.0 * cen and e["point"] < 10.0 * pnt and e["rms"] < 10.0 * rms
    assert rec["registered"] == PIPELINE_REGISTERED[name] and rec["final"]["failed"] == []
    assert sorted(rec["registered"]) == list(range(7 if name == "edges" else 6))
    assert e["mixed"] == [] and len(e["compared"]) >= 120
    assert len(rec["bundles"]) == (3 if name == "edges" else 2)            # seven views: one adjustment on the way
    assert all(len(set(m[:, 0])) == len(m) and len(set(m[:, 1])) == len(m) for m in matches.values())
