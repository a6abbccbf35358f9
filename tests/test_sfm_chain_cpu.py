"""The chain of the sparse-reconstruction stages without a GPU: the restatements of the four headers, chained by the
bookkeeping of tests/sfm_chain.py on the planted scenes of tests/sfm_chain_inputs.py, against the planted truth.  This
shows that the restatement chain does what it should -- that its stages agree with each other on x2^T F x1 = 0, on
Xc = R X + t, on which view of a pair is [I | 0] -- so that tests/test_hip_sfm_chain.py, which compares the device's chain
with it bit for bit, compares with something right.

Where a bound is "ten times the measured value", the measured value stands next to it, as in tests/test_bundle_cpu.py.

The seed of the scenes (sfm_chain_inputs.SEED) was chosen among 1 .. 12 for the conditions below that are no
measurements: with other seeds a true correspondence whose point was made from two keypoints with two sigma of noise
in opposite directions is rejected by the 8 px of the registration, a false match of the 20 % passes the fundamental
matrix and a registration, or one of the 50 sampled candidates of the pure-rotation pair passes the seven comparisons.

The restatement chain of a scene takes 6 to 9 s on one core of the machine this was written on (clean 7.3 s, noisy 6.3 s,
edges 8.8 s; without the memo of identical calls, which halves the F-RANSACs, about 11 s)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_inputs as bi  # noqa: E402
import sfm_chain as ch  # noqa: E402
import sfm_chain_inputs as ci  # noqa: E402

# measured on the restatement chain: (largest rotation error in degrees, largest centre error in baselines, largest point
# error in baselines, final RMS reprojection error in pixels); asserted: ten times each
MEASURED = {"clean": (1.02e-6, 1.87e-7, 5.93e-7, 2.27e-5),
            "noisy": (0.117, 0.0146, 0.0345, 0.771),
            "edges": (0.112, 0.0151, 0.0368, 0.749)}
REGISTERED = {"clean": [1, 2, 4, 3, 5, 0], "noisy": [1, 2, 4, 3, 5, 0], "edges": [1, 2, 6, 4, 3, 5, 0]}


# ---------------------------------------------------------------------------------------------------- the scenes ---
def test_the_scenes_are_what_they_are_for():
    clean, noisy, edges = (ci.scene(n) for n in ci.NAMES)
    for sc, V in ((clean, 6), (noisy, 6), (edges, 8)):
        assert len(sc["R"]) == V and sc["X"].shape == (160, 3) and sorted(sc["matches"]) == sorted(set(sc["matches"]))
        seen = np.zeros((160, V), int)
        for v in range(V):
            assert sc["keypoints"][v].dtype == np.float32 and len(sc["keypoints"][v]) == len(sc["track"][v])
            ids = sc["track"][v][sc["track"][v] >= 0]
            np.add.at(seen[:, v], ids, 1)
        assert (seen[:, :6].sum(axis=1) >= 3).all() and 0.6 < seen[:, :6].mean() < 0.8
        for (i, j), m in sc["matches"].items():
            assert i < j and len(set(m[:, 0])) == len(m) and len(set(m[:, 1])) == len(m)      # a keypoint is matched once per pair
            true = np.array([ci.true_match(sc, (i, j), r) for r in m])
            n_both = int(np.count_nonzero((seen[:, i] > 0) & (seen[:, j] > 0)))
            if j < 6:
                assert 50 <= n_both and int(round(0.2 * n_both)) == np.count_nonzero(~true) - (0 if sc is clean else int(round(0.1 * n_both)))
    # the exact projections of the clean scene, rounded to float32
    k = clean["track"][3]
    exact = bi.project(clean["R"], clean["t"], clean["X"], np.full(len(k), 3), k)
    assert np.array_equal(clean["keypoints"][3], exact.astype(np.float32))
    # 0.5 px of noise
    k = noisy["track"][3][:len(clean["track"][3])]
    d = noisy["keypoints"][3][:len(k)] - bi.project(noisy["R"], noisy["t"], noisy["X"], np.full(len(k), 3), k)
    assert 0.4 < d.std() < 0.6
    # a replaced match is consistent with the true epipolar geometry of its pair, and its point is a wrong one
    Kinv = np.linalg.inv(ci.K)
    for (i, j) in ((0, 1), (1, 4), (2, 5)):
        Ri, Rj = noisy["R"][i].reshape(3, 3), noisy["R"][j].reshape(3, 3)
        Rr = Rj @ Ri.T
        tr_ = noisy["t"][j] - Rr @ noisy["t"][i]
        tx = np.array([[0.0, -tr_[2], tr_[1]], [tr_[2], 0.0, -tr_[0]], [-tr_[1], tr_[0], 0.0]])
        F = Kinv.T @ tx @ Rr @ Kinv
        planted = [r for r in noisy["matches"][(i, j)] if noisy["track"][j][r[1]] == ci.FALSE_TRACK]
        assert len(planted) == int(round(0.1 * np.count_nonzero((seen[:, i] > 0) & (seen[:, j] > 0)))) >= 5
        for a, b in planted:
            x1, x2 = np.append(noisy["keypoints"][i][a], 1.0), np.append(noisy["keypoints"][j][b], 1.0)
            line = F @ x1
            assert abs(x2 @ line) / np.hypot(line[0], line[1]) < 2.5                           # five sigma of the noise of view i
            own = noisy["keypoints"][j][noisy["track"][j] == noisy["track"][i][a]]
            assert len(own) == 0 or np.linalg.norm(own[0] - noisy["keypoints"][j][b]) > 20.0      # far from the track's own pixel
    # edges is noisy and two more views: view 6 at the centre of view 2, view 7 with five keypoints
    for v in range(6):
        assert np.array_equal(edges["keypoints"][v][:len(noisy["keypoints"][v])], noisy["keypoints"][v])
    for p, m in noisy["matches"].items():
        assert np.array_equal(edges["matches"][p], m)
    assert np.abs(ci.centre(edges["R"][6], edges["t"][6]) - ci.centre(edges["R"][2], edges["t"][2])).max() < 1e-12
    turn = edges["R"][6].reshape(3, 3) @ edges["R"][2].reshape(3, 3).T
    assert abs(np.degrees(np.arccos((np.trace(turn) - 1.0) / 2.0)) - 4.0) < 1e-9 and abs(turn[1, 1] - 1.0) < 1e-15
    assert np.allclose(ci.centre(edges["R"][7], edges["t"][7]), (1.0, 1.5, -6.5)) and len(edges["keypoints"][7]) == 5
    assert all(len(edges["matches"][(v, 7)]) <= 5 for v in range(7))


# ----------------------------------------------------------------------------------------------------- the truth ---
@pytest.mark.parametrize("name", ci.NAMES)
def test_the_restatement_chain_finds_the_planted_scene(name):
    """Measured: largest rotation error 1.02e-6 degrees (clean), 0.117 (noisy), 0.112 (edges); asserted 1.02e-5, 1.17, 1.12.
    Measured: largest centre error 1.87e-7 baselines (clean), 0.0146 (noisy), 0.0151 (edges); asserted 1.87e-6, 0.146, 0.151.
    Measured: largest point error 5.93e-7 baselines (clean), 0.0345 (noisy; median 0.0249), 0.0368 (edges; median 0.0247);
    asserted 5.93e-6, 0.345, 0.368.
    Measured: final RMS reprojection error 2.27e-5 px (clean), 0.771 (noisy), 0.749 (edges); asserted 2.27e-4, 7.71, 7.49.
    Compared points: 160 (clean), 141 (noisy), 147 (edges) of the 160 planted; at least 120 asserted.

    The errors of the noisy scenes are those of the relative pose of the initial pair, which the fundamental matrix of
    some 80 matches with 0.5 px of noise gives to 0.11 degrees and which both bundle adjustments hold fixed: every other
    view is within 0.12 degrees of it.  On these scenes the filter between the two bundle adjustments drops nothing: the
    registrations have rejected every planted false correspondence before."""
    sc, rec, _, seconds = ch.restated(name)
    e = ch.truth_errors(sc, rec)
    print(f"{name}: rotation {e['rotation']:.3g} degrees, centre {e['centre']:.3g}, point {e['point']:.3g} (median {e['point_median']:.3g}) "
          f"baselines, rms {e['rms']:.3g} px, {len(e['compared'])} points compared, chain {seconds:.1f} s")
    rot, cen, pnt, rms = MEASURED[name]
    assert e["rotation"] < 10.0 * rot and e["centre"] < 10.0 * cen and e["point"] < 10.0 * pnt and e["rms"] < 10.0 * rms
    assert rec["registered"] == REGISTERED[name]                           # all six; on edges views 0 .. 6 and not 7
    assert sorted(rec["registered"]) == list(range(7 if name == "edges" else 6))
    assert e["mixed"] == []                                                # no point of three observations mixes tracks
    assert len(set(e["compared"])) >= 120
    i0, j0 = rec["registered"][:2]
    assert rec["initial"]["winner"]["pair"] == (i0, j0) == rec["initial"]["candidates"][0]["pair"]
    final = rec["bundles"][-1]
    assert len(rec["bundles"]) == 2 and final["fixed"] == [i0, j0]
    for v in (i0, j0):                                                     # the fixed views have not moved
        assert ch.same_bits(final["after"]["poses"][v]["R"], rec["bundles"][0]["before"]["poses"][v]["R"])
        assert ch.same_bits(final["after"]["poses"][v]["t"], rec["bundles"][0]["before"]["poses"][v]["t"])
    assert np.array_equal(final["after"]["poses"][i0]["R"], np.eye(3)) and not final["after"]["poses"][i0]["t"].any()
    assert abs(np.linalg.norm(final["after"]["poses"][j0]["t"]) - 1.0) < 1e-12
    rows = final["rows"]                                                   # what the bundle adjustment demands
    assert all(len(o) >= 2 for o in rec["observations"].values()) and len(rows) == sum(len(o) for o in rec["observations"].values())


def test_noisy_registrations_reject_planted_false_correspondences_and_nothing_else():
    """Rejected: 13 of 56, 15 of 84, 20 of 91 and 5 of 101 correspondences (views 4, 3, 5, 0), every one a planted false one."""
    sc, rec, _, _ = ch.restated("noisy")
    seen = []
    for r in rec["registrations"]:
        false = ch.planted_false(sc, rec, r)
        seen.append((r["view"], len(false), int((~r["mask"]).sum())))
        assert (~r["mask"]).sum() >= 1 and false[~r["mask"]].all() and not false[r["mask"]].any()
        assert r["info"]["n_inliers"] == r["mask"].sum()
    print(seen)
    assert len(seen) == 4
    # on the clean scene the one false match that passed the fundamental matrix of its pair is rejected as well
    sc, rec, _, _ = ch.restated("clean")
    for r in rec["registrations"]:
        assert np.array_equal(~r["mask"], ch.planted_false(sc, rec, r))


def test_edges_pure_rotation_and_the_view_with_five_keypoints():
    sc, rec, _, _ = ch.restated("edges")
    dropped = rec["aside"]["dropped"]
    assert dropped[(2, 6)] == ("valid", 0)                                 # none of the 50 sampled candidates is valid
    for v in range(7):
        assert dropped[(v, 7)] == ("matches", len(sc["matches"][(v, 7)]))
        assert not rec["pairs"][(v, 7)]["model"] and not rec["pairs"][(v, 7)]["mask"].any() and rec["pairs"][(v, 7)]["info"] is None
    assert rec["pairs"][(2, 6)]["model"] and rec["pairs"][(2, 6)]["mask"].sum() >= 50       # the F-RANSAC alone does not see it
    both = [t for t in rec["triangulations"] if t["pair"] == (2, 6)]
    assert len(both) == 1 and len(both[0]["valid"]) >= 10 and not both[0]["valid"].any() and both[0]["added"] == []
    assert (both[0]["cos"] > np.cos(np.deg2rad(1.0))).all()                # no parallax: the gate that refuses them
    last = rec["registrations"][-1]
    assert last["view"] == 7 and len(last["keypoints"]) < ch.MIN_CORRESPONDENCES and last["pose"] is None and last["mask"] is None
    assert 7 not in rec["registered"] and 6 in rec["registered"]
    scores = [c["score"] for c in rec["initial"]["candidates"]]
    pairs = [c["pair"] for c in rec["initial"]["candidates"]]
    assert scores == sorted(scores, reverse=True)
    at = pairs.index((4, 6))                                               # a tie: the order of pair_points decides
    assert pairs[at + 1] == (5, 6) and scores[at] == scores[at + 1] == 67.0


# ------------------------------------------------------------------------------------ the check must be able to fail ---
@pytest.mark.parametrize("variant,outcome", [("F transposed", "stops"), ("pose inverted", "wrong"), ("pixels swapped", "stops"),
                                             ("points rolled", "stops"), ("second view identity", "stops")])
def test_a_slip_at_one_boundary_is_seen(variant, outcome):
    """On the clean scene each variant of RestatementOps either stops before all six views are registered or fails the
    truth check.  F transposed: another pair wins, (0, 1), and the chain stops at its two views.  Pose inverted: all six
    register, each against the points of the views before, with rotation errors up to 91 degrees.  Pixels swapped, points
    rolled, second view identity: the chain stops at the two views of the initial pair."""
    sc, _, ops, _ = ch.restated("clean")
    rec = ch.run(sc, ch.RestatementOps(sc["K"], variant, ops.memo))        # (the calls a variant leaves as they are, are not made again)
    print(variant, rec["registered"])
    if outcome == "stops":
        assert len(rec["registered"]) < 6
        return
    assert len(rec["registered"]) == 6
    e = ch.truth_errors(sc, rec)
    rot, cen, pnt, _ = MEASURED["clean"]
    assert e["rotation"] > 1e6 * rot and e["centre"] > 1e6 * cen
    assert not (e["rotation"] < 10.0 * rot and e["centre"] < 10.0 * cen and e["point"] < 10.0 * pnt)


def test_first_difference_names_the_boundary():
    _, rec, _, _ = ch.restated("clean")
    assert ch.first_difference(rec, rec) is None
    other = dict(rec, registrations=[dict(r) for r in rec["registrations"]])
    R = other["registrations"][1]["pose"]["R"].copy()
    R[0, 0] = np.nextafter(R[0, 0], 2.0)
    other["registrations"][1] = dict(other["registrations"][1], pose={"R": R, "t": other["registrations"][1]["pose"]["t"]})
    assert ch.first_difference(rec, other) == "record['registrations'][1]['pose']['R']: values differ"
    other = dict(rec, registered=rec["registered"][::-1])
    assert ch.first_difference(rec, other).startswith("record['registered'][0]")
