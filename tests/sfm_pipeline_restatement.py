"""The driver of core/sfm_pipeline.py SfMPipeline.reconstruct_from_features restated for the tests: the same rules over the
track-state restatement (tests/sfm_state_restatement.py) and the restatements of the numerical stages
(tests/sfm_chain.py RestatementOps), recording what crosses every boundary in the shape SfMPipeline's record= hook does.
tests/test_hip_sfm_pipeline.py compares the two records bit for bit; tests/test_sfm_state_cpu.py compares this one with
the planted truth.

The rules (every tie to the lowest index):
 1. The matches handed in are verified already.  The initial pair is picked from all of them, in ascending (i, j).
 2. View i0 is [I | 0], view j0 is (R, t); the track state begins, both enter without observations, and the rows of
    (i0, j0) are triangulated.
 3. The unregistered view with the highest score that has not failed is next; it needs a score of at least MIN_SCORE.  Its
    correspondences go to the registration; refused, the view has failed; else the inliers become observations and its
    matches with every registered view are triangulated.  Without a next view the failed ones are tried again, in
    ascending order, and the loop goes on if one of them came back.
 4. After every BA_EVERY newly registered views, and at the end: all registered views and all observed points are
    bundle-adjusted with i0 and j0 fixed; observations above MAX_ERROR_PX or behind their camera are dropped, then points
    left with fewer than MIN_OBS.  After the last one the rest is adjusted once more, and the failed views tried once more."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sfm_state_restatement as sr  # noqa: E402

MIN_SCORE, BA_EVERY, MAX_ERROR_PX, MIN_OBS = 12, 5, 4.0, 2


def _state(poses, X, ids):
    return {"poses": {v: {"R": np.array(R, np.float64), "t": np.array(t, np.float64)} for v, (R, t) in sorted(poses.items())},
            "points": {int(p): np.array(X[p], np.float64) for p in ids}}


def run(keypoints, matches, K, ops):
    """The record of the pipeline; ops as tests/sfm_chain.py describes it."""
    kps = [np.asarray(k, np.float32).reshape(-1, 2) for k in keypoints]
    matches = {tuple(p): np.asarray(m, np.int32).reshape(-1, 2) for p, m in sorted(matches.items())}
    n = len(kps)
    pair_points = {p: (kps[p[0]][m[:, 0]], kps[p[1]][m[:, 1]]) for p, m in matches.items()}
    _, winner, _ = ops.initial_pair(pair_points)
    if winner is None:
        raise ValueError("no initial pair")
    i0, j0 = winner["pair"]
    rec = {"aside": {}, "initial": {"pair": (i0, j0), "R": np.array(winner["R"], np.float64), "t": np.ravel(winner["t"]).astype(np.float64)},
           "registered": [i0, j0], "steps": [], "bundles": []}
    state = sr.State(kps, list(matches.items()))
    poses = {i0: (np.eye(3), np.zeros(3)), j0: (np.array(winner["R"], np.float64), np.ravel(winner["t"]).astype(np.float64))}
    for v in (i0, j0):
        state.register(v, *poses[v])
    rec["first_points"] = state.triangulate(j0, K)
    failed = set()

    def try_register(v, scores=None):
        kp, pid, X, x = state.correspondences(v)
        step = {"view": v, "scores": scores, "keypoints": kp, "points": pid, "X": X, "x": x, "pose": None, "mask": None, "set": 0, "new": None}
        rec["steps"].append(step)
        pose, mask, _ = ops.register(X, x)
        if pose is None:
            return False
        poses[v], step["mask"] = (np.array(pose[0], np.float64), np.array(pose[1], np.float64)), mask
        step["pose"] = {"R": poses[v][0], "t": poses[v][1]}
        step["set"] = state.register(v, poses[v][0], poses[v][1], kp, pid, mask)
        step["new"] = state.triangulate(v, K)
        rec["registered"].append(v)
        return True

    def adjust(drop):
        cam, pt, uv = state.observations()
        if len(cam) == 0:
            return
        X, alive = state.points()
        ids = np.unique(pt)
        rows = np.column_stack([cam, pt, uv.astype(np.float64)])
        entry = {"rows": rows, "before": _state(poses, X, ids)}
        new_poses, new_points, entry["report"] = ops.bundle(poses, {int(p): X[p] for p in ids}, rows, [i0, j0])
        for p in ids:
            X[p] = new_points[int(p)]
        state.set_points(X, alive)
        for v, (R, t) in new_poses.items():
            poses[v] = (np.array(R, np.float64), np.array(t, np.float64))
            state.set_pose(v, *poses[v])
        entry["after"] = _state(poses, X, ids)
        if drop:
            err = ops.errors(poses, new_points, rows)
            with np.errstate(invalid="ignore"):
                bad = np.isnan(err) | (err > MAX_ERROR_PX)
            entry["errors"], entry["dropped"] = err, state.drop(cam[bad], pt[bad], MIN_OBS)
        rec["bundles"].append(entry)

    def recover():
        back = [v for v in sorted(failed) if try_register(v)]
        failed.difference_update(back)
        return len(back)

    last_ba = 2
    while True:
        scores = state.scores()
        best = None
        for v in range(n):
            if scores[v] >= MIN_SCORE and v not in failed and (best is None or scores[v] > scores[best]):
                best = v
        if best is None:
            if failed and recover() > 0:
                continue
            break
        if not try_register(best, scores):
            failed.add(best)
            continue
        if len(poses) >= last_ba + BA_EVERY:
            adjust(True)
            last_ba = len(poses)
    adjust(True)
    adjust(False)
    if failed:
        recover()
    cam, pt, uv = state.observations()
    X, alive = state.points()
    ids = np.flatnonzero(alive)
    rec["final"] = {"observations": np.column_stack([cam, pt, uv.astype(np.float64)]).reshape(-1, 4), "points": X[ids], "ids": ids,
                    "failed": sorted(failed)}
    # for tests/sfm_chain.py truth_errors: point id -> {view: keypoint}
    rec["aside"]["observations"] = {}
    for v, owners in enumerate(state.owner):
        for k, p in enumerate(owners):
            if p >= 0:
                rec["aside"]["observations"].setdefault(p, {})[v] = k
    return rec


def verified_matches(chain_record, scene):
    """The matches of a scene that the chain's F-RANSAC kept (tests/sfm_chain.py rule 2), from its record: nothing is
    computed again."""
    out = {}
    for p, m in scene["matches"].items():
        entry = chain_record["pairs"][p]
        if entry["model"] and entry["mask"].any():
            out[p] = np.asarray(m, np.int32)[entry["mask"]]
    return out


_RESTATED = {}


def restated(name):
    """(scene, verified matches, record, ops) of this pipeline on a scene of tests/sfm_chain_inputs.py, once per process.  The
    matches are those the chain of tests/sfm_chain.py verified, and the ops share that chain's memo of identical calls."""
    import sfm_chain as ch
    if name not in _RESTATED:
        sc, chain_record, chain_ops, _ = ch.restated(name)
        ops = ch.RestatementOps(sc["K"], memo=chain_ops.memo)
        matches = verified_matches(chain_record, sc)
        _RESTATED[name] = (sc, matches, run(sc["keypoints"], matches, sc["K"], ops), ops)
    return _RESTATED[name]
