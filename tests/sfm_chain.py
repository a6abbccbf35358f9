"""The bookkeeping a caller puts around the sparse-reconstruction stages, written once for the tests: the library's
docstrings leave it to the caller, and no caller is in the tree.  run() chains fundamental-matrix RANSAC, the initial
pair, triangulation, registration and bundle adjustment on a scene of tests/sfm_chain_inputs.py through an `ops` object
and records what crosses every boundary between two stages.  DeviceOps calls the public layer of the library,
RestatementOps the restatements of the headers (tests/*_restatement.py); tests/test_hip_sfm_chain.py compares their
records bit for bit, tests/test_sfm_chain_cpu.py compares the restatement's with the planted truth.

These rules are the test's own, not a pipeline of the library.  Every tie goes to the lowest index.
 1. The initial pair is picked from all pairs, pair_points in ascending (i, j).
 2. Every pair is verified by the F-RANSAC; its inlier matches are kept, or none when there is no model.  A pair with
    fewer than MIN_MATCHES matches is not handed to it (the entry point refuses fewer) and keeps none.
 3. View i0 of the initial pair is [I | 0] and view j0 is (R, t).  Their verified matches are triangulated; each valid
    candidate becomes a point that owns its two keypoints.
 4. For every unregistered view the correspondences are collected: its keypoints matched through a verified pair to an
    owned keypoint of a registered view, the registered views in ascending order and each pair's matches in match
    order; a keypoint keeps its first point and a point its first keypoint.  The view with the most correspondences is
    registered; the chain stops when that one has fewer than MIN_CORRESPONDENCES or is refused.  The inliers become
    observations of their points.  The new view's verified matches with every registered view, in ascending order, are
    triangulated where neither keypoint is owned.
 5. All registered views and all points are bundle-adjusted with i0 and j0 fixed.
 6. Observations with an error above MAX_ERROR_PX (squared: 16 px^2) or behind their camera are dropped, then points left
    with fewer than two observations; the rest is bundle-adjusted once more.

An ops object has
    initial_pair(pair_points) -> (candidates best first, winner or None, dropped or None)
    verify(pts1, pts2) -> (F (3, 3) or None, mask, info)
    triangulate(R1, t1, R2, t2, pts1, pts2) -> (X, valid, cos)
    register(X, x) -> ((R (3, 3), t (3,)) or None, mask, info)
    bundle(poses, points, rows, fixed) -> (poses, points, report)
    errors(poses, points, rows) -> (N,) pixels, NaN behind the camera
with poses a dict view -> (R, t), points a dict id -> xyz and rows an (N, 4) float64 array of (view, id, u, v)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_restatement as br  # noqa: E402
import epipolar_restatement as er  # noqa: E402
import resection_restatement as rr  # noqa: E402
import twoview_restatement as tr  # noqa: E402

F_THRESHOLD, F_CONFIDENCE, F_HYPOTHESES = 1.0, 0.999, 4096
PNP_THRESHOLD, PNP_CONFIDENCE, PNP_HYPOTHESES = 8.0, 0.99, 5000
SEED = 0
MIN_MATCHES = 8                 # fewer are a parameter error of amvs_fmat_ransac
MIN_CORRESPONDENCES = 6
MAX_ERROR_PX = 4.0
CANDIDATE_KEYS = ("pair", "mask", "R", "t", "parallax", "score", "pts1", "pts2", "valid_ratio")
VARIANTS = (None, "F transposed", "pose inverted", "pixels swapped", "points rolled", "second view identity")


# ---- the two implementations of ops ------------------------------------------------------------------------------------------
class DeviceOps:
    """The public layer on one shared Engine, or with fresh=True on an Engine(8, 8, 1, eye) of its own for every call."""

    def __init__(self, K, engine=None, fresh=False):
        from amvs.core.camera import Camera
        self.camera, self.K, self.engine, self.fresh = Camera(K), np.asarray(K, np.float64), engine, fresh
        assert fresh != (engine is not None)

    def _call(self, fn):
        if not self.fresh:
            return fn(self.engine)
        import amvs
        with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as e:
            return fn(e)

    def initial_pair(self, pair_points):
        """The library returns the winner alone; the list is put together from the pairs taken one at a time, each of
        which is then its own largest component."""
        from amvs.core import find_best_initial_pair
        winner = self._call(lambda e: find_best_initial_pair(self.camera, pair_points, engine=e))
        found = [self._call(lambda e: find_best_initial_pair(self.camera, {pair: pair_points[pair]}, engine=e)) for pair in pair_points]
        found = sorted([c for c in found if c is not None], key=lambda c: -c["score"])
        return found, winner, None

    def verify(self, pts1, pts2):
        return self._call(lambda e: e.fundamental_ransac(pts1, pts2, threshold=F_THRESHOLD, confidence=F_CONFIDENCE,
                                                         max_hypotheses=F_HYPOTHESES, seed=SEED))

    def triangulate(self, R1, t1, R2, t2, pts1, pts2):
        from amvs.core import triangulate_points
        from amvs.core.camera import CameraPose
        return self._call(lambda e: triangulate_points(self.camera, CameraPose(R1, t1), CameraPose(R2, t2), pts1, pts2,
                                                       return_cos=True, engine=e))

    def register(self, X, x):
        """register_view, and the same call once more one layer down for the info and the mask it does not hand on."""
        from amvs.core import register_view
        got = self._call(lambda e: register_view(self.camera, X, x, engine=e))
        _, _, mask, info = self._call(lambda e: e.pnp_ransac(np.asarray(X, np.float32), x, self.K, threshold=PNP_THRESHOLD,
                                                             confidence=PNP_CONFIDENCE, max_hypotheses=PNP_HYPOTHESES, seed=SEED))
        if got is None:
            return None, mask, info
        assert np.array_equal(got[1], mask)
        return (got[0].R, np.ravel(got[0].t)), got[1], info

    @staticmethod
    def _poses(poses):
        from amvs.core.camera import CameraPose
        return {v: CameraPose(R, t) for v, (R, t) in poses.items()}

    def bundle(self, poses, points, rows, fixed):
        from amvs.core import bundle_adjust
        new, pts, report = self._call(lambda e: bundle_adjust(self.camera, self._poses(poses), points, rows, fixed=fixed, engine=e))
        return {v: (p.R, np.ravel(p.t)) for v, p in new.items()}, pts, report

    def errors(self, poses, points, rows):
        from amvs.core import reprojection_errors
        return self._call(lambda e: reprojection_errors(self.camera, self._poses(poses), points, rows, engine=e))


def _key(*args):
    out = []
    for a in args:
        if isinstance(a, np.ndarray):
            out.append((a.dtype.str, a.shape, a.tobytes()))
        else:
            out.append(a)
    return tuple(out)


class RestatementOps:
    """The restatements of the headers with the defaults of the Python layer.  Identical calls are computed once (the
    memo may be shared between instances).  variant: one of VARIANTS, a slip planted at one boundary.  log_decided
    collects, per RANSAC call, the (done, N) of the batches whose N came from a logarithm: the device takes log from
    another library, so a comparison with it holds only where no stop is decided within 2 of N."""

    def __init__(self, K, variant=None, memo=None):
        assert variant in VARIANTS
        self.K, self.variant, self.memo, self.log_decided = np.asarray(K, np.float64), variant, {} if memo is None else memo, []

    def _memo(self, name, fn, *args):
        key = (name,) + _key(*args)
        if key not in self.memo:
            self.memo[key] = fn()
        return self.memo[key]

    def _fmat(self, pts1, pts2, threshold=F_THRESHOLD, confidence=F_CONFIDENCE):
        pts1, pts2 = np.ascontiguousarray(pts1, np.float32), np.ascontiguousarray(pts2, np.float32)
        F, mask, n, info, trace = self._memo("fmat", lambda: er.ransac(pts1, pts2, threshold, confidence, F_HYPOTHESES, SEED),
                                             pts1, pts2, threshold, confidence)
        self.log_decided += [(done, N) for done, N, from_log in trace if from_log]
        out = {"hypotheses": int(info[0]), "best_hypothesis": int(info[1]), "best_count": int(info[2]), "n_inliers": int(n)}
        return (F.reshape(3, 3).copy() if n >= 8 else None), mask.copy(), out

    def initial_pair(self, pair_points):
        def ransac(p1, p2, threshold, confidence):
            F, mask, _ = self._fmat(p1, p2, threshold, confidence)
            if F is not None and self.variant == "F transposed":
                F = F.T
            return F, mask

        dropped = {}
        found = tr.find_best_initial_pair(self.K, pair_points, ransac, dropped)
        winner = dict(found[0]) if found else None
        if winner is not None and self.variant == "second view identity":
            winner["R"], winner["t"] = np.eye(3), np.zeros((3, 1))
        return found, winner, dropped

    def verify(self, pts1, pts2):
        return self._fmat(pts1, pts2)

    def triangulate(self, R1, t1, R2, t2, pts1, pts2):
        if self.variant == "pixels swapped":
            pts1, pts2 = pts2, pts1
        pts1, pts2 = np.ascontiguousarray(pts1, np.float32), np.ascontiguousarray(pts2, np.float32)
        a = [np.ascontiguousarray(x, np.float64) for x in (R1, t1, R2, t2)]
        X, valid, cs = self._memo("tri", lambda: tr.triangulate(self.K, *a, pts1, pts2), *a, pts1, pts2)
        return X.copy(), valid.copy(), cs.copy()

    def register(self, X, x):
        X, x = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(x, np.float32)
        if self.variant == "points rolled":
            X = np.roll(X, 1, axis=0)
        if len(X) < MIN_CORRESPONDENCES:
            return None, np.zeros(len(X), bool), None
        R, t, mask, n, info, trace, _ = self._memo(
            "pnp", lambda: rr.ransac(X, x, self.K, PNP_THRESHOLD, PNP_CONFIDENCE, PNP_HYPOTHESES, SEED), X, x)
        self.log_decided += [(done, N) for done, N, from_log in trace if from_log]
        out = {"hypotheses": int(info[0]), "best_hypothesis": int(info[1]), "best_count": int(info[2]), "n_inliers": int(n)}
        if n < MIN_CORRESPONDENCES:
            return None, mask.copy(), out
        R, t = R.reshape(3, 3).copy(), t.copy()
        if self.variant == "pose inverted":
            R, t = R.T.copy(), -(R.T @ t)
        return (R, t), mask.copy(), out

    def _problem(self, poses, points, rows, fixed=None):
        """The arrays of include/amvs_bundle.h: views and ids ascending, observations strictly ascending in (pt, cam)."""
        views, ids = sorted(poses), sorted(points)
        rows = np.asarray(rows, np.float64).reshape(-1, 4)
        cam = np.array([views.index(int(v)) for v in rows[:, 0]], np.int64)
        pt = np.searchsorted(ids, rows[:, 1].astype(np.int64))
        order = np.argsort(pt * len(views) + cam, kind="stable")
        fx = None if fixed is None else np.array([v in fixed for v in views], np.uint8)
        q = br.Problem(cam[order], pt[order], rows[order, 2:4].astype(np.float32), self.K, len(views), len(ids), fx)
        R = np.array([np.asarray(poses[v][0], np.float64).reshape(9) for v in views])
        t = np.array([np.asarray(poses[v][1], np.float64).reshape(3) for v in views])
        X = np.array([np.asarray(points[p], np.float64).reshape(3) for p in ids])
        return views, ids, q, R, t, X, order

    @staticmethod
    def _mean(err2):
        front = err2[err2 >= 0.0]
        return float(np.sqrt(front).mean()) if front.size else float("nan")

    def bundle(self, poses, points, rows, fixed):
        views, ids, q, R, t, X, _ = self._problem(poses, points, rows, fixed)

        def work():
            Rn, tn, Xn, info = br.solve(q, R, t, X)
            return Rn, tn, Xn, info, br.cost(q, R, t, X)[2], br.cost(q, Rn, tn, Xn)[2]

        Rn, tn, Xn, info, before, after = self._memo("ba", work, q.cam, q.pt, q.uv, q.fixed, R, t, X)
        report = {"trials": int(info[0]), "kept": int(info[1]), "lambda": float(info[2]), "first_cost": float(info[3]),
                  "cost": float(info[4]), "active": int(info[5]), "mean_error_before": self._mean(before),
                  "mean_error_after": self._mean(after)}
        return ({v: (Rn[i].reshape(3, 3).copy(), tn[i].copy()) for i, v in enumerate(views)},
                {p: Xn[i].copy() for i, p in enumerate(ids)}, report)

    def errors(self, poses, points, rows):
        _, _, q, R, t, X, order = self._problem(poses, points, rows)
        err2 = self._memo("cost", lambda: br.cost(q, R, t, X)[2], q.cam, q.pt, q.uv, R, t, X)
        out = np.empty(len(order), np.float64)
        with np.errstate(invalid="ignore"):
            out[order] = np.where(err2 < 0.0, np.nan, np.sqrt(err2))
        return out


# ---- the bookkeeping ---------------------------------------------------------------------------------------------------------
def _candidate(c):
    return None if c is None else {k: (tuple(c[k]) if k == "pair" else c[k]) for k in CANDIDATE_KEYS}


def _state(poses, points):
    return {"poses": {v: {"R": np.array(R, np.float64), "t": np.array(t, np.float64)} for v, (R, t) in sorted(poses.items())},
            "points": {p: np.array(x, np.float64) for p, x in sorted(points.items())}}


def run(sc, ops):
    """The record of the chain on the scene sc: a tree of dicts, lists, arrays and numbers, every boundary in it.  What
    only one implementation can give stands under "aside" and is left out of a comparison."""
    kp, matches = sc["keypoints"], sc["matches"]
    pairs = sorted(matches)
    pair_points = {p: (kp[p[0]][matches[p][:, 0]], kp[p[1]][matches[p][:, 1]]) for p in pairs}
    rec = {"aside": {}, "pairs": {}, "triangulations": [], "registrations": [], "registered": [], "created": {},
           "bundles": []}

    found, winner, dropped = ops.initial_pair(pair_points)                                          # rule 1
    rec["initial"] = {"candidates": [_candidate(c) for c in found], "winner": _candidate(winner)}
    rec["aside"]["dropped"] = dropped

    verified = {}                                                                                   # rule 2
    for p in pairs:
        if len(matches[p]) < MIN_MATCHES:
            F, mask, info = None, np.zeros(len(matches[p]), bool), None
        else:
            F, mask, info = ops.verify(*pair_points[p])
        rec["pairs"][p] = {"F": np.zeros((3, 3)) if F is None else F, "model": F is not None, "mask": mask, "info": info}
        verified[p] = matches[p][mask] if F is not None else matches[p][:0]
    if winner is None:
        return rec

    poses, points, obs, owner = {}, {}, {}, {}

    def triangulate(a, b):
        """The verified matches of the pair (a, b), a < b, both posed, where neither keypoint is owned: new points."""
        rows = np.array([r for r in verified.get((a, b), ()) if (a, int(r[0])) not in owner and (b, int(r[1])) not in owner],
                        np.int32).reshape(-1, 2)
        if len(rows) == 0:
            return
        X, valid, cs = ops.triangulate(*poses[a], *poses[b], kp[a][rows[:, 0]], kp[b][rows[:, 1]])
        added = []
        for r, x, ok in zip(rows, X, valid):
            ka, kb = (a, int(r[0])), (b, int(r[1]))
            if ok and ka not in owner and kb not in owner:
                pid = len(points)
                points[pid], obs[pid] = np.array(x, np.float64), {a: ka[1], b: kb[1]}
                owner[ka] = owner[kb] = pid
                rec["created"][pid] = (ka, kb)
                added.append(pid)
        rec["triangulations"].append({"pair": (a, b), "matches": rows, "X": X, "valid": valid, "cos": cs, "added": added})

    i0, j0 = winner["pair"]                                                                         # rule 3
    poses[i0] = (np.eye(3), np.zeros(3))
    poses[j0] = (np.array(winner["R"], np.float64), np.ravel(winner["t"]).astype(np.float64))
    rec["registered"] += [i0, j0]
    triangulate(i0, j0)

    n_views = len(kp)
    while len(poses) < n_views:                                                                     # rule 4
        best, best_c = None, None
        for v in range(n_views):
            if v in poses:
                continue
            c, taken = {}, set()
            for r in sorted(poses):
                p, col = ((r, v), 1) if r < v else ((v, r), 0)
                for m in verified.get(p, ()):
                    kv, pid = int(m[col]), owner.get((r, int(m[1 - col])))
                    if pid is not None and kv not in c and pid not in taken:
                        c[kv] = pid
                        taken.add(pid)
            if best is None or len(c) > len(best_c):
                best, best_c = v, c
        kps, pids = np.array(list(best_c), np.int64), np.array(list(best_c.values()), np.int64)
        entry = {"view": best, "keypoints": kps, "points": pids, "pose": None, "mask": None, "info": None}
        rec["registrations"].append(entry)
        if len(kps) < MIN_CORRESPONDENCES:
            break
        X = np.array([points[p] for p in pids], np.float64)
        pose, entry["mask"], entry["info"] = ops.register(X, kp[best][kps])
        if pose is None:
            break
        entry["pose"] = {"R": pose[0], "t": pose[1]}
        others = sorted(poses)
        poses[best] = (np.array(pose[0], np.float64), np.array(pose[1], np.float64))
        rec["registered"].append(best)
        for k, pid, ok in zip(kps, pids, entry["mask"]):
            if ok:
                owner[(best, int(k))] = int(pid)
                obs[int(pid)][best] = int(k)
        for r in others:
            triangulate(min(r, best), max(r, best))

    fixed = [i0, j0]
    for again in (False, True):                                                                     # rules 5 and 6
        if again:
            err = ops.errors(poses, points, rows)
            keep = ~(np.isnan(err) | (err > MAX_ERROR_PX))
            for (v, pid), ok in zip(rows[:, :2].astype(np.int64), keep):
                if not ok:
                    del obs[int(pid)][int(v)]
            for pid in [p for p in obs if len(obs[p]) < 2]:
                del obs[pid], points[pid]
            rec["filter"] = {"errors": err, "kept": keep, "points": np.array(sorted(points), np.int64)}
        rows = np.array([(v, pid, *kp[v][k].astype(np.float64)) for pid in sorted(obs) for v, k in sorted(obs[pid].items())],
                        np.float64).reshape(-1, 4)
        if len(rows) == 0:                                                                          # (nothing to adjust)
            break
        entry = {"fixed": fixed, "rows": rows, "before": _state(poses, points)}
        new_poses, new_points, entry["report"] = ops.bundle(poses, points, rows, fixed)
        poses = {v: (np.array(R, np.float64), np.array(t, np.float64)) for v, (R, t) in new_poses.items()}
        points = {p: np.array(x, np.float64) for p, x in new_points.items()}
        entry["after"] = _state(poses, points)
        rec["bundles"].append(entry)
    rec["observations"] = {p: dict(sorted(o.items())) for p, o in sorted(obs.items())}
    return rec


_RESTATED = {}


def restated(name):
    """(scene, record, ops, seconds) of the restatement chain on a scene of tests/sfm_chain_inputs.py; once per process."""
    import time

    import sfm_chain_inputs as ci
    if name not in _RESTATED:
        sc = ci.scene(name)
        ops = RestatementOps(sc["K"])
        start = time.perf_counter()
        rec = run(sc, ops)
        _RESTATED[name] = (sc, rec, ops, time.perf_counter() - start)
    return _RESTATED[name]


# ---- comparing two records ---------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """Equal as bit patterns, a NaN matching any NaN (the same_bits of tests/test_hip_bundle.py)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


def first_difference(a, b, where="record", same=same_bits):
    """The path of the first boundary at which two records differ, or None.  Floats are compared with `same`, everything
    else for equality, types and shapes included; "aside" is skipped."""
    if isinstance(a, dict) or isinstance(b, dict):
        if not (isinstance(a, dict) and isinstance(b, dict)) or list(a) != list(b):
            return f"{where}: keys {list(a) if isinstance(a, dict) else a!r} / {list(b) if isinstance(b, dict) else b!r}"
        for k in a:
            if k != "aside":
                d = first_difference(a[k], b[k], f"{where}[{k!r}]", same)
                if d:
                    return d
        return None
    if isinstance(a, (list, tuple)) or isinstance(b, (list, tuple)):
        if not (isinstance(a, (list, tuple)) and isinstance(b, (list, tuple))) or len(a) != len(b):
            return f"{where}: {a!r} / {b!r}"
        for i, (x, y) in enumerate(zip(a, b)):
            d = first_difference(x, y, f"{where}[{i}]", same)
            if d:
                return d
        return None
    if a is None or b is None or isinstance(a, (str, bool)) or isinstance(b, (str, bool)):
        return None if (type(a) is type(b) and a == b) else f"{where}: {a!r} / {b!r}"
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or (a.dtype.kind == "f") != (b.dtype.kind == "f") or (a.dtype.kind == "b") != (b.dtype.kind == "b"):
        return f"{where}: {a.dtype}{a.shape} / {b.dtype}{b.shape}"
    equal = same(a, b) if a.dtype.kind == "f" else np.array_equal(a, b)
    return None if equal else f"{where}: values differ"


# ---- the planted truth in the chain's frame -----------------------------------------------------------------------------------
def planted_false(sc, rec, registration):
    """(m,) bool over a registration's correspondences: True where the keypoint and the two keypoints its point was
    made from are not all of one planted track."""
    v, out = registration["view"], []
    for k, pid in zip(registration["keypoints"], registration["points"]):
        tracks = {int(sc["track"][v][k])} | {int(sc["track"][a][ka]) for a, ka in rec["created"][int(pid)]}
        out.append(len(tracks) != 1 or min(tracks) < 0)
    return np.array(out, bool)



def truth_errors(sc, rec, min_observations=3):
    """The final state of a record against the planted scene in the chain's gauge: view i0 at the origin and the
    baseline |C_j0 - C_i0| of length 1, so nothing is fitted.  Returns a dict: "rotation" (the largest angle in degrees
    between a registered view's rotation and the truth), "centre" (the largest distance of a view's centre from the
    truth, in baselines), "point" and "point_median" (over the compared points: those with at least min_observations
    observations, all of one planted track), "compared" (the track ids of those), "mixed" (the ids of points with at
    least min_observations observations that carry more than one track id or a false one) and "rms" (of the last
    bundle adjustment, in pixels)."""
    i0, j0 = rec["registered"][:2]
    R0, t0 = sc["R"][i0].reshape(3, 3), sc["t"][i0]

    def centre(v):
        return -(sc["R"][v].reshape(3, 3).T @ sc["t"][v])

    b = float(np.linalg.norm(centre(j0) - centre(i0)))
    final = rec["bundles"][-1]["after"]
    per_view = {}
    for v, pose in final["poses"].items():
        D = pose["R"] @ (sc["R"][v].reshape(3, 3) @ R0.T).T
        s = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
        angle = float(np.degrees(np.arctan2(s, 0.5 * (np.trace(D) - 1.0))))     # (exact for small angles, unlike arccos)
        Ct = (R0 @ centre(v) + t0) / b
        per_view[v] = (angle, float(np.linalg.norm(-(pose["R"].T @ pose["t"]) - Ct)))
    rot, cen = max(a for a, _ in per_view.values()), max(c for _, c in per_view.values())
    errs, compared, mixed = [], [], []
    for pid, o in rec["observations"].items():
        if len(o) < min_observations:
            continue
        tracks = {int(sc["track"][v][k]) for v, k in o.items()}
        if len(tracks) != 1 or min(tracks) < 0:
            mixed.append(pid)
            continue
        p = tracks.pop()
        compared.append(p)
        errs.append(float(np.linalg.norm(final["points"][pid] - (R0 @ sc["X"][p] + t0) / b)))
    report = rec["bundles"][-1]["report"]
    return {"rotation": rot, "centre": cen, "per_view": per_view, "point": max(errs) if errs else float("nan"),
            "point_median": float(np.median(errs)) if errs else float("nan"), "compared": compared, "mixed": mixed,
            "rms": float(np.sqrt(report["cost"] / max(report["active"], 1)))}
