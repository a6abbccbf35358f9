"""Two-view geometry on the device (include/amvs_twoview.h): the relative pose of two views from their fundamental matrix,
the triangulation of their matches, and the choice of the pair a reconstruction starts from.

The module carries the surface of the reference's src/core/geometry.py without OpenCV: decompose_essential is its
cv.recoverPose call (geometry.py:160), triangulate_points its cv.triangulatePoints call followed by
validate_triangulation (geometry.py:15-125).  find_best_initial_pair follows SfMPipeline.find_best_initial_pair
(sfm_pipeline.py:331-433) step for step; the observation bookkeeping of SfMPipeline.initialize (sfm_pipeline.py:435-471)
around it stays with the caller.  Parity with cv2 is UNPINNED; in particular the masks here are
bool (N,), where cv's are 0 / 255 or 0 / 1 of shape (N, 1).  Lens distortion is not modelled: the views are undistorted
before they are matched."""
from typing import Optional, Tuple

import numpy as np

from .camera import CameraPose
from .registration import _engine_for

MAX_DEPTH = 50.0                  # cv.recoverPose's distance threshold, in baselines
DEPTH_MIN = 0.01                  # geometry.py:86, :92
DEPTH_BASELINES = 200.0           # geometry.py:97
MIN_PARALLAX_DEG = 1.0            # geometry.py:62
MAX_REPROJ = 4.0                  # geometry.py:61
MIN_MATCHES_FOR_INIT = 50         # sfm_pipeline.py:344, applied to the matches (:350) and to the inliers (:366)
F_THRESHOLD, F_CONFIDENCE = 1.0, 0.999      # sfm_pipeline.py:357
SAMPLE_SIZE = 50                  # sfm_pipeline.py:375
MIN_VALID = 20                    # sfm_pipeline.py:384
PARALLAX_WINDOW = (1.5, 40.0)     # sfm_pipeline.py:400, both ends kept
BONUS_WINDOW, BONUS = (3.0, 20.0), 1.5      # sfm_pipeline.py:404-405, both ends excluded


def _points(points1, points2):
    p1 = np.asarray(points1, dtype=np.float32).reshape(-1, 2)
    p2 = np.asarray(points2, dtype=np.float32).reshape(-1, 2)
    if len(p1) != len(p2):
        raise ValueError("points1 and points2 must have one row per match")
    return p1, p2


def compute_essential_matrix(camera, F) -> np.ndarray:
    """E = K^T F K (on the host)."""
    return camera.K.T @ np.asarray(F, dtype=np.float64).reshape(3, 3) @ camera.K


def relative_pose(camera, F, points1, points2, *, max_depth: float = MAX_DEPTH, engine=None,
                  device: int = 0) -> Optional[Tuple[CameraPose, np.ndarray]]:
    """(pose of the second view, mask (N,) bool of the matches in front of both cameras), the first view being [I | 0], or
    None: no match, F has no model (rank below 2, not finite), or no candidate puts a match in front.  The translation
    has unit length."""
    p1, p2 = _points(points1, points2)
    if len(p1) == 0:
        return None
    R, t, mask, _ = _engine_for(engine, device).twoview_pose(F, camera.K, p1, p2, max_depth=float(max_depth))
    if R is None:
        return None
    return CameraPose(R, t), mask


def decompose_essential(E, camera, points1, points2, *, engine=None, device: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(R (3, 3), t (3, 1) of unit length, mask (N,) bool) from an essential matrix, as the reference's function of this
    name.  The engine's entry point takes F, so this passes K^-T E K^-1: the E it then forms differs from the argument by
    the rounding of those four products, some 1e-16 of its size.  Raises ValueError when there is no model."""
    Ki = np.linalg.inv(camera.K)
    got = relative_pose(camera, Ki.T @ np.asarray(E, dtype=np.float64).reshape(3, 3) @ Ki, points1, points2, engine=engine,
                        device=device)
    if got is None:
        raise ValueError("the essential matrix has no pose: rank below 2, not finite, or no match in front of both cameras")
    pose, mask = got
    return pose.R, np.reshape(pose.t, (3, 1)), mask


def triangulate_points(camera, pose1, pose2, points1, points2, *, return_cos: bool = False, engine=None, device: int = 0):
    """(points_3d (N, 3) float64, valid (N,) bool) of the matches of two posed views, and with return_cos the cosine (N,) of
    every point's parallax angle as well.  valid: both depths above 0.01 and at most 200 baselines, a parallax angle of
    at least 1 degree, both reprojection errors at most 4 px (the reference's validate_triangulation; a point that is not
    finite is never valid here).  No match: the reference's (np.array([]), np.array([], dtype=bool))."""
    if len(points1) == 0:
        empty = (np.array([]), np.array([], dtype=bool))
        return empty + (np.array([]),) if return_cos else empty
    p1, p2 = _points(points1, points2)
    t1, t2 = np.ravel(pose1.t), np.ravel(pose2.t)
    baseline = float(np.linalg.norm(pose2.center - pose1.center))
    X, valid, cs = _engine_for(engine, device).twoview_triangulate(
        camera.K, pose1.R, t1, pose2.R, t2, p1, p2, depth_min=DEPTH_MIN, depth_max=baseline * DEPTH_BASELINES,
        cos_max_parallax=float(np.cos(np.deg2rad(MIN_PARALLAX_DEG))), max_reproj=MAX_REPROJ)
    return (X, valid, cs) if return_cos else (X, valid)


def compute_reprojection_error(camera, pose, points_3d, points_2d) -> np.ndarray:
    """Per-point reprojection error (N,) in pixels (NumPy)."""
    proj = camera.project(pose.transform_points(np.asarray(points_3d, dtype=np.float64)))
    return np.linalg.norm(proj - np.asarray(points_2d, dtype=np.float64), axis=1)


def _components(pairs):
    """The connected components of the pair graph, each sorted, in ascending order of their smallest view."""
    adj = {}
    for i, j in pairs:
        adj.setdefault(i, set()).add(j)
        adj.setdefault(j, set()).add(i)
    seen, out = set(), []
    for start in sorted(adj):
        if start in seen:
            continue
        comp, stack = [], [start]
        while stack:
            node = stack.pop()
            if node in seen:
                continue
            seen.add(node)
            comp.append(node)
            stack.extend(n for n in adj[node] if n not in seen)
        out.append(sorted(comp))
    return out


def find_best_initial_pair(camera, pair_points, *, engine=None, device: int = 0) -> Optional[dict]:
    """The pair of views a reconstruction starts from, or None.  pair_points maps (i, j) to (pts1, pts2), the matched pixels
    (N, 2) of views i and j.  Returns {'pair', 'mask' (N,) bool over the pair's input matches: the inliers of F, 'R',
    't' (3, 1), 'parallax' (the median parallax angle of the sample in degrees), 'score', 'pts1', 'pts2' (the inliers),
    'valid_ratio'}; view i is [I | 0] and view j is (R, t)."""
    comps = _components(pair_points.keys())
    if not comps:
        return None
    largest = set(max(comps, key=len))                       # the first of the largest ones
    eng = _engine_for(engine, device)
    candidates = []
    for (i, j), (pts1, pts2) in pair_points.items():
        if i not in largest or j not in largest:
            continue
        p1, p2 = _points(pts1, pts2)
        if len(p1) < MIN_MATCHES_FOR_INIT:
            continue
        F, mask, _ = eng.fundamental_ransac(p1, p2, threshold=F_THRESHOLD, confidence=F_CONFIDENCE)
        if F is None:
            continue
        mask = np.asarray(mask, dtype=bool)
        in1, in2 = p1[mask], p2[mask]
        if len(in1) < MIN_MATCHES_FOR_INIT:
            continue
        got = relative_pose(camera, F, in1, in2, engine=eng)
        if got is None:
            continue
        pose2 = got[0]
        sample = np.linspace(0, len(in1) - 1, min(SAMPLE_SIZE, len(in1)), dtype=int)
        _, valid, cs = triangulate_points(camera, CameraPose.identity(), pose2, in1[sample], in2[sample], return_cos=True, engine=eng)
        n_valid = int(np.sum(valid))
        if n_valid < MIN_VALID:
            continue
        parallax = float(np.median(np.degrees(np.arccos(np.clip(cs[valid], -1, 1)))))
        if parallax < PARALLAX_WINDOW[0] or parallax > PARALLAX_WINDOW[1]:
            continue
        ratio = n_valid / len(sample)
        score = len(in1) * ratio
        if BONUS_WINDOW[0] < parallax < BONUS_WINDOW[1]:
            score *= BONUS
        candidates.append({"pair": (i, j), "mask": mask, "R": pose2.R, "t": np.reshape(pose2.t, (3, 1)), "parallax": parallax,
                           "score": score, "pts1": in1, "pts2": in2, "valid_ratio": ratio})
    if not candidates:
        return None
    candidates.sort(key=lambda c: c["score"], reverse=True)  # stable: equal scores keep the order of pair_points
    return candidates[0]
