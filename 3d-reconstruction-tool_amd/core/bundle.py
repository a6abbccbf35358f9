"""Bundle adjustment: the poses of the registered views and the points of the cloud refined together on the device
(include/amvs_bundle.h), and the reprojection errors a caller filters outliers by.

bundle_adjust stands where the reference's SfMPipeline.bundle_adjustment_light does (sfm_pipeline.py:694-776): that one
polishes each camera against points it never moves, which is the mode refine_points=False here; the default moves
cameras and points together by Levenberg-Marquardt through the Schur complement.  The bookkeeping of observations
(which view saw which point where) stays with the caller, as in registration.py.  Lens distortion is not modelled: the
views are undistorted before they are matched."""
from typing import Dict, Iterable, Optional, Tuple

import numpy as np

from .camera import CameraPose
from .registration import _engine_for


def _problem(poses: Dict[int, CameraPose], points, observations):
    """The arrays of include/amvs_bundle.h from the caller's dicts: (views, point ids, R, t, X, cam, pt, uv)."""
    views = sorted(poses)
    if isinstance(points, dict):
        ids = sorted(points)
        X = np.array([np.asarray(points[i], np.float64).reshape(3) for i in ids], np.float64).reshape(-1, 3)
    else:
        X = np.asarray(points, np.float64).reshape(-1, 3)
        ids = list(range(len(X)))
    obs = np.asarray(list(observations), np.float64).reshape(-1, 4)
    view_at, point_at = {v: i for i, v in enumerate(views)}, {p: i for i, p in enumerate(ids)}
    try:
        cam = np.array([view_at[int(v)] for v in obs[:, 0]], np.int64)
        pt = np.array([point_at[int(p)] for p in obs[:, 1]], np.int64)
    except KeyError as e:
        raise ValueError(f"an observation names the unknown view or point {e.args[0]}") from None
    key = pt * max(len(views), 1) + cam
    order = np.argsort(key, kind="stable")
    if np.any(np.diff(key[order]) == 0):
        raise ValueError("a point is observed twice by one view")
    R = np.array([np.asarray(poses[v].R, np.float64).reshape(9) for v in views]).reshape(-1, 9)
    t = np.array([np.asarray(poses[v].t, np.float64).reshape(3) for v in views]).reshape(-1, 3)
    return views, ids, R, t, X, cam[order].astype(np.int32), pt[order].astype(np.int32), obs[order, 2:4].astype(np.float32), order


def reprojection_errors(camera, poses: Dict[int, CameraPose], points, observations, *, engine=None, device: int = 0) -> np.ndarray:
    """The reprojection error in pixels of every observation row (view, point id, u, v), in the caller's order; NaN for a
    point behind its camera."""
    views, ids, R, t, X, cam, pt, uv, order = _problem(poses, points, observations)
    _, _, err2 = _engine_for(engine, device).ba_cost(R, t, X, cam, pt, uv, camera.K)
    out = np.empty(len(order), np.float64)
    with np.errstate(invalid="ignore"):
        out[order] = np.where(err2 < 0.0, np.nan, np.sqrt(err2))
    return out


def bundle_adjust(camera, poses: Dict[int, CameraPose], points, observations: Iterable, *, fixed: Optional[Iterable[int]] = None,
                  refine_points: bool = True, lambda0: float = 1e-3, ftol: float = 1e-10, max_trials: int = 50, engine=None,
                  device: int = 0) -> Tuple[Dict[int, CameraPose], object, dict]:
    """(poses, points, report): the poses (a dict from view index to CameraPose) and the points (a dict from id to xyz, or an
    (P, 3) array, as given) after Levenberg-Marquardt on the reprojection error of the observations, rows
    (view, point id, u, v) in any order.

    fixed names the views that do not move; None fixes the lowest view index, as the reference does.  One fixed view
    leaves the scale of the reconstruction free (the damping keeps it where it is, nothing more); fixing a second view
    also fixes the scale.  refine_points=False is the reference's motion-only pass: every free camera is polished against
    the points as they are.

    report has the fields of the solver's info ("trials", "kept", "lambda", "first_cost", "cost", "active") and
    "mean_error_before" / "mean_error_after", the mean reprojection error in pixels over the observations in front of
    their cameras, the number the reference prints."""
    views, ids, R, t, X, cam, pt, uv, _ = _problem(poses, points, observations)
    eng = _engine_for(engine, device)
    fx = None
    if fixed is not None:
        names = set(int(v) for v in fixed)
        if not names <= set(views):
            raise ValueError("fixed names a view without a pose")
        fx = np.array([v in names for v in views], np.uint8)
    _, _, before = eng.ba_cost(R, t, X, cam, pt, uv, camera.K)
    Rn, tn, Xn, info = eng.ba_solve(R, t, X, cam, pt, uv, camera.K, fixed=fx, refine_points=refine_points, lambda0=lambda0, ftol=ftol,
                                    max_trials=max_trials)
    _, _, after = eng.ba_cost(Rn, tn, Xn, cam, pt, uv, camera.K)
    report = dict(info)
    for name, e2 in (("mean_error_before", before), ("mean_error_after", after)):
        front = e2[e2 >= 0.0]
        report[name] = float(np.sqrt(front).mean()) if front.size else float("nan")
    new_poses = {v: CameraPose(Rn[i], tn[i]) for i, v in enumerate(views)}
    new_points = {p: Xn[i].copy() for i, p in enumerate(ids)} if isinstance(points, dict) else Xn
    return new_poses, new_points, report
