"""Registration of a view against the cloud: its pose from 2D-3D correspondences by RANSAC on the device
(include/amvs_resection.h), and the polish of a pose it already has.

register_view is the numerical core of the reference's SfMPipeline.register_image (sfm_pipeline.py:512-633): where that
runs cv.solvePnPRansac three times with three solvers and keeps the best, this makes one call, because there is one
solver; the polish on the inliers is inside that call.  refine_pose is the per-camera step of its
bundle_adjustment_light (sfm_pipeline.py:694-776).  The bookkeeping of observations around both stays with the caller.
Lens distortion is not modelled: the views are undistorted before they are matched."""
from typing import Optional, Tuple

import numpy as np

from .camera import CameraPose

PNP_THRESHOLD = 8.0           # the reference's first and tightest solvePnPRansac call
PNP_CONFIDENCE = 0.99
PNP_MAX_HYPOTHESES = 5000
MIN_CORRESPONDENCES = 6       # what a hypothesis draws

_engines = {}                 # device -> Engine, created on first use and kept, as FeatureMatcher keeps its own


def _engine_for(engine, device):
    if engine is not None:
        return engine
    device = int(device)
    if device not in _engines:
        from ..engine import Engine
        _engines[device] = Engine(8, 8, 1, np.eye(3, dtype=np.float32), device=device)
    return _engines[device]


def _correspondences(points_3d, points_2d):
    p3 = np.asarray(points_3d, dtype=np.float32).reshape(-1, 3)
    p2 = np.asarray(points_2d, dtype=np.float32).reshape(-1, 2)
    if len(p3) != len(p2):
        raise ValueError("points_3d and points_2d must have one row per correspondence")
    return p3, p2


def register_view(camera, points_3d, points_2d, *, threshold: float = PNP_THRESHOLD, min_inliers: int = MIN_CORRESPONDENCES,
                  engine=None, device: int = 0) -> Optional[Tuple[CameraPose, np.ndarray]]:
    """(pose, inlier mask (m,) bool) of the view that sees points_3d (m, 3) at the pixels points_2d (m, 2), or None: fewer
    than 6 correspondences, no model, or fewer than min_inliers inliers."""
    p3, p2 = _correspondences(points_3d, points_2d)
    if len(p3) < MIN_CORRESPONDENCES:
        return None
    R, t, mask, info = _engine_for(engine, device).pnp_ransac(p3, p2, camera.K, threshold=float(threshold), confidence=PNP_CONFIDENCE,
                                                             max_hypotheses=PNP_MAX_HYPOTHESES)
    if R is None or int(np.count_nonzero(mask)) < max(int(min_inliers), MIN_CORRESPONDENCES):
        return None
    return CameraPose(R, t), mask


def refine_pose(camera, pose, points_3d, points_2d, mask=None, *, engine=None, device: int = 0) -> CameraPose:
    """The pose polished on the reprojection error of the correspondences of `mask` (None: all of them; at least 6)."""
    p3, p2 = _correspondences(points_3d, points_2d)
    R, t, _, _ = _engine_for(engine, device).pnp_refine(p3, p2, camera.K, pose.R, np.ravel(pose.t), mask)
    return CameraPose(R, t)
