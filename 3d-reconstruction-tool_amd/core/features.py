"""Feature matching with geometric verification (the reference's src/core/features.py: ImageFeatures, FeatureMatch and
FeatureMatcher) without OpenCV: the exact descriptor search, Lowe's ratio test and the cross check of
include/amvs_match.h, then the fundamental-matrix RANSAC of include/amvs_epipolar.h, all on the GPU.

The reference's FeatureExtractor (CLAHE + SIFT) is no part of this: features come from the caller.  The match set is the
exact one FLANN approximates, and the RANSAC is this library's own definition, so parity with cv2 is unpinned
(DESIGN.md sections 12 and 13)."""
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from .dense import descriptors_u8

RANSAC_THRESHOLD = 2.0        # the reference's cv.findFundamentalMat arguments
RANSAC_CONFIDENCE = 0.999


@dataclass
class ImageFeatures:
    """Features of one image: keypoints (objects with .pt, or an (n, 2) array of pixel positions) and descriptors."""
    keypoints: object
    descriptors: np.ndarray
    image_shape: Tuple[int, int]

    @property
    def points(self) -> np.ndarray:
        """(n, 2) float32 keypoint coordinates."""
        kps = self.keypoints
        if len(kps) and hasattr(kps[0], "pt"):
            return np.array([kp.pt for kp in kps], dtype=np.float32).reshape(-1, 2)
        return np.ascontiguousarray(kps, dtype=np.float32).reshape(-1, 2)

    def __len__(self):
        return len(self.keypoints)


@dataclass
class FeatureMatch:
    """Match between two images."""
    idx1: int
    idx2: int
    distance: float


class FeatureMatcher:
    """Lowe's ratio test on the exact nearest neighbours, the symmetric filter, and verification by a fundamental matrix."""

    def __init__(self, ratio_threshold: float = 0.8, device: int = 0, engine=None):
        self.ratio_threshold = float(ratio_threshold)
        self.device_id = int(device)
        self._engine = engine          # created on first use and kept, as the reconstructors keep theirs

    def _eng(self):
        if self._engine is None:
            from ..engine import Engine
            self._engine = Engine(8, 8, 1, np.eye(3, dtype=np.float32), device=self.device_id)
        return self._engine

    def match(self, features1: ImageFeatures, features2: ImageFeatures, cross_check: bool = True) -> List[FeatureMatch]:
        if len(features1.descriptors) < 2 or len(features2.descriptors) < 2:
            return []
        d1, d2 = descriptors_u8(features1.descriptors), descriptors_u8(features2.descriptors)
        eng = self._eng()
        eng.set_descriptors(0, d1)
        eng.set_descriptors(1, d2)
        qi, ti, s1 = eng.match_descriptors(0, 1, ratio=self.ratio_threshold, cross_check=cross_check)
        dist = np.sqrt(s1.astype(np.float64)).astype(np.float32)
        return [FeatureMatch(int(a), int(b), float(d)) for a, b, d in zip(qi, ti, dist)]

    def match_pair_geometric(self, features1: ImageFeatures, features2: ImageFeatures,
                             min_matches: int = 20) -> Tuple[List[FeatureMatch], Optional[np.ndarray]]:
        """(the matches a fundamental matrix verifies, that F) or ([], None): fewer than min_matches symmetric matches
        (or than the 8 a model needs), or no model."""
        raw = self.match(features1, features2, cross_check=True)
        if len(raw) < max(int(min_matches), 8):
            return [], None
        p1, p2 = features1.points, features2.points
        pts1 = p1[[m.idx1 for m in raw]]
        pts2 = p2[[m.idx2 for m in raw]]
        F, mask, _ = self._eng().fundamental_ransac(pts1, pts2, threshold=RANSAC_THRESHOLD, confidence=RANSAC_CONFIDENCE)
        if F is None:
            return [], None
        return [m for m, keep in zip(raw, mask) if keep], F
