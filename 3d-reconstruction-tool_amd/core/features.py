"""Feature extraction and matching with geometric verification (the reference's src/core/features.py: FeatureExtractor,
ImageFeatures, FeatureMatch and FeatureMatcher) without OpenCV: CLAHE and SIFT as include/amvs_features.h defines them,
the exact descriptor search, Lowe's ratio test and the cross check of include/amvs_match.h, then the fundamental-matrix
RANSAC of include/amvs_epipolar.h, all on the GPU.

FeatureExtractor has the reference's constructor values; its SIFT is this library's own definition of Lowe's, the match
set is the exact one FLANN approximates, and the RANSAC is this library's own definition too, so parity with cv2 is
unpinned (DESIGN.md sections 12, 13 and 19)."""
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
class SiftFeatures(ImageFeatures):
    """What FeatureExtractor.extract returns: keypoints is the (n, 2) float32 array of positions, descriptors (n, 128) uint8."""
    sizes: np.ndarray = None
    angles: np.ndarray = None
    responses: np.ndarray = None
    octaves: np.ndarray = None


class FeatureExtractor:
    """CLAHE, then SIFT, on the device (include/amvs_features.h); the arguments and defaults are the reference's."""

    def __init__(self, n_features: int = 10000, contrast_threshold: float = 0.03, edge_threshold: float = 15, sigma: float = 1.6,
                 clahe_clip: float = 2.0, clahe_grid: Tuple[int, int] = (8, 8), device: int = 0, engine=None):
        self.n_features, self.contrast_threshold = int(n_features), float(contrast_threshold)
        self.edge_threshold, self.sigma = float(edge_threshold), float(sigma)
        self.clahe_clip, self.clahe_grid = float(clahe_clip), (int(clahe_grid[0]), int(clahe_grid[1]))
        if self.n_features < 0:
            raise ValueError("n_features must not be negative (0 keeps every keypoint)")
        if not (np.isfinite(self.contrast_threshold) and self.contrast_threshold >= 0):
            raise ValueError("contrast_threshold must be finite and not negative")
        if not (np.isfinite(self.edge_threshold) and self.edge_threshold > 0):
            raise ValueError("edge_threshold must be finite and positive")
        if not (np.isfinite(self.sigma) and self.sigma > 0):
            raise ValueError("sigma must be finite and positive")
        if not (np.isfinite(self.clahe_clip) and self.clahe_clip >= 0):
            raise ValueError("clahe_clip must be finite and not negative")
        if min(self.clahe_grid) < 1:
            raise ValueError("clahe_grid must be at least (1, 1)")
        self.device_id = int(device)
        self._engine, self._own_engine = engine, False

    def _eng(self):
        if self._engine is None:
            from ..engine import Engine
            self._engine, self._own_engine = Engine(8, 8, 1, np.eye(3, dtype=np.float32), device=self.device_id), True
        return self._engine

    def close(self):
        """Ends the context this extractor created for itself (one it was given stays open)."""
        if self._own_engine:
            self._engine.close()
            self._engine, self._own_engine = None, False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def gray(image) -> np.ndarray:
        """(h, w) uint8 from a BGR (h, w, 3) or gray (h, w) uint8 image, by the view preparation's rule."""
        img = np.asarray(image)
        if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3):
            raise ValueError("expected an (h, w, 3) BGR or (h, w) gray uint8 image")
        from ..engine import Engine
        if img.ndim == 2:
            return Engine._gray8(img)
        from .imageprep import _bgr_to_gray_u8
        return Engine._gray8(_bgr_to_gray_u8(img))             # (refuses a side above AMVS_FEATURES_MAX_SIDE)

    def extract(self, image) -> SiftFeatures:
        g = self.gray(image)
        kps, desc = self._eng().sift_extract(g, self.n_features, self.contrast_threshold, self.edge_threshold, self.sigma,
                                             clahe=(self.clahe_clip, self.clahe_grid))
        return SiftFeatures(np.ascontiguousarray(kps[:, :2]), desc, g.shape, sizes=kps[:, 2].copy(), angles=kps[:, 3].copy(),
                            responses=kps[:, 4].copy(), octaves=kps[:, 5].astype(np.int32))


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
