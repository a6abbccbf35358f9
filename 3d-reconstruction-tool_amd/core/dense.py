"""Dense-SIFT reconstruction (the reference's src/core/dense.py, its `--dense` mode) with everything after the feature
extractor on the GPU: exact descriptor matching on the matrix cores, Lowe's ratio test, DLT triangulation with the depth,
parallax and reprojection filters, the 19-neighbour outlier statistic and the voxel grid anchored at the cloud's minimum
(include/amvs_match.h).

The extractor stays OpenCV's (CLAHE + SIFT): `reconstruct` needs cv2 for that and for nothing else.
`reconstruct_from_features` takes the features from the caller and needs no OpenCV.

The search is exact where the reference's FLANN index (trees=5, checks=100) is approximate, so the match set is not the
reference's; at equal descriptors it is the set FLANN approximates.  Parity with cv2 is unpinned.
"""
import time
from typing import Dict, List, Tuple

import numpy as np

from .camera import Camera, CameraPose
from ..engine import Engine

MIN_PARALLAX_DEG = 0.3
MAX_REPROJ_ERROR = 6.0
DEPTH_RANGE = (0.1, 50.0)
MIN_PAIR_MATCHES = 10
FILTER_MIN_POINTS = 100
FILTER_K = 20                 # the point itself and its 19 nearest neighbours
FILTER_STD_RATIO = 2.5
VOXELS_PER_DIAGONAL = 1200.0


def camera_pairs(n_cameras: int, window: int) -> List[Tuple[int, int]]:
    """Positions (i, j), i < j, in the sorted pose keys: nearby cameras and the loop closure."""
    return [(i, j) for i in range(n_cameras) for j in range(i + 1, n_cameras)
            if abs(i - j) <= window or abs(i - j) >= n_cameras - window]


def descriptors_u8(desc) -> np.ndarray:
    """(n, 128) uint8 from what an extractor returned: uint8, or float32 holding integers in 0 .. 255 (SIFT as OpenCV
    computes it).  Anything else is out of scope and raises."""
    d = np.asarray(desc)
    if d.ndim != 2 or d.shape[1] != 128:
        raise ValueError(f"descriptors must be (n, 128), got {d.shape}")
    if d.dtype == np.uint8:
        return np.ascontiguousarray(d)
    if d.dtype == np.float32:
        r = np.rint(d)
        if d.size == 0 or (np.array_equal(r, d) and d.min() >= 0.0 and d.max() <= 255.0):
            return np.ascontiguousarray(r.astype(np.uint8))
    raise ValueError("descriptors must be uint8, or float32 with integer values in 0 .. 255 (SIFT); RootSIFT and learned "
                     "(float) descriptors are out of scope of the exact integer matcher")


def keypoints_xy(feature) -> np.ndarray:
    """(n, 2) float32 pixel positions of a feature record: its 'points', or the .pt of its 'keypoints'."""
    if "points" in feature:
        return np.ascontiguousarray(feature["points"], dtype=np.float32).reshape(-1, 2)
    return np.float32([kp.pt for kp in feature["keypoints"]]).reshape(-1, 2)


class DenseReconstructor:
    """Dense point cloud from multi-view triangulation of all features (the reference's constructor and call surface)."""

    def __init__(self, camera: Camera, device: int = 0):
        self.camera = camera
        self.device_id = int(device)
        self.min_parallax = MIN_PARALLAX_DEG
        self.max_reproj_error = MAX_REPROJ_ERROR

    # -- the extractor on the device (include/amvs_features.h) --------------------------------------------------------------
    def device_extractor(self, engine=None):
        """A FeatureExtractor with the dense mode's values (the reference's: CLAHE 3.0 on 8 x 8, SIFT with 100000 features,
        contrast 0.01, edge 20, sigma 1.4), on `engine`, or on a context of its own that its close() ends."""
        from .features import FeatureExtractor
        return FeatureExtractor(n_features=100000, contrast_threshold=0.01, edge_threshold=20, sigma=1.4, clahe_clip=3.0,
                                clahe_grid=(8, 8), device=self.device_id, engine=engine)

    def extract_features(self, images: List[dict], poses: Dict[int, CameraPose], extractor="device") -> Dict[int, dict]:
        """The feature records reconstruct_from_features takes, of the posed views' "gray" images.  With "device" the
        extraction has one context, closed before this returns."""
        if isinstance(extractor, str) and extractor == "device":
            with Engine(8, 8, 1, np.eye(3, dtype=np.float32), device=self.device_id) as eng:
                return self.extract_features(images, poses, self.device_extractor(eng))
        features = {}
        for idx in sorted(poses.keys()):
            if idx < len(images):
                f = extractor.extract(images[idx]["gray"])
                if len(f) > 0:
                    features[idx] = {"points": f.points, "descriptors": f.descriptors}
        return features

    # -- the reference's entry point: extractor on the CPU (OpenCV) by default, the rest on the GPU -----------------------
    def reconstruct(self, images: List[dict], poses: Dict[int, CameraPose], window: int = 20,
                    extractor=None) -> Tuple[np.ndarray, np.ndarray]:
        """extractor=None: the reference's path, the extractor OpenCV's.  extractor="device" or a FeatureExtractor: CLAHE
        and SIFT on the device (include/amvs_features.h), nothing of OpenCV."""
        if extractor is not None:
            self._banner()
            features = self.extract_features(images, poses, extractor)
            print(f"  {sum(len(f['points']) for f in features.values()):,} keypoints found")
            return self._match_and_triangulate(features, images, poses, window, 0.85, False)
        try:
            import cv2 as cv
        except ImportError as e:
            raise ImportError("DenseReconstructor.reconstruct extracts its features with OpenCV (CLAHE + SIFT) and cv2 is "
                              "not importable; extract (n, 128) uint8 descriptors and keypoints yourself and call "
                              "reconstruct_from_features, which needs no OpenCV") from e
        self._banner()
        camera_indices = sorted(poses.keys())
        print(f"Extracting dense features from {len(camera_indices)} images...")
        t0 = time.time()
        extractor = cv.SIFT_create(nfeatures=100000, contrastThreshold=0.01, edgeThreshold=20, sigma=1.4)
        features = {}
        for idx in camera_indices:
            if idx >= len(images):
                continue
            clahe = cv.createCLAHE(clipLimit=3.0, tileGridSize=(8, 8))
            kp, desc = extractor.detectAndCompute(clahe.apply(images[idx]["gray"]), None)
            if desc is not None and len(kp) > 0:
                features[idx] = {"keypoints": kp, "descriptors": desc.astype(np.float32)}
        total_kp = sum(len(f["keypoints"]) for f in features.values())
        print(f"  {total_kp:,} keypoints found ({time.time()-t0:.1f}s)")
        return self._match_and_triangulate(features, images, poses, window, 0.85, False)

    @staticmethod
    def _banner():
        print("\n" + "=" * 60)
        print("DENSE RECONSTRUCTION (HIGH DENSITY MODE)")
        print("=" * 60)

    # -- everything after the extractor ---------------------------------------------------------------------------------------
    def reconstruct_from_features(self, features: Dict[int, dict], images: List[dict], poses: Dict[int, CameraPose],
                                  window: int = 20, ratio: float = 0.85, cross_check: bool = False,
                                  with_normals: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        if with_normals:
            raise ValueError("with_normals is not available in the dense-SIFT mode: the cloud's normals are fitted from depth "
                             "maps (amvs_cloud_normals) and this mode has none")
        self._banner()
        return self._match_and_triangulate(features, images, poses, window, ratio, cross_check)

    def _match_and_triangulate(self, features, images, poses, window, ratio, cross_check):
        camera_indices = sorted(poses.keys())
        n_cameras = len(camera_indices)
        feats = {}
        for idx in camera_indices:
            if idx in features and idx < len(images):
                d = descriptors_u8(features[idx]["descriptors"])
                xy = keypoints_xy(features[idx])
                if len(xy) != len(d):
                    raise ValueError(f"view {idx}: {len(d)} descriptors for {len(xy)} keypoints")
                if len(d) > 0:
                    feats[idx] = (d, xy)
        pairs = [(camera_indices[i], camera_indices[j]) for i, j in camera_pairs(n_cameras, window)]
        print(f"Matching {len(pairs)} camera pairs...")
        t0 = time.time()
        K = np.asarray(self.camera.K, np.float64).reshape(3, 3)
        cos_floor = float(np.cos(np.deg2rad(self.min_parallax)))
        with Engine(8, 8, 1, K.astype(np.float32), device=self.device_id) as eng:
            slot = {idx: s for s, idx in enumerate(feats)}
            for idx, (d, _) in feats.items():                       # one upload per image
                eng.set_descriptors(slot[idx], d)
            eng.pair_cloud_begin()
            mapped_points = 0
            for pair_idx, (idx1, idx2) in enumerate(pairs):
                if idx1 not in feats or idx2 not in feats:
                    continue
                if len(feats[idx1][0]) < 2 or len(feats[idx2][0]) < 2:
                    continue
                q_idx, t_idx, _ = eng.match_descriptors(slot[idx1], slot[idx2], ratio, cross_check)
                if len(q_idx) < MIN_PAIR_MATCHES:
                    continue
                pts1, pts2 = feats[idx1][1][q_idx], feats[idx2][1][t_idx]
                image = images[idx1]["image"]
                h, w = image.shape[:2]
                x_coords = np.clip(pts1[:, 0], 0, w - 1).astype(int)
                y_coords = np.clip(pts1[:, 1], 0, h - 1).astype(int)
                rgb = image[y_coords, x_coords][:, ::-1]            # BGR to RGB, of every candidate
                pose1, pose2 = poses[idx1], poses[idx2]
                mapped_points += eng.pair_triangulate(K, pose1.R, pose1.t, pose2.R, pose2.t, pts1, pts2, rgb,
                                                      DEPTH_RANGE[0], DEPTH_RANGE[1], cos_floor, self.max_reproj_error)
                if (pair_idx + 1) % 20 == 0:
                    print(f"  [{pair_idx+1}/{len(pairs)}] Total accumulated: {mapped_points:,} points")
            total = eng.pair_cloud_finish()
            if total == 0:
                print("No points generated.")
                return np.array([]), np.array([])
            print("Merging point clouds...")
            print(f"Raw points generated: {total:,}")
            total = self._filter_points_device(eng, total)
            points, colors = eng.fetch_cloud(total)
        print(f"Final filtered points: {len(points):,}")
        print(f"Dense reconstruction time: {time.time()-t0:.1f}s")
        return points, colors

    def _filter_points_device(self, eng, total):
        """The reference's _filter_points on the resident cloud: the neighbour statistic on the GPU, mean + 2.5 std and
        the mask in NumPy on the host, then the voxel grid anchored at the kept points' minimum.  Returns the new count."""
        if total < FILTER_MIN_POINTS:
            return total
        print("  Filtering outliers...")
        mean_dists = eng.cloud_knn_mean_distance(total, FILTER_K)
        mask = mean_dists < np.mean(mean_dists) + FILTER_STD_RATIO * np.std(mean_dists)
        kept = int(mask.sum())
        print(f"  Statistical filter: kept {kept} points")
        if kept == 0:
            eng.cloud_take(np.empty(0, np.int64))
            return 0
        min_pt, max_pt = eng.cloud_bounds(mask)
        voxel_size = np.linalg.norm(max_pt - min_pt) / VOXELS_PER_DIAGONAL
        if not voxel_size > 0.0:           # (every kept point is the same point)
            eng.cloud_take(np.nonzero(mask)[0][:1])
            return 1
        m = eng.cloud_voxel_downsample_grid(min_pt, voxel_size, mask)
        print(f"  Voxel grid: downsampled to {m} points")
        return m
