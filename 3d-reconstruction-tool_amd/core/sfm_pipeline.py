"""Incremental structure from motion: from the features of a set of views to their poses and a sparse cloud.

SfMPipeline stands where the reference's SfMPipeline does (src/core/sfm_pipeline.py) and is the caller the docstrings of
registration.py, geometry.py and bundle.py leave the bookkeeping to.  The numerical stages are the existing ones
(FeatureMatcher.match_pair_geometric, find_best_initial_pair, register_view, bundle_adjust, reprojection_errors); the
bookkeeping between them -- which keypoint observes which point, which view comes next, its 2-D / 3-D correspondences, the
new points of its matches, the observation list of a bundle adjustment -- is the track state resident in the engine's context
(include/amvs_sfm.h, Engine.sfm_*), so the loop below holds no per-match Python.

How it differs from the reference, on purpose: the rules of include/amvs_sfm.h (distinct keypoints in the score, conflicts
of correspondences resolved by match rank, keypoints named by index); one registration call, not three solvers
(registration.py); a bundle adjustment that moves cameras and points together (bundle.py) with the initial pair fixed,
followed by a filter of observations above MAX_ERROR_PX or behind their camera; no OpenCV anywhere but in reconstruct()."""
from typing import Dict, List, Optional, Tuple

import numpy as np

from .. import _lib
from .camera import CameraPose

MIN_MATCHES, MIN_BRIDGE_MATCHES = 15, 12          # the reference's match_image_pairs
MIN_SCORE = _lib.SFM_MIN_SCORE                    # find_next_image: a view needs 12 matched observed points
BA_EVERY = 5                                      # a bundle adjustment every 5 registered views
MAX_ERROR_PX = 4.0
MIN_OBS = _lib.SFM_MIN_OBS
TARGET_SCALE = 10.0                               # _normalize_reconstruction


def pair_schedule(n: int, window_size: int) -> List[Tuple[int, int]]:
    """The pairs the reference matches first: a sliding window, the loop closure between the first and last views, and the
    offsets 5 .. 30."""
    pairs = set()
    for i in range(n):
        for j in range(i + 1, min(i + window_size + 1, n)):
            pairs.add((i, j))
    loop = min(15, n // 3)
    for i in range(loop):
        for j in range(n - loop, n):
            if i < j:
                pairs.add((i, j))
    for i in range(n):
        for offset in (5, 10, 15, 20, 25, 30):
            if i + offset < n:
                pairs.add((i, i + offset))
    return sorted(pairs)


def components(pairs, n: int) -> List[List[int]]:
    adj = {}
    for i, j in pairs:
        adj.setdefault(i, set()).add(j)
        adj.setdefault(j, set()).add(i)
    seen, out = set(), []
    for start in range(n):
        if start in seen or start not in adj:
            continue
        comp, todo = set(), [start]
        while todo:
            node = todo.pop()
            if node not in comp:
                comp.add(node)
                todo.extend(adj[node] - comp)
        seen |= comp
        out.append(sorted(comp))
    return out


def bridge_pairs(comps: List[List[int]]) -> List[Tuple[int, int]]:
    """First, last and middle view of every two components, paired: what the reference tries when the graph falls apart."""
    comps = sorted(comps, key=len, reverse=True)
    out = set()
    for a, c1 in enumerate(comps):
        for c2 in comps[a + 1:]:
            s1 = [c1[0], c1[-1], c1[len(c1) // 2]] if len(c1) > 2 else c1
            s2 = [c2[0], c2[-1], c2[len(c2) // 2]] if len(c2) > 2 else c2
            out |= {(min(i, j), max(i, j)) for i in s1 for j in s2}
    return sorted(out)


class SfMPipeline:
    """Sparse reconstruction of a set of views with one camera.  fast_mode selects, as in the reference, the feature
    extractor's n_features (4000, else 8000) where this class extracts itself (reconstruct_images)."""

    def __init__(self, camera, fast_mode: bool = False, device: int = 0, engine=None):
        self.camera, self.fast_mode, self.device_id = camera, bool(fast_mode), int(device)
        self._engine = engine
        self.poses: Dict[int, CameraPose] = {}
        self.points = np.zeros((0, 3))
        self.colors = np.zeros((0, 3), np.uint8)
        self.failed: set = set()

    def _eng(self):
        if self._engine is None:
            from ..engine import Engine
            self._engine = Engine(8, 8, 1, np.eye(3, dtype=np.float32), device=self.device_id)
        return self._engine

    # ---- matching ------------------------------------------------------------------------------------------------------
    def match_image_pairs(self, features, window_size: int = 10) -> Dict[Tuple[int, int], np.ndarray]:
        """Verified matches (m, 2) int32 (keypoint of i, keypoint of j) of the reference's pair schedule; pairs with fewer
        than 15 stay out; when the graph falls apart, bridges between its components are tried with 12."""
        from .features import FeatureMatcher
        matcher = FeatureMatcher(device=self.device_id, engine=self._eng())
        n, matches = len(features), {}

        def try_pair(i, j, least):
            found, _ = matcher.match_pair_geometric(features[i], features[j], min_matches=least)
            if len(found) >= least:
                matches[(i, j)] = np.array([(m.idx1, m.idx2) for m in found], np.int32).reshape(-1, 2)

        for i, j in pair_schedule(n, window_size):
            try_pair(i, j, MIN_MATCHES)
        comps = components(matches, n)
        if len(comps) > 1:
            for i, j in bridge_pairs(comps):
                if (i, j) not in matches:
                    try_pair(i, j, MIN_BRIDGE_MATCHES)
        return matches

    # ---- reconstruction --------------------------------------------------------------------------------------------------
    def reconstruct_from_features(self, features, images=None, matches=None, record: Optional[dict] = None):
        """(points (n, 3), colors (n, 3) uint8, poses {view: CameraPose}) from one ImageFeatures (or (n_v, 2) pixel array) per
        view.  matches: verified matches {(i, j): (m, 2) keypoint indices} that bypass descriptor matching.  images: the
        views' BGR images, for the colours (else 127).  record: a dict that receives what crosses every boundary."""
        from .bundle import bundle_adjust, reprojection_errors
        from .geometry import find_best_initial_pair
        from .registration import register_view
        rec = record if record is not None else {}
        n = len(features)
        if n < 2:
            raise ValueError("Need at least 2 views")
        if n > _lib.BA_MAX_CAMERAS:
            raise ValueError(f"{n} views: the bundle adjustment takes at most {_lib.BA_MAX_CAMERAS} (include/amvs_bundle.h)")
        kps = [np.ascontiguousarray(f.points if hasattr(f, "points") else f, dtype=np.float32).reshape(-1, 2) for f in features]
        if matches is None:
            matches = self.match_image_pairs(features, window_size=min(12, n // 3 + 4))
        matches = {tuple(p): np.ascontiguousarray(m, dtype=np.int32).reshape(-1, 2) for p, m in sorted(matches.items())}
        if not matches:
            raise ValueError("No valid image pairs found")
        eng, K = self._eng(), np.asarray(self.camera.K, np.float64)
        pair_points = {p: (kps[p[0]][m[:, 0]], kps[p[1]][m[:, 1]]) for p, m in matches.items()}
        init = find_best_initial_pair(self.camera, pair_points, engine=eng)
        if init is None:
            raise ValueError("Could not find good initial pair")
        i0, j0 = init["pair"]
        rec.update({"aside": {}, "initial": {"pair": (i0, j0), "R": np.array(init["R"], np.float64), "t": np.ravel(init["t"]).astype(np.float64)},
                    "registered": [i0, j0], "steps": [], "bundles": []})

        eng.sfm_begin(kps, matches)
        poses = {i0: CameraPose(np.eye(3), np.zeros(3)), j0: CameraPose(init["R"], np.ravel(init["t"]))}
        for v in (i0, j0):
            eng.sfm_register(v, poses[v].R, np.ravel(poses[v].t))
        rec["first_points"] = eng.sfm_triangulate(j0, K)
        failed = set()

        def try_register(v, scores=None):
            kp, pid, X, x = eng.sfm_correspondences(v)
            step = {"view": v, "scores": scores, "keypoints": kp, "points": pid, "X": X, "x": x, "pose": None, "mask": None, "set": 0,
                    "new": None}
            rec["steps"].append(step)
            got = register_view(self.camera, X, x, engine=eng)
            if got is None:
                return False
            poses[v], step["mask"] = got
            step["pose"] = {"R": np.array(got[0].R, np.float64), "t": np.ravel(got[0].t).astype(np.float64)}
            step["set"] = eng.sfm_register(v, got[0].R, np.ravel(got[0].t), kp, pid, got[1])
            step["new"] = eng.sfm_triangulate(v, K)
            rec["registered"].append(v)
            return True

        def adjust(drop):
            cam, pt, uv = eng.sfm_observations()
            if len(cam) == 0:
                return
            X, alive = eng.sfm_points()
            ids = np.unique(pt)
            rows = np.column_stack([cam, pt, uv.astype(np.float64)])
            entry = {"rows": rows, "before": _state(poses, X, ids)}
            new_poses, new_points, entry["report"] = bundle_adjust(self.camera, poses, {int(p): X[p] for p in ids}, rows, fixed=[i0, j0],
                                                                   engine=eng)
            for p in ids:
                X[p] = new_points[int(p)]
            eng.sfm_set_points(X, alive)
            for v, pose in new_poses.items():
                poses[v] = pose
                eng.sfm_set_pose(v, pose.R, np.ravel(pose.t))
            entry["after"] = _state(poses, X, ids)
            if drop:
                err = reprojection_errors(self.camera, poses, new_points, rows, engine=eng)
                with np.errstate(invalid="ignore"):
                    bad = np.isnan(err) | (err > MAX_ERROR_PX)
                entry["errors"], entry["dropped"] = err, eng.sfm_drop(cam[bad], pt[bad], MIN_OBS)
            rec["bundles"].append(entry)

        def recover():
            back = [v for v in sorted(failed) if try_register(v)]
            failed.difference_update(back)
            return len(back)

        last_ba = 2
        while True:
            scores = eng.sfm_scores()
            open_views = [v for v in range(n) if scores[v] >= MIN_SCORE and v not in failed]
            if not open_views:
                if failed and recover() > 0:
                    continue
                break
            best = max(open_views, key=lambda v: (scores[v], -v))            # the best score, the lowest index on a tie
            if not try_register(best, scores):
                failed.add(best)
                continue
            if len(poses) >= last_ba + BA_EVERY:
                adjust(drop=True)
                last_ba = len(poses)
        adjust(drop=True)
        adjust(drop=False)
        if failed:
            recover()

        cam, pt, uv = eng.sfm_observations()
        X, alive = eng.sfm_points()
        ids = np.flatnonzero(alive)
        rec["final"] = {"observations": np.column_stack([cam, pt, uv.astype(np.float64)]).reshape(-1, 4), "points": X[ids], "ids": ids,
                        "failed": sorted(failed)}
        colors = np.full((len(ids), 3), 127, np.uint8)
        if images is not None and len(cam):
            first = np.unique(pt, return_index=True)[1]                      # (id, view) ascending: the first row of an id
            where = np.searchsorted(ids, pt[first])
            for row, at in zip(first, where):
                img = np.asarray(images[cam[row]])
                x, y = int(round(float(uv[row, 0]))), int(round(float(uv[row, 1])))
                if 0 <= y < img.shape[0] and 0 <= x < img.shape[1]:
                    colors[at] = img[y, x][::-1] if img.ndim == 3 else img[y, x]
        self.points, self.poses = normalize(X[ids], poses)
        self.colors, self.failed = colors, failed
        return self.points, self.colors, self.poses

    def _extractor(self, extractor):
        if extractor is None or (isinstance(extractor, str) and extractor == "device"):
            from .features import FeatureExtractor
            return FeatureExtractor(n_features=4000 if self.fast_mode else 8000, device=self.device_id, engine=self._eng())
        return extractor

    def reconstruct_images(self, images, max_images: Optional[int] = None, extractor=None):
        """reconstruct_from_features on the features a FeatureExtractor (default: the reference's values, on this
        pipeline's engine) extracts from `images`, BGR or gray uint8 arrays, already undistorted.  The points' colours are
        sampled from the same arrays (a gray value gives all three channels)."""
        images = list(images)[:max_images] if max_images else list(images)
        if len(images) < 2:
            raise ValueError("Need at least 2 images")
        ex = self._extractor(extractor)
        return self.reconstruct_from_features([ex.extract(im) for im in images], images=images)

    def _load_images(self, image_dir, max_images):
        """The folder's images as BGR uint8 arrays, through cv2 or PIL, whichever imports."""
        import os
        names = sorted(f for f in os.listdir(image_dir) if f.lower().endswith((".jpg", ".jpeg", ".png", ".tif", ".tiff", ".bmp")))
        names = names[:max_images] if max_images else names
        try:
            import cv2 as cv
            images = [cv.imread(os.path.join(image_dir, f)) for f in names]
        except ImportError:
            try:
                from PIL import Image
            except ImportError:
                raise RuntimeError("loading images needs OpenCV (cv2) or PIL, and neither is installed; load them yourself "
                                   "and call reconstruct_images") from None
            images = []
            for f in names:
                try:
                    images.append(np.ascontiguousarray(np.asarray(Image.open(os.path.join(image_dir, f)).convert("RGB"))[:, :, ::-1]))
                except OSError:
                    images.append(None)
        return [im for im in images if im is not None]

    def reconstruct(self, image_dir: str, max_images: Optional[int] = None, extractor=None):
        """The reference's reconstruct: the images of a folder, undistorted, SIFT features, then reconstruct_from_features.
        With extractor=None loading, undistortion and extraction are OpenCV's.  With extractor="device" or a
        FeatureExtractor the images are loaded through cv2 or PIL, undistorted and extracted on the device."""
        if extractor is not None:
            images = self._load_images(image_dir, max_images)
            if len(images) < 2:
                raise ValueError("Need at least 2 images")
            dist = getattr(self.camera, "dist", None)
            if dist is not None and np.any(np.asarray(dist) != 0):
                images = [self._eng().undistort_bgr8(im, np.asarray(self.camera.K, np.float64), dist)[0] for im in images]
            return self.reconstruct_images(images, extractor=extractor)
        try:
            import cv2 as cv
        except ImportError:
            raise RuntimeError("SfMPipeline.reconstruct loads images and extracts SIFT features with OpenCV (cv2), which is not "
                               "installed; extract the features yourself and call reconstruct_from_features") from None
        import os
        from .features import ImageFeatures
        names = sorted(f for f in os.listdir(image_dir) if f.lower().endswith((".jpg", ".jpeg", ".png", ".tif", ".tiff", ".bmp")))
        names = names[:max_images] if max_images else names
        images = [cv.imread(os.path.join(image_dir, f)) for f in names]
        images = [im for im in images if im is not None]
        if len(images) < 2:
            raise ValueError("Need at least 2 images")
        dist = getattr(self.camera, "dist", None)
        if dist is not None and np.any(np.asarray(dist) != 0):
            images = [cv.undistort(im, np.asarray(self.camera.K, np.float64), np.asarray(dist, np.float64)) for im in images]
        sift = cv.SIFT_create(nfeatures=4000 if self.fast_mode else 8000)
        features = []
        for im in images:
            kp, desc = sift.detectAndCompute(cv.cvtColor(im, cv.COLOR_BGR2GRAY), None)
            desc = np.zeros((0, 128), np.float32) if desc is None else desc
            features.append(ImageFeatures(np.array([k.pt for k in kp], np.float32).reshape(-1, 2), desc, im.shape[:2]))
        return self.reconstruct_from_features(features, images=images)

    def save_ply(self, output_path: str):
        from .utils import save_ply
        save_ply(self.points, self.colors, output_path)


def _state(poses, X, ids):
    return {"poses": {v: {"R": np.array(p.R, np.float64), "t": np.ravel(p.t).astype(np.float64)} for v, p in sorted(poses.items())},
            "points": {int(p): np.array(X[p], np.float64) for p in ids}}


def normalize(points: np.ndarray, poses: Dict[int, CameraPose]):
    """The reference's _normalize_reconstruction: the median of the points to the origin, their 90th percentile radius to 10."""
    if len(points) == 0:
        return points, dict(poses)
    centroid = np.median(points, axis=0)
    points = points - centroid
    scale = float(np.percentile(np.linalg.norm(points, axis=1), 90))
    factor = TARGET_SCALE / scale if scale > 0 else 1.0
    out = {}
    for v, pose in poses.items():
        R, t = np.asarray(pose.R, np.float64).reshape(3, 3), np.ravel(pose.t).astype(np.float64)
        C = -R.T @ t - centroid
        out[v] = CameraPose(R, (-R @ C) * factor)
    return points * factor, out
