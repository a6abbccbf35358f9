"""The resident-view cache of the reconstructors: one device context (Engine) that holds every view of the
scene, kept across calls while the same prepared images, poses and intrinsics are in use.

PatchMatchMVS and DenseStereoReconstructor inherit it.  It reads `scale`, `K_scaled` and `device_id` of the
object it is mixed into (and, with `undistort`, its `camera`); `_engine_mode` is the one thing the two classes answer
differently.
"""
from typing import Dict, List, Optional

import numpy as np

from .camera import CameraPose
from .imageprep import prepare_views
from .. import engine as _engine


def _imageprep_has_cv2():
    from . import imageprep
    return imageprep._cv is not None


class ResidentViews:
    def __init__(self, device_prep: Optional[bool] = None, undistort: bool = False):
        # undistort: the images are the camera's own and obey camera.dist; every view is undistorted on the device at its
        # source resolution between the upload and the resize (include/amvs_lens.h, csrc/amvs_undistort.hip).  Off by
        # default, and then nothing changes.  There is one definition of the undistortion and it is the device's: the
        # host path is cv2's and the reference's dense classes never undistort, so device_prep=False is refused.
        self.undistort = bool(undistort)
        if self.undistort:
            if device_prep is not None and not device_prep:
                raise ValueError("undistort=True runs on the device: it cannot be combined with device_prep=False")
            device_prep = True
        # resize / gray conversion on the GPU (amvs_set_view_bgr8).  The device arithmetic restates
        # OpenCV's 8-bit algorithm and cannot be pinned against cv2 in the build container (DESIGN.md
        # section 2), so the default is the device path only where cv2 is NOT importable; where it is,
        # the host path calls cv2 itself and is the reference's by construction.
        self.device_prep = (not _imageprep_has_cv2()) if device_prep is None else bool(device_prep)
        self._engine = None
        self._engine_key = None
        self._engine_images = None       # strong reference to the prepared dict the engine holds
        self._resident_colors = False    # the engine holds the prepared colour images (device image prep)
        self._slot = {}

    def _engine_mode(self) -> str:
        """Arithmetic mode the engine is created in (a class that names the mode per call keeps "exact")."""
        return "exact"

    def _lens(self):
        """(K at the source resolution (3,3) float64, distortion coefficients) of the camera for the undistorting upload;
        raises ValueError for a distortion model the undistortion does not know."""
        return np.ascontiguousarray(self.camera.K, dtype=np.float64).reshape(3, 3), _engine.lens_coefficients(self.camera.dist)

    def _job_slots(self, jobs, js):
        """(engine slots of the reference views, of their source views) of the jobs jobs[j] = (ref, sources), j in js."""
        return [self._slot[jobs[j][0]] for j in js], [[self._slot[s] for s in jobs[j][1]] for j in js]

    def _prepare_images(self, images: List[dict], indices: List[int]) -> Dict:
        """Scaled colour + float32 gray in [0,1] per view (reference mvs_patchmatch.py:167-191; the Sobel
        gradients computed there are never read and are not produced here)."""
        prepared = prepare_views([images[idx]["image"] for idx in indices], self.scale)
        return dict(zip(indices, prepared))

    def _prepare_images_device(self, images: List[dict], indices: List[int], poses: Dict[int, CameraPose]) -> Dict:
        """_prepare_images on the GPU: every view's 8-bit BGR image is uploaded as it is (3 B/pixel) and
        resized / converted there (amvs_set_view_bgr8), which also leaves it resident for the sweep.
        Returns the prepared dict without host gray maps ('gray': None); the engine is cached for it."""
        h, w = images[indices[0]]["image"].shape[:2]
        H, W = int(h * self.scale), int(w * self.scale)
        lens = self._lens() if self.undistort else None
        # invalidate before the first upload into the engine, reused or new: an upload that fails part-way leaves no
        # key that a later _ensure_engine could match (the context may hold a mix of two scenes by then)
        self._engine_key = self._engine_images = None
        eng = self._engine
        if eng is None or not eng.reusable_for(H, W, len(indices), self.K_scaled, self.device_id, self._engine_mode()):
            if eng is not None:
                eng.close()
                self._engine = None
            eng = _engine.Engine(H, W, len(indices), self.K_scaled.astype(np.float32), device=self.device_id,
                                 mode=self._engine_mode())
        slot = {idx: s for s, idx in enumerate(indices)}
        prepared = {}
        for idx in indices:
            img = images[idx]["image"]
            if img.shape[:2] != (h, w):
                raise ValueError("all views must share one size")
            # the prepared colour image stays on the device for the fusion; the host copy the reference's
            # dict holds is the input itself at scale 1 and a (small) download otherwise
            same = (H, W) == (h, w)
            if lens is not None:                 # (the colour image is the undistorted one at every scale)
                color = eng.set_view_bgr8_undistorted(slot[idx], img, lens[0], lens[1], poses[idx].R, poses[idx].t)
                prepared[idx] = {"color": color, "gray": None, "shape": (H, W)}
                continue
            color = eng.set_view_bgr8(slot[idx], img, poses[idx].R, poses[idx].t, want_color=not same)
            prepared[idx] = {"color": img if same else color, "gray": None, "shape": (H, W)}
        self._engine, self._engine_images, self._resident_colors, self._slot = eng, prepared, True, slot
        self._engine_key = self._make_engine_key(prepared, poses, indices)
        return prepared

    def _make_engine_key(self, images: Dict, poses: Dict[int, CameraPose], indices: List[int]):
        H, W = images[indices[0]]["shape"]
        pose_print = b"".join(np.asarray(poses[i].R, np.float64).tobytes() + np.asarray(poses[i].t, np.float64).tobytes()
                              for i in indices)
        key = (tuple(indices), (int(H), int(W)), pose_print, self.K_scaled.tobytes(), self.device_id)
        if getattr(self, "undistort", False):    # the resident views also depend on the lens they were undistorted with
            K_src, dist = self._lens()
            key += (K_src.tobytes(), dist.tobytes())
        return key

    def _ensure_engine(self, images: Dict, poses: Dict[int, CameraPose], indices: Optional[List[int]] = None):
        """Upload every view once; cached while the same prepared-image dict, the same poses and
        the same intrinsics are in use.  The key holds a strong reference to the dict (an id() of a
        freed dict can be reused by CPython) and a fingerprint of every R|t, so a second call with
        refined poses re-uploads instead of sweeping with stale ones."""
        indices = sorted(images) if indices is None else indices
        H, W = images[indices[0]]["shape"]
        key = self._make_engine_key(images, poses, indices)
        if self._engine is not None and self._engine_images is images and self._engine_key == key:
            return self._engine
        self._engine_key = self._engine_images = None      # (as in _prepare_images_device)
        if self._engine is not None:
            self._engine.close()
            self._engine = None
        for idx in indices:
            if tuple(images[idx]["shape"]) != (H, W):
                raise ValueError("all views must share one processed size")
        eng = _engine.Engine(H, W, len(indices), self.K_scaled.astype(np.float32), device=self.device_id,
                             mode=self._engine_mode())
        slot = {idx: s for s, idx in enumerate(indices)}
        for idx in indices:
            eng.set_view(slot[idx], images[idx]["gray"], poses[idx].R, poses[idx].t)
        self._engine, self._engine_key, self._engine_images, self._slot = eng, key, images, slot
        self._resident_colors = False            # gray uploads: the colour images stay on the host
        return eng
