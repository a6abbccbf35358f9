"""Engine: one device context holding every view of a scene (thin wrapper of the C ABI)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import AmvsError, PmParams, Timing, XpmParams, f32p, i32p


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def _p(a):
    return a.ctypes.data_as(f32p)


def _ids(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(i32p)


# Pointers into arrays: the array stays referenced by the caller (a local, or the tuple `keep` a helper returns)
# until the C call has returned.
def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _f64(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _r32(a, *shape):
    """float64 values rounded to a contiguous float32 array of `shape`."""
    return _f32(np.asarray(a, np.float64).astype(np.float32).reshape(shape))


def _pose32(R, t):
    return _r32(R, 3, 3), _r32(t, 3)


def _poses64(poses):
    """(n, 12) float64: R (row-major) | t of every (R, t)."""
    return np.ascontiguousarray(np.stack([np.concatenate([np.asarray(R, np.float64).reshape(9),
                                                          np.asarray(t, np.float64).reshape(3)]) for R, t in poses]))


def _kinv64(K_inv64):
    return np.ascontiguousarray(K_inv64, dtype=np.float64).reshape(9)


def lens_coefficients(dist):
    """The distortion coefficients as include/amvs_lens.h takes them: float64 k1, k2, p1, p2, k3, k4, k5, k6 with the
    trailing zeros trimmed to 8, 5 or 4 entries.  The model ends at the rational one: a non-zero coefficient beyond the
    eighth (thin prism s1 .. s4, tilt tau_x, tau_y) is refused, not ignored."""
    d = np.asarray(dist, np.float64).reshape(-1)
    if np.any(d[8:] != 0.0):
        raise ValueError("unsupported distortion model: thin-prism / tilt coefficients (beyond k6, the eighth) are "
                         "non-zero; the undistortion knows k1, k2, p1, p2, k3, k4, k5, k6")
    d = np.concatenate([d[:8], np.zeros(max(0, 8 - d.size))])
    n = 8 if np.any(d[5:] != 0.0) else (5 if d[4] != 0.0 else 4)
    return np.ascontiguousarray(d[:n])


def _lens(K, dist):
    return np.ascontiguousarray(K, dtype=np.float64).reshape(9), lens_coefficients(dist)


def _bgr8(image):
    img = np.ascontiguousarray(image, dtype=np.uint8)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("expected an (h, w, 3) uint8 BGR image")
    return img


def _job_ids(ref_ids, src_ids):
    """(n jobs, reference id pointer, source id pointer, sources per job, keep) of n reference views and their
    (n, S) source views; keep holds the two int32 arrays the pointers point into."""
    ref, refp = _ids(ref_ids)
    src, srcp = _ids(src_ids)
    n = ref.shape[0]
    return n, refp, srcp, src.reshape(n, -1).shape[1], (ref, src)


def make_pm_params(patch_size, num_iterations, num_samples, depth_min, depth_max, tile_rows=0,
                   views_per_launch=0, mode="default", schedule="auto", first_iteration=0, confidence=True):
    """amvs_pm_params with the log-range formed in double as mvs_patchmatch.py:268-271 does.
    mode: "default" (the engine's), "exact" or "fast" (include/amvs.h AMVS_MODE_*).
    first_iteration > 0 continues the previous call's sweep (include/amvs.h); confidence=False skips the
    confidence pass of this call."""
    log_min = np.log(float(depth_min))
    log_max = np.log(float(depth_max))
    return PmParams(int(patch_size), int(num_iterations), int(num_samples), int(tile_rows),
                    int(views_per_launch), float(depth_min), float(depth_max),
                    float(np.float32(log_max - log_min)), float(np.float32(log_min)), _lib.MODES[mode],
                    _lib.SCHEDULES[schedule], int(first_iteration), 0 if confidence else _lib.PM_NO_CONFIDENCE)


def make_xpm_params(patch_size, depth_min, depth_max, window_stride=2, num_refine=2, view_propagation=True,
                    consistency_px=1.0, consistency_rel=0.01):
    """amvs_xpm_params of the extended mode (include/amvs.h)."""
    log_min = np.log(float(depth_min))
    log_max = np.log(float(depth_max))
    return XpmParams(int(patch_size), int(window_stride), int(num_refine), int(bool(view_propagation)),
                     float(depth_min), float(depth_max), float(np.float32(log_max - log_min)), float(np.float32(log_min)),
                     float(consistency_px), float(consistency_rel))


class Engine:
    def __init__(self, H, W, n_views, K, K_inv=None, device=0, mode="exact"):
        self._lib = _lib.load()
        self.H, self.W, self.n_views, self.device = int(H), int(W), int(n_views), int(device)
        self.K = _f32(np.asarray(K, np.float32).reshape(3, 3))
        if K_inv is None:
            # float32 inverse, as torch.inverse(K) in mvs_patchmatch.py:237-238
            K_inv = np.linalg.inv(self.K)
        self.K_inv = _f32(np.asarray(K_inv, np.float32).reshape(3, 3))
        h = C.c_void_p()
        rc = self._lib.amvs_create(self.device, self.H, self.W, self.n_views, _p(self.K), _p(self.K_inv),
                                   C.byref(h))
        if rc != 0:
            raise AmvsError(f"amvs_create failed ({rc}): {self._lib.amvs_last_error(None).decode()}")
        self._h = h
        self._render_views = 0           # views of the last mesh_render: the image count mesh_color_views expects
        self._desc_rows = {}             # rows of every descriptor slot that was set: the sizes of knn2's outputs
        self._clahe_shape = None         # (h, w) of the context's resident CLAHE result
        self._sift_rows = None           # keypoints of the last sift_extract
        if mode != "exact":
            self.set_mode(mode)

    def reusable_for(self, H, W, n_views, K, device, mode="exact"):
        """True if this (open) context was created for exactly this problem: the classes then upload the next call's
        views into it instead of destroying and re-creating it (some twenty device buffers: 1.5 ms a call)."""
        return (self._h is not None and (self.H, self.W, self.n_views, self.device) == (int(H), int(W), int(n_views), int(device))
                and np.array_equal(self.K, np.asarray(K, np.float32).reshape(3, 3)) and self.mode() == mode)

    # -- arithmetic mode ------------------------------------------------------
    def set_mode(self, mode):
        """'exact' (bit-identical to the reference's float32 chain) or 'fast' (tolerance mode,
        8-bit images only): applies to every later sweep call of this engine."""
        self._chk(self._lib.amvs_set_mode(self._h, _lib.MODES[mode]))

    def mode(self):
        return {1: "exact", 2: "fast"}[int(self._lib.amvs_get_mode(self._h))]

    def set_sampling(self, force_f32):
        self._chk(self._lib.amvs_set_sampling(self._h, int(bool(force_f32))))

    def set_sweep_tuning(self, tile_rows=0, planes_per_wave=0):
        self._chk(self._lib.amvs_set_sweep_tuning(self._h, int(tile_rows), int(planes_per_wave)))

    def set_split_tuning(self, groups=0, sample_rows=0, sample_lds_bytes=0):
        """Split schedule (schedule="split"): view groups pipelined against each other, rows per strip
        of the sampling kernel, unused LDS bytes per sampling workgroup; 0 = automatic."""
        self._chk(self._lib.amvs_set_split_tuning(self._h, int(groups), int(sample_rows), int(sample_lds_bytes)))

    def set_step_tuning(self, tile_rows=None, wgs_per_cu=None):
        """Launch shape of the PatchMatch sweep steps by iteration: lists of (propagation, refinement)
        pairs, one per iteration (0 = automatic; later iterations repeat the last pair); both None
        clears the table.  Performance only."""
        n = max(len(tile_rows or []), len(wgs_per_cu or []))
        if n == 0:
            self._chk(self._lib.amvs_set_step_tuning(self._h, 0, None, None))
            return

        def table(t):
            t = list(t or [])
            t = t + [t[-1] if t else (0, 0)] * (n - len(t))
            return np.ascontiguousarray(np.asarray(t, dtype=np.int32).reshape(n, 2))
        r, w = table(tile_rows), table(wgs_per_cu)
        self._chk(self._lib.amvs_set_step_tuning(self._h, n, r.ctypes.data_as(i32p), w.ctypes.data_as(i32p)))

    def set_launch_order(self, edge_first=None, group_overlap=None):
        """Dispatch order of the sweep steps (include/amvs.h amvs_set_launch_order): edge_first -- every XCD walks
        each view's bands from the image edge to its centre; group_overlap -- 0 one stream, 1 / 2 the view groups on
        two streams of equal / high-low priority.  None = the library's default.  Performance only."""
        self._chk(self._lib.amvs_set_launch_order(self._h, -1 if edge_first is None else int(bool(edge_first)),
                                                  -1 if group_overlap is None else int(group_overlap)))

    def set_step_sources(self, ref_stats=None, centre_depth=None):
        """Inputs of the fast sweep step (include/amvs_step.h amvs_set_step_sources): ref_stats -- False the (mean1, var1)
        maps, True formed in the kernel; centre_depth -- False loaded again, True kept in registers from the sampling
        load.  None = the library's choice.  Performance only."""
        self._chk(self._lib.amvs_set_step_sources(self._h, -1 if ref_stats is None else int(bool(ref_stats)),
                                                  -1 if centre_depth is None else int(bool(centre_depth))))

    def step_sources(self, patch_size):
        """(ref_stats, centre_depth) as booleans: what a fast sweep step of this engine takes from registers at this
        patch size as the switch stands (amvs_get_step_sources)."""
        r, d = C.c_int(0), C.c_int(0)
        self._chk(self._lib.amvs_get_step_sources(self._h, int(patch_size), C.byref(r), C.byref(d)))
        return bool(r.value), bool(d.value)

    def step_trace(self):
        """(n_launches, blocks_per_launch, 4) uint64 workgroup timeline of the last PatchMatch call; needs a library
        built with -DAMVS_STEP_TRACE (None from the shipped build)."""
        nl, nb = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.amvs_fetch_step_trace(self._h, None, 0, C.byref(nl), C.byref(nb)))
        if nl.value == 0:
            return None
        out = np.zeros((nl.value, nb.value, 4), np.uint64)
        self._chk(self._lib.amvs_fetch_step_trace(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size,
                                                  C.byref(nl), C.byref(nb)))
        return out

    def set_step_timing(self, enable=True):
        self._chk(self._lib.amvs_set_step_timing(self._h, int(bool(enable))))

    def step_times(self):
        """Device time (ms) of every sweep launch of the last PatchMatch call (set_step_timing)."""
        n = C.c_int(0)
        self._chk(self._lib.amvs_get_step_times(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.float32)
        self._chk(self._lib.amvs_get_step_times(self._h, _p(out), out.size, C.byref(n)))
        return out[: n.value]

    # -- native exchange (RCCL behind the C ABI; the classes use torch.distributed) ------------
    @staticmethod
    def comm_unique_id():
        """128-byte RCCL id (rank 0 creates it, the caller hands it to the other ranks)."""
        lib = _lib.load()
        buf = (C.c_uint8 * 128)()
        rc = lib.amvs_comm_unique_id(buf)
        if rc != 0:
            raise AmvsError(f"amvs_comm_unique_id failed ({rc}): {lib.amvs_last_error(None).decode()}")
        return bytes(buf)

    def comm_init(self, rank, world, unique_id):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._chk(self._lib.amvs_comm_init(self._h, int(rank), int(world), buf))

    def allgather_maps(self, local_ptr, full_ptr, floats_per_rank):
        """ncclAllGather of floats_per_rank float32 per rank, device pointers, on the engine's stream."""
        self._chk(self._lib.amvs_allgather_maps(self._h, C.c_void_p(local_ptr), C.c_void_p(full_ptr), int(floats_per_rank)))

    def comm_destroy(self):
        self._chk(self._lib.amvs_comm_destroy(self._h))

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.amvs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc):
        if rc != 0:
            raise AmvsError(f"amvs call failed ({rc}): {self._lib.amvs_last_error(self._h).decode()}")

    def sync(self):
        self._chk(self._lib.amvs_sync(self._h))

    def set_stream(self, stream_ptr):
        self._chk(self._lib.amvs_set_stream(self._h, C.c_void_p(stream_ptr or 0)))

    # -- scene -------------------------------------------------------------
    def set_view(self, view, gray, R, t):
        gray = _f32(gray, (self.H, self.W))
        R, t = _pose32(R, t)
        self._chk(self._lib.amvs_set_view(self._h, int(view), _p(gray), _p(R), _p(t)))

    def set_view_bgr8(self, view, image_bgr_u8, R, t, want_color=True):
        """Upload the 8-bit BGR image as it is and prepare it on the device (resize to the engine's
        H x W, BGR -> gray, /255: mvs_patchmatch.py:167-191).  Returns the resized colour image
        (H, W, 3) uint8, or None."""
        img = np.ascontiguousarray(image_bgr_u8, dtype=np.uint8)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("expected an (h, w, 3) uint8 BGR image")
        R, t = _pose32(R, t)
        out = np.empty((self.H, self.W, 3), np.uint8) if want_color else None
        self._chk(self._lib.amvs_set_view_bgr8(
            self._h, int(view), _u8(img), img.shape[0], img.shape[1], _p(R), _p(t), _u8(out) if want_color else None))
        return out

    # -- lens undistortion (include/amvs_lens.h) --
    def undistort_bgr8(self, image, K, dist):
        """(image undistorted at its own size (h, w, 3) uint8, number of pixels whose source lies outside the image and
        which are zero) of an 8-bit BGR image (include/amvs_lens.h amvs_undistort_bgr8): K (3,3) float64 of that image,
        dist as lens_coefficients takes it.  Touches no view."""
        img = _bgr8(image)
        K9, d = _lens(K, dist)
        out = np.empty_like(img)
        n_outside = C.c_int64(0)
        self._chk(self._lib.amvs_undistort_bgr8(self._h, _u8(img), img.shape[0], img.shape[1], _f64(K9), _f64(d), d.size,
                                                _u8(out), C.byref(n_outside)))
        return out, int(n_outside.value)

    def set_view_bgr8_undistorted(self, view, image, K_src, dist, R, t, want_color=True):
        """set_view_bgr8 with the lens undistortion on the device between the upload and the resize (include/amvs_lens.h
        amvs_set_view_bgr8_undistorted): K_src (3,3) float64 is the calibration's matrix at the image's own resolution,
        not the engine's scaled K."""
        img = _bgr8(image)
        K9, d = _lens(K_src, dist)
        R, t = _pose32(R, t)
        out = np.empty((self.H, self.W, 3), np.uint8) if want_color else None
        self._chk(self._lib.amvs_set_view_bgr8_undistorted(
            self._h, int(view), _u8(img), img.shape[0], img.shape[1], _f64(K9), _f64(d), d.size, _p(R), _p(t),
            _u8(out) if want_color else None))
        return out

    # -- CLAHE and SIFT (include/amvs_features.h) --
    @staticmethod
    def _gray8(gray):
        g = np.ascontiguousarray(gray)
        if g.dtype != np.uint8 or g.ndim != 2:
            raise ValueError("expected an (h, w) uint8 gray image")
        if max(g.shape) > _lib.FEATURES_MAX_SIDE:
            raise ValueError(f"image side above {_lib.FEATURES_MAX_SIDE} (AMVS_FEATURES_MAX_SIDE)")
        return g

    def clahe(self, gray, clip_limit=2.0, grid=(8, 8)):
        """The (h, w) uint8 gray image after CLAHE with `grid` = (tiles across, tiles down) (amvs_clahe_u8).  The result
        also stays resident for sift_scale_space(None).  Touches no view."""
        g = self._gray8(gray)
        out = np.empty_like(g)
        self._clahe_shape = None         # (a call that fails leaves none resident)
        self._chk(self._lib.amvs_clahe_u8(self._h, _u8(g), g.shape[0], g.shape[1], float(np.float32(clip_limit)),
                                          int(grid[0]), int(grid[1]), _u8(out)))
        self._clahe_shape = g.shape
        return out

    def sift_scale_space(self, gray, sigma=1.6):
        """Builds the Gaussian / difference-of-Gaussian scale space of a (h, w) uint8 gray image, or with gray=None of the
        resident result of the last clahe(), and keeps it resident (amvs_sift_scale_space).  Returns the list of the
        octaves' (rows, columns); octave 0 has twice the image's size."""
        if gray is None:
            if self._clahe_shape is None:
                raise ValueError("sift_scale_space(None) needs a clahe() before it")
            g, (h, w) = None, self._clahe_shape
        else:
            g = self._gray8(gray)
            h, w = g.shape
        n = C.c_int32(0)
        self._sift_rows = None           # (the library drops the resident keypoints with their scale space)
        self._chk(self._lib.amvs_sift_scale_space(self._h, None if g is None else _u8(g), h, w, float(sigma), C.byref(n)))
        shapes = [(2 * h, 2 * w)]
        for _ in range(1, n.value):
            shapes.append((shapes[-1][0] // 2, shapes[-1][1] // 2))
        return shapes

    def sift_extract(self, gray, n_features=0, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6, clahe=None):
        """SIFT keypoints and descriptors of a (h, w) uint8 gray image (amvs_sift_extract, amvs_sift_fetch): (keypoints
        (n, 6) float32 with the columns x, y, size, angle in degrees, response, packed octave + 256 * layer; descriptors
        (n, 128) uint8), in the canonical order, the n_features strongest (0: all).  clahe=(clip_limit, (tiles across,
        tiles down)) applies CLAHE first, on the device.  The descriptors stay resident for sift_to_slot."""
        g = self._gray8(gray)
        self._sift_rows = None
        if clahe is not None:
            self._clahe_shape = None
            self._chk(self._lib.amvs_clahe_u8(self._h, _u8(g), g.shape[0], g.shape[1], float(np.float32(clahe[0])),
                                              int(clahe[1][0]), int(clahe[1][1]), None))
            self._clahe_shape = g.shape
        n = C.c_int32(0)
        self._chk(self._lib.amvs_sift_extract(self._h, None if clahe is not None else _u8(g), g.shape[0], g.shape[1], int(n_features),
                                              float(np.float32(contrast_threshold)), float(np.float32(edge_threshold)),
                                              float(sigma), C.byref(n)))
        kps = np.empty((n.value, 6), np.float32)
        desc = np.empty((n.value, 128), np.uint8)
        self._chk(self._lib.amvs_sift_fetch(self._h, _p(kps), _u8(desc), n.value))
        self._sift_rows = n.value
        return kps, desc

    def sift_to_slot(self, slot):
        """The descriptors of the last sift_extract into descriptor slot `slot`, as set_descriptors of them would, without
        a visit to the host (amvs_sift_to_slot)."""
        if self._sift_rows is None:
            raise ValueError("sift_to_slot needs a sift_extract before it")
        self._chk(self._lib.amvs_sift_to_slot(self._h, int(slot)))
        self._desc_rows[int(slot)] = self._sift_rows

    def sift_level(self, octave, index, dog=False):
        """Gaussian image `index` (0 .. 5) or, with dog, difference image `index` (0 .. 4) of an octave of the resident
        scale space, float32 (amvs_sift_fetch_level)."""
        h, w = C.c_int32(0), C.c_int32(0)
        args = (self._h, int(octave), int(index), int(bool(dog)))
        self._chk(self._lib.amvs_sift_fetch_level(*args, None, C.byref(h), C.byref(w)))
        out = np.empty((h.value, w.value), np.float32)
        self._chk(self._lib.amvs_sift_fetch_level(*args, _p(out), None, None))
        return out

    def set_view_colors(self, view, image_bgr_u8):
        """Keep the (H, W, 3) uint8 BGR image of a view on the device for fuse_filter_views /
        stereo_backproject_views (views prepared with set_view_bgr8 have theirs already)."""
        img = np.ascontiguousarray(image_bgr_u8, dtype=np.uint8)
        if img.shape != (self.H, self.W, 3):
            raise ValueError(f"expected a ({self.H}, {self.W}, 3) uint8 BGR image")
        self._chk(self._lib.amvs_set_view_colors(self._h, int(view), _u8(img)))

    def set_view_device(self, view, gray_ptr, R, t):
        R, t = _pose32(R, t)
        self._chk(self._lib.amvs_set_view_device(self._h, int(view), C.c_void_p(gray_ptr), _p(R), _p(t)))

    # -- PatchMatch --------------------------------------------------------
    def patchmatch(self, ref_ids, src_ids, params, seed):
        """Returns depth (n,H,W), normal (n,H,W,3), confidence (n,H,W) as numpy arrays."""
        n, refp, srcp, n_src, keep = _job_ids(ref_ids, src_ids)
        depth = np.empty((n, self.H, self.W), np.float32)
        normal = np.empty((n, self.H, self.W, 3), np.float32)
        conf = np.empty((n, self.H, self.W), np.float32)
        self._chk(self._lib.amvs_patchmatch(self._h, n, refp, srcp, n_src, C.byref(params),
                                            int(seed), _p(depth), _p(normal), _p(conf)))
        return depth, normal, conf

    def patchmatch_device(self, ref_ids, src_ids, params, seed, depth_ptr, normal_ptr, conf_ptr):
        n, refp, srcp, n_src, keep = _job_ids(ref_ids, src_ids)
        self._chk(self._lib.amvs_patchmatch_device(self._h, n, refp, srcp, n_src, C.byref(params),
                                                   int(seed), C.c_void_p(depth_ptr),
                                                   C.c_void_p(normal_ptr), C.c_void_p(conf_ptr)))

    def timing(self):
        t = Timing()
        self._chk(self._lib.amvs_get_timing(self._h, C.byref(t)))
        return {"init_ms": t.init_ms, "sweep_ms": t.sweep_ms, "confidence_ms": t.confidence_ms,
                "sweep_launches": t.sweep_launches, "pixel_hypotheses": t.pixel_hypotheses}

    def sampling_mode(self):
        """'u8-pairs' when the packed 8-bit maps are sampled, 'f32' otherwise."""
        return "u8-pairs" if self._lib.amvs_sampling_mode(self._h) else "f32"

    def last_tile_rows(self):
        return int(self._lib.amvs_last_tile_rows(self._h))

    def last_views_per_launch(self):
        return int(self._lib.amvs_last_views_per_launch(self._h))

    # -- plane sweep -------------------------------------------------------
    def plane_sweep(self, ref, nbr_ids, depths, patch_size, thresh):
        nbr, nbrp = _ids(nbr_ids)
        depths = _r32(depths, -1)
        d = np.empty((self.H, self.W), np.float32)
        conf = np.empty((self.H, self.W), np.float32)
        self._chk(self._lib.amvs_plane_sweep(self._h, int(ref), nbrp, nbr.size, _p(depths), depths.size,
                                             int(patch_size), float(thresh), _p(d), _p(conf)))
        return d, conf

    def plane_sweep_device(self, ref_ids, nbr_ids, depths, patch_size, thresh, depth_ptr, conf_ptr):
        n, refp, nbrp, n_nbr, keep = _job_ids(ref_ids, nbr_ids)
        depths = _r32(depths, -1)
        self._chk(self._lib.amvs_plane_sweep_device(self._h, n, refp, nbrp, n_nbr, _p(depths),
                                                    depths.size, int(patch_size), float(thresh),
                                                    C.c_void_p(depth_ptr), C.c_void_p(conf_ptr)))

    def plane_sweep_batch(self, ref_ids, nbr_ids, depths, patch_size, thresh):
        """All reference views in one launch; the maps stay in the context (fetch_sweep_maps,
        stereo_backproject(resident=True))."""
        n, refp, nbrp, n_nbr, keep = _job_ids(ref_ids, nbr_ids)
        depths = _r32(depths, -1)
        self._chk(self._lib.amvs_plane_sweep_batch(self._h, n, refp, nbrp, n_nbr, _p(depths), depths.size,
                                                   int(patch_size), float(thresh)))
        return n

    def fetch_sweep_maps(self, first, count):
        d = np.empty((count, self.H, self.W), np.float32)
        c = np.empty((count, self.H, self.W), np.float32)
        self._chk(self._lib.amvs_fetch_sweep_maps(self._h, int(first), int(count), _p(d), _p(c)))
        return d, c

    # -- extended mode ----------------------------------------------------------
    def _xpm_call(self, fn, ref_ids, src_ids, params, extra, ptrs):
        n, refp, srcp, n_src, keep = _job_ids(ref_ids, src_ids)
        self._chk(fn(self._h, n, refp, srcp, n_src, C.byref(params), *extra, *[C.c_void_p(p) for p in ptrs]))

    def xpm_init(self, ref_ids, src_ids, params, seed, depth_ptr, normal_ptr, cost_ptr):
        self._xpm_call(self._lib.amvs_xpm_init, ref_ids, src_ids, params, (int(seed),), (depth_ptr, normal_ptr, cost_ptr))

    def xpm_iterate(self, ref_ids, src_ids, params, iteration, seed, depth_ptr, normal_ptr, cost_ptr,
                    snapshot_depth_ptr=0, snapshot_normal_ptr=0):
        """One iteration (view candidates, red and black half sweeps).  snapshot_*: device copies of the
        depth / normal maps the view candidates read (0 = the live maps); pass them when the views of one
        iteration are split over several calls."""
        self._xpm_call(self._lib.amvs_xpm_iterate, ref_ids, src_ids, params, (int(iteration), int(seed)),
                       (depth_ptr, normal_ptr, cost_ptr, snapshot_depth_ptr or None, snapshot_normal_ptr or None))

    XPM_PHASES = {"candidates": 0, "red": 1, "black": 2, "eval": 3}

    def xpm_step(self, ref_ids, src_ids, params, iteration, seed, phase, depth_ptr, normal_ptr, cost_ptr,
                 snapshot_depth_ptr=0, snapshot_normal_ptr=0, cost_out_ptr=0):
        """One phase of an iteration ("candidates", "red", "black") or the test hook "eval" (cost of the
        current planes into cost_out_ptr)."""
        self._xpm_call(self._lib.amvs_xpm_step, ref_ids, src_ids, params, (int(iteration), int(seed), self.XPM_PHASES[phase]),
                       (depth_ptr, normal_ptr, cost_ptr, snapshot_depth_ptr or None, snapshot_normal_ptr or None,
                        cost_out_ptr or None))

    def xpm_fetch_candidates(self, n_ref):
        d = np.empty((n_ref, self.H, self.W), np.float32)
        n = np.empty((n_ref, self.H, self.W, 3), np.float32)
        self._chk(self._lib.amvs_xpm_fetch_candidates(self._h, int(n_ref), _p(d), _p(n)))
        return d, n

    def xpm_consistency(self, ref_ids, src_ids, params, depth_ptr, normal_ptr, cost_ptr, conf_ptr):
        self._xpm_call(self._lib.amvs_xpm_consistency, ref_ids, src_ids, params, (),
                       (depth_ptr, normal_ptr, cost_ptr, conf_ptr))

    # -- stereo post-steps on the device --------------------------------------
    def stereo_backproject(self, colors_bgr, K_inv64, poses, min_confidence, depth=None, conf=None, fetch=False,
                           device_ptrs=None):
        """dense_stereo.py:407-437 for all views at once.  depth / conf None: the resident maps of the
        last plane_sweep_batch; device_ptrs=(depth_ptr, conf_ptr): maps in caller device memory, (n, H*W)
        float32 each.  Returns (per-view point counts, total); the cloud stays on the device
        (fetch=True additionally returns points, colours)."""
        cols = np.ascontiguousarray(colors_bgr, dtype=np.uint8)
        n = cols.shape[0]
        cols = cols.reshape(n, self.H, self.W, 3)
        kinv = _kinv64(K_inv64)
        pp = _poses64(poses)
        if device_ptrs is not None:
            dptr, cptr, where = C.c_void_p(device_ptrs[0]), C.c_void_p(device_ptrs[1]), 1
        elif depth is None:
            dptr, cptr, where = C.c_void_p(0), C.c_void_p(0), 2
        else:
            depth, conf = _f32(depth), _f32(conf)
            dptr, cptr, where = depth.ctypes.data_as(C.c_void_p), conf.ctypes.data_as(C.c_void_p), 0
        per = (C.c_int64 * n)()
        total = C.c_int64(0)
        self._chk(self._lib.amvs_stereo_backproject(
            self._h, n, dptr, cptr, where, _u8(cols), _f64(kinv), _f64(pp), float(min_confidence), per, C.byref(total)))
        counts = [int(x) for x in per]
        if not fetch:
            return counts, int(total.value)
        return (counts, int(total.value)) + self.fetch_cloud(int(total.value))

    def fetch_cloud(self, m):
        pts = np.empty((m, 3), np.float64)
        rgb = np.empty((m, 3), np.uint8)
        if m:
            self._chk(self._lib.amvs_fetch_cloud(self._h, _f64(pts), _u8(rgb)))
        return pts, rgb

    def cloud_knn_mean_distance(self, n_points, k=20):
        out = np.empty(int(n_points), np.float64)
        self._chk(self._lib.amvs_cloud_knn_mean_distance(self._h, int(k), _f64(out)))
        return out

    def cloud_voxel_downsample(self, voxel_size, keep_mask=None):
        """dense_stereo.py:475-492 on the resident cloud (after the optional boolean keep mask);
        returns the new point count."""
        cnt = C.c_int64(0)
        km = None if keep_mask is None else np.ascontiguousarray(keep_mask, dtype=np.uint8)
        self._chk(self._lib.amvs_cloud_voxel_downsample(self._h, None if km is None else _u8(km), float(voxel_size),
                                                        C.byref(cnt)))
        return int(cnt.value)

    def cloud_take(self, indices):
        """The resident cloud <- its rows `indices` in that order (points[chosen], dense_stereo.py:449-455)."""
        idx = np.ascontiguousarray(indices, dtype=np.int64)
        self._chk(self._lib.amvs_cloud_take(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), idx.size))
        return int(idx.size)

    def knn_supported(self, k):
        return bool(self._lib.amvs_knn_supported(int(k)))

    # -- normals from the depth maps (include/amvs.h amvs_depth_normals ...) --
    def _normal_maps(self, poses, depth, conf, device_ptrs):
        """(n maps, depth pointer, confidence pointer, maps_where, poses array, keep) of the three ways the maps reach
        amvs_depth_normals / amvs_cloud_normals: host arrays (n,H,W), device_ptrs=(depth_ptr, conf_ptr), or neither --
        the resident maps of the last plane_sweep_batch."""
        pp = _poses64(poses)
        n = pp.shape[0]
        if device_ptrs is not None:
            return n, C.c_void_p(device_ptrs[0]), C.c_void_p(device_ptrs[1]), 1, pp, None
        if depth is None:
            return n, C.c_void_p(0), C.c_void_p(0), 2, pp, None
        depth, conf = _f32(depth, (n, self.H, self.W)), _f32(conf, (n, self.H, self.W))
        return n, depth.ctypes.data_as(C.c_void_p), conf.ctypes.data_as(C.c_void_p), 0, pp, (depth, conf)

    def depth_normals(self, K, poses, min_confidence, radius=2, jump=0.05, min_points=3, world=False, depth=None, conf=None,
                      device_ptrs=None, fetch=True):
        """Per-view normal maps fitted to the inverse depths (include/amvs.h amvs_depth_normals): K (3,3) float64, poses =
        list of (R, t) float64, maps as _normal_maps takes them.  Returns (normals (n,H,W,3) float32 -- zero where a pixel
        has none --, pixels with a normal), or the count alone with fetch=False (the maps stay on the device)."""
        n, dptr, cptr, where, pp, keep = self._normal_maps(poses, depth, conf, device_ptrs)
        Kd = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        cnt = C.c_int64(0)
        self._chk(self._lib.amvs_depth_normals(self._h, n, dptr, cptr, where, _f64(Kd), _f64(pp), float(min_confidence),
                                               int(radius), float(jump), int(min_points), int(bool(world)), C.byref(cnt)))
        if not fetch:
            return int(cnt.value)
        out = np.empty((n, self.H, self.W, 3), np.float32)
        self._chk(self._lib.amvs_fetch_depth_normals(self._h, 0, n, _p(out)))
        return out, int(cnt.value)

    def cloud_normals(self, K, poses, min_confidence, radius=2, jump=0.05, min_points=3, depth_tolerance=0.01, min_views=1,
                      depth=None, conf=None, device_ptrs=None):
        """Normals of the resident cloud from the views that see it (include/amvs.h amvs_cloud_normals).  Returns (pixels
        with a normal, points with a normal); fetch_cloud_normals copies the result."""
        n, dptr, cptr, where, pp, keep = self._normal_maps(poses, depth, conf, device_ptrs)
        Kd = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        counts = (C.c_int64 * 2)()
        self._chk(self._lib.amvs_cloud_normals(self._h, n, dptr, cptr, where, _f64(Kd), _f64(pp), float(min_confidence),
                                               int(radius), float(jump), int(min_points), float(depth_tolerance),
                                               int(min_views), counts))
        return int(counts[0]), int(counts[1])

    def fetch_cloud_normals(self, m):
        """(normals (m,3) float32, seen (m,) int32) of the m points of the resident cloud."""
        nrm = np.empty((m, 3), np.float32)
        seen = np.empty(m, np.int32)
        self._chk(self._lib.amvs_fetch_cloud_normals(self._h, _p(nrm), seen.ctypes.data_as(i32p)))
        return nrm, seen

    def cloud_set(self, points, colors=None):
        """Replace the resident cloud by host arrays (test hook; colours default to zero).  Returns the point count."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        m = len(pts)
        rgb = np.zeros((m, 3), np.uint8) if colors is None else np.ascontiguousarray(colors, dtype=np.uint8).reshape(m, 3)
        self._chk(self._lib.amvs_cloud_set(self._h, _f64(pts), _u8(rgb), m))
        return m

    # -- dense-SIFT mode (include/amvs_match.h): exact descriptor matching, pair triangulation, grid voxels --
    def set_descriptors(self, slot, descriptors):
        """One image's descriptors, (n, 128) uint8, into the resident slot `slot` (amvs_desc_set).  Returns n."""
        d = np.ascontiguousarray(descriptors)
        if d.dtype != np.uint8 or d.ndim != 2:
            raise ValueError("descriptors must be a 2-D uint8 array")
        self._chk(self._lib.amvs_desc_set(self._h, int(slot), _u8(d) if d.size else None, d.shape[0], d.shape[1]))
        self._desc_rows[int(slot)] = d.shape[0]
        return d.shape[0]

    def _slot_rows(self, slot):
        if int(slot) not in self._desc_rows:
            raise AmvsError(f"descriptor slot {slot} was never set")
        return self._desc_rows[int(slot)]

    def knn2(self, slot_q, slot_t):
        """(idx (n_q, 2) int32, dist2 (n_q, 2) int32): for every query row the two train rows smallest under (s, j), s the
        exact squared distance, j the train index (amvs_desc_knn2)."""
        n_q = self._slot_rows(slot_q)
        idx = np.empty((n_q, 2), np.int32)
        d2 = np.empty((n_q, 2), np.int32)
        self._chk(self._lib.amvs_desc_knn2(self._h, int(slot_q), int(slot_t), idx.ctypes.data_as(i32p), d2.ctypes.data_as(i32p)))
        return idx, d2

    def match_descriptors(self, slot_q, slot_t, ratio=0.85, cross_check=False):
        """(q_idx, t_idx, dist2), int32 each, in query order: the matches that pass Lowe's ratio test on the exact
        squared distances and, with cross_check, the symmetric filter (amvs_desc_match)."""
        n_q = self._slot_rows(slot_q)
        out = np.empty((3, max(n_q, 1)), np.int32)
        m = C.c_int64(0)
        self._chk(self._lib.amvs_desc_match(self._h, int(slot_q), int(slot_t), float(np.float32(ratio)), int(bool(cross_check)),
                                            out[0].ctypes.data_as(i32p), out[1].ctypes.data_as(i32p),
                                            out[2].ctypes.data_as(i32p), C.byref(m)))
        k = int(m.value)
        return out[0, :k].copy(), out[1, :k].copy(), out[2, :k].copy()

    def pair_cloud_begin(self):
        self._chk(self._lib.amvs_pair_cloud_begin(self._h))

    def pair_triangulate(self, K, R1, t1, R2, t2, pts1, pts2, rgb, depth_min=0.1, depth_max=50.0, cos_min_parallax=None,
                         max_reproj=6.0):
        """Triangulates the candidates (pts1, pts2: (m, 2) float32; rgb: (m, 3) uint8, the colour of every candidate) of
        one pair, appends the accepted ones to the accumulating cloud and returns their number (amvs_pair_triangulate).
        cos_min_parallax defaults to cos(0.3 degrees), the reference's floor."""
        if cos_min_parallax is None:
            cos_min_parallax = float(np.cos(np.deg2rad(0.3)))
        a = [np.ascontiguousarray(x, dtype=np.float64).reshape(n) for x, n in ((K, 9), (R1, 9), (t1, 3), (R2, 9), (t2, 3))]
        p1 = np.ascontiguousarray(pts1, dtype=np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(pts2, dtype=np.float32).reshape(-1, 2)
        m = len(p1)
        col = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1, 3)
        if len(p2) != m or len(col) != m:
            raise ValueError("pts1, pts2 and rgb must have one row per candidate")
        k = C.c_int64(0)
        self._chk(self._lib.amvs_pair_triangulate(self._h, *[_f64(x) for x in a], _p(p1) if m else None, _p(p2) if m else None,
                                                  _u8(col) if m else None, m, float(depth_min), float(depth_max),
                                                  float(cos_min_parallax), float(max_reproj), C.byref(k)))
        return int(k.value)

    def pair_cloud_finish(self):
        """The accumulated cloud becomes the resident cloud; returns its point count."""
        total = C.c_int64(0)
        self._chk(self._lib.amvs_pair_cloud_finish(self._h, C.byref(total)))
        return int(total.value)

    def cloud_bounds(self, keep_mask=None):
        """(min (3,), max (3,)) float64 of the resident cloud's kept points (amvs_cloud_bounds)."""
        km = None if keep_mask is None else np.ascontiguousarray(keep_mask, dtype=np.uint8)
        mn, mx = np.empty(3, np.float64), np.empty(3, np.float64)
        self._chk(self._lib.amvs_cloud_bounds(self._h, None if km is None else _u8(km), _f64(mn), _f64(mx)))
        return mn, mx

    def cloud_voxel_downsample_grid(self, origin, voxel_size, keep_mask=None):
        """The voxel de-duplication of the reference's dense mode on the resident cloud: voxels anchored at `origin`, the
        first point of every voxel in lexicographic voxel order (amvs_cloud_voxel_downsample_grid).  Returns the count."""
        km = None if keep_mask is None else np.ascontiguousarray(keep_mask, dtype=np.uint8)
        o = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        cnt = C.c_int64(0)
        self._chk(self._lib.amvs_cloud_voxel_downsample_grid(self._h, None if km is None else _u8(km), _f64(o), float(voxel_size),
                                                             C.byref(cnt)))
        return int(cnt.value)

    def selftest_sqrt(self, values):
        """sqrt of float64 values on the device (amvs_match_selftest_sqrt)."""
        v = np.ascontiguousarray(values, dtype=np.float64).ravel()
        out = np.empty_like(v)
        if v.size:
            self._chk(self._lib.amvs_match_selftest_sqrt(self._h, _f64(v), v.size, _f64(out)))
        return out

    # -- geometric verification (include/amvs_epipolar.h): fundamental-matrix RANSAC on the matches of two views --
    @staticmethod
    def _match_points(pts1, pts2):
        p1 = np.ascontiguousarray(pts1, dtype=np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(pts2, dtype=np.float32).reshape(-1, 2)
        if len(p1) != len(p2):
            raise ValueError("pts1 and pts2 must have one row per match")
        return p1, p2, len(p1)

    def fmat_hypotheses(self, pts1, pts2, seed=0, first=0, count=_lib.FMAT_BATCH):
        """(idx (count, 8) int32, F (count, 3, 3) float64): the samples of hypotheses first .. first + count - 1 in draw
        order and their 8-point fits, not forced to rank 2 (amvs_fmat_hypotheses)."""
        p1, p2, m = self._match_points(pts1, pts2)
        n = max(int(count), 1)
        idx = np.empty((n, 8), np.int32)
        F = np.empty((n, 3, 3), np.float64)
        self._chk(self._lib.amvs_fmat_hypotheses(self._h, _p(p1), _p(p2), m, int(seed) & (2 ** 64 - 1), int(first), int(count),
                                                 idx.ctypes.data_as(i32p), _f64(F)))
        return idx, F

    def fmat_score(self, F, pts1, pts2, threshold=2.0):
        """Inlier counts (n,) int32 of n fundamental matrices F (n, 3, 3) among the matches (amvs_fmat_score)."""
        p1, p2, m = self._match_points(pts1, pts2)
        Fs = np.ascontiguousarray(F, dtype=np.float64).reshape(-1, 9)
        counts = np.empty(max(len(Fs), 1), np.int32)
        self._chk(self._lib.amvs_fmat_score(self._h, _f64(Fs), len(Fs), _p(p1), _p(p2), m, float(threshold),
                                            counts.ctypes.data_as(i32p)))
        return counts[:len(Fs)]

    def fmat_inliers(self, F, pts1, pts2, threshold=2.0):
        """The inlier mask (m,) bool of one F (amvs_fmat_inliers)."""
        p1, p2, m = self._match_points(pts1, pts2)
        F9 = np.ascontiguousarray(F, dtype=np.float64).reshape(9)
        mask = np.zeros(max(m, 1), np.uint8)
        k = C.c_int64(0)
        self._chk(self._lib.amvs_fmat_inliers(self._h, _f64(F9), _p(p1), _p(p2), m, float(threshold), _u8(mask), C.byref(k)))
        return mask[:m].astype(bool)

    def fmat_fit(self, pts1, pts2, mask=None):
        """F (3, 3) float64 fitted to the matches of `mask` (None: all): normalised 8-point, rank 2, unit Frobenius norm, the
        entry of largest magnitude positive (amvs_fmat_fit)."""
        p1, p2, m = self._match_points(pts1, pts2)
        km = None if mask is None else np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
        if km is not None and len(km) != m:
            raise ValueError("mask must have one entry per match")
        F = np.empty((3, 3), np.float64)
        used = C.c_int64(0)
        self._chk(self._lib.amvs_fmat_fit(self._h, _p(p1), _p(p2), None if km is None else _u8(km), m, _f64(F), C.byref(used)))
        return F

    def fundamental_ransac(self, pts1, pts2, threshold=2.0, confidence=0.999, max_hypotheses=4096, seed=0):
        """(F (3, 3) float64 or None, mask (m,) bool, info): the fundamental matrix of the matches by RANSAC and its inliers
        (amvs_fmat_ransac).  info = {"hypotheses", "best_hypothesis", "best_count", "n_inliers"}; F is None when no
        hypothesis kept 8 matches or the refit kept fewer."""
        p1, p2, m = self._match_points(pts1, pts2)
        F = np.zeros((3, 3), np.float64)
        mask = np.zeros(max(m, 1), np.uint8)
        k = C.c_int64(0)
        info = np.zeros(3, np.int32)
        self._chk(self._lib.amvs_fmat_ransac(self._h, _p(p1), _p(p2), m, float(threshold), float(confidence), int(max_hypotheses),
                                             int(seed) & (2 ** 64 - 1), _f64(F), _u8(mask), C.byref(k), info.ctypes.data_as(i32p)))
        out = {"hypotheses": int(info[0]), "best_hypothesis": int(info[1]), "best_count": int(info[2]), "n_inliers": int(k.value)}
        return (F if k.value >= 8 else None), mask[:m].astype(bool), out

    # -- camera resection (include/amvs_resection.h): the pose of a view from 2D-3D correspondences by RANSAC --
    @staticmethod
    def _correspondences(points3d, points2d, K):
        p3 = np.ascontiguousarray(points3d, dtype=np.float32).reshape(-1, 3)
        p2 = np.ascontiguousarray(points2d, dtype=np.float32).reshape(-1, 2)
        if len(p3) != len(p2):
            raise ValueError("points3d and points2d must have one row per correspondence")
        return p3, p2, len(p3), np.ascontiguousarray(K, dtype=np.float64).reshape(9)

    @staticmethod
    def _poses(R, t):
        Rs = np.ascontiguousarray(R, dtype=np.float64).reshape(-1, 9)
        ts = np.ascontiguousarray(t, dtype=np.float64).reshape(-1, 3)
        if len(Rs) != len(ts):
            raise ValueError("R and t must hold one pose each per row")
        return Rs, ts

    def pnp_hypotheses(self, points3d, points2d, K, seed=0, first=0, count=_lib.PNP_BATCH):
        """(idx (count, 6) int32, R (count, 3, 3), t (count, 3) float64): the samples of hypotheses first .. first + count - 1
        in draw order and their poses, the 6-point DLT and the nearest rotation (amvs_pnp_hypotheses)."""
        p3, p2, m, Kd = self._correspondences(points3d, points2d, K)
        n = max(int(count), 1)
        idx = np.empty((n, 6), np.int32)
        R, t = np.empty((n, 3, 3), np.float64), np.empty((n, 3), np.float64)
        self._chk(self._lib.amvs_pnp_hypotheses(self._h, _p(p3), _p(p2), m, _f64(Kd), int(seed) & (2 ** 64 - 1), int(first),
                                                int(count), idx.ctypes.data_as(i32p), _f64(R), _f64(t)))
        return idx, R, t

    def pnp_score(self, R, t, points3d, points2d, K, threshold=8.0):
        """Inlier counts (n,) int32 of n poses R (n, 3, 3), t (n, 3) among the correspondences (amvs_pnp_score)."""
        p3, p2, m, Kd = self._correspondences(points3d, points2d, K)
        Rs, ts = self._poses(R, t)
        counts = np.empty(max(len(Rs), 1), np.int32)
        self._chk(self._lib.amvs_pnp_score(self._h, _f64(Rs), _f64(ts), len(Rs), _p(p3), _p(p2), m, _f64(Kd), float(threshold),
                                           counts.ctypes.data_as(i32p)))
        return counts[:len(Rs)]

    def pnp_inliers(self, R, t, points3d, points2d, K, threshold=8.0):
        """The inlier mask (m,) bool of one pose: reprojection error <= threshold and a positive depth (amvs_pnp_inliers)."""
        p3, p2, m, Kd = self._correspondences(points3d, points2d, K)
        R9 = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
        t3 = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        mask = np.zeros(max(m, 1), np.uint8)
        k = C.c_int64(0)
        self._chk(self._lib.amvs_pnp_inliers(self._h, _f64(R9), _f64(t3), _p(p3), _p(p2), m, _f64(Kd), float(threshold), _u8(mask),
                                             C.byref(k)))
        return mask[:m].astype(bool)

    def pnp_refine(self, points3d, points2d, K, R, t, mask=None):
        """(R (3, 3), t (3,), steps, cost): the pose polished by Gauss-Newton on the reprojection error of the correspondences
        of `mask` (None: all); cost is the sum of squared residuals in pixels (amvs_pnp_refine)."""
        p3, p2, m, Kd = self._correspondences(points3d, points2d, K)
        R9 = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
        t3 = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        km = None if mask is None else np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
        if km is not None and len(km) != m:
            raise ValueError("mask must have one entry per correspondence")
        Ro, to = np.empty((3, 3), np.float64), np.empty(3, np.float64)
        steps, cost, used = C.c_int32(0), C.c_double(0.0), C.c_int64(0)
        self._chk(self._lib.amvs_pnp_refine(self._h, _p(p3), _p(p2), m, _f64(Kd), _f64(R9), _f64(t3), None if km is None else _u8(km),
                                            _f64(Ro), _f64(to), C.byref(steps), C.byref(cost), C.byref(used)))
        return Ro, to, int(steps.value), float(cost.value)

    def pnp_ransac(self, points3d, points2d, K, threshold=8.0, confidence=0.99, max_hypotheses=5000, seed=0):
        """(R (3, 3) or None, t (3,) or None, mask (m,) bool, info): the pose of the view by RANSAC, polished on its inliers,
        and those inliers (amvs_pnp_ransac).  info = {"hypotheses", "best_hypothesis", "best_count", "n_inliers"}; R and t
        are None when no hypothesis kept 6 correspondences or the refit kept fewer."""
        p3, p2, m, Kd = self._correspondences(points3d, points2d, K)
        R, t = np.zeros((3, 3), np.float64), np.zeros(3, np.float64)
        mask = np.zeros(max(m, 1), np.uint8)
        k = C.c_int64(0)
        info = np.zeros(3, np.int32)
        self._chk(self._lib.amvs_pnp_ransac(self._h, _p(p3), _p(p2), m, _f64(Kd), float(threshold), float(confidence),
                                            int(max_hypotheses), int(seed) & (2 ** 64 - 1), _f64(R), _f64(t), _u8(mask), C.byref(k),
                                            info.ctypes.data_as(i32p)))
        out = {"hypotheses": int(info[0]), "best_hypothesis": int(info[1]), "best_count": int(info[2]), "n_inliers": int(k.value)}
        found = k.value >= 6
        return (R if found else None), (t if found else None), mask[:m].astype(bool), out

    # -- the first two views (include/amvs_twoview.h): the relative pose from F, triangulation with everything returned --
    @staticmethod
    def _intrinsics(K):
        return np.ascontiguousarray(K, dtype=np.float64).reshape(9)

    def twoview_decompose(self, F, K):
        """(R (2, 3, 3), t (3,), w (3,)) float64, or None when F has no model: the two rotations Ra, Rb and the unit
        translation of the four pose candidates (Ra, t) (Rb, t) (Ra, -t) (Rb, -t) of E = K^T F K, and the squared singular
        values of E in descending order (amvs_twoview_decompose; host arithmetic)."""
        F9 = np.ascontiguousarray(F, dtype=np.float64).reshape(9)
        R, t, w = np.empty((2, 3, 3), np.float64), np.empty(3, np.float64), np.empty(3, np.float64)
        ok = C.c_int32(0)
        self._chk(self._lib.amvs_twoview_decompose(self._h, _f64(F9), _f64(self._intrinsics(K)), _f64(R), _f64(t), _f64(w),
                                                   C.byref(ok)))
        return (R, t, w) if ok.value else None

    def twoview_score(self, R, t, pts1, pts2, K, max_depth=_lib.TWOVIEW_MAX_DEPTH):
        """Counts (n,) int32 of the matches that n poses R (n, 3, 3), t (n, 3) put in front of both cameras and nearer than
        max_depth (amvs_twoview_score)."""
        p1, p2, m = self._match_points(pts1, pts2)
        Rs, ts = self._poses(R, t)
        counts = np.empty(max(len(Rs), 1), np.int32)
        self._chk(self._lib.amvs_twoview_score(self._h, _f64(Rs), _f64(ts), len(Rs), _p(p1), _p(p2), m, _f64(self._intrinsics(K)),
                                               float(max_depth), counts.ctypes.data_as(i32p)))
        return counts[:len(Rs)]

    def twoview_front(self, R, t, pts1, pts2, K, max_depth=_lib.TWOVIEW_MAX_DEPTH):
        """The mask (m,) bool of the matches in front of both cameras under one pose (amvs_twoview_front)."""
        p1, p2, m = self._match_points(pts1, pts2)
        R9 = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
        t3 = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        mask = np.zeros(max(m, 1), np.uint8)
        k = C.c_int64(0)
        self._chk(self._lib.amvs_twoview_front(self._h, _f64(R9), _f64(t3), _p(p1), _p(p2), m, _f64(self._intrinsics(K)),
                                               float(max_depth), _u8(mask), C.byref(k)))
        return mask[:m].astype(bool)

    def twoview_pose(self, F, K, pts1, pts2, max_depth=_lib.TWOVIEW_MAX_DEPTH):
        """(R (3, 3) or None, t (3,) or None, mask (m,) bool, info): the relative pose of the second view from F by the
        cheirality vote over the four candidates, and the matches in front under it (amvs_twoview_pose; what
        cv.recoverPose does).  info = {"best", "counts" (4,), "n_front"}; R and t are None when F has no model or no
        candidate puts a match in front."""
        p1, p2, m = self._match_points(pts1, pts2)
        F9 = np.ascontiguousarray(F, dtype=np.float64).reshape(9)
        R, t = np.zeros((3, 3), np.float64), np.zeros(3, np.float64)
        mask = np.zeros(max(m, 1), np.uint8)
        k = C.c_int64(0)
        info = np.zeros(5, np.int32)
        self._chk(self._lib.amvs_twoview_pose(self._h, _f64(F9), _f64(self._intrinsics(K)), _p(p1), _p(p2), m, float(max_depth),
                                              _f64(R), _f64(t), _u8(mask), C.byref(k), info.ctypes.data_as(i32p)))
        out = {"best": int(info[0]), "counts": info[1:].copy(), "n_front": int(k.value)}
        found = k.value > 0
        return (R if found else None), (t if found else None), mask[:m].astype(bool), out

    def twoview_triangulate(self, K, R1, t1, R2, t2, pts1, pts2, depth_min=_lib.TWOVIEW_DEPTH_MIN, depth_max=None,
                            cos_max_parallax=None, max_reproj=_lib.TWOVIEW_MAX_REPROJ):
        """(X (m, 3) float64, valid (m,) bool, cos (m,) float64): every candidate's point, whether it passes the depth,
        parallax and reprojection tests, and the cosine of its parallax angle (amvs_twoview_triangulate).  depth_max
        defaults to 200 baselines and cos_max_parallax to cos(1 degree), the reference's."""
        a = [np.ascontiguousarray(x, dtype=np.float64).reshape(n) for x, n in ((K, 9), (R1, 9), (t1, 3), (R2, 9), (t2, 3))]
        p1, p2, m = self._match_points(pts1, pts2)
        if depth_max is None:
            c1, c2 = -(a[1].reshape(3, 3).T @ a[2]), -(a[3].reshape(3, 3).T @ a[4])
            depth_max = float(np.linalg.norm(c2 - c1)) * _lib.TWOVIEW_DEPTH_BASELINES
        if cos_max_parallax is None:
            cos_max_parallax = float(np.cos(np.deg2rad(_lib.TWOVIEW_MIN_PARALLAX_DEG)))
        X, valid, cs = np.empty((m, 3), np.float64), np.zeros(m, np.uint8), np.empty(m, np.float64)
        k = C.c_int64(0)
        self._chk(self._lib.amvs_twoview_triangulate(self._h, *[_f64(x) for x in a], _p(p1) if m else None, _p(p2) if m else None, m,
                                                     float(depth_min), float(depth_max), float(cos_max_parallax), float(max_reproj),
                                                     _f64(X) if m else None, _u8(valid) if m else None, _f64(cs) if m else None,
                                                     C.byref(k)))
        return X, valid.astype(bool), cs

    # -- bundle adjustment (include/amvs_bundle.h): poses and points refined together through the Schur complement --
    @staticmethod
    def _ba_problem(R, t, X, cam, pt, uv, K, fixed=None):
        """The arrays of a problem and the leading arguments of every amvs_ba_* call after the context."""
        Rs = np.ascontiguousarray(R, dtype=np.float64).reshape(-1, 9)
        ts = np.ascontiguousarray(t, dtype=np.float64).reshape(-1, 3)
        Xs = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
        cams, pts = np.ascontiguousarray(cam, dtype=np.int32).reshape(-1), np.ascontiguousarray(pt, dtype=np.int32).reshape(-1)
        uvs = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        if len(Rs) != len(ts):
            raise ValueError("R and t must hold one pose each per row")
        if not (len(cams) == len(pts) == len(uvs)):
            raise ValueError("cam, pt and uv must have one row per observation")
        Kd = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        fx = None if fixed is None else np.ascontiguousarray(np.asarray(fixed).reshape(-1) != 0, dtype=np.uint8)
        if fx is not None and len(fx) != len(Rs):
            raise ValueError("fixed must have one entry per camera")
        keep = (Rs, ts, Xs, cams, pts, uvs, Kd, fx)
        args = (_f64(Rs), _f64(ts), len(Rs), _f64(Xs), len(Xs), cams.ctypes.data_as(i32p), pts.ctypes.data_as(i32p), _p(uvs), len(cams),
                _f64(Kd))
        return keep, args, (None if fx is None else _u8(fx))

    def ba_cost(self, R, t, X, cam, pt, uv, K):
        """(cost, active, err2 (N,)): the sum of squared reprojection errors in pixels over the observations in front of
        their cameras, their number, and the squared error of each observation, -1.0 behind the camera (amvs_ba_cost)."""
        keep, args, _ = self._ba_problem(R, t, X, cam, pt, uv, K)
        cost, act, err2 = C.c_double(0.0), C.c_int64(0), np.empty(max(len(keep[3]), 1), np.float64)
        self._chk(self._lib.amvs_ba_cost(self._h, *args, C.byref(cost), C.byref(act), _f64(err2)))
        return float(cost.value), int(act.value), err2[:len(keep[3])]

    def ba_normal(self, R, t, X, cam, pt, uv, K, fixed=None):
        """(U (C, 21), gc (C, 6), V (P, 6), gp (P, 3), counts (P,) int32): the blocks of the normal equations, upper
        triangles row by row (amvs_ba_normal)."""
        keep, args, fx = self._ba_problem(R, t, X, cam, pt, uv, K, fixed)
        nc, npt = len(keep[0]), len(keep[2])
        U, gc = np.empty((max(nc, 1), 21), np.float64), np.empty((max(nc, 1), 6), np.float64)
        V, gp, cnt = np.empty((max(npt, 1), 6), np.float64), np.empty((max(npt, 1), 3), np.float64), np.empty(max(npt, 1), np.int32)
        self._chk(self._lib.amvs_ba_normal(self._h, *args, fx, _f64(U), _f64(gc), _f64(V), _f64(gp), cnt.ctypes.data_as(i32p)))
        return U[:nc], gc[:nc], V[:npt], gp[:npt], cnt[:npt]

    @staticmethod
    def _ba_free(n_cameras, fixed):
        return n_cameras - 1 if fixed is None else int(np.count_nonzero(np.asarray(fixed).reshape(-1) == 0))

    def ba_schur(self, R, t, X, cam, pt, uv, K, lam, fixed=None, refine_points=True):
        """(S (n, n), rhs (n,), slot (C,) int32, held (P,) bool): the reduced camera system under the damping lam, n = 6 x
        the number of free cameras; slot is -1 for a fixed camera (amvs_ba_schur)."""
        keep, args, fx = self._ba_problem(R, t, X, cam, pt, uv, K, fixed)
        nc, npt = len(keep[0]), len(keep[2])
        n = 6 * max(self._ba_free(nc, fixed), 0)
        S, rhs = np.empty((max(n, 1), max(n, 1)), np.float64), np.empty(max(n, 1), np.float64)
        slot, held = np.empty(max(nc, 1), np.int32), np.empty(max(npt, 1), np.uint8)
        self._chk(self._lib.amvs_ba_schur(self._h, *args, fx, int(bool(refine_points)), float(lam), _f64(S), _f64(rhs),
                                          slot.ctypes.data_as(i32p), _u8(held)))
        return S[:n, :n], rhs[:n], slot[:nc], held[:npt].astype(bool)

    def ba_step(self, R, t, X, cam, pt, uv, K, lam, fixed=None, refine_points=True):
        """(ok, dc (C, 6), dp (P, 3), R (C, 3, 3), t (C, 3), X (P, 3)): one Levenberg-Marquardt step under the damping lam
        and the candidate state; ok is False and everything zero when the reduced system has no Cholesky factor
        (amvs_ba_step)."""
        keep, args, fx = self._ba_problem(R, t, X, cam, pt, uv, K, fixed)
        nc, npt = max(len(keep[0]), 1), max(len(keep[2]), 1)
        ok = C.c_int32(0)
        dc, dp = np.empty((nc, 6), np.float64), np.empty((npt, 3), np.float64)
        Ro, to, Xo = np.empty((nc, 3, 3), np.float64), np.empty((nc, 3), np.float64), np.empty((npt, 3), np.float64)
        self._chk(self._lib.amvs_ba_step(self._h, *args, fx, int(bool(refine_points)), float(lam), C.byref(ok), _f64(dc), _f64(dp),
                                         _f64(Ro), _f64(to), _f64(Xo)))
        return bool(ok.value), dc, dp, Ro, to, Xo

    def ba_solve(self, R, t, X, cam, pt, uv, K, fixed=None, refine_points=True, lambda0=1e-3, ftol=1e-10, max_trials=50):
        """(R (C, 3, 3), t (C, 3), X (P, 3), info): the state after the Levenberg-Marquardt iteration (amvs_ba_solve).
        info = {"trials", "kept", "lambda", "first_cost", "cost", "active"}; the costs are sums of squared pixel errors."""
        keep, args, fx = self._ba_problem(R, t, X, cam, pt, uv, K, fixed)
        nc, npt = max(len(keep[0]), 1), max(len(keep[2]), 1)
        Ro, to, Xo = np.empty((nc, 3, 3), np.float64), np.empty((nc, 3), np.float64), np.empty((npt, 3), np.float64)
        info = np.zeros(6, np.float64)
        self._chk(self._lib.amvs_ba_solve(self._h, *args, fx, int(bool(refine_points)), float(lambda0), float(ftol), int(max_trials),
                                          _f64(Ro), _f64(to), _f64(Xo), _f64(info)))
        out = {"trials": int(info[0]), "kept": int(info[1]), "lambda": float(info[2]), "first_cost": float(info[3]),
               "cost": float(info[4]), "active": int(info[5])}
        return Ro, to, Xo, out

    # -- the track state of an incremental reconstruction (include/amvs_sfm.h), resident in the context --
    _sfm_views, _sfm_n_kp = 0, np.zeros(0, np.int32)       # until sfm_begin

    def sfm_begin(self, keypoints, pairs):
        """Uploads and resets the track state.  keypoints: one (n_v, 2) array of pixels per view; pairs: a dict or a list of
        ((i, j), rows) with i < j and rows (m, 2) int32 keypoint indices (k_i, k_j); the pairs are put in (i, j) order."""
        kps = [np.ascontiguousarray(k, dtype=np.float32).reshape(-1, 2) for k in keypoints]
        items = sorted(pairs.items() if isinstance(pairs, dict) else pairs, key=lambda it: tuple(it[0]))
        n_kp = np.array([len(k) for k in kps], np.int32)
        kp = np.ascontiguousarray(np.concatenate(kps) if kps else np.zeros((0, 2)), dtype=np.float32)
        rows = [np.ascontiguousarray(r, dtype=np.int32).reshape(-1, 2) for _, r in items]
        views = np.ascontiguousarray([tuple(p) for p, _ in items], dtype=np.int32).reshape(-1, 2)
        start = np.zeros(len(items) + 1, np.int32)
        start[1:] = np.cumsum([len(r) for r in rows])
        flat = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 2)), dtype=np.int32)
        self._chk(self._lib.amvs_sfm_begin(self._h, len(kps), n_kp.ctypes.data_as(i32p), _p(kp), len(items), views.ctypes.data_as(i32p),
                                           start.ctypes.data_as(i32p), flat.ctypes.data_as(i32p)))
        self._sfm_views, self._sfm_n_kp = len(kps), n_kp

    def sfm_register(self, view, R, t, kp=(), pid=(), mask=None):
        """Marks `view` registered with the pose (R, t) and lets its keypoints kp[i] observe the points pid[i] where mask[i]
        (None: everywhere); returns the number of owners set (dead points are skipped)."""
        Rd, td = np.ascontiguousarray(R, dtype=np.float64).reshape(9), np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        (k, kptr), (p, pptr) = _ids(np.asarray(kp).reshape(-1)), _ids(np.asarray(pid).reshape(-1))
        if len(k) != len(p):
            raise ValueError("kp and pid must have one entry per row")
        mk = None if mask is None else np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
        if mk is not None and len(mk) != len(k):
            raise ValueError("mask must have one entry per row")
        n = C.c_int64(0)
        self._chk(self._lib.amvs_sfm_register(self._h, int(view), _f64(Rd), _f64(td), kptr, pptr, None if mk is None else _u8(mk),
                                              len(k), C.byref(n)))
        return int(n.value)

    def sfm_scores(self):
        """(V,) int32: per unregistered view the number of its keypoints matched to an observed point, -1 for a registered
        view (amvs_sfm_scores)."""
        out = np.zeros(self._sfm_views, np.int32)
        self._chk(self._lib.amvs_sfm_scores(self._h, out.ctypes.data_as(i32p)))
        return out

    def sfm_correspondences(self, view):
        """(kp (m,) int32, pid (m,) int32, X (m, 3) float32, x (m, 2) float32) of an unregistered view, keypoints ascending
        (amvs_sfm_correspondences)."""
        n = max(int(self._sfm_n_kp[int(view)]), 1) if 0 <= int(view) < self._sfm_views else 1
        kp, pid = np.zeros(n, np.int32), np.zeros(n, np.int32)
        X, x = np.zeros((n, 3), np.float32), np.zeros((n, 2), np.float32)
        m = C.c_int64(0)
        self._chk(self._lib.amvs_sfm_correspondences(self._h, int(view), kp.ctypes.data_as(i32p), pid.ctypes.data_as(i32p), _p(X), _p(x),
                                                     C.byref(m)))
        m = int(m.value)
        return kp[:m].copy(), pid[:m].copy(), X[:m].copy(), x[:m].copy()

    def sfm_triangulate(self, view, K, depth_min=_lib.TWOVIEW_DEPTH_MIN, depth_baselines=_lib.TWOVIEW_DEPTH_BASELINES,
                        cos_max_parallax=None, max_reproj=_lib.TWOVIEW_MAX_REPROJ):
        """New points from the matches of a registered view with every other registered view; returns (n_new, new_per_view
        (V,) int32) (amvs_sfm_triangulate).  cos_max_parallax defaults to cos(1 degree), the reference's."""
        Kd = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        if cos_max_parallax is None:
            cos_max_parallax = float(np.cos(np.deg2rad(_lib.TWOVIEW_MIN_PARALLAX_DEG)))
        per = np.zeros(self._sfm_views, np.int32)
        n = C.c_int64(0)
        self._chk(self._lib.amvs_sfm_triangulate(self._h, int(view), _f64(Kd), float(depth_min), float(depth_baselines),
                                                 float(cos_max_parallax), float(max_reproj), C.byref(n), per.ctypes.data_as(i32p)))
        return int(n.value), per

    def sfm_counts(self):
        """(points made, points alive, observations) (amvs_sfm_counts)."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.amvs_sfm_counts(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def sfm_observations(self):
        """(cam (n,) int32, pt (n,) int32, uv (n, 2) float32): every observation of a live point, ascending in (pt, cam), the
        order bundle_adjust takes (amvs_sfm_observations)."""
        cap = max(self.sfm_counts()[2], 1)
        cam, pt, uv = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros((cap, 2), np.float32)
        n = C.c_int64(0)
        self._chk(self._lib.amvs_sfm_observations(self._h, cam.ctypes.data_as(i32p), pt.ctypes.data_as(i32p), _p(uv), cap, C.byref(n)))
        n = int(n.value)
        return cam[:n].copy(), pt[:n].copy(), uv[:n].copy()

    def sfm_points(self):
        """(X (n_points, 3) float64, alive (n_points,) bool), dead points included (amvs_sfm_points_get)."""
        n = self.sfm_counts()[0]
        X, alive = np.zeros((max(n, 1), 3), np.float64), np.zeros(max(n, 1), np.uint8)
        self._chk(self._lib.amvs_sfm_points_get(self._h, _f64(X), _u8(alive), max(n, 1)))
        return X[:n].copy(), alive[:n].astype(bool)

    def sfm_set_points(self, X, alive):
        """Replaces the points and their alive flags; a point may die, and its observations go with it (amvs_sfm_points_set)."""
        Xd = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
        al = np.ascontiguousarray(np.asarray(alive).reshape(-1) != 0, dtype=np.uint8)
        if len(al) != len(Xd):
            raise ValueError("X and alive must have one row per point")
        self._chk(self._lib.amvs_sfm_points_set(self._h, _f64(Xd), _u8(al), len(Xd)))

    def sfm_set_pose(self, view, R, t):
        """Replaces the pose of a registered view (amvs_sfm_pose_set)."""
        Rd, td = np.ascontiguousarray(R, dtype=np.float64).reshape(9), np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        self._chk(self._lib.amvs_sfm_pose_set(self._h, int(view), _f64(Rd), _f64(td)))

    def sfm_drop(self, cam, pt, min_obs=_lib.SFM_MIN_OBS):
        """Takes the observations (cam[i], pt[i]) away, then lets every live point with fewer than min_obs observations die;
        returns (observations dropped, points dropped) (amvs_sfm_drop)."""
        (c, cptr), (p, pptr) = _ids(np.asarray(cam).reshape(-1)), _ids(np.asarray(pt).reshape(-1))
        if len(c) != len(p):
            raise ValueError("cam and pt must have one entry per observation")
        a, b = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.amvs_sfm_drop(self._h, cptr, pptr, len(c), int(min_obs), C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    # -- cross-view depth-map filter (include/amvs_depth.h amvs_depth_filter) --
    def depth_filter(self, K, poses, min_confidence, max_px=1.0, max_rel=0.01, min_consistent=2, refine=True, neighbours=None,
                     depth=None, conf=None, device_ptrs=None, out_ptrs=None, in_place=False):
        """Consistent-view counts and fused depths of n depth maps (include/amvs_depth.h amvs_depth_filter): K (3,3) float64
        (K_inv is np.linalg.inv(K)), poses = list of (R, t) float64, maps as _normal_maps takes them.  neighbours: None --
        every other map in ascending index -- or (n, n_nbr) int32 map indices, -1 for none.  Returns (depth (n,H,W) float32,
        count (n,H,W) float32, (valid input pixels, pixels kept)); a pixel with fewer than min_consistent agreeing
        neighbours has depth 0, a kept one its input depth or, with refine, the mean of its own and the agreeing depths.
        With out_ptrs=(depth_ptr, count_ptr) -- device memory apart from the inputs -- or in_place=True -- the resident maps
        of the last plane_sweep_batch are replaced by (depth, count) -- the maps stay on the device and the counts alone
        are returned."""
        n, dptr, cptr, where, pp, keep = self._normal_maps(poses, depth, conf, device_ptrs)
        Kd = np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        Ki = np.ascontiguousarray(np.linalg.inv(Kd)).reshape(9)
        Kd = Kd.reshape(9)
        nbr, nbrp, n_nbr = None, None, 0
        if neighbours is not None:
            nbr = np.ascontiguousarray(neighbours, dtype=np.int32)
            if nbr.ndim != 2 or nbr.shape[0] != n:
                raise ValueError(f"expected neighbours of shape ({n}, n_nbr), got {nbr.shape}")
            nbrp, n_nbr = nbr.ctypes.data_as(i32p), nbr.shape[1]
        if in_place and out_ptrs is not None:
            raise ValueError("in_place and out_ptrs exclude each other")
        counts = (C.c_int64 * 2)()
        out = None
        if in_place:
            optr, kptr, out_where = C.c_void_p(0), C.c_void_p(0), 2
        elif out_ptrs is not None:
            optr, kptr, out_where = C.c_void_p(out_ptrs[0]), C.c_void_p(out_ptrs[1]), 1
        else:
            out = np.empty((2, n, self.H, self.W), np.float32)
            optr, kptr, out_where = out[0].ctypes.data_as(C.c_void_p), out[1].ctypes.data_as(C.c_void_p), 0
        self._chk(self._lib.amvs_depth_filter(self._h, n, dptr, cptr, where, _f64(Kd), _f64(Ki), _f64(pp), nbrp, n_nbr,
                                              float(min_confidence), float(max_px), float(max_rel), int(min_consistent),
                                              int(bool(refine)), optr, kptr, out_where, counts))
        totals = (int(counts[0]), int(counts[1]))
        return totals if out is None else (out[0], out[1], totals)

    # -- single steps (parity tests) ----------------------------------------
    def eval_cost(self, ref, src_ids, patch_size, depth):
        src, srcp = _ids(src_ids)
        depth = _f32(depth, (self.H, self.W))
        out = np.empty((self.H, self.W), np.float32)
        self._chk(self._lib.amvs_eval_cost(self._h, int(ref), srcp, src.size, int(patch_size), _p(depth), _p(out)))
        return out

    def sample_sources(self, ref, src_ids, patch_size, depth, bounds=0):
        """(sampled (S,H,W) float32, valid (S,H,W) bool) of the stage before the box filter; in
        fast mode the samples are in 8-bit code units (gray * 255)."""
        src, srcp = _ids(src_ids)
        depth = _f32(depth, (self.H, self.W))
        out = np.empty((src.size, self.H, self.W), np.float32)
        bits = np.empty((self.H, self.W), np.uint8)
        self._chk(self._lib.amvs_sample_sources(self._h, int(ref), srcp, src.size, int(patch_size), int(bounds),
                                                _p(depth), _p(out), _u8(bits)))
        valid = np.stack([(bits >> s) & 1 for s in range(src.size)]).astype(bool)
        return out, valid

    def confidence(self, ref, src_ids, patch_size, depth):
        src, srcp = _ids(src_ids)
        depth = _f32(depth, (self.H, self.W))
        out = np.empty((self.H, self.W), np.float32)
        self._chk(self._lib.amvs_confidence(self._h, int(ref), srcp, src.size, int(patch_size), _p(depth), _p(out)))
        return out

    def _state(self, depth, normal, cost):
        d = np.array(depth, np.float32, order="C", copy=True).reshape(self.H, self.W)
        n = np.array(normal, np.float32, order="C", copy=True).reshape(self.H, self.W, 3)
        c = np.array(cost, np.float32, order="C", copy=True).reshape(self.H, self.W)
        return d, n, c

    def propagate_step(self, ref, src_ids, patch_size, depth, normal, cost, oy, ox, depth_min):
        src, srcp = _ids(src_ids)
        d, n, c = self._state(depth, normal, cost)
        self._chk(self._lib.amvs_propagate_step(self._h, int(ref), srcp, src.size, int(patch_size),
                                                _p(d), _p(n), _p(c), int(oy), int(ox), float(depth_min)))
        return d, n, c

    def refine_step(self, ref, src_ids, patch_size, depth, normal, cost, seed, stream_view, draw,
                    depth_range, normal_range, depth_min, depth_max):
        src, srcp = _ids(src_ids)
        d, n, c = self._state(depth, normal, cost)
        self._chk(self._lib.amvs_refine_step(self._h, int(ref), srcp, src.size, int(patch_size),
                                             _p(d), _p(n), _p(c), int(seed), int(stream_view), int(draw),
                                             float(depth_range), float(normal_range),
                                             float(depth_min), float(depth_max)))
        return d, n, c

    def init_state(self, seed, stream_view, depth_min, depth_max):
        p = make_pm_params(7, 0, 0, depth_min, depth_max)
        d = np.empty((self.H, self.W), np.float32)
        n = np.empty((self.H, self.W, 3), np.float32)
        c = np.empty((self.H, self.W), np.float32)
        self._chk(self._lib.amvs_init_state(self._h, int(seed), int(stream_view), p.log_depth_scale,
                                            p.log_depth_min, _p(d), _p(n), _p(c)))
        return d, n, c

    def box_stats(self, view, patch_size):
        m = np.empty((self.H, self.W), np.float32)
        v = np.empty((self.H, self.W), np.float32)
        self._chk(self._lib.amvs_box_stats(self._h, int(view), int(patch_size), _p(m), _p(v)))
        return m, v

    # -- fusion / filter ----------------------------------------------------
    def fuse_filter(self, depth, conf, colors_bgr, K_inv64, poses, min_views, do_filter=True, device_ptrs=None):
        """Device fusion (+ filter): depth/conf (n,H,W) float32 host arrays -- or, with
        device_ptrs=(depth_ptr, conf_ptr, n), maps already resident on the GPU --, colors (n,H,W,3)
        uint8 BGR, poses = list of (R, t) float64.  Returns (points (M,3) float64, colors (M,3)
        uint8 RGB, raw_count)."""
        if device_ptrs is None:
            depth = _f32(depth)
            conf = _f32(conf)
            n = depth.shape[0]
            dptr, cptr, on_dev = depth.ctypes.data_as(C.c_void_p), conf.ctypes.data_as(C.c_void_p), 0
        else:
            dptr, cptr, n = C.c_void_p(device_ptrs[0]), C.c_void_p(device_ptrs[1]), int(device_ptrs[2])
            on_dev = 1
        cols = np.ascontiguousarray(colors_bgr, dtype=np.uint8).reshape(n, self.H, self.W, 3)
        kinv = _kinv64(K_inv64)
        pp = _poses64(poses)
        counts = (C.c_int64 * 2)()
        self._chk(self._lib.amvs_fuse_filter(self._h, n, dptr, cptr, on_dev, _u8(cols), _f64(kinv), _f64(pp),
                                             float(min_views), int(bool(do_filter)), counts))
        return self.fetch_cloud(int(counts[1])) + (int(counts[0]),)

    def stereo_backproject_views(self, view_ids, K_inv64, poses, min_confidence):
        """stereo_backproject for the resident maps of the last plane_sweep_batch with the colour images
        set_view_bgr8 left on the device (map j belongs to view view_ids[j]).  Returns (per-view point
        counts, total); the cloud stays on the device."""
        ids, idp = _ids(view_ids)
        n = ids.shape[0]
        kinv = _kinv64(K_inv64)
        pp = _poses64(poses)
        per = (C.c_int64 * n)()
        total = C.c_int64(0)
        self._chk(self._lib.amvs_stereo_backproject_views(
            self._h, n, idp, _f64(kinv), _f64(pp), float(min_confidence), per, C.byref(total)))
        return [int(x) for x in per], int(total.value)

    def fuse_filter_views(self, view_ids, depth_ptr, conf_ptr, K_inv64, poses, min_views, do_filter=True):
        """Device fusion (+ filter) of resident maps whose colour images are resident as well
        (set_view_bgr8): map j belongs to view view_ids[j].  Returns (points, colors RGB, raw_count)."""
        ids, idp = _ids(view_ids)
        n = ids.shape[0]
        kinv = _kinv64(K_inv64)
        pp = _poses64(poses)
        counts = (C.c_int64 * 2)()
        self._chk(self._lib.amvs_fuse_filter_views(
            self._h, n, idp, C.c_void_p(depth_ptr), C.c_void_p(conf_ptr), _f64(kinv), _f64(pp), float(min_views),
            int(bool(do_filter)), counts))
        return self.fetch_cloud(int(counts[1])) + (int(counts[0]),)

    # -- surface mesh (TSDF fusion + marching tetrahedra) -------------------
    def tsdf_integrate(self, K, poses, min_views, origin, voxel, dims, trunc, depth=None, conf=None, device_ptrs=None,
                       view_ids=None, colors_bgr=None):
        """Fuse depth maps into the context's TSDF volume (include/amvs.h amvs_tsdf_integrate).  Maps: depth / conf
        (n,H,W) float32 host arrays, or device_ptrs=(depth_ptr, conf_ptr, n) of maps resident on the GPU.  Colours:
        view_ids (map j takes the resident colour image of view view_ids[j]) or colors_bgr (n,H,W,3) uint8 BGR.
        K (3,3) and poses = list of (R, t) are used in float32; dims = (nx, ny, nz) grid points."""
        if device_ptrs is None:
            depth = _f32(depth)
            conf = _f32(conf)
            n = depth.shape[0]
            if depth.shape != (n, self.H, self.W) or conf.shape != depth.shape:
                raise ValueError(f"maps must be (n, {self.H}, {self.W})")
            dptr, cptr, on_dev = depth.ctypes.data_as(C.c_void_p), conf.ctypes.data_as(C.c_void_p), 0
        else:
            dptr, cptr, n = C.c_void_p(device_ptrs[0]), C.c_void_p(device_ptrs[1]), int(device_ptrs[2])
            on_dev = 1
        if len(poses) != n:
            raise ValueError(f"{len(poses)} poses for {n} maps")
        ids, idp, cols, colp = None, None, None, None
        if view_ids is not None:
            ids, idp = _ids(view_ids)
            if ids.shape != (n,):
                raise ValueError(f"{ids.shape[0]} view ids for {n} maps")
        if colors_bgr is not None:
            cols = np.ascontiguousarray(colors_bgr, dtype=np.uint8).reshape(n, self.H, self.W, 3)
            colp = _u8(cols)
        Kf = _r32(K, 9)
        pp = _r32(_poses64(poses), n, 12)
        org = _r32(origin, 3)
        dims = [int(d) for d in np.asarray(dims).reshape(3)]
        if any(d < 2 or d > 2 ** 31 - 1 for d in dims):
            raise ValueError(f"TSDF dims {dims}: every dimension must be in [2, 2^31)")
        dm, dmp = _ids(dims)
        self._chk(self._lib.amvs_tsdf_integrate(self._h, n, dptr, cptr, on_dev, idp, colp, _p(Kf), _p(pp),
                                                float(min_views), _p(org), float(np.float32(voxel)), dmp,
                                                float(np.float32(trunc))))
        self._tsdf_dims = tuple(int(d) for d in dm)

    def tsdf_extract(self):
        """Marching tetrahedra of the last integrated volume: (vertices (V,3) float32, faces (F,3) int32,
        colors (V,3) uint8 RGB)."""
        nv, nf = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.amvs_tsdf_extract(self._h, C.byref(nv), C.byref(nf)))
        self._mesh_counts = (nv.value, nf.value)
        return self.mesh_fetch()

    def tsdf_mesh(self, K, poses, min_views, origin, voxel, dims, trunc, **maps_and_colors):
        """tsdf_integrate(...) then tsdf_extract(): (vertices, faces, colors)."""
        self.tsdf_integrate(K, poses, min_views, origin, voxel, dims, trunc, **maps_and_colors)
        return self.tsdf_extract()

    def tsdf_volume(self):
        """The last integrated volume: tsdf (nz,ny,nx), weight (nz,ny,nx), colour sums (nz,ny,nx,3) RGB, float32."""
        dims = getattr(self, "_tsdf_dims", None)
        if dims is None:
            raise AmvsError("no TSDF volume: call tsdf_integrate first")
        nx, ny, nz = dims
        tsdf = np.empty((nz, ny, nx), np.float32)
        weight = np.empty((nz, ny, nx), np.float32)
        color = np.empty((nz, ny, nx, 3), np.float32)
        self._chk(self._lib.amvs_tsdf_fetch_volume(self._h, _p(tsdf), _p(weight), _p(color)))
        return tsdf, weight, color

    def tsdf_set_volume(self, tsdf, weight, color_sum, origin, voxel):
        """Test hook (include/amvs.h amvs_tsdf_set_volume): make host arrays in tsdf_volume()'s layout the context's
        volume -- tsdf, weight (nz,ny,nx) and colour sums (nz,ny,nx,3) RGB, float32 -- for tsdf_extract()."""
        tsdf = _f32(tsdf)
        if tsdf.ndim != 3:
            raise ValueError("tsdf must be (nz, ny, nx)")
        nz, ny, nx = tsdf.shape
        weight = _f32(weight)
        color = _f32(color_sum)
        if weight.shape != tsdf.shape or color.shape != tsdf.shape + (3,):
            raise ValueError(f"weight must be {tsdf.shape} and color_sum {tsdf.shape + (3,)}")
        org = _r32(origin, 3)
        dm, dmp = _ids([nx, ny, nz])
        self._chk(self._lib.amvs_tsdf_set_volume(self._h, _p(tsdf), _p(weight), _p(color), _p(org),
                                                 float(np.float32(voxel)), dmp))
        self._tsdf_dims = (nx, ny, nz)

    def tsdf_fill(self, steps, min_neighbours=1):
        """Hole filling in the current volume (include/amvs.h amvs_tsdf_fill): `steps` times (1 .. 64) every unobserved grid
        point with at least `min_neighbours` (1 .. 6) observed or already filled 6-neighbours becomes their mean, in signed
        distance and colour, with weight 1.  Drops the mesh: tsdf_extract() then meshes the filled volume.  Returns the
        number of points filled; the per-step counts are kept in last_fill_counts."""
        counts = np.zeros(max(int(steps), 1), np.int64)
        total = C.c_int64(0)
        self.last_fill_counts = None
        self._chk(self._lib.amvs_tsdf_fill(self._h, int(steps), int(min_neighbours), counts.ctypes.data_as(C.POINTER(C.c_int64)),
                                           C.byref(total)))
        self.last_fill_counts = [int(c) for c in counts]
        return total.value

    def tsdf_fill_generations(self):
        """Test hook (include/amvs.h amvs_tsdf_fetch_fill): the generations of the last tsdf_fill on the current volume,
        (nz,ny,nx) uint8 -- 0 still unobserved, 1 observed before the call, s + 1 filled by step s."""
        dims = getattr(self, "_tsdf_dims", None)
        if dims is None:
            raise AmvsError("no TSDF volume: call tsdf_integrate first")
        nx, ny, nz = dims
        gen = np.empty((nz, ny, nx), np.uint8)
        self._chk(self._lib.amvs_tsdf_fetch_fill(self._h, gen.ctypes.data_as(C.POINTER(C.c_uint8))))
        return gen

    # -- mesh clean-up (components, Taubin smoothing, decimation, normals), in place on the context's current mesh ----
    def mesh_set(self, vertices, faces, colors=None):
        """Make host arrays the context's mesh (include/amvs.h amvs_mesh_set): vertices (V,3) float32, faces (F,3)
        int32, colors (V,3) uint8 RGB or None for zeros.  Finite positions, ids in [0, V) and no face with a repeated
        id, else AmvsError."""
        verts = _f32(np.asarray(vertices).reshape(-1, 3))
        tris = np.ascontiguousarray(np.asarray(faces).reshape(-1, 3), dtype=np.int32)
        cols = None
        if colors is not None:
            cols = np.ascontiguousarray(np.asarray(colors).reshape(-1, 3), dtype=np.uint8)
            if len(cols) != len(verts):
                raise ValueError(f"colors must be ({len(verts)}, 3)")
        self._chk(self._lib.amvs_mesh_set(self._h, _p(verts), len(verts), tris.ctypes.data_as(i32p), len(tris),
                                          None if cols is None else _u8(cols)))
        self._mesh_counts = (len(verts), len(tris))

    def mesh_filter_components(self, min_faces=0, keep_largest=False):
        """Label the connected components and keep those with at least min_faces faces (keep_largest: only the one
        with the most faces).  Returns (components before the filter, vertices, faces after it)."""
        nc, nv, nf = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.amvs_mesh_filter_components(self._h, int(min_faces), int(bool(keep_largest)), C.byref(nc),
                                                        C.byref(nv), C.byref(nf)))
        self._mesh_counts = (nv.value, nf.value)
        return nc.value, nv.value, nf.value

    def mesh_smooth(self, iterations, lam=0.5, mu=-0.53, fix_boundary=True):
        """Taubin smoothing of the current mesh's positions (include/amvs.h amvs_mesh_smooth)."""
        self._chk(self._lib.amvs_mesh_smooth(self._h, int(iterations), float(lam), float(mu), int(bool(fix_boundary))))

    def mesh_normals(self):
        """Area-weighted vertex normals of the current mesh, fetched with mesh_fetch(normals=True)."""
        self._chk(self._lib.amvs_mesh_normals(self._h))

    def mesh_decimate(self, origin, cell):
        """Vertex clustering of the current mesh on the grid of cubic cells of side `cell` with a corner at `origin`
        (include/amvs.h amvs_mesh_decimate).  Returns (vertices, faces) after it; drops labels and normals."""
        org = _r32(origin, 3)
        nv, nf = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.amvs_mesh_decimate(self._h, _p(org), float(np.float32(cell)), C.byref(nv), C.byref(nf)))
        self._mesh_counts = (nv.value, nf.value)
        return nv.value, nf.value

    def mesh_decimate_quadric(self, origin, cell, regularisation=1e-3):
        """mesh_decimate with every cluster's vertex placed by its members' plane quadrics instead of at their mean
        (include/amvs.h amvs_mesh_decimate_quadric); faces, colours and counts are mesh_decimate's.  Returns (vertices,
        faces, clusters that kept the mean); drops labels and normals."""
        org = _r32(origin, 3)
        nv, nf, nk = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.amvs_mesh_decimate_quadric(self._h, _p(org), float(np.float32(cell)), float(np.float32(regularisation)),
                                                       C.byref(nv), C.byref(nf), C.byref(nk)))
        self._mesh_counts = (nv.value, nf.value)
        return nv.value, nf.value, nk.value

    def mesh_fetch(self, normals=False, labels=False):
        """The current mesh: (vertices (V,3) float32, faces (F,3) int32, colors (V,3) uint8[, normals (V,3) float32]
        [, labels (V,) int32])."""
        counts = getattr(self, "_mesh_counts", None)
        if counts is None:
            raise AmvsError("no mesh: call tsdf_extract or mesh_set first")
        nv, nf = counts
        verts = np.empty((nv, 3), np.float32)
        faces = np.empty((nf, 3), np.int32)
        rgb = np.empty((nv, 3), np.uint8)
        self._chk(self._lib.amvs_fetch_mesh(self._h, _p(verts), faces.ctypes.data_as(i32p), _u8(rgb)))
        out = [verts, faces, rgb]
        nrm = np.empty((nv, 3), np.float32) if normals else None
        lab = np.empty(nv, np.int32) if labels else None
        if normals or labels:
            self._chk(self._lib.amvs_fetch_mesh_attributes(self._h, None if nrm is None else _p(nrm),
                                                           None if lab is None else lab.ctypes.data_as(i32p)))
        out += [a for a in (nrm, lab) if a is not None]
        return tuple(out)

    # -- rendering and visibility of the current mesh (csrc/amvs_mesh_render.hip) ----
    def set_render_tuning(self, large_face_pixels=0):
        """Performance only: faces whose clamped bounding box holds more pixels than this are drawn by a workgroup
        instead of by one lane (0 = automatic).  The maps do not depend on it."""
        self._chk(self._lib.amvs_set_render_tuning(self._h, int(large_face_pixels)))

    def mesh_render(self, K, poses, near=1e-3, skipped=False, fetch=True):
        """Z-buffer render of the current mesh into the cameras poses = list of (R, t) with the intrinsics K (3,3), both
        used in float32 (include/amvs.h amvs_mesh_render): (depth (n,H,W) float32, 0 where nothing was drawn, face
        (n,H,W) int32, -1 there)[, faces skipped per view (n,) int64 with skipped=True].  The maps stay on the device
        for mesh_visibility until the mesh changes; fetch=False leaves them there and returns only the skipped counts
        (mesh_render_fetch copies them later)."""
        n = len(poses)
        Kf = _r32(K, 9)
        pp = _r32(_poses64(poses), n, 12) if n else np.zeros((0, 12), np.float32)
        skip = np.zeros(max(n, 1), np.int64)
        self._chk(self._lib.amvs_mesh_render(self._h, n, _p(Kf), _p(pp), float(np.float32(near)),
                                             skip.ctypes.data_as(C.POINTER(C.c_int64))))
        self._render_views = n
        if not fetch:
            return skip[:n]
        out = self.mesh_render_fetch(0, n)
        return out + (skip[:n],) if skipped else out

    def mesh_render_fetch(self, first, count):
        """(depth, face) of `count` views of the current render from view `first` on."""
        depth = np.empty((count, self.H, self.W), np.float32)
        face = np.empty((count, self.H, self.W), np.int32)
        self._chk(self._lib.amvs_fetch_render(self._h, int(first), int(count), _p(depth), face.ctypes.data_as(i32p)))
        return depth, face

    def mesh_visibility(self, depth_tolerance):
        """In how many of the rendered views every vertex of the current mesh is seen: in front of the render's near,
        inside the image, and not behind the rendered depth at its nearest pixel by more than depth_tolerance
        (include/amvs.h amvs_mesh_visibility).  Returns counts (V,) int32; needs mesh_render."""
        seen = C.c_int64(0)
        self._chk(self._lib.amvs_mesh_visibility(self._h, float(np.float32(depth_tolerance)), C.byref(seen)))
        counts = np.empty(self._mesh_counts[0], np.int32)
        self._chk(self._lib.amvs_fetch_mesh_visibility(self._h, counts.ctypes.data_as(i32p)))
        return counts

    def mesh_filter_visible(self, min_views=1):
        """Keep the faces whose three vertices are each seen by at least min_views views (needs mesh_visibility).
        Returns (vertices, faces) after it; drops the render, the counts, labels and normals."""
        nv, nf = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.amvs_mesh_filter_visible(self._h, int(min_views), C.byref(nv), C.byref(nf)))
        self._mesh_counts = (nv.value, nf.value)
        return nv.value, nf.value

    # -- colours from the views and the render in colour (csrc/amvs_mesh_color.hip) ----
    def mesh_color_views(self, depth_tolerance, min_cos=0.2, best_view=False, view_ids=None, colors_bgr=None):
        """Recolour the current mesh's vertices from the images of the rendered views (include/amvs.h
        amvs_mesh_color_views): a view contributes where the vertex's 2 x 2 footprint lies in the image and on the
        rendered surface within depth_tolerance, and the cosine between the normal and the direction to the camera
        exceeds min_cos; the bilinear samples are blended with the cosine as weight, or with best_view the view with the
        largest cosine is taken.  Image j belongs to rendered view j: view_ids (resident colour images) or colors_bgr
        (n,H,W,3) uint8 BGR, exactly one of them.  Needs mesh_render and mesh_normals.  Returns the number of vertices
        recoloured; the others keep their colour."""
        n = self._render_views           # whether that render is still current is the library's check
        idp, colp = None, None
        if view_ids is not None:
            ids, idp = _ids(view_ids)
            if ids.shape != (n,):
                raise ValueError(f"{ids.size} view ids for {n} rendered views")
        if colors_bgr is not None:
            cols = np.ascontiguousarray(colors_bgr, dtype=np.uint8)
            if cols.shape != (n, self.H, self.W, 3):
                raise ValueError(f"colors_bgr must be ({n}, {self.H}, {self.W}, 3)")
            colp = _u8(cols)
        done = C.c_int64(0)
        self._chk(self._lib.amvs_mesh_color_views(self._h, idp, colp, float(np.float32(depth_tolerance)),
                                                  float(np.float32(min_cos)), int(bool(best_view)), C.byref(done)))
        return done.value

    def mesh_render_color(self, first, count):
        """The current render of `count` views from view `first` on, shaded with the current vertex colours
        (include/amvs.h amvs_fetch_render_color): (count,H,W,3) uint8 RGB, 0 where nothing was drawn."""
        out = np.empty((max(int(count), 0), self.H, self.W, 3), np.uint8)
        self._chk(self._lib.amvs_fetch_render_color(self._h, int(first), int(count), _u8(out)))
        return out

    # -- texture from the views and the render shaded with it (csrc/amvs_mesh_texture.hip) ----
    def mesh_texture(self, depth_tolerance, texels=8, min_cos=0.2, best_view=False, cells_per_row=0, view_ids=None,
                     colors_bgr=None):
        """A per-face texture atlas of the current mesh from the images of the rendered views (include/amvs.h
        amvs_mesh_texture): every face gets a right triangle of `texels` texel intervals per leg, two faces to a square
        cell, cells_per_row cells to a row (0 = a square atlas).  A texel is coloured as mesh_color_views colours a
        vertex, at its point on the face with the face's normal, and falls back to the interpolated vertex colours where
        no view reaches it.  Image j belongs to rendered view j: view_ids or colors_bgr, exactly one.  Needs mesh_render.
        Returns (atlas (Ht,Wt,3) uint8 RGB, uv (F,3,2) float32 with v up, texels a view reached); n_texels of the last
        call is kept in last_texture_texels."""
        n = self._render_views           # whether that render is still current is the library's check
        idp, colp = None, None
        if view_ids is not None:
            ids, idp = _ids(view_ids)
            if ids.shape != (n,):
                raise ValueError(f"{ids.size} view ids for {n} rendered views")
        if colors_bgr is not None:
            cols = np.ascontiguousarray(colors_bgr, dtype=np.uint8)
            if cols.shape != (n, self.H, self.W, 3):
                raise ValueError(f"colors_bgr must be ({n}, {self.H}, {self.W}, 3)")
            colp = _u8(cols)
        wt, ht, total, done = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.amvs_mesh_texture(self._h, idp, colp, float(np.float32(depth_tolerance)), float(np.float32(min_cos)),
                                              int(bool(best_view)), int(texels), int(cells_per_row), C.byref(wt), C.byref(ht),
                                              C.byref(total), C.byref(done)))
        self.last_texture_texels = total.value
        atlas = np.empty((ht.value, wt.value, 3), np.uint8)
        uv = np.empty((self._mesh_counts[1], 3, 2), np.float32)
        self._chk(self._lib.amvs_fetch_mesh_texture(self._h, _u8(atlas) if atlas.size else None, _p(uv) if uv.size else None))
        return atlas, uv, done.value

    def mesh_render_texture(self, first, count):
        """The current render of `count` views from view `first` on, shaded with the current texture (include/amvs.h
        amvs_fetch_render_texture): (count,H,W,3) uint8 RGB, 0 where nothing was drawn."""
        out = np.empty((max(int(count), 0), self.H, self.W, 3), np.uint8)
        self._chk(self._lib.amvs_fetch_render_texture(self._h, int(first), int(count), _u8(out)))
        return out

    def knn_mean_distance(self, points, k=20):
        """Mean distance of every point to its k-1 nearest other points, bit-identical to
        np.mean(NearestNeighbors(n_neighbors=k).fit(p).kneighbors(p)[0][:, 1:], axis=1)."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        out = np.empty(pts.shape[0], np.float64)
        self._chk(self._lib.amvs_knn_mean_distance(self._h, _f64(pts), pts.shape[0], int(k), _f64(out)))
        return out

    def selftest_lean_math(self):
        """(reciprocal mismatches, sqrt mismatches) against IEEE over all 2^32 float patterns."""
        out = (C.c_uint64 * 2)()
        self._chk(self._lib.amvs_selftest_lean_math(self._h, out))
        return int(out[0]), int(out[1])

    def rng_fill(self, seed, stream_view, draw, n):
        u = np.empty(n, np.float32)
        nz = np.empty((n, 3), np.float32)
        self._chk(self._lib.amvs_rng_fill(self._h, int(seed), int(stream_view), int(draw), int(n), _p(u), _p(nz)))
        return u, nz
