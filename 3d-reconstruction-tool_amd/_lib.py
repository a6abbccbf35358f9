"""ctypes binding of libamvs.so (the C ABI declared in include/amvs.h, include/amvs_depth.h, include/amvs_lens.h,
include/amvs_match.h, include/amvs_epipolar.h, include/amvs_resection.h, include/amvs_twoview.h, include/amvs_bundle.h, include/amvs_sfm.h, include/amvs_features.h, include/amvs_step.h and include/amvs_plan.h).

There is no CPU fallback: if the shared library is missing or no HIP device is
present, loading / context creation raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# AMVS_LIB selects an alternative build of the same ABI (A/B runs of kernel variants)
LIB_PATH = os.environ.get("AMVS_LIB") or os.path.join(_HERE, "libamvs.so")

AMVS_MAX_SRC = 6
MODES = {"default": 0, "exact": 1, "fast": 2}
SCHEDULES = {"auto": 0, "view-major": 1, "band-major": 2, "split": 3, "paired": 4}
SUPPORTED_PATCH_SIZES = tuple(range(3, 32, 2))        # compiled: 3 ... 29; 31 runs the run-time-k kernels
TSDF_MAX_POINTS = 1 << 27                              # include/amvs.h AMVS_TSDF_MAX_POINTS

f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int)


class PmParams(C.Structure):
    _fields_ = [("patch_size", C.c_int32), ("num_iterations", C.c_int32),
                ("num_samples", C.c_int32), ("tile_rows", C.c_int32), ("views_per_launch", C.c_int32),
                ("depth_min", C.c_float), ("depth_max", C.c_float),
                ("log_depth_scale", C.c_float), ("log_depth_min", C.c_float), ("mode", C.c_int32),
                ("schedule", C.c_int32), ("first_iteration", C.c_int32), ("flags", C.c_int32)]


PM_NO_CONFIDENCE = 1


class XpmParams(C.Structure):
    _fields_ = [("patch_size", C.c_int32), ("window_stride", C.c_int32), ("num_refine", C.c_int32),
                ("view_propagation", C.c_int32), ("depth_min", C.c_float), ("depth_max", C.c_float),
                ("log_depth_scale", C.c_float), ("log_depth_min", C.c_float),
                ("consistency_px", C.c_float), ("consistency_rel", C.c_float)]


def _i32_struct(name, fields):
    return type(name, (C.Structure,), {"_fields_": [(f, C.c_int32) for f in fields.split()]})


# include/amvs_plan.h: the launch planner's inputs and outputs (plan_patchmatch, plan_plane_sweep)
PlanDevice = _i32_struct("PlanDevice", "H W n_cu packed_maps")
PlanSweep = _i32_struct("PlanSweep", "tile_rows tiles_x tiles_y chunk n_chunks key8")


class PlanCall(C.Structure):
    _fields_ = [("n_ref", C.c_int32), ("n_src", C.c_int32), ("fast", C.c_int32), ("p", PmParams)]


class PlanTuning(C.Structure):
    _fields_ = [("default_band_major", C.c_int32), ("n_tune", C.c_int32),
                ("tune_rows", C.POINTER(C.c_int32)), ("tune_cap", C.POINTER(C.c_int32))] + \
               [(f, C.c_int32) for f in "split_groups split_sample_rows split_sample_lds edge_first group_overlap "
                                         "sweep_tile_rows sweep_chunk sweep_key8 ref_stats_source depth_source".split()]


class PlanFacts(C.Structure):
    _fields_ = [("out_width", C.c_int32), ("waves_per_cu", C.c_int32 * 9)] + \
               [(f, C.c_int32) for f in "patch_compiled pair_supported fast_pair_supported fast_regs_supported "
                                         "sweep_max_th sweep_max_th8 sweep_max_chunk sweep_max_chunk8".split()]


class PlanStep(C.Structure):
    _fields_ = [("mode", C.c_int32), ("oy", C.c_int32), ("ox", C.c_int32), ("depth_range", C.c_float),
                ("normal_range", C.c_float), ("draw", C.c_uint32), ("flip_d", C.c_int32), ("iter", C.c_int32),
                ("rows", C.c_int32), ("wg_cap", C.c_int32), ("tiles_y", C.c_int32)]


class PmPlan(C.Structure):
    _fields_ = [(f, C.c_int32) for f in "band_major paired views_per_launch n_groups tile_rows tiles_x tiles_y overlap "
                                         "edge_first n_steps final_parity last_tile_rows".split()] + \
               [("launches", C.c_int64)] + \
               [(f, C.c_int32) for f in "split_groups split_vpl split_tile_rows s_tile_rows s_lds s_tiles_x s_tiles_y "
                                         "ref_in_kernel depth_hist single_step_rows".split()]


class Timing(C.Structure):
    _fields_ = [("init_ms", C.c_double), ("sweep_ms", C.c_double), ("confidence_ms", C.c_double),
                ("sweep_launches", C.c_int64), ("pixel_hypotheses", C.c_int64)]


# name -> (restype, argtypes); every symbol include/amvs.h declares
SIGNATURES = {
    "amvs_version": (C.c_char_p, []),
    "amvs_last_error": (C.c_char_p, [C.c_void_p]),
    "amvs_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, C.POINTER(C.c_void_p)]),
    "amvs_destroy": (C.c_int, [C.c_void_p]),
    "amvs_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "amvs_sync": (C.c_int, [C.c_void_p]),
    "amvs_set_view": (C.c_int, [C.c_void_p, C.c_int, f32p, f32p, f32p]),
    "amvs_set_view_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, f32p, f32p]),
    "amvs_set_view_bgr8": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_int, f32p, f32p,
                                     C.POINTER(C.c_uint8)]),
    "amvs_patchmatch": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p, C.c_int, C.POINTER(PmParams),
                                  C.c_uint64, f32p, f32p, f32p]),
    "amvs_patchmatch_device": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p, C.c_int,
                                         C.POINTER(PmParams), C.c_uint64,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "amvs_get_timing": (C.c_int, [C.c_void_p, C.POINTER(Timing)]),
    "amvs_sampling_mode": (C.c_int, [C.c_void_p]),
    "amvs_set_sampling": (C.c_int, [C.c_void_p, C.c_int]),
    "amvs_set_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "amvs_get_mode": (C.c_int, [C.c_void_p]),
    "amvs_set_sweep_tuning": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "amvs_set_split_tuning": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "amvs_set_step_tuning": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p]),
    "amvs_set_step_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "amvs_get_step_times": (C.c_int, [C.c_void_p, f32p, C.c_int, i32p]),
    "amvs_set_launch_order": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "amvs_sweep_order": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, i32p, i32p]),
    "amvs_fetch_step_trace": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int64, C.POINTER(C.c_int64),
                                        C.POINTER(C.c_int64)]),
    "amvs_last_tile_rows": (C.c_int, [C.c_void_p]),
    "amvs_last_views_per_launch": (C.c_int, [C.c_void_p]),
    "amvs_plane_sweep": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_int, f32p, C.c_int, C.c_int,
                                   C.c_float, f32p, f32p]),
    "amvs_plane_sweep_device": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p, C.c_int, f32p, C.c_int,
                                          C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "amvs_plane_sweep_batch": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p, C.c_int, f32p, C.c_int, C.c_int, C.c_float]),
    "amvs_fetch_sweep_maps": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f32p, f32p]),
    "amvs_stereo_backproject": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_uint8),
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_float,
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "amvs_cloud_knn_mean_distance": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    "amvs_cloud_voxel_downsample": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_double, C.POINTER(C.c_int64)]),
    "amvs_cloud_take": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int64]),
    "amvs_knn_supported": (C.c_int, [C.c_int]),
    "amvs_xpm_init": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p, C.c_int, C.POINTER(XpmParams), C.c_uint64,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "amvs_xpm_iterate": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p, C.c_int, C.POINTER(XpmParams), C.c_int, C.c_uint64,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "amvs_xpm_step": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p, C.c_int, C.POINTER(XpmParams), C.c_int, C.c_uint64, C.c_int,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "amvs_xpm_fetch_candidates": (C.c_int, [C.c_void_p, C.c_int, f32p, f32p]),
    "amvs_xpm_consistency": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p, C.c_int, C.POINTER(XpmParams),
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "amvs_eval_cost": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_int, C.c_int, f32p, f32p]),
    "amvs_sample_sources": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_int, C.c_int, C.c_int, f32p, f32p,
                                      C.POINTER(C.c_uint8)]),
    "amvs_confidence": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_int, C.c_int, f32p, f32p]),
    "amvs_propagate_step": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_int, C.c_int, f32p, f32p, f32p,
                                      C.c_int, C.c_int, C.c_float]),
    "amvs_refine_step": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_int, C.c_int, f32p, f32p, f32p,
                                   C.c_uint64, C.c_uint32, C.c_uint32,
                                   C.c_float, C.c_float, C.c_float, C.c_float]),
    "amvs_init_state": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_float, C.c_float,
                                  f32p, f32p, f32p]),
    "amvs_box_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f32p, f32p]),
    "amvs_fuse_filter": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_uint8),
                                   C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_float, C.c_int,
                                   C.POINTER(C.c_int64)]),
    "amvs_fuse_filter_views": (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                               C.POINTER(C.c_double), C.c_float, C.c_int, C.POINTER(C.c_int64)]),
    "amvs_stereo_backproject_views": (C.c_int, [C.c_void_p, C.c_int, i32p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.c_float, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "amvs_set_view_colors": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint8)]),
    "amvs_fetch_cloud": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint8)]),
    "amvs_depth_normals": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.c_float, C.c_int, C.c_float, C.c_int, C.c_int,
                                     C.POINTER(C.c_int64)]),
    "amvs_fetch_depth_normals": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f32p]),
    "amvs_cloud_normals": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.c_float, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int,
                                     C.POINTER(C.c_int64)]),
    "amvs_fetch_cloud_normals": (C.c_int, [C.c_void_p, f32p, i32p]),
    "amvs_cloud_set": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.c_int64]),
    "amvs_tsdf_integrate": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, i32p, C.POINTER(C.c_uint8),
                                      f32p, f32p, C.c_float, f32p, C.c_float, i32p, C.c_float]),
    "amvs_tsdf_extract": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "amvs_fetch_mesh": (C.c_int, [C.c_void_p, f32p, i32p, C.POINTER(C.c_uint8)]),
    "amvs_tsdf_fetch_volume": (C.c_int, [C.c_void_p, f32p, f32p, f32p]),
    "amvs_tsdf_set_volume": (C.c_int, [C.c_void_p, f32p, f32p, f32p, f32p, C.c_float, i32p]),
    "amvs_tsdf_fill": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "amvs_tsdf_fetch_fill": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8)]),
    "amvs_mesh_set": (C.c_int, [C.c_void_p, f32p, C.c_int64, i32p, C.c_int64, C.POINTER(C.c_uint8)]),
    "amvs_mesh_filter_components": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                              C.POINTER(C.c_int64)]),
    "amvs_mesh_smooth": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int]),
    "amvs_mesh_normals": (C.c_int, [C.c_void_p]),
    "amvs_mesh_decimate": (C.c_int, [C.c_void_p, f32p, C.c_float, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "amvs_mesh_decimate_quadric": (C.c_int, [C.c_void_p, f32p, C.c_float, C.c_float, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                             C.POINTER(C.c_int64)]),
    "amvs_fetch_mesh_attributes": (C.c_int, [C.c_void_p, f32p, i32p]),
    "amvs_mesh_render": (C.c_int, [C.c_void_p, C.c_int, f32p, f32p, C.c_float, C.POINTER(C.c_int64)]),
    "amvs_fetch_render": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f32p, i32p]),
    "amvs_mesh_visibility": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(C.c_int64)]),
    "amvs_fetch_mesh_visibility": (C.c_int, [C.c_void_p, i32p]),
    "amvs_mesh_filter_visible": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "amvs_set_render_tuning": (C.c_int, [C.c_void_p, C.c_int]),
    "amvs_mesh_color_views": (C.c_int, [C.c_void_p, i32p, C.POINTER(C.c_uint8), C.c_float, C.c_float, C.c_int,
                                        C.POINTER(C.c_int64)]),
    "amvs_fetch_render_color": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint8)]),
    "amvs_mesh_texture": (C.c_int, [C.c_void_p, i32p, C.POINTER(C.c_uint8), C.c_float, C.c_float, C.c_int, C.c_int, C.c_int,
                                    C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "amvs_fetch_mesh_texture": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), f32p]),
    "amvs_fetch_render_texture": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint8)]),
    "amvs_comm_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
    "amvs_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint8)]),
    "amvs_allgather_maps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "amvs_comm_destroy": (C.c_int, [C.c_void_p]),
    "amvs_write_ply": (C.c_int, [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int64]),
    "amvs_write_ply_normals": (C.c_int, [C.c_char_p, C.POINTER(C.c_double), f32p, C.POINTER(C.c_int64), C.c_int64]),
    "amvs_knn_mean_distance": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int64, C.c_int, C.POINTER(C.c_double)]),
    "amvs_selftest_lean_math": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "amvs_index_check": (C.c_int, [C.POINTER(C.c_uint64), C.c_int]),
    "amvs_rng_fill": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int64, f32p, f32p]),
}

# name -> (restype, argtypes); every symbol include/amvs_depth.h declares.  A table of its own because
# tests/test_cloud_normals_cpu.py holds SIGNATURES to the 92 declarations of include/amvs.h; load() binds both.
DEPTH_SIGNATURES = {
    "amvs_depth_filter": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double), i32p, C.c_int, C.c_float, C.c_float,
                                    C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64)]),
}

# name -> (restype, argtypes); every symbol include/amvs_lens.h declares (a table of its own for the same reason)
LENS_SIGNATURES = {
    "amvs_undistort_bgr8": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_int64)]),
    "amvs_set_view_bgr8_undistorted": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_int,
                                                 C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, f32p, f32p,
                                                 C.POINTER(C.c_uint8)]),
}

# name -> (restype, argtypes); every symbol include/amvs_match.h declares (a table of its own for the same reason)
f64p = C.POINTER(C.c_double)
MATCH_SIGNATURES = {
    "amvs_desc_set": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_int]),
    "amvs_desc_knn2": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p]),
    "amvs_desc_match": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, i32p, i32p, i32p, C.POINTER(C.c_int64)]),
    "amvs_pair_cloud_begin": (C.c_int, [C.c_void_p]),
    "amvs_pair_triangulate": (C.c_int, [C.c_void_p, f64p, f64p, f64p, f64p, f64p, f32p, f32p, C.POINTER(C.c_uint8), C.c_int,
                                        C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int64)]),
    "amvs_pair_cloud_finish": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "amvs_cloud_bounds": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), f64p, f64p]),
    "amvs_cloud_voxel_downsample_grid": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), f64p, C.c_double, C.POINTER(C.c_int64)]),
    "amvs_match_selftest_sqrt": (C.c_int, [C.c_void_p, f64p, C.c_int, f64p]),
}
# include/amvs_match.h: the launch shape of the matcher (its tests aim at these edges) and its limits
DESC_DIM, DESC_TILE, DESC_CHUNK, DESC_QUERY_BLOCK = 128, 32, 256, 512
DESC_MAX_ROWS, DESC_MAX_SLOTS = 1 << 20, 1 << 16

# name -> (restype, argtypes); every symbol include/amvs_epipolar.h declares (a table of its own for the same reason)
u8p, i64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int64)
EPIPOLAR_SIGNATURES = {
    "amvs_fmat_hypotheses": (C.c_int, [C.c_void_p, f32p, f32p, C.c_int, C.c_uint64, C.c_int, C.c_int, i32p, f64p]),
    "amvs_fmat_score": (C.c_int, [C.c_void_p, f64p, C.c_int, f32p, f32p, C.c_int, C.c_double, i32p]),
    "amvs_fmat_inliers": (C.c_int, [C.c_void_p, f64p, f32p, f32p, C.c_int, C.c_double, u8p, i64p]),
    "amvs_fmat_fit": (C.c_int, [C.c_void_p, f32p, f32p, u8p, C.c_int, f64p, i64p]),
    "amvs_fmat_ransac": (C.c_int, [C.c_void_p, f32p, f32p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_uint64, f64p, u8p, i64p,
                                   i32p]),
}
# include/amvs_epipolar.h: hypotheses per RANSAC batch, matches per block of a sum, and the limits
FMAT_BATCH, FMAT_BLOCK, FMAT_MAX_MATCHES, FMAT_MAX_HYP = 1024, 64, 1 << 20, 1 << 20

# name -> (restype, argtypes); every symbol include/amvs_resection.h declares (a table of its own for the same reason)
PNP_SIGNATURES = {
    "amvs_pnp_hypotheses": (C.c_int, [C.c_void_p, f32p, f32p, C.c_int, f64p, C.c_uint64, C.c_int, C.c_int, i32p, f64p, f64p]),
    "amvs_pnp_score": (C.c_int, [C.c_void_p, f64p, f64p, C.c_int, f32p, f32p, C.c_int, f64p, C.c_double, i32p]),
    "amvs_pnp_inliers": (C.c_int, [C.c_void_p, f64p, f64p, f32p, f32p, C.c_int, f64p, C.c_double, u8p, i64p]),
    "amvs_pnp_refine": (C.c_int, [C.c_void_p, f32p, f32p, C.c_int, f64p, f64p, f64p, u8p, f64p, f64p, i32p, f64p, i64p]),
    "amvs_pnp_ransac": (C.c_int, [C.c_void_p, f32p, f32p, C.c_int, f64p, C.c_double, C.c_double, C.c_int, C.c_uint64, f64p, f64p,
                                  u8p, i64p, i32p]),
}
# include/amvs_resection.h: hypotheses per RANSAC batch, correspondences per block of a sum, refit steps, and the limits
PNP_BATCH, PNP_BLOCK, PNP_REFINE_STEPS, PNP_MAX_POINTS, PNP_MAX_HYP = 1024, 64, 10, 1 << 20, 1 << 20

# name -> (restype, argtypes); every symbol include/amvs_twoview.h declares (a table of its own for the same reason)
TWOVIEW_SIGNATURES = {
    "amvs_twoview_decompose": (C.c_int, [C.c_void_p, f64p, f64p, f64p, f64p, f64p, i32p]),
    "amvs_twoview_score": (C.c_int, [C.c_void_p, f64p, f64p, C.c_int, f32p, f32p, C.c_int, f64p, C.c_double, i32p]),
    "amvs_twoview_front": (C.c_int, [C.c_void_p, f64p, f64p, f32p, f32p, C.c_int, f64p, C.c_double, u8p, i64p]),
    "amvs_twoview_pose": (C.c_int, [C.c_void_p, f64p, f64p, f32p, f32p, C.c_int, C.c_double, f64p, f64p, u8p, i64p, i32p]),
    "amvs_twoview_triangulate": (C.c_int, [C.c_void_p, f64p, f64p, f64p, f64p, f64p, f32p, f32p, C.c_int, C.c_double, C.c_double,
                                           C.c_double, C.c_double, f64p, u8p, f64p, i64p]),
}
# include/amvs_twoview.h: the limits, the poses a scoring workgroup walks, and the defaults of the Python layer
TWOVIEW_MAX_MATCHES, TWOVIEW_MAX_POSES, TWOVIEW_POSE_TILE = 1 << 20, 1 << 20, 32
TWOVIEW_MAX_DEPTH, TWOVIEW_DEPTH_MIN, TWOVIEW_DEPTH_BASELINES, TWOVIEW_MIN_PARALLAX_DEG, TWOVIEW_MAX_REPROJ = 50.0, 0.01, 200.0, 1.0, 4.0

# name -> (restype, argtypes); every symbol include/amvs_bundle.h declares (a table of its own for the same reason)
_BA_PROBLEM = [C.c_void_p, f64p, f64p, C.c_int, f64p, C.c_int, i32p, i32p, f32p, C.c_int, f64p]      # ctx, R, t, C, X, P, cam, pt, uv, N, K
BA_SIGNATURES = {
    "amvs_ba_cost": (C.c_int, _BA_PROBLEM + [f64p, i64p, f64p]),
    "amvs_ba_normal": (C.c_int, _BA_PROBLEM + [u8p, f64p, f64p, f64p, f64p, i32p]),
    "amvs_ba_schur": (C.c_int, _BA_PROBLEM + [u8p, C.c_int, C.c_double, f64p, f64p, i32p, u8p]),
    "amvs_ba_step": (C.c_int, _BA_PROBLEM + [u8p, C.c_int, C.c_double, i32p, f64p, f64p, f64p, f64p, f64p]),
    "amvs_ba_solve": (C.c_int, _BA_PROBLEM + [u8p, C.c_int, C.c_double, C.c_double, C.c_int, f64p, f64p, f64p, f64p]),
}
# include/amvs_bundle.h: list positions per block of a sum, the limits, and the bounds of the damping
BA_BLOCK, BA_MAX_CAMERAS, BA_MAX_POINTS, BA_MAX_OBS, BA_MAX_PAIRS = 64, 256, 1 << 22, 1 << 24, 1 << 25
BA_LAMBDA_MIN, BA_LAMBDA_MAX = 1e-12, 1e12

# name -> (restype, argtypes); every symbol include/amvs_sfm.h declares (a table of its own for the same reason)
SFM_SIGNATURES = {
    "amvs_sfm_begin": (C.c_int, [C.c_void_p, C.c_int, i32p, f32p, C.c_int, i32p, i32p, i32p]),
    "amvs_sfm_register": (C.c_int, [C.c_void_p, C.c_int, f64p, f64p, i32p, i32p, u8p, C.c_int, i64p]),
    "amvs_sfm_scores": (C.c_int, [C.c_void_p, i32p]),
    "amvs_sfm_correspondences": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p, f32p, f32p, i64p]),
    "amvs_sfm_triangulate": (C.c_int, [C.c_void_p, C.c_int, f64p, C.c_double, C.c_double, C.c_double, C.c_double, i64p, i32p]),
    "amvs_sfm_counts": (C.c_int, [C.c_void_p, i64p, i64p, i64p]),
    "amvs_sfm_observations": (C.c_int, [C.c_void_p, i32p, i32p, f32p, C.c_int64, i64p]),
    "amvs_sfm_points_get": (C.c_int, [C.c_void_p, f64p, u8p, C.c_int64]),
    "amvs_sfm_points_set": (C.c_int, [C.c_void_p, f64p, u8p, C.c_int64]),
    "amvs_sfm_pose_set": (C.c_int, [C.c_void_p, C.c_int, f64p, f64p]),
    "amvs_sfm_drop": (C.c_int, [C.c_void_p, i32p, i32p, C.c_int, C.c_int, i64p, i64p]),
}
# include/amvs_sfm.h: lanes (rows, keypoints or points) per workgroup, the limits, and the defaults of the Python layer
SFM_BLOCK, SFM_MAX_VIEWS, SFM_MAX_KEYPOINTS, SFM_MAX_ROWS, SFM_MAX_POINTS = 256, 4096, 1 << 28, 1 << 28, BA_MAX_POINTS
SFM_MIN_SCORE, SFM_MIN_OBS = 12, 2

# name -> (restype, argtypes); every symbol include/amvs_step.h declares (a table of its own for the same reason)
STEP_SIGNATURES = {
    "amvs_set_step_sources": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "amvs_get_step_sources": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p]),
    "amvs_step_sources_max_patch": (C.c_int, []),
}

# name -> (restype, argtypes); every symbol include/amvs_plan.h declares (a table of its own for the same reason)
PLAN_SIGNATURES = {
    "amvs_plan_patchmatch": (C.c_int, [C.POINTER(PlanDevice), C.POINTER(PlanCall), C.POINTER(PlanTuning), C.POINTER(PlanFacts),
                                       C.POINTER(PmPlan), C.POINTER(PlanStep), C.c_int32]),
    "amvs_plan_plane_sweep": (C.c_int, [C.POINTER(PlanDevice), C.POINTER(PlanTuning), C.POINTER(PlanFacts), C.c_int, C.c_int,
                                        C.POINTER(PlanSweep)]),
}

# name -> (restype, argtypes); every symbol include/amvs_features.h declares (a table of its own for the same reason)
FEATURE_SIGNATURES = {
    "amvs_clahe_u8": (C.c_int, [C.c_void_p, u8p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, u8p]),
    "amvs_sift_scale_space": (C.c_int, [C.c_void_p, u8p, C.c_int, C.c_int, C.c_double, i32p]),
    "amvs_sift_extract": (C.c_int, [C.c_void_p, u8p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_double, i32p]),
    "amvs_sift_fetch": (C.c_int, [C.c_void_p, f32p, u8p, C.c_int]),
    "amvs_sift_to_slot": (C.c_int, [C.c_void_p, C.c_int]),
    "amvs_sift_fetch_level": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, f32p, i32p, i32p]),
}
# include/amvs_features.h: the limits of the image side, the CLAHE grid and sigma, and the shape of an octave
FEATURES_MAX_SIDE, CLAHE_MAX_GRID, SIFT_MIN_SIDE, SIFT_MAX_SIGMA, SIFT_MAX_RADIUS = 8192, 64, 3, 4.0, 32
SIFT_LAYERS, SIFT_GAUSS, SIFT_DOG = 3, 6, 5
SIFT_MIN_SIGMA, SIFT_MAX_FEATURES = 0.1, 1048576

_lib = None


class AmvsError(RuntimeError):
    pass


def _share_torch_hip_runtime():
    """One HIP runtime per process.  libamvs.so links /opt/rocm's libamdhip64.so.7; a PyTorch-ROCm
    wheel bundles its own copy under the same SONAME, so whichever is loaded first serves both -- and
    PyTorch cannot see the GPU ("No HIP GPUs are available") once the system copy got in first.  When
    torch is installed its copy is therefore loaded first, whatever the import order (torch is located
    without importing it).  Without torch the system runtime is used as linked."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:  # noqa: BLE001  (best effort: the linked runtime still works on its own)
        pass


def load():
    """Load libamvs.so and bind every declared entry point (raises if absent)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AmvsError(
                f"{LIB_PATH} not found: build it with `python __graft_entry__.py` "
                "(or `make -C 3d-reconstruction-tool_amd/csrc`). There is no CPU fallback.")
        _share_torch_hip_runtime()
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(DEPTH_SIGNATURES.items()) + list(LENS_SIGNATURES.items()) \
                + list(MATCH_SIGNATURES.items()) + list(EPIPOLAR_SIGNATURES.items()) + list(PNP_SIGNATURES.items()) + list(TWOVIEW_SIGNATURES.items()) \
                + list(BA_SIGNATURES.items()) + list(SFM_SIGNATURES.items()) + list(STEP_SIGNATURES.items()) \
                + list(FEATURE_SIGNATURES.items()) + list(PLAN_SIGNATURES.items()):
            fn = getattr(lib, name)      # AttributeError if a declared symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def index_check(reset=True):
    """(violations, translation unit, source line, index, extent) of the index-checked build (include/amvs.h
    amvs_index_check); zeros from the shipped build."""
    r = (C.c_uint64 * 4)()
    load().amvs_index_check(r, int(bool(reset)))
    return int(r[0]), int(r[1]) >> 32, int(r[1]) & 0xFFFFFFFF, int(r[2]), int(r[3])


def sweep_order(n_jobs, tiles_x, tiles_y, band_major=False, paired=False, edge_first=True):
    """[n_blocks][4][5] int32 (job, strip row, strip column, up, partner) of every wave of a sweep step launch, -1 for a
    wave without a strip (include/amvs.h amvs_sweep_order; no GPU involved)."""
    import numpy as np
    lib = load()
    n = C.c_int32(0)
    args = (int(n_jobs), int(tiles_x), int(tiles_y), int(bool(band_major)), int(bool(paired)), int(bool(edge_first)))
    if lib.amvs_sweep_order(*args, 0, None, C.byref(n)) != 0:
        raise AmvsError("amvs_sweep_order: bad launch shape")
    out = np.full((n.value, 4, 5), -2, np.int32)
    lib.amvs_sweep_order(*args, out.size, out.ctypes.data_as(i32p), C.byref(n))
    return out


def _struct_dict(s):
    return {f: (list(v) if hasattr(v, "__len__") else v) for f, _ in s._fields_ for v in [getattr(s, f)]}


def _plan_inputs(device, tuning, facts):
    """(PlanDevice, PlanTuning, PlanFacts, keep) from dicts keyed by the fields of include/amvs_plan.h; tuning's
    tune_rows / tune_cap are flat lists of one length (two values per iteration) or absent, facts' waves_per_cu a list of 9."""
    t = dict(tuning)
    rows, cap = [(C.c_int32 * len(v))(*v) if v else None for v in (t.pop("tune_rows", None), t.pop("tune_cap", None))]
    if rows and cap and len(rows) != len(cap):
        raise ValueError("tune_rows and tune_cap are tables of one size")
    tun = PlanTuning(n_tune=len(rows or cap or ()), tune_rows=rows, tune_cap=cap, **t)
    f = dict(facts)
    return PlanDevice(**device), tun, PlanFacts(waves_per_cu=(C.c_int32 * 9)(*f.pop("waves_per_cu")), **f), (rows, cap)


def plan_patchmatch(device, call, tuning, facts):
    """(plan, steps) -- dicts keyed by the fields of amvs_pm_plan / amvs_plan_step -- of a PatchMatch call as the entry
    points plan it (include/amvs_plan.h amvs_plan_patchmatch; no GPU involved).  call: n_ref, n_src, fast, p (PmParams)."""
    lib = load()
    dev, tun, fac, _keep = _plan_inputs(device, tuning, facts)
    cal, plan = PlanCall(**call), PmPlan()
    if lib.amvs_plan_patchmatch(dev, cal, tun, fac, plan, None, 0) != 0:
        raise AmvsError("amvs_plan_patchmatch: bad argument")
    steps = (PlanStep * max(plan.n_steps, 1))()
    lib.amvs_plan_patchmatch(dev, cal, tun, fac, plan, steps, plan.n_steps)
    return _struct_dict(plan), [_struct_dict(s) for s in steps[:plan.n_steps]]


def plan_plane_sweep(device, tuning, facts, n_ref, n_planes):
    """The amvs_sweep_plan of a plane sweep as a dict (include/amvs_plan.h amvs_plan_plane_sweep; no GPU involved)."""
    dev, tun, fac, _keep = _plan_inputs(device, tuning, facts)
    plan = PlanSweep()
    if load().amvs_plan_plane_sweep(dev, tun, fac, int(n_ref), int(n_planes), plan) != 0:
        raise AmvsError("amvs_plan_plane_sweep: bad argument")
    return _struct_dict(plan)


def index_checks_enabled():
    return b"+index-checks" in load().amvs_version()
