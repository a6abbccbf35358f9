/* amvs_plan.h -- the launch plan of a PatchMatch call / a plane sweep of libamvs.so as its entry points compute it: the same
 * functions (csrc/amvs_launch_plan.h), without a context and without a GPU.  Test infrastructure, like amvs_sweep_order of
 * amvs.h (tests/test_launch_plan_cpu.py).  Bound from _lib.PLAN_SIGNATURES.  The error codes are those of amvs.h.
 *
 * The inputs are what a context holds and what the kernels' launch interface says, as plain values:
 *   amvs_plan_device  the images and the device; packed_maps = amvs_sampling_mode
 *   amvs_plan_call    the batch, its arithmetic (fast = 1) and the call's parameters
 *   amvs_plan_tuning  the knobs of the amvs_set_* setters, as stored (tune_rows / tune_cap: n_tune values each, two per
 *                     iteration, NULL = zeros; edge_first -1 = where the groups overlap; *_source -1 = the automatic table)
 *   amvs_plan_facts   for the call's patch size, source count and arithmetic: columns a strip writes, resident waves per
 *                     CU of the step kernel by workgroup cap 0..8 (the plan reads entry 0 and those of the caps in
 *                     tune_cap; AMVS_EINVAL if one it reads is < 1), which kernels are compiled, the plane sweep's limits
 * amvs_plan_patchmatch writes the plan and as many of its steps as `capacity` holds (plan->n_steps is their number);
 * whether the call is valid (the split schedule in fast mode only, ...) is the entry points' business, not the plan's.
 * AMVS_EINVAL for a NULL pointer, a size below 1, a negative count or a workgroup cap outside 0..8.                       */
#ifndef AMVS_PLAN_H
#define AMVS_PLAN_H

#include "amvs.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { int32_t H, W, n_cu, packed_maps; } amvs_plan_device;
typedef struct { int32_t n_ref, n_src, fast; amvs_pm_params p; } amvs_plan_call;
typedef struct {
    int32_t default_band_major;
    int32_t n_tune;
    const int32_t *tune_rows, *tune_cap;
    int32_t split_groups, split_sample_rows, split_sample_lds;
    int32_t edge_first, group_overlap;
    int32_t sweep_tile_rows, sweep_chunk, sweep_key8;
    int32_t ref_stats_source, depth_source;
} amvs_plan_tuning;
typedef struct {
    int32_t out_width;
    int32_t waves_per_cu[9];
    int32_t patch_compiled, pair_supported, fast_pair_supported, fast_regs_supported;
    int32_t sweep_max_th, sweep_max_th8, sweep_max_chunk, sweep_max_chunk8;
} amvs_plan_facts;
typedef struct {                /* one launch of the schedule (the same for every view group) */
    int32_t mode, oy, ox;       /* 1 = propagation from (y + oy, x + ox), 2 = refinement */
    float depth_range, normal_range;
    uint32_t draw;
    int32_t flip_d;             /* depth buffers ping-ponged by the step */
    int32_t iter;
    int32_t rows, wg_cap;       /* strip rows, resident workgroups per CU (0 = default) */
    int32_t tiles_y;
} amvs_plan_step;
typedef struct {
    int32_t band_major, paired, views_per_launch, n_groups;
    int32_t tile_rows, tiles_x, tiles_y;        /* base strips: initialisation and confidence launches */
    int32_t overlap, edge_first;                /* effective values */
    int32_t n_steps, final_parity, last_tile_rows;
    int64_t launches;
    int32_t split_groups, split_vpl, split_tile_rows, s_tile_rows, s_lds, s_tiles_x, s_tiles_y;   /* split schedule, else 0 */
    int32_t ref_in_kernel, depth_hist;          /* amvs_get_step_sources */
    int32_t single_step_rows;                   /* strip rows of the single-step entry points (0: waves_per_cu[0] < 1) */
} amvs_pm_plan;
typedef struct { int32_t tile_rows, tiles_x, tiles_y, chunk, n_chunks, key8; } amvs_sweep_plan;

int amvs_plan_patchmatch(const amvs_plan_device *dev, const amvs_plan_call *call, const amvs_plan_tuning *tuning,
                         const amvs_plan_facts *facts, amvs_pm_plan *plan, amvs_plan_step *steps, int32_t capacity);
int amvs_plan_plane_sweep(const amvs_plan_device *dev, const amvs_plan_tuning *tuning, const amvs_plan_facts *facts,
                          int n_ref, int D, amvs_sweep_plan *plan);

#ifdef __cplusplus
}
#endif

#endif
