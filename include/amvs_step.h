/* amvs_step.h -- where the fast-arithmetic sweep step of libamvs.so takes two of its per-row inputs from
 * (csrc/amvs_kernels_fast.hip, csrc/amvs_kernels_fast_regs.hip).  Bound from _lib.STEP_SIGNATURES.  The library, the
 * context and the error codes are those of amvs.h.
 *
 * amvs_set_step_sources is a per-context tuning switch in the style of amvs_set_launch_order: performance only, the
 * maps do not depend on it (tests/test_hip_step_ref_stats.py).
 *   ref_stats     0 = the reference window's (mean1, var1) are loaded from the per-view maps computed at upload;
 *                 1 = they are formed in the kernel from the reference codes the wave carries (exact integer sums,
 *                     then the same two operations: the same bits), and the maps are not built for such a call.
 *   centre_depth  0 = the centre pixel's depth (propagation: its neighbour's) is loaded when the window is complete;
 *                 1 = it is kept in registers from the load that sampled that pixel patch_size / 2 rows earlier
 *                     (the sweep's propagation and refinement launches; the split schedule's window kernel, cost
 *                     evaluation and confidence have no such load and are unaffected).
 *   -1            the library's choice: a table by patch size (measured: DESIGN.md section 5, round 9).
 * Patch sizes above amvs_step_sources_max_patch() (15: a k x k window's sum of squared codes fits float32's 24 bits up
 * to 15 x 15), the run-time patch sizes, the exact arithmetic and the plane sweeps always use the maps and the loads;
 * the switch is accepted and ignored there.  AMVS_EINVAL for a value outside -1 .. 1.
 *
 * amvs_get_step_sources reports what a fast-arithmetic sweep step of this context takes at `patch_size` as the switch
 * stands (the table resolved, unsupported sizes as 0): *ref_stats and *centre_depth are set to 0 or 1.  AMVS_EINVAL
 * for a NULL pointer.  No GPU work.                                                                                 */
#ifndef AMVS_STEP_H
#define AMVS_STEP_H

#include "amvs.h"

#ifdef __cplusplus
extern "C" {
#endif

int amvs_set_step_sources(amvs_ctx *ctx, int ref_stats, int centre_depth);
int amvs_get_step_sources(amvs_ctx *ctx, int patch_size, int *ref_stats, int *centre_depth);
int amvs_step_sources_max_patch(void);

#ifdef __cplusplus
}
#endif

#endif
