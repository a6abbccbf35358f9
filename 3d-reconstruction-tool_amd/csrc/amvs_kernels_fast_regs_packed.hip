// amvs_kernels_fast_regs_packed.hip -- the instantiations of amvs_kernels_fast_regs.hip for the source counts of
// PackedRegsSourceCounts (amvs_dispatch.h; launch_step_fast_regs_packed), built with the flags of every other unit:
// without the packing of f32 pairs the backend refuses the six-source kernels ("illegal VGPR to SGPR copy",
// DESIGN.md section 5, round 11).  In the index-checked build a violation is reported with this unit's id and the
// source line of amvs_kernels_fast.hip.
#define AMVS_FAST_STEP_REGS_TU
#define AMVS_FAST_STEP_REGS_PACKED
#define AMVS_TU_ID 27
#include "amvs_kernels_fast.hip"
