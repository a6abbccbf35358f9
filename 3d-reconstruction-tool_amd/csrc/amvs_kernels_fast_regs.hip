// amvs_kernels_fast_regs.hip -- the fast sweep step with the reference statistics formed in the kernel and / or the
// centre depth kept in registers (StepArgs::ref_in_kernel, depth_hist; launch_step_fast_regs), for the source counts
// of UnpackedRegsSourceCounts (amvs_dispatch.h).  The kernel is the one of amvs_kernels_fast.hip, instantiated here
// with those template flags: a translation unit of its own so that these instantiations compile beside the others
// instead of doubling that file's build time, and so that they can be built without the compiler's packing of
// adjacent f32 operations into v_pk_*_f32 (csrc/Makefile).  In the index-checked build
// a violation is reported with this unit's id and the source line of amvs_kernels_fast.hip.
#define AMVS_FAST_STEP_REGS_TU
#define AMVS_TU_ID 22
#include "amvs_kernels_fast.hip"
