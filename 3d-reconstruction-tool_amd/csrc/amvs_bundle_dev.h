// amvs_bundle_dev.h -- the host interface of the bundle adjustment's kernels (amvs_bundle.hip; include/amvs_bundle.h).
// Private to the library.  Every function takes host arrays, runs on `st` with scratch from `cache`, synchronises `st`
// before it returns; the caller has validated the problem (amvs_bundle_host.h: ba_problem_error).
#pragma once
#include "amvs_buffer.h"
#include "amvs_bundle_host.h"

#include <hip/hip_runtime.h>

namespace amvs {

hipError_t ba_cost(const BaProblem &h, double *cost, long long *active, double *err2, ScratchCache &cache, hipStream_t st);
hipError_t ba_normal(const BaProblem &h, double *U, double *gc, double *V, double *gp, int *counts, ScratchCache &cache, hipStream_t st);
hipError_t ba_schur(const BaProblem &h, int refine_points, double lambda, double *S, double *rhs, int *slot, unsigned char *held,
                    ScratchCache &cache, hipStream_t st);
hipError_t ba_step(const BaProblem &h, int refine_points, double lambda, int *ok, double *dc, double *dp, double *R_out, double *t_out,
                   double *X_out, ScratchCache &cache, hipStream_t st);
hipError_t ba_solve(const BaProblem &h, int refine_points, double lambda0, double ftol, int max_trials, double *R_out, double *t_out,
                    double *X_out, double info[6], ScratchCache &cache, hipStream_t st);

}  // namespace amvs
