// amvs_pnp_host.h -- the host interface of the resection kernels (amvs_pnp.hip; include/amvs_resection.h).  Private to the
// library.  Every function takes host arrays, runs on `st` with scratch from `cache`, synchronises `st` before it
// returns; the caller has validated the parameters.  K is the header's double[9]; R is [9] and t [3] per pose.
#pragma once
#include "amvs_buffer.h"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace amvs {

hipError_t pnp_hypotheses(const float *pts3d_h, const float *pts2d_h, int m, const double *K, uint64_t seed, int first, int count,
                          int *idx_h, double *R_h, double *t_h, ScratchCache &cache, hipStream_t st);
hipError_t pnp_score(const double *R_h, const double *t_h, int n, const float *pts3d_h, const float *pts2d_h, int m, const double *K,
                     double threshold, int *counts_h, ScratchCache &cache, hipStream_t st);
hipError_t pnp_inliers(const double R[9], const double t[3], const float *pts3d_h, const float *pts2d_h, int m, const double *K,
                       double threshold, unsigned char *mask_h, long long *count, ScratchCache &cache, hipStream_t st);
// mask_h NULL: every correspondence
hipError_t pnp_refine(const float *pts3d_h, const float *pts2d_h, int m, const double *K, const double R_in[9], const double t_in[3],
                      const unsigned char *mask_h, double R_out[9], double t_out[3], int *steps, double *cost, ScratchCache &cache,
                      hipStream_t st);
hipError_t pnp_ransac(const float *pts3d_h, const float *pts2d_h, int m, const double *K, double threshold, double confidence,
                      int max_hypotheses, uint64_t seed, double R_out[9], double t_out[3], unsigned char *mask_h, long long *n_inliers,
                      int info[3], ScratchCache &cache, hipStream_t st);

}  // namespace amvs
