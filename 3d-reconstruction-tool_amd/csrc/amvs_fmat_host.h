// amvs_fmat_host.h -- the host interface of the fundamental-matrix kernels (amvs_fmat.hip; include/amvs_epipolar.h).
// Private to the library.  Every function takes host arrays, runs on `st` with scratch from `cache`, synchronises `st`
// before it returns; the caller has validated the parameters.
#pragma once
#include "amvs_buffer.h"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace amvs {

hipError_t fmat_hypotheses(const float *pts1_h, const float *pts2_h, int m, uint64_t seed, int first, int count, int *idx_h,
                           double *F_h, ScratchCache &cache, hipStream_t st);
hipError_t fmat_score(const double *F_h, int n, const float *pts1_h, const float *pts2_h, int m, double threshold, int *counts_h,
                      ScratchCache &cache, hipStream_t st);
hipError_t fmat_inliers(const double F[9], const float *pts1_h, const float *pts2_h, int m, double threshold,
                        unsigned char *mask_h, long long *count, ScratchCache &cache, hipStream_t st);
// mask_h NULL: every match; n_set: the non-zero bytes of mask_h (m without a mask), >= 8
hipError_t fmat_fit(const float *pts1_h, const float *pts2_h, const unsigned char *mask_h, int m, long long n_set, double F_out[9],
                    ScratchCache &cache, hipStream_t st);
hipError_t fmat_ransac(const float *pts1_h, const float *pts2_h, int m, double threshold, double confidence, int max_hypotheses,
                       uint64_t seed, double F_out[9], unsigned char *mask_h, long long *n_inliers, int info[3],
                       ScratchCache &cache, hipStream_t st);

}  // namespace amvs
