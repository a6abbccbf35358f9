// amvs_twoview_dev.h -- the host interface of the two-view kernels (amvs_twoview.hip; include/amvs_twoview.h).  Private to
// the library.  Every function takes host arrays, runs on `st` with scratch from `cache`, synchronises `st` before it
// returns; the caller has validated the parameters.  K is the header's double[9]; R is [9] and t [3] per pose.
#pragma once
#include "amvs_buffer.h"

#include <hip/hip_runtime.h>

namespace amvs {

struct TwoviewThresholds { double depth_min, depth_max, cos_max_parallax, max_reproj; };

hipError_t twoview_score(const double *R_h, const double *t_h, int n, const float *pts1_h, const float *pts2_h, int m, const double *K,
                         double max_depth, int *counts_h, ScratchCache &cache, hipStream_t st);
hipError_t twoview_front(const double R[9], const double t[3], const float *pts1_h, const float *pts2_h, int m, const double *K,
                         double max_depth, unsigned char *mask_h, long long *count, ScratchCache &cache, hipStream_t st);
// info = [best index, the four counts]; *model false: no model, every output zero
hipError_t twoview_pose(const double F[9], const double *K, const float *pts1_h, const float *pts2_h, int m, double max_depth,
                        double R_out[9], double t_out[3], unsigned char *mask_h, long long *n_front, int info[5], bool *model,
                        ScratchCache &cache, hipStream_t st);
hipError_t twoview_triangulate(const double *K, const double R1[9], const double t1[3], const double R2[9], const double t2[3],
                               const float *pts1_h, const float *pts2_h, int m, const TwoviewThresholds &thr, double *X_h,
                               unsigned char *valid_h, double *cos_h, long long *n_valid, ScratchCache &cache, hipStream_t st);

}  // namespace amvs
