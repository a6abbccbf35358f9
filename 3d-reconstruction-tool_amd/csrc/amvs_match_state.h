// amvs_match_state.h -- what the dense-SIFT mode (include/amvs_match.h) keeps in a context, and the host interface of
// its kernels (amvs_match.hip, amvs_triangulate.hip).  Private to the library.
#pragma once
#include "amvs_buffer.h"

#include <hip/hip_runtime.h>

namespace amvs {

// one image's descriptors, resident: signed bytes in matrix-fragment order, padded to 32 rows (amvs_match.hip)
struct DescSlot {
    DeviceBuffer<uint4> frag;        // [n_pad / 32][4 steps][64 lanes] x 16 bytes
    DeviceBuffer<int> norm;          // [n_pad] sum of squares of the signed bytes (0 for padding)
    DeviceBuffer<unsigned> normk;    // [n_pad] 2^31 - (norm << 8) + 255 - (row & 255); 0 for padding
    int n = -1;                      // rows; -1: never set
};

// the cloud amvs_pair_triangulate appends to (grown by doubling, contents kept)
struct PairCloud {
    DeviceBuffer<double> pts;
    DeviceBuffer<unsigned char> rgb;
    long long n = 0;
    bool open = false;
};

// amvs_match.hip.  desc_set and desc_knn2_host / desc_match synchronise `st`; the caller has validated the parameters.
int desc_knn2_splits(int n_q, int n_t, int *chunks_per_split);
hipError_t desc_set(const unsigned char *desc_h, int n, ScratchCache &cache, DescSlot &slot, hipStream_t st);
// the same from [n][128] bytes already on the device, 16-byte aligned (amvs_sift_to_slot)
hipError_t desc_set_device(const unsigned char *desc_d, int n, ScratchCache &cache, DescSlot &slot, hipStream_t st);
hipError_t desc_knn2_host(const DescSlot &q, const DescSlot &t, ScratchCache &cache, int *idx_h, int *dist2_h, hipStream_t st);
hipError_t desc_match(const DescSlot &q, const DescSlot &t, float ratio, bool cross_check, ScratchCache &cache, int *q_idx_h,
                      int *t_idx_h, int *dist2_h, long long *n_matches, hipStream_t st);

// amvs_triangulate.hip.  The thresholds and matrices are the header's; all synchronise `st`.
struct PairThresholds { double depth_min, depth_max, cos_min_parallax, max_reproj; };
hipError_t pair_triangulate(const double K[9], const double R1[9], const double t1[3], const double R2[9], const double t2[3],
                            const float *pts1_h, const float *pts2_h, const unsigned char *rgb_h, int m, const PairThresholds &thr,
                            ScratchCache &cache, PairCloud &acc, long long *n_accepted, hipStream_t st);
// hipErrorInvalidValue: no kept point.  n_not_finite (optional): kept points with a coordinate that is not finite
hipError_t cloud_bounds(const double *pts, long long n, const unsigned char *keep_h, ScratchCache &cache, double mn[3], double mx[3],
                        hipStream_t st, long long *n_not_finite = nullptr);
hipError_t selftest_sqrt(const double *in_h, int n, double *out_h, ScratchCache &cache, hipStream_t st);

}  // namespace amvs
