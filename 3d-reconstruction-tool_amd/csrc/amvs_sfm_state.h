// amvs_sfm_state.h -- what the track state of include/amvs_sfm.h keeps in a context, and the host interface of its kernels
// (amvs_sfm.hip).  Private to the library.  The entry points (amvs_capi_sfm.hip) validate every parameter and decide on the
// host WHICH pairs a call walks (the registered flags live there); the kernels walk those pairs' rows.
#pragma once
#include "amvs_buffer.h"
#include "amvs_twoview_dev.h"

#include <hip/hip_runtime.h>

#include <vector>

namespace amvs {

struct SfmState {
    bool open = false;                    // a successful amvs_sfm_begin
    int V = 0, P = 0;
    long long G = 0, M = 0, n_points = 0;
    // host side: the layout, the pairs, which views are registered and their poses
    std::vector<int> off;                 // [V + 1]
    std::vector<int> pair_views;          // [P][2]
    std::vector<int> pair_start;          // [P + 1]
    std::vector<std::vector<int>> pairs_of;   // per view: its pairs, the other view ascending
    std::vector<char> registered;         // [V]
    std::vector<double> pose;             // [V][12]: R row-major, then t
    // device side
    DeviceBuffer<float2> kp;              // [G] pixels
    DeviceBuffer<int> kview;              // [G] the view of a keypoint
    DeviceBuffer<int2> rows;              // [M] the two GLOBAL keypoint indices of a row
    DeviceBuffer<int> owner;              // [G]
    DeviceBuffer<double> X;               // [capacity][3], n_points used
    DeviceBuffer<unsigned char> alive;    // [capacity]
};

// rows [row0, row0 + count) laid at position `first` of a call's walk; `side` is the column (0 / 1) of the keypoint that
// belongs to the REGISTERED view of the pair
struct SfmSeg { int row0, first, side; };

// the pair of one step of amvs_sfm_triangulate
struct SfmTriPair { int r, row0, count; double R1[9], t1[3], R2[9], t2[3], depth_max; };

// amvs_sfm.hip.  All synchronise `st` before they return; the caller has validated the parameters.
hipError_t sfm_upload(SfmState &s, const float *kp_h, const int *rows_h, ScratchCache &cache, hipStream_t st);
hipError_t sfm_register(SfmState &s, int view, const int *kp_h, const int *pid_h, int n, long long *n_set, ScratchCache &cache,
                        hipStream_t st);
// counts_h[V]: distinct keypoints per view the segments flag (the caller writes the -1 of the registered views)
hipError_t sfm_scores(SfmState &s, const std::vector<SfmSeg> &segs, int total, int *counts_h, ScratchCache &cache, hipStream_t st);
hipError_t sfm_correspondences(SfmState &s, int view, const std::vector<SfmSeg> &segs, int total, int *kp_h, int *pid_h, float *X_h,
                               float *x_h, long long *m, ScratchCache &cache, hipStream_t st);
// max_new: an upper bound of the points the call can make (the keypoints of its view)
hipError_t sfm_triangulate(SfmState &s, const double *K, const std::vector<SfmTriPair> &pairs, long long max_new, double depth_min,
                           double cos_max_parallax, double max_reproj, int *new_h, long long *n_new, ScratchCache &cache, hipStream_t st);
hipError_t sfm_counts(SfmState &s, long long *n_alive, long long *n_obs, ScratchCache &cache, hipStream_t st);
hipError_t sfm_observations(SfmState &s, int *cam_h, int *pt_h, float *uv_h, long long n_obs, ScratchCache &cache, hipStream_t st);
hipError_t sfm_points_get(SfmState &s, double *X_h, unsigned char *alive_h, hipStream_t st);     // X_h may be NULL: the flags alone
hipError_t sfm_points_set(SfmState &s, const double *X_h, const unsigned char *alive_h, ScratchCache &cache, hipStream_t st);
// keys_h: (pt << 12 | cam) ascending, distinct
hipError_t sfm_drop(SfmState &s, const long long *keys_h, int n, int min_obs, long long *obs_dropped, long long *points_dropped,
                    ScratchCache &cache, hipStream_t st);

}  // namespace amvs
