// amvs_features_state.h -- what the feature stages (include/amvs_features.h) keep in a context, and the host interface
// of their kernels (amvs_clahe.hip, amvs_sift.hip).  Private to the library.
#pragma once
#include "amvs_buffer.h"
#include "amvs_sift_math.h"

#include <hip/hip_runtime.h>

namespace amvs {

constexpr int SIFT_GAUSS = 6, SIFT_DOG = 5, SIFT_LAYERS = 3, SIFT_MAX_OCTAVES = 16;

// the result of the last amvs_clahe_u8, resident for amvs_sift_scale_space
struct ClaheState {
    DeviceBuffer<unsigned char> out;     // [h][w]
    int h = 0, w = 0;                    // 0: none
};

// the scale space of the last amvs_sift_scale_space: octave o holds SIFT_GAUSS images at gauss + g_off[o] and SIFT_DOG
// images at dog + d_off[o], each [h[o]][w[o]]
struct SiftState {
    DeviceBuffer<float> gauss, dog;
    int n_octaves = 0;                   // 0: none
    int h[SIFT_MAX_OCTAVES] = {}, w[SIFT_MAX_OCTAVES] = {};
    size_t g_off[SIFT_MAX_OCTAVES] = {}, d_off[SIFT_MAX_OCTAVES] = {};
    // the keypoints of the last amvs_sift_extract, in the canonical order
    DeviceBuffer<float> kp;              // [n_kp][6]
    DeviceBuffer<uint4> desc;            // [n_kp][128] bytes
    int n_kp = -1;                       // -1: none
};

// the scale space as the keypoint kernels see it, by value in their argument block
struct SiftPyramid {
    const float *gauss, *dog;
    int n_octaves;
    int h[SIFT_MAX_OCTAVES], w[SIFT_MAX_OCTAVES];
    unsigned long long g_off[SIFT_MAX_OCTAVES], d_off[SIFT_MAX_OCTAVES];
};

struct SiftParams { float pre_threshold, contrast_threshold, edge_threshold, sigma; };

// amvs_clahe.hip.  The image is on the device already; lut is [grid_y * grid_x][256]; nothing synchronises.
hipError_t launch_clahe_luts(const unsigned char *gray, int h, int w, int grid_x, int grid_y, int limit, unsigned char *lut,
                             hipStream_t st);
hipError_t launch_clahe_apply(const unsigned char *gray, int h, int w, int grid_x, int grid_y, const unsigned char *lut,
                              unsigned char *out, hipStream_t st);

// amvs_sift.hip.  Nothing synchronises.
hipError_t launch_sift_upsample(const unsigned char *gray, int h, int w, float *up, hipStream_t st);
// out = blur of in (tmp: an image of the same size for the row pass); with prev, also dog = out - prev
hipError_t launch_sift_blur(const float *in, int h, int w, const GaussTaps &taps, float *tmp, float *out, const float *prev,
                            float *dog, hipStream_t st);
hipError_t launch_sift_halve(const float *in, int h, int w, float *out, hipStream_t st);

// amvs_sift_keypoints.hip: extrema, refinement, orientations, canonical order, selection of the n_features strongest
// (0: all) and descriptors of a resident scale space, into s.kp / s.desc / s.n_kp.  Synchronises.  *too_many: more than
// max_features keypoints before the selection (nothing is stored then).
hipError_t sift_keypoints(SiftState &s, const SiftParams &prm, int n_features, int max_features, ScratchCache &cache,
                          bool *too_many, hipStream_t st);

}  // namespace amvs
