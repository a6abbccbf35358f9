// amvs_undistort.hip -- lens undistortion of one raw 8-bit BGR image at its own resolution (include/amvs_lens.h; the
// definition is the header's).  The reference's loader calls cv.undistort on the CPU before the dense stage sees an image;
// OpenCV is not a dependency here, so the header states the arithmetic (modelled on cv.undistort: a float64 map, 5-bit
// fractions, zero outside) and this file is judged against tests/undistort_restatement.py, byte for byte; parity with cv2
// itself is UNPINNED.
//
// undistort_bgr8_kernel: one lane per destination pixel.  A workgroup is a tile of 64 x 4 pixels -- a wave is 64
// consecutive pixels of one row, the four waves are four neighbouring rows, whose taps hit the same or adjacent source
// lines -- and walks the tiles in row-major order with a grid stride.  The map is about 35 float64 operations and one
// division per pixel; the gather is 12 byte loads (4 taps x 3 channels) that neighbouring lanes share cache lines for,
// the result 3 byte stores.  OUTSIDE pixels are counted per wave (ballot + popcount, in a register across the trips)
// and added once per wave to a 64-bit counter.
//
// -ffp-contract=off (Makefile): a * b + c below is two roundings, as the header says.
#define AMVS_TU_ID 18
#include "amvs_check.h"
#include "amvs_kernels.h"

namespace amvs {

namespace {

// workgroups of a launch at most (as launch_prep_bgr8): an image of more tiles walks the grid-stride loop
constexpr long long UNDISTORT_MAX_BLOCKS = 8192;
constexpr int TILE_W = 64, TILE_H = 4;

struct LensArgs {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6;
};

__global__ __launch_bounds__(256) void undistort_bgr8_kernel(const unsigned char *__restrict__ src, int h, int w,
                                                             const LensArgs a, unsigned char *__restrict__ dst,
                                                             unsigned long long *__restrict__ n_outside)
{
    const int lx = (int)(threadIdx.x & 63u), ly = (int)(threadIdx.x >> 6);
    const long long tiles_x = (w + TILE_W - 1) / TILE_W, n_tiles = tiles_x * ((h + TILE_H - 1) / TILE_H);
    [[maybe_unused]] const long long n = (long long)h * w;      // (the extent the index-checked build compares with)
    const double u_end = 32.0 * (double)w, v_end = 32.0 * (double)h;
    unsigned long long outside_seen = 0;                        // of this wave: the same in every lane
    // (the trip count is the same for every lane of a workgroup: the waves stay whole for the ballot)
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long ty = tile / tiles_x;
        const int i = (int)ty * TILE_H + ly, j = (int)(tile - ty * tiles_x) * TILE_W + lx;
        const bool live = i < h && j < w;
        bool outside = false;
        if (live) {
            const double x = ((double)j - a.cx) / a.fx, y = ((double)i - a.cy) / a.fy;
            const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = (2.0 * x) * y;
            const double num = 1.0 + ((a.k3 * r2 + a.k2) * r2 + a.k1) * r2;
            const double den = 1.0 + ((a.k6 * r2 + a.k5) * r2 + a.k4) * r2;
            const double kr = num / den;
            const double xd = (x * kr + a.p1 * xy2) + a.p2 * (r2 + 2.0 * x2);
            const double yd = (y * kr + a.p1 * (r2 + 2.0 * y2)) + a.p2 * xy2;
            const double u = a.fx * xd + a.cx, v = a.fy * yd + a.cy;
            const double fu = rint(u * 32.0), fv = rint(v * 32.0);
            outside = !(fu >= -32.0 && fu < u_end && fv >= -32.0 && fv < v_end);     // (NaN and +-inf fail; before any conversion)
            unsigned acc[3] = {0u, 0u, 0u};
            if (!outside) {
                const int iu = (int)fu, iv = (int)fv;
                const int sx = iu >> 5, sy = iv >> 5;              // -1 .. w - 1, -1 .. h - 1
                const unsigned ax = (unsigned)(iu & 31), ay = (unsigned)(iv & 31);
                const bool x0 = sx >= 0, x1 = sx + 1 < w, y0 = sy >= 0, y1 = sy + 1 < h;
                const long long p00 = (long long)sy * w + sx;
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = 512u;
                if (x0 && y0) {
                    const unsigned char *p = src + 3 * AMVS_IDX(p00, n);
                    const unsigned wt = (32u - ax) * (32u - ay);
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c] += wt * p[c];
                }
                if (x1 && y0) {
                    const unsigned char *p = src + 3 * AMVS_IDX(p00 + 1, n);
                    const unsigned wt = ax * (32u - ay);
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c] += wt * p[c];
                }
                if (x0 && y1) {
                    const unsigned char *p = src + 3 * AMVS_IDX(p00 + w, n);
                    const unsigned wt = (32u - ax) * ay;
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c] += wt * p[c];
                }
                if (x1 && y1) {
                    const unsigned char *p = src + 3 * AMVS_IDX(p00 + w + 1, n);
                    const unsigned wt = ax * ay;
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c] += wt * p[c];
                }
            }
            unsigned char *q = dst + 3 * AMVS_IDX((long long)i * w + j, n);
#pragma unroll
            for (int c = 0; c < 3; ++c) q[c] = (unsigned char)(acc[c] >> 10);
        }
        outside_seen += (unsigned long long)__popcll(__ballot(live && outside));
    }
    if (n_outside && lx == 0 && outside_seen) atomicAdd(n_outside, outside_seen);
}

}  // namespace

hipError_t launch_undistort_bgr8(const unsigned char *src, int h, int w, const double K[9], const double dist8[8],
                                 unsigned char *dst, unsigned long long *n_outside, hipStream_t st)
{
    const LensArgs a{K[0], K[4], K[2], K[5], dist8[0], dist8[1], dist8[2], dist8[3], dist8[4], dist8[5], dist8[6], dist8[7]};
    const long long n_tiles = (long long)((w + TILE_W - 1) / TILE_W) * ((h + TILE_H - 1) / TILE_H);
    const unsigned blocks = (unsigned)(n_tiles < UNDISTORT_MAX_BLOCKS ? n_tiles : UNDISTORT_MAX_BLOCKS);
    hipLaunchKernelGGL(undistort_bgr8_kernel, dim3(blocks), dim3(TILE_W * TILE_H), 0, st, src, h, w, a, dst, n_outside);
    return hipGetLastError();
}

}  // namespace amvs

AMVS_CHECK_TU(undistort)
