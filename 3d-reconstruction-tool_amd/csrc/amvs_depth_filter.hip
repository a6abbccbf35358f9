// amvs_depth_filter.hip -- the cross-view depth-map filter (include/amvs_depth.h amvs_depth_filter; the definition is the
// header's): per pixel the number of other maps whose own depth agrees after forward-backward reprojection, and the mean
// of the agreeing depths.  No reference counterpart: the reference's maps are never checked against each other.  Judged
// against tests/depth_filter_restatement.py, a statement of the header's definition in Python floats and integers
// (bit-identical depths, counts and totals).  It is not xpm_consistency_kernel (amvs_extended.hip), which belongs to the
// extended mode's state -- job table, cost test, float32 -- and returns a count only.
//
// depth_filter_kernel, one lane per pixel, x on consecutive lanes, grid-stride over the pixels of a map; blockIdx.y walks
// the maps.  The map j, its neighbour row and the neighbour i of every trip of the neighbour loop are the same for every
// lane of a wave, so K, K_inv (a by-value argument struct), the poses and the neighbour row (a constant device table
// indexed by uniform values) are scalar loads into scalar registers; what a lane keeps in vector registers is its pixel,
// its depth, one projection in flight and the two sums.  The loop itself is uniform: a lane whose centre pixel is invalid,
// or whose neighbour fails a guard, sits the trip out under the exec mask.  The one data-dependent access is the gather of
// map i at the projected pixel.
//
// The sums live in registers in the neighbour row's order: no atomics on floating-point data and no result that depends
// on arrival order.  The only atomics are the two integer totals, one 64-bit add per wave.
//
// -ffp-contract=off (Makefile): a * b + c below is two roundings, as the header says.
#define AMVS_TU_ID 17
#include "amvs_check.h"
#include "amvs_kernels.h"
#include "amvs_buffer.h"

#include <cfloat>
#include <cmath>

namespace amvs {

namespace {

// pixels of one map a launch covers in one trip of the grid-stride loop: FILTER_MAX_BLOCKS_X workgroups of 256 lanes
constexpr int FILTER_MAX_BLOCKS_X = 256;

struct FilterCamera {
    double K[9], Ki[9];
};

__device__ __forceinline__ bool pixel_valid(float d, float c, float min_conf)
{
    return d > 0.0f && d <= FLT_MAX && c >= min_conf;      // (NaN fails each)
}

// the sum of `v` over the wave's lanes (all 64 active), in lane 0
__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// pixel (x, y) at depth d of the camera with pose A (12 doubles), into the camera with pose B: steps 1 to 3 of the header
__device__ __forceinline__ void reproject(const double *__restrict__ Ki, const double *__restrict__ A,
                                          const double *__restrict__ B, double x, double y, double d, double out[3])
{
    double Q[3], Xw[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double r = (Ki[3 * c] * x + Ki[3 * c + 1] * y) + Ki[3 * c + 2];
        Q[c] = r * d - A[9 + c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) Xw[c] = (A[c] * Q[0] + A[3 + c] * Q[1]) + A[6 + c] * Q[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = ((B[3 * c] * Xw[0] + B[3 * c + 1] * Xw[1]) + B[3 * c + 2] * Xw[2]) + B[9 + c];
}

__global__ __launch_bounds__(256) void depth_filter_kernel(const float *__restrict__ depth, const float *__restrict__ conf,
                                                           int n_maps, int H, int W, const FilterCamera cam,
                                                           const double *__restrict__ poses, const int *__restrict__ nbr,
                                                           int n_nbr, float min_conf, double max_px2, double max_rel,
                                                           int min_consistent, int refine, float *__restrict__ depth_out,
                                                           float *__restrict__ count_out,
                                                           unsigned long long *__restrict__ totals)
{
    // 32-bit pixel indices: the caller holds n_maps * H * W below 2^31, and a lane's last index stays below HW + stride < 2^32
    const unsigned HW = (unsigned)H * (unsigned)W;
    const unsigned stride = gridDim.x * blockDim.x;
    const unsigned first = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned rounds = (HW + stride - 1) / stride;          // the same for every lane: the wave stays whole
    [[maybe_unused]] const long long n = (long long)n_maps * HW;      // (the extent the index-checked build compares with)
    int n_valid = 0, n_kept = 0;
    for (int j = (int)blockIdx.y; j < n_maps; j += (int)gridDim.y) {
        const double *Pj = poses + 12 * (long long)j;
        const int *row = nbr + (long long)j * n_nbr;
        const size_t base = (size_t)j * HW;
        for (unsigned it = 0; it < rounds; ++it) {
            const unsigned p = first + it * stride;
            if (p >= HW) continue;
            const int y0 = (int)(p / (unsigned)W), x0 = (int)(p - (unsigned)y0 * (unsigned)W);
            const float df = depth[base + p];
            const bool valid = pixel_valid(df, conf[base + p], min_conf);
            const double d = (double)df, x = (double)x0, y = (double)y0;
            const double lim = max_rel * d;
            int cnt = 0;
            double s = d;
            for (int k = 0; k < n_nbr; ++k) {
                const int i = row[k];                                                  // (uniform: a scalar load)
                if (i < 0) continue;
                const double *Pi = poses + 12 * (long long)AMVS_IDX(i, n_maps);        // (pose of the neighbour map)
                if (!valid) continue;
                double Xi[3], uvw[3];
                reproject(cam.Ki, Pj, Pi, x, y, d, Xi);
                if (!(Xi[2] > 0.0)) continue;
#pragma unroll
                for (int c = 0; c < 3; ++c) uvw[c] = (cam.K[3 * c] * Xi[0] + cam.K[3 * c + 1] * Xi[1]) + cam.K[3 * c + 2] * Xi[2];
                if (!(uvw[2] > 0.0)) continue;
                const double px = floor(uvw[0] / uvw[2] + 0.5), py = floor(uvw[1] / uvw[2] + 0.5);
                if (!(px >= 0.0 && px < (double)W && py >= 0.0 && py < (double)H)) continue;   // (NaN fails; before any conversion)
                const long long g = AMVS_IDX((long long)i * HW + (long long)py * W + (long long)px, n);   // (the gather of map i)
                const float dif = depth[g];
                if (!pixel_valid(dif, conf[g], min_conf)) continue;
                double Y[3];
                reproject(cam.Ki, Pi, Pj, px, py, (double)dif, Y);
                if (!(Y[2] > 0.0)) continue;
#pragma unroll
                for (int c = 0; c < 3; ++c) uvw[c] = (cam.K[3 * c] * Y[0] + cam.K[3 * c + 1] * Y[1]) + cam.K[3 * c + 2] * Y[2];
                if (!(uvw[2] > 0.0)) continue;
                const double eu = uvw[0] / uvw[2] - x, ev = uvw[1] / uvw[2] - y;
                const double e2 = eu * eu + ev * ev;
                if (!(e2 <= max_px2 && fabs(Y[2] - d) <= lim)) continue;
                ++cnt;
                s = s + Y[2];
            }
            const bool keep = valid && cnt >= min_consistent;
            n_valid += valid ? 1 : 0;
            n_kept += keep ? 1 : 0;
            count_out[base + p] = (float)cnt;
            depth_out[base + p] = !keep ? 0.0f : (refine ? (float)(s / (double)(cnt + 1)) : df);
        }
    }
    const int tv = wave_sum(n_valid), tk = wave_sum(n_kept);
    if ((threadIdx.x & 63) == 0) {
        if (tv) atomicAdd(totals, (unsigned long long)tv);
        if (tk) atomicAdd(totals + 1, (unsigned long long)tk);
    }
}

}  // namespace

hipError_t depth_filter(const float *depth, const float *conf, int n_maps, int H, int W, const double *K_h, const double *Ki_h,
                        const double *poses_h, const int *nbr_h, int n_nbr, float min_confidence, float max_px, float max_rel,
                        int min_consistent, bool refine, ScratchCache &cache, float *depth_out, float *count_out,
                        long long counts[2], hipStream_t st)
{
    counts[0] = counts[1] = 0;
    const long long hw = (long long)H * W, n = (long long)n_maps * hw;
    if (n <= 0 || n > 0x7FFFFFFFll || n_nbr < 0) return hipErrorInvalidValue;
    // the poses, two zeroed totals and the neighbour rows on the device: [12 n_maps doubles][2 x uint64][n_maps n_nbr int32]
    const size_t nd = 12 * (size_t)n_maps, ni = (size_t)n_maps * (size_t)n_nbr;
    ScratchCache::Lease consts;
    STCHK(cache.lease(consts, sizeof(double) * nd + 16 + sizeof(int) * ni));
    double *d_poses = consts.get<double>();
    unsigned long long *totals = (unsigned long long *)(d_poses + nd);
    int *d_nbr = (int *)(totals + 2);
    STCHK(hipMemcpyAsync(d_poses, poses_h, sizeof(double) * nd, hipMemcpyHostToDevice, st));
    STCHK(hipMemsetAsync(totals, 0, 16, st));
    if (ni) STCHK(hipMemcpyAsync(d_nbr, nbr_h, sizeof(int) * ni, hipMemcpyHostToDevice, st));
    FilterCamera cam;
    for (int k = 0; k < 9; ++k) { cam.K[k] = K_h[k]; cam.Ki[k] = Ki_h[k]; }
    // at most FILTER_MAX_BLOCKS_X workgroups along a map (an image above 65 536 pixels walks the grid-stride loop) and
    // at most 65 535 maps along y (more walk the map loop)
    long long bx = (hw + 255) / 256;
    if (bx > FILTER_MAX_BLOCKS_X) bx = FILTER_MAX_BLOCKS_X;
    const int by = n_maps < 65535 ? n_maps : 65535;
    hipLaunchKernelGGL(depth_filter_kernel, dim3((unsigned)bx, (unsigned)by), dim3(256), 0, st, depth, conf, n_maps, H, W, cam,
                       (const double *)d_poses, (const int *)d_nbr, n_nbr, min_confidence, (double)max_px * (double)max_px,
                       (double)max_rel, min_consistent, refine ? 1 : 0, depth_out, count_out, totals);
    STCHK(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    STCHK(hipMemcpyAsync(h, totals, 16, hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
    counts[0] = (long long)h[0]; counts[1] = (long long)h[1];
    return hipSuccess;
}

}  // namespace amvs

AMVS_CHECK_TU(depth_filter)
