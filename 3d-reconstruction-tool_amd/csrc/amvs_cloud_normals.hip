// amvs_cloud_normals.hip -- oriented normals for the dense cloud, fitted from the depth maps (include/amvs.h
// amvs_depth_normals, amvs_cloud_normals; the definition is the header's).  No reference counterpart: the reference's
// cloud has no normals, and the normal maps its PatchMatch returns are never read by its cost.  Judged against
// tests/cloud_normals_restatement.py, a statement of the header's definition in Python floats and integers (bit-identical
// normal maps, cloud normals, seen counts and counts).
//
// depth_normal_kernel, one lane per pixel of the stacked maps, x on consecutive lanes, grid-stride.  The plain version:
// every lane reads its (2r+1)^2 window from global memory.  The lanes of a wave hold 64 consecutive pixels of a row, so
// one row of the window is 64 + 2r consecutive floats -- two or three 128-byte lines for the whole wave -- and the rows
// above and below were read by the waves of those rows a moment ago: the window is served by the vector L1 and the L2,
// and the compulsory traffic stays the 8 B a pixel of the two maps plus the 12 B written.  The sums are exact integers
// (32-bit: at most 81 terms of at most 16; so are the pixel indices, the stacked maps holding fewer than 2^31 pixels) and three float64 accumulators in the header's walk order; the determinant
// and the adjugate are 64-bit integers (below 2^40), converted exactly where they meet a float64.
//
// cloud_normal_kernel, one lane per point: the maps in ascending order, the weighted sum in three registers.  No atomics
// on floating-point data and no result that depends on arrival order.  The only atomics are the integer counts, one
// 64-bit add per wave.
//
// -ffp-contract=off (Makefile): a * b + c below is two roundings, as the header says.
#define AMVS_TU_ID 16
#include "amvs_check.h"
#include "amvs_kernels.h"
#include "amvs_buffer.h"

#include <cfloat>
#include <cmath>

namespace amvs {

namespace {

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

__global__ __launch_bounds__(256) void depth_normal_kernel(const float *__restrict__ depth, const float *__restrict__ conf,
                                                           int n_maps, int H, int W, const double *__restrict__ K,
                                                           const double *__restrict__ poses, float min_conf, int radius,
                                                           float jump, int min_points, int world, float *__restrict__ nrm,
                                                           unsigned long long *__restrict__ n_normals)
{
    // 32-bit pixel indices: the caller holds n_maps * H * W below 2^31, and a lane's last index stays below n + stride < 2^32
    const unsigned HW = (unsigned)H * (unsigned)W, n = (unsigned)n_maps * HW;
    const unsigned stride = gridDim.x * blockDim.x;
    const unsigned first = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned rounds = (n + stride - 1) / stride;           // the same for every lane: the wave stays whole
    int have = 0;
    for (unsigned it = 0; it < rounds; ++it) {
        const unsigned i = first + it * stride;
        if (i >= n) continue;
        const int map = (int)(i / HW);
        const unsigned p = i - (unsigned)map * HW;
        const int y0 = (int)(p / (unsigned)W), x0 = (int)(p - (unsigned)y0 * (unsigned)W);
        float out[3] = {0.0f, 0.0f, 0.0f};
        const float dcf = depth[i];
        if (pixel_valid(dcf, conf[i], min_conf)) {
            const double dc = (double)dcf, lim = (double)jump * dc;
            int cnt = 0, sx = 0, sy = 0, sxx = 0, sxy = 0, syy = 0;
            double Sq = 0.0, Sxq = 0.0, Syq = 0.0;
            for (int dy = -radius; dy <= radius; ++dy) {
                const int y = y0 + dy;
                if (y < 0 || y >= H) continue;
                for (int dx = -radius; dx <= radius; ++dx) {
                    const int x = x0 + dx;
                    if (x < 0 || x >= W) continue;
                    const int q = AMVS_IDX((int)i + dy * W + dx, n);                   // (window pixel of the same map)
                    const float dnf = depth[q];
                    if (!pixel_valid(dnf, conf[q], min_conf)) continue;
                    if (!(fabs((double)dnf - dc) <= lim)) continue;
                    const double qq = 1.0 / (double)dnf;
                    ++cnt; sx += dx; sy += dy; sxx += dx * dx; sxy += dx * dy; syy += dy * dy;
                    Sq = Sq + qq;
                    Sxq = Sxq + (double)dx * qq;
                    Syq = Syq + (double)dy * qq;
                }
            }
            // M = [[sxx, sxy, sx], [sxy, syy, sy], [sx, sy, n]]: adjugate and determinant
            const long long A = sxx, B = sxy, C = sx, D = syy, E = sy, F = cnt;
            const long long C00 = D * F - E * E, C01 = C * E - B * F, C02 = B * E - C * D;
            const long long C11 = A * F - C * C, C12 = B * C - A * E, C22 = A * D - B * B;
            const long long det = A * C00 + B * C01 + C * C02;
            if (cnt >= min_points && det != 0) {
                const double a = ((double)C00 * Sxq + (double)C01 * Syq) + (double)C02 * Sq;
                const double b = ((double)C01 * Sxq + (double)C11 * Syq) + (double)C12 * Sq;
                const double c = ((double)C02 * Sxq + (double)C12 * Syq) + (double)C22 * Sq;
                if (c > 0.0) {
                    const double cp = (c - a * (double)x0) - b * (double)y0;
                    double m[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) m[k] = (K[k] * a + K[3 + k] * b) + K[6 + k] * cp;
                    const double len = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
                    if (len > 0.0 && len <= DBL_MAX) {
                        double v[3] = {-m[0] / len, -m[1] / len, -m[2] / len};
                        if (world) {
                            const double *R = poses + 12 * (long long)AMVS_IDX(map, n_maps);      // (pose of the pixel's map)
                            const double w0 = (R[0] * v[0] + R[3] * v[1]) + R[6] * v[2];
                            const double w1 = (R[1] * v[0] + R[4] * v[1]) + R[7] * v[2];
                            const double w2 = (R[2] * v[0] + R[5] * v[1]) + R[8] * v[2];
                            v[0] = w0; v[1] = w1; v[2] = w2;
                        }
                        out[0] = (float)v[0]; out[1] = (float)v[1]; out[2] = (float)v[2];
                        ++have;
                    }
                }
            }
        }
        float *o = nrm + 3 * (size_t)i;
        o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
    }
    const int total = wave_sum(have);
    if ((threadIdx.x & 63) == 0 && total) atomicAdd(n_normals, (unsigned long long)total);
}

__global__ __launch_bounds__(256) void cloud_normal_kernel(const double *__restrict__ pts, long long n_pts,
                                                           const float *__restrict__ depth, const float *__restrict__ nrm_maps,
                                                           int n_maps, int H, int W, const double *__restrict__ K,
                                                           const double *__restrict__ poses, float depth_tolerance, int min_views,
                                                           float *__restrict__ nrm_out, int *__restrict__ seen_out,
                                                           unsigned long long *__restrict__ n_normals)
{
    const long long HW = (long long)H * W;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int have = 0;
    if (i < n_pts) {
        const double X0 = pts[3 * i], X1 = pts[3 * i + 1], X2 = pts[3 * i + 2];
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        int seen = 0;
        for (int j = 0; j < n_maps; ++j) {
            const double *R = poses + 12 * (long long)AMVS_IDX(j, n_maps), *t = R + 9;      // (pose of map j)
            double Xc[3], uvw[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) Xc[k] = ((R[3 * k] * X0 + R[3 * k + 1] * X1) + R[3 * k + 2] * X2) + t[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) uvw[k] = (K[3 * k] * Xc[0] + K[3 * k + 1] * Xc[1]) + K[3 * k + 2] * Xc[2];
            if (!(uvw[2] > 0.0 && Xc[2] > 0.0)) continue;
            const double px = floor(uvw[0] / uvw[2] + 0.5), py = floor(uvw[1] / uvw[2] + 0.5);
            if (!(px >= 0.0 && px < (double)W && py >= 0.0 && py < (double)H)) continue;      // (NaN fails; before any conversion)
            const long long g = AMVS_IDX((long long)j * HW + (long long)py * W + (long long)px, (long long)n_maps * HW);
            const double n0 = (double)nrm_maps[3 * g], n1 = (double)nrm_maps[3 * g + 1], n2 = (double)nrm_maps[3 * g + 2];
            if (!(n0 != 0.0 || n1 != 0.0 || n2 != 0.0)) continue;
            const double d = (double)depth[g];
            if (!(fabs(d - Xc[2]) <= (double)depth_tolerance * d)) continue;
            double nc[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) nc[k] = (R[3 * k] * n0 + R[3 * k + 1] * n1) + R[3 * k + 2] * n2;
            const double w = -((nc[0] * Xc[0] + nc[1] * Xc[1]) + nc[2] * Xc[2])
                             / sqrt((Xc[0] * Xc[0] + Xc[1] * Xc[1]) + Xc[2] * Xc[2]);
            if (!(w > 0.0)) continue;
            s0 = s0 + w * n0; s1 = s1 + w * n1; s2 = s2 + w * n2;
            ++seen;
        }
        const double L = sqrt((s0 * s0 + s1 * s1) + s2 * s2);
        float out[3] = {0.0f, 0.0f, 0.0f};
        if (seen >= min_views && L > 0.0) {
            out[0] = (float)(s0 / L); out[1] = (float)(s1 / L); out[2] = (float)(s2 / L);
            have = 1;
        }
        nrm_out[3 * i] = out[0]; nrm_out[3 * i + 1] = out[1]; nrm_out[3 * i + 2] = out[2];
        seen_out[i] = seen;
    }
    const int total = wave_sum(have);
    if ((threadIdx.x & 63) == 0 && total) atomicAdd(n_normals, (unsigned long long)total);
}

// K and the poses on the device, and two zeroed counters behind them: [9 + 12 n_maps doubles][2 x uint64]
hipError_t stage_constants(ScratchCache &cache, ScratchCache::Lease &consts, int n_maps, const double *K_h, const double *poses_h,
                           hipStream_t st)
{
    const size_t nd = 9 + 12 * (size_t)n_maps;
    STCHK(cache.lease(consts, sizeof(double) * nd + 16));
    double *d = consts.get<double>();
    STCHK(hipMemcpyAsync(d, K_h, sizeof(double) * 9, hipMemcpyHostToDevice, st));
    STCHK(hipMemcpyAsync(d + 9, poses_h, sizeof(double) * 12 * (size_t)n_maps, hipMemcpyHostToDevice, st));
    STCHK(hipMemsetAsync(d + nd, 0, 16, st));
    return hipSuccess;
}

void launch_fit(const float *depth, const float *conf, int n_maps, int H, int W, const double *d_consts, float min_confidence,
                int radius, float jump, int min_points, bool world, float *nrm, unsigned long long *counter, hipStream_t st)
{
    // at most 2048 workgroups (8 per CU), and at least two pixels a lane: every input above one workgroup walks the
    // grid-stride loop, with a ragged last round
    const long long n = (long long)n_maps * H * W;
    long long blocks = ((n + 255) / 256 + 1) / 2;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(depth_normal_kernel, dim3((unsigned)blocks), dim3(256), 0, st, depth, conf, n_maps, H, W, d_consts,
                       d_consts + 9, min_confidence, radius, jump, min_points, world ? 1 : 0, nrm, counter);
}

}  // namespace

hipError_t depth_normals(const float *depth, const float *conf, int n_maps, int H, int W, const double *K_h, const double *poses_h,
                         float min_confidence, int radius, float jump, int min_points, bool world, ScratchCache &cache,
                         DeviceBuffer<float> &normals, long long *n_normals, hipStream_t st)
{
    *n_normals = 0;
    const long long n = (long long)n_maps * H * W;
    if (n <= 0 || n > 0x7FFFFFFFll) return hipErrorInvalidValue;
    ScratchCache::Lease consts;
    STCHK(stage_constants(cache, consts, n_maps, K_h, poses_h, st));
    STCHK(normals.reserve(3 * (size_t)n, cache));
    unsigned long long *counters = (unsigned long long *)(consts.get<double>() + 9 + 12 * (size_t)n_maps);
    launch_fit(depth, conf, n_maps, H, W, consts.get<double>(), min_confidence, radius, jump, min_points, world, normals.get(),
               counters, st);
    STCHK(hipGetLastError());
    unsigned long long h = 0;
    STCHK(hipMemcpyAsync(&h, counters, 8, hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
    *n_normals = (long long)h;
    return hipSuccess;
}

hipError_t cloud_normals(const double *pts, long long n_pts, const float *depth, const float *conf, int n_maps, int H, int W,
                         const double *K_h, const double *poses_h, float min_confidence, int radius, float jump, int min_points,
                         float depth_tolerance, int min_views, ScratchCache &cache, DeviceBuffer<float> &map_normals,
                         DeviceBuffer<float> &nrm_out, DeviceBuffer<int> &seen_out, long long counts[2], hipStream_t st)
{
    counts[0] = counts[1] = 0;
    const long long n = (long long)n_maps * H * W;
    if (n <= 0 || n > 0x7FFFFFFFll || n_pts <= 0 || n_pts > 0x7FFFFFFFll) return hipErrorInvalidValue;
    ScratchCache::Lease consts;
    STCHK(stage_constants(cache, consts, n_maps, K_h, poses_h, st));
    STCHK(map_normals.reserve(3 * (size_t)n, cache));
    STCHK(nrm_out.reserve(3 * (size_t)n_pts, cache));
    STCHK(seen_out.reserve((size_t)n_pts, cache));
    const double *d_consts = consts.get<double>();
    unsigned long long *counters = (unsigned long long *)(consts.get<double>() + 9 + 12 * (size_t)n_maps);
    launch_fit(depth, conf, n_maps, H, W, d_consts, min_confidence, radius, jump, min_points, true, map_normals.get(), counters, st);
    STCHK(hipGetLastError());
    hipLaunchKernelGGL(cloud_normal_kernel, dim3((unsigned)((n_pts + 255) / 256)), dim3(256), 0, st, pts, n_pts, depth,
                       (const float *)map_normals.get(), n_maps, H, W, d_consts, d_consts + 9, depth_tolerance, min_views,
                       nrm_out.get(), seen_out.get(), counters + 1);
    STCHK(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    STCHK(hipMemcpyAsync(h, counters, 16, hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
    counts[0] = (long long)h[0]; counts[1] = (long long)h[1];
    return hipSuccess;
}

}  // namespace amvs

AMVS_CHECK_TU(cloud_normals)
