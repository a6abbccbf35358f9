// amvs_triangulate.hip -- two-view DLT triangulation with the depth, parallax and reprojection filters, appended to an
// accumulating cloud in candidate order; the per-axis bounds of a cloud; the float64 square root for the tests
// (include/amvs_match.h; the definition is the header's, the judge tests/match_restatement.py, bit for bit).
//
// pair_triangulate_kernel: one lane per candidate, float64 throughout, M and V of the Jacobi iteration in registers
// (amvs_dlt4.h, shared with amvs_twoview.hip).  The projection matrices and camera centres
// are formed once on the host in the order the header writes.  The accepted candidates are selected in order
// (hipCUB) and gathered behind the points the cloud holds already.
//
// -ffp-contract=off (Makefile): a * b + c below is two roundings, on the device and on the host.
#define AMVS_TU_ID 20
#include "amvs_check.h"
#include "amvs_dlt4.h"
#include "amvs_kernels.h"
#include "amvs_match_state.h"
#include "../../include/amvs_match.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <vector>

namespace amvs {

namespace {

inline dim3 grid_for(long long n) { long long b = (n + 255) / 256; return dim3((unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b))); }

struct PairArgs {
    double P1[12], P2[12], C1[3], C2[3], R1[9], t1[3], R2[9], t2[3], K[9];
    PairThresholds thr;
};

__device__ __forceinline__ void cam_point(const double R[9], const double t[3], const double X[3], double pc[3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) pc[r] = ((R[3 * r] * X[0] + R[3 * r + 1] * X[1]) + R[3 * r + 2] * X[2]) + t[r];
}

__device__ __forceinline__ double reproj_error(const double K[9], const double pc[3], double x, double y)
{
    double h[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) h[r] = (K[3 * r] * pc[0] + K[3 * r + 1] * pc[1]) + K[3 * r + 2] * pc[2];
    const double du = h[0] / h[2] - x, dv = h[1] / h[2] - y;
    return sqrt(du * du + dv * dv);
}

__global__ __launch_bounds__(256) void pair_triangulate_kernel(const PairArgs a, const float *__restrict__ pts1,
                                                               const float *__restrict__ pts2, int m, double *__restrict__ X_out,
                                                               unsigned char *__restrict__ flag)
{
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < m; i += (int)(gridDim.x * blockDim.x)) {
        const double x1 = (double)pts1[2 * i], y1 = (double)pts1[2 * i + 1];
        const double x2 = (double)pts2[2 * i], y2 = (double)pts2[2 * i + 1];
        double v[4];
        dlt4_null_vector(a.P1, a.P2, x1, y1, x2, y2, v);
        const double X[3] = {v[0] / v[3], v[1] / v[3], v[2] / v[3]};
        double pc1[3], pc2[3];
        cam_point(a.R1, a.t1, X, pc1);
        cam_point(a.R2, a.t2, X, pc2);
        bool keep = pc1[2] > a.thr.depth_min && pc1[2] < a.thr.depth_max && pc2[2] > a.thr.depth_min && pc2[2] < a.thr.depth_max;
        if (keep) {
            const double w1[3] = {X[0] - a.C1[0], X[1] - a.C1[1], X[2] - a.C1[2]};
            const double w2[3] = {X[0] - a.C2[0], X[1] - a.C2[1], X[2] - a.C2[2]};
            const double dot = (w1[0] * w2[0] + w1[1] * w2[1]) + w1[2] * w2[2];
            const double n1 = sqrt((w1[0] * w1[0] + w1[1] * w1[1]) + w1[2] * w1[2]);
            const double n2 = sqrt((w2[0] * w2[0] + w2[1] * w2[1]) + w2[2] * w2[2]);
            const double cs = dot / (n1 * n2 + 1e-8);
            keep = cs < a.thr.cos_min_parallax;
        }
        if (keep) keep = reproj_error(a.K, pc1, x1, y1) < a.thr.max_reproj && reproj_error(a.K, pc2, x2, y2) < a.thr.max_reproj;
        X_out[3 * (size_t)i] = X[0];
        X_out[3 * (size_t)i + 1] = X[1];
        X_out[3 * (size_t)i + 2] = X[2];
        flag[i] = keep ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void pair_append_kernel(const int *__restrict__ sel, int k_n, int m, const double *__restrict__ X,
                                                          const unsigned char *__restrict__ rgb, double *__restrict__ pts_out,
                                                          unsigned char *__restrict__ rgb_out)
{
    for (int k = (int)(blockIdx.x * blockDim.x + threadIdx.x); k < k_n; k += (int)(gridDim.x * blockDim.x)) {
        const int i = AMVS_IDX(sel[k], m);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            pts_out[3 * (size_t)k + j] = X[3 * (size_t)i + j];
            rgb_out[3 * (size_t)k + j] = rgb[3 * (size_t)i + j];
        }
    }
}

// the header's order of two equal zeros: -0 is the smaller
__device__ __forceinline__ bool below(double x, double y) { return x < y || (x == y && signbit(x) && !signbit(y)); }

// per block: min and max of the kept points' coordinates, their number and the number of them with a coordinate that
// is not finite, [block][8] doubles
__global__ __launch_bounds__(256) void cloud_bounds_kernel(const double *__restrict__ pts, long long n,
                                                           const unsigned char *__restrict__ keep, double *__restrict__ part)
{
    __shared__ double sh[256][8];
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY}, cnt = 0.0, bad = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if (keep && !keep[i]) continue;
        cnt += 1.0;
        if (!(isfinite(pts[3 * i]) && isfinite(pts[3 * i + 1]) && isfinite(pts[3 * i + 2]))) bad += 1.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = pts[3 * i + a];
            if (below(x, mn[a])) mn[a] = x;
            if (below(mx[a], x)) mx[a] = x;
        }
    }
    const int t = (int)threadIdx.x;
#pragma unroll
    for (int a = 0; a < 3; ++a) { sh[t][a] = mn[a]; sh[t][3 + a] = mx[a]; }
    sh[t][6] = cnt;
    sh[t][7] = bad;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if (t < step) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (below(sh[t + step][a], sh[t][a])) sh[t][a] = sh[t + step][a];
                if (below(sh[t][3 + a], sh[t + step][3 + a])) sh[t][3 + a] = sh[t + step][3 + a];
            }
            sh[t][6] += sh[t + step][6];
            sh[t][7] += sh[t + step][7];
        }
        __syncthreads();
    }
    if (t < 8) part[(size_t)blockIdx.x * 8 + t] = sh[0][t];
}

__global__ __launch_bounds__(256) void sqrt_kernel(const double *__restrict__ in, int n, double *__restrict__ out)
{
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x)) out[i] = sqrt(in[i]);
}

bool host_below(double x, double y) { return x < y || (x == y && std::signbit(x) && !std::signbit(y)); }

}  // namespace

hipError_t pair_triangulate(const double K[9], const double R1[9], const double t1[3], const double R2[9], const double t2[3],
                            const float *pts1_h, const float *pts2_h, const unsigned char *rgb_h, int m, const PairThresholds &thr,
                            ScratchCache &cache, PairCloud &acc, long long *n_accepted, hipStream_t st)
{
    *n_accepted = 0;
    if (m <= 0) return hipSuccess;
    PairArgs a;
    const double *R[2] = {R1, R2}, *t[2] = {t1, t2};
    double *P[2] = {a.P1, a.P2}, *C[2] = {a.C1, a.C2};
    for (int k = 0; k < 2; ++k) {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) {
                const double rt0 = c < 3 ? R[k][c] : t[k][0], rt1 = c < 3 ? R[k][3 + c] : t[k][1], rt2 = c < 3 ? R[k][6 + c] : t[k][2];
                P[k][4 * r + c] = (K[3 * r] * rt0 + K[3 * r + 1] * rt1) + K[3 * r + 2] * rt2;
            }
        for (int i = 0; i < 3; ++i) C[k][i] = -((R[k][i] * t[k][0] + R[k][3 + i] * t[k][1]) + R[k][6 + i] * t[k][2]);
    }
    for (int i = 0; i < 9; ++i) { a.R1[i] = R1[i]; a.R2[i] = R2[i]; a.K[i] = K[i]; }
    for (int i = 0; i < 3; ++i) { a.t1[i] = t1[i]; a.t2[i] = t2[i]; }
    a.thr = thr;

    ScratchCache::Lease in, X, flag, sel, cnt, tmp;
    const size_t pt_bytes = sizeof(float) * 2 * (size_t)m;
    STCHK(cache.lease(in, 2 * pt_bytes + 3 * (size_t)m));
    float *d1 = in.get<float>(), *d2 = d1 + 2 * (size_t)m;
    unsigned char *drgb = (unsigned char *)(d2 + 2 * (size_t)m);
    STCHK(cache.lease(X, sizeof(double) * 3 * (size_t)m));
    STCHK(cache.lease(flag, (size_t)m));
    STCHK(cache.lease(sel, sizeof(int) * (size_t)m));
    STCHK(cache.lease(cnt, sizeof(int)));
    STCHK(hipMemcpyAsync(d1, pts1_h, pt_bytes, hipMemcpyHostToDevice, st));
    STCHK(hipMemcpyAsync(d2, pts2_h, pt_bytes, hipMemcpyHostToDevice, st));
    STCHK(hipMemcpyAsync(drgb, rgb_h, 3 * (size_t)m, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pair_triangulate_kernel, grid_for(m), dim3(256), 0, st, a, (const float *)d1, (const float *)d2, m,
                       X.get<double>(), flag.get<unsigned char>());
    STCHK(hipGetLastError());
    hipcub::CountingInputIterator<int> iota(0);
    size_t bytes = 0;
    STCHK(hipcub::DeviceSelect::Flagged(nullptr, bytes, iota, flag.get<unsigned char>(), sel.get<int>(), cnt.get<int>(), m, st));
    STCHK(cache.lease(tmp, bytes));
    STCHK(hipcub::DeviceSelect::Flagged(tmp.get(), bytes, iota, flag.get<unsigned char>(), sel.get<int>(), cnt.get<int>(), m, st));
    int k_n = 0;
    STCHK(hipMemcpyAsync(&k_n, cnt.get(), sizeof(int), hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
    if (k_n > 0) {
        const size_t need = (size_t)acc.n + (size_t)k_n;
        if (3 * need > acc.pts.capacity()) {
            const size_t cap = std::max<size_t>(std::max<size_t>(need, 2 * (acc.pts.capacity() / 3)), 4096);
            DeviceBuffer<double> np;
            DeviceBuffer<unsigned char> nc;
            STCHK(np.reserve(3 * cap, cache));
            STCHK(nc.reserve(3 * cap, cache));
            if (acc.n > 0) {
                STCHK(hipMemcpyAsync(np.get(), acc.pts.get(), sizeof(double) * 3 * (size_t)acc.n, hipMemcpyDeviceToDevice, st));
                STCHK(hipMemcpyAsync(nc.get(), acc.rgb.get(), 3 * (size_t)acc.n, hipMemcpyDeviceToDevice, st));
                STCHK(hipStreamSynchronize(st));
            }
            acc.pts = std::move(np);
            acc.rgb = std::move(nc);
        }
        hipLaunchKernelGGL(pair_append_kernel, grid_for(k_n), dim3(256), 0, st, (const int *)sel.get(), k_n, m, (const double *)X.get(),
                           (const unsigned char *)drgb, acc.pts.get() + 3 * (size_t)acc.n, acc.rgb.get() + 3 * (size_t)acc.n);
        STCHK(hipGetLastError());
        STCHK(hipStreamSynchronize(st));
        acc.n += k_n;
    }
    *n_accepted = k_n;
    return hipSuccess;
}

hipError_t cloud_bounds(const double *pts, long long n, const unsigned char *keep_h, ScratchCache &cache, double mn[3], double mx[3],
                        hipStream_t st, long long *n_not_finite)
{
    if (n <= 0) return hipErrorInvalidValue;
    const dim3 grid = grid_for(n);
    ScratchCache::Lease keep, part;
    STCHK(cache.lease(part, sizeof(double) * 8 * grid.x));
    if (keep_h) {
        STCHK(cache.lease(keep, (size_t)n));
        STCHK(hipMemcpyAsync(keep.get(), keep_h, (size_t)n, hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(cloud_bounds_kernel, grid, dim3(256), 0, st, pts, n, keep_h ? (const unsigned char *)keep.get() : nullptr,
                       part.get<double>());
    STCHK(hipGetLastError());
    std::vector<double> h(8 * (size_t)grid.x);
    STCHK(hipMemcpyAsync(h.data(), part.get(), sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
    double kept = 0.0, bad = 0.0;
    for (int a = 0; a < 3; ++a) { mn[a] = INFINITY; mx[a] = -INFINITY; }
    for (unsigned b = 0; b < grid.x; ++b) {
        const double *p = &h[8 * (size_t)b];
        for (int a = 0; a < 3; ++a) {
            if (host_below(p[a], mn[a])) mn[a] = p[a];
            if (host_below(mx[a], p[3 + a])) mx[a] = p[3 + a];
        }
        kept += p[6];
        bad += p[7];
    }
    if (n_not_finite) *n_not_finite = (long long)bad;
    return kept > 0.0 ? hipSuccess : hipErrorInvalidValue;
}

hipError_t selftest_sqrt(const double *in_h, int n, double *out_h, ScratchCache &cache, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    ScratchCache::Lease buf;
    STCHK(cache.lease(buf, sizeof(double) * 2 * (size_t)n));
    double *in = buf.get<double>(), *out = in + n;
    STCHK(hipMemcpyAsync(in, in_h, sizeof(double) * n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(sqrt_kernel, grid_for(n), dim3(256), 0, st, (const double *)in, n, out);
    STCHK(hipGetLastError());
    STCHK(hipMemcpyAsync(out_h, out, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

}  // namespace amvs

AMVS_CHECK_TU(triangulate)
