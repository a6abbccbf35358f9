// amvs_pnp.hip -- camera resection by RANSAC and the Gauss-Newton polish of a pose (include/amvs_resection.h; the
// definition is the header's, the judge tests/resection_restatement.py, bit for bit).
//
// pnp_hypotheses_kernel: one hypothesis per lane, one wave per workgroup, as fmat_hypotheses_kernel.  The 78 + 144
//     doubles of the 12 x 12 Jacobi state live in LDS laid out [entry][lane] (113 664 B a workgroup, so one workgroup a
//     CU; a batch of 1024 hypotheses is 16 waves and the kernel is latency-bound whatever its occupancy, DESIGN.md
//     section 14).  The 3 x 3 Jacobi of the nearest rotation reuses the first 15 entries of the same columns.
// pnp_score_kernel: the hot path, poses x correspondences.  A lane holds one correspondence (five doubles), a wave walks
//     a tile of poses whose twelve doubles are wave-uniform (read through the scalar cache), the inlier predicate goes
//     through a ballot and a population count, and lane 0 adds the count to the pose's counter (no add for a zero).
//     Integers only: any grid shape gives the same counts.
// pnp_partials_kernel / fmat_total_kernel: the 29 sums of a refit pass, one lane per (block of 64 correspondences,
//     entry), then one lane per entry adding the partials in ascending order.  The 6 x 6 solve and the rotation update of
//     a step run on the host (amvs_pnp_step.h).
//
// -ffp-contract=off (Makefile): a * b + c below is two roundings, on the device and on the host.
#define AMVS_TU_ID 23
#include "amvs_check.h"
#include "amvs_pnp_host.h"
#include "amvs_pnp_step.h"
#include "amvs_ransac_common.h"
#include "../../include/amvs_resection.h"

#include <cmath>
#include <cstring>

namespace amvs {

namespace {

#define PCHK(call)                                                  \
    do {                                                            \
        hipError_t e_ = (call);                                     \
        if (e_ != hipSuccess) { (void)hipStreamSynchronize(st); return e_; } \
    } while (0)

constexpr int HYP_TILE = 32;          // poses a scoring workgroup walks
constexpr int N_TRI = 78;             // entries of the upper triangle of the 12 x 12 M
constexpr double ROOT3 = 1.7320508075688772;

struct Intr { double fx, fy, cx, cy; };
struct Pose { double R[9], t[3]; };

inline Intr intrinsics_of(const double *K) { return Intr{K[0], K[4], K[2], K[5]}; }

// Xc = R X + t in the header's order
__device__ __forceinline__ void camera_point(const double *R, const double *t, double X, double Y, double Z, double Xc[3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) Xc[r] = ((R[3 * r] * X + R[3 * r + 1] * Y) + R[3 * r + 2] * Z) + t[r];
}

// the inlier test with cu = cx - u, cv = cy - v
__device__ __forceinline__ bool pnp_is_inlier(const double *R, const double *t, double fx, double fy, double X, double Y, double Z,
                                              double cu, double cv, double t2)
{
    double Xc[3];
    camera_point(R, t, X, Y, Z, Xc);
    const double z = Xc[2];
    const double ex = fx * Xc[0] + cu * z, ey = fy * Xc[1] + cv * z;
    const double ee = ex * ex + ey * ey;
    return z > 0.0 && ee <= t2 * (z * z) && ee < INFINITY;
}

// One hypothesis per lane, one wave per workgroup: sample, 6-point DLT, nearest rotation.
__global__ __launch_bounds__(64) void pnp_hypotheses_kernel(const float *__restrict__ pts3d, const float *__restrict__ pts2d, int m,
                                                            const Intr k, unsigned long long seed, int first, int count,
                                                            int *__restrict__ idx_out, double *__restrict__ R_out,
                                                            double *__restrict__ t_out)
{
    __shared__ double lds[(N_TRI + 144) * 64];
    const int j = (int)(blockIdx.x * 64 + threadIdx.x);
    if (j >= count) return;                     // (no barrier below: a lane touches its own LDS column only)
    const unsigned long long h = (unsigned long long)first + (unsigned long long)j;

    int idx[6], sorted[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        int r = (int)(mix64(seed ^ mix64(6ull * h + (unsigned long long)s)) % (unsigned long long)(m - s));
#pragma unroll
        for (int i = 0; i < s; ++i)
            if (r >= sorted[i]) r += 1;
        idx[s] = AMVS_IDX(r, m);
        int v = r;                              // insert into the ascending list
#pragma unroll
        for (int i = 0; i < s; ++i)
            if (v < sorted[i]) { const int tmp = sorted[i]; sorted[i] = v; v = tmp; }
        sorted[s] = v;
        idx_out[6 * (size_t)j + s] = r;
    }

    double Px[6], Py[6], Pz[6], xn[6], yn[6];
    double sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        Px[s] = (double)pts3d[3 * (size_t)idx[s]]; Py[s] = (double)pts3d[3 * (size_t)idx[s] + 1]; Pz[s] = (double)pts3d[3 * (size_t)idx[s] + 2];
        xn[s] = ((double)pts2d[2 * (size_t)idx[s]] - k.cx) / k.fx;
        yn[s] = ((double)pts2d[2 * (size_t)idx[s] + 1] - k.cy) / k.fy;
        sx = sx + Px[s]; sy = sy + Py[s]; sz = sz + Pz[s];
    }
    const double c0 = sx / 6.0, c1 = sy / 6.0, c2 = sz / 6.0;
    double sd = 0.0;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        Px[s] = Px[s] - c0; Py[s] = Py[s] - c1; Pz[s] = Pz[s] - c2;
        sd = sd + sqrt((Px[s] * Px[s] + Py[s] * Py[s]) + Pz[s] * Pz[s]);
    }
    const double scale = ROOT3 / (sd / 6.0);
#pragma unroll
    for (int s = 0; s < 6; ++s) { Px[s] = Px[s] * scale; Py[s] = Py[s] * scale; Pz[s] = Pz[s] * scale; }

    const JacobiState<12, 64> S{lds + threadIdx.x, lds + N_TRI * 64 + threadIdx.x};
    // M by blocks, a row of P at a time: rows i and 4 + i share the P P^T entries
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double pp[4], px[4], py[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) pp[c] = px[c] = py[c] = 0.0;
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const double P[4] = {Px[s], Py[s], Pz[s], 1.0};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double gx = -(xn[s] * P[c]), gy = -(yn[s] * P[c]);
                if (c >= i) pp[c] = pp[c] + P[i] * P[c];
                px[c] = px[c] + P[i] * gx;
                py[c] = py[c] + P[i] * gy;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c >= i) { S.M(i, c) = pp[c]; S.M(4 + i, 4 + c) = pp[c]; }
            S.M(i, 4 + c) = 0.0;
            S.M(i, 8 + c) = px[c];
            S.M(4 + i, 8 + c) = py[c];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double gg[4];
#pragma unroll
        for (int c = i; c < 4; ++c) gg[c] = 0.0;
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const double P[4] = {Px[s], Py[s], Pz[s], 1.0};
            const double gxi = -(xn[s] * P[i]), gyi = -(yn[s] * P[i]);
#pragma unroll
            for (int c = i; c < 4; ++c) {
                const double gx = -(xn[s] * P[c]), gy = -(yn[s] * P[c]);
                gg[c] = gg[c] + (gxi * gx + gyi * gy);
            }
        }
#pragma unroll
        for (int c = i; c < 4; ++c) S.M(8 + i, 8 + c) = gg[c];
    }
    double p[12];
    jacobi<12, 64>(S, p);

    // undo the scaling, make det A positive
    double A[9], b[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) A[3 * r + c] = p[4 * r + c] * scale;
        b[r] = ((p[4 * r + 3] - A[3 * r] * c0) - A[3 * r + 1] * c1) - A[3 * r + 2] * c2;
    }
    const double det = (A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6])) + A[2] * (A[3] * A[7] - A[4] * A[6]);
    if (det < 0.0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) A[e] = -A[e];
#pragma unroll
        for (int r = 0; r < 3; ++r) b[r] = -b[r];
    }
    // the nearest rotation: Jacobi on A^T A in the first entries of the same LDS columns
    const JacobiState<3, 64> G{lds + threadIdx.x, lds + 6 * 64 + threadIdx.x};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = i; c < 3; ++c) G.M(i, c) = (A[i] * A[c] + A[3 + i] * A[3 + c]) + A[6 + i] * A[6 + c];
    double unused[3];
    jacobi<3, 64>(G, unused);
    double sw[3], V[9], C[9];
#pragma unroll
    for (int e = 0; e < 3; ++e) sw[e] = sqrt(G.M(e, e));
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) V[3 * r + c] = G.V(r, c);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int e = 0; e < 3; ++e) C[3 * r + e] = ((A[3 * r] * V[e] + A[3 * r + 1] * V[3 + e]) + A[3 * r + 2] * V[6 + e]) / sw[e];
    const double sc = ((sw[0] + sw[1]) + sw[2]) / 3.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            R_out[9 * (size_t)j + 3 * r + c] = (C[3 * r] * V[3 * c] + C[3 * r + 1] * V[3 * c + 1]) + C[3 * r + 2] * V[3 * c + 2];
        t_out[3 * (size_t)j + r] = b[r] / sc;
    }
}

// counts[h] += inliers of pose h among this workgroup's 256 correspondences, for the HYP_TILE poses of blockIdx.y
__global__ __launch_bounds__(256) void pnp_score_kernel(const double *__restrict__ R, const double *__restrict__ t, int n,
                                                        const float *__restrict__ pts3d, const float *__restrict__ pts2d, int m,
                                                        const Intr k, double t2, int *__restrict__ counts)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    const bool live = i < m;
    const size_t ii = live ? (size_t)i : 0;
    const double X = (double)pts3d[3 * ii], Y = (double)pts3d[3 * ii + 1], Z = (double)pts3d[3 * ii + 2];
    const double cu = k.cx - (double)pts2d[2 * ii], cv = k.cy - (double)pts2d[2 * ii + 1];
    const int h0 = (int)blockIdx.y * HYP_TILE, h1 = h0 + HYP_TILE < n ? h0 + HYP_TILE : n;
    const bool lane0 = (threadIdx.x & 63) == 0;
    for (int h = h0; h < h1; ++h) {
        const bool in = live && pnp_is_inlier(R + 9 * (size_t)h, t + 3 * (size_t)h, k.fx, k.fy, X, Y, Z, cu, cv, t2);   // wave-uniform pose
        const int c = __popcll(__ballot(in));
        if (c != 0 && lane0) atomicAdd(&counts[h], c);
    }
}

// mask[i] and *count for one pose
__global__ __launch_bounds__(256) void pnp_inliers_kernel(const Pose P, const float *__restrict__ pts3d, const float *__restrict__ pts2d,
                                                          int m, const Intr k, double t2, unsigned char *__restrict__ mask,
                                                          int *__restrict__ count)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    bool in = false;
    if (i < m) {
        const size_t ii = (size_t)i;
        in = pnp_is_inlier(P.R, P.t, k.fx, k.fy, (double)pts3d[3 * ii], (double)pts3d[3 * ii + 1], (double)pts3d[3 * ii + 2],
                           k.cx - (double)pts2d[2 * ii], k.cy - (double)pts2d[2 * ii + 1], t2);
        mask[i] = in ? 1 : 0;
    }
    const int c = __popcll(__ballot(in));
    if (c != 0 && (threadIdx.x & 63) == 0) atomicAdd(count, c);
}

// The block partials of a refit pass under P: entries 0 .. 20 the upper triangle of H row by row, 21 .. 26 g, 27 the cost,
// 28 the members in front.  One lane per (block of 64 correspondences, entry); part[block][entry].
__global__ __launch_bounds__(256) void pnp_partials_kernel(const Pose P, const Intr k, const float *__restrict__ pts3d,
                                                           const float *__restrict__ pts2d, const unsigned char *__restrict__ mask,
                                                           int m, int n_blocks, double *__restrict__ part)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n_blocks * PNP_SUMS) return;
    const int b = (int)(t / PNP_SUMS), e = (int)(t % PNP_SUMS);
    int ei = 0, ej = 0;                         // e < 21: entry e is H[ei][ej]; 21 <= e < 27: g[ei]
    if (e < 21) {
        ej = e;
        while (ej >= 6 - ei) { ej -= 6 - ei; ei += 1; }
        ej += ei;
    } else if (e < PNP_COST) {
        ei = e - 21;
    }
    const int i1 = (b + 1) * AMVS_PNP_BLOCK < m ? (b + 1) * AMVS_PNP_BLOCK : m;
    double acc = 0.0;
    for (int i = b * AMVS_PNP_BLOCK; i < i1; ++i) {
        if (mask && !mask[i]) continue;
        const size_t ii = (size_t)i;
        double Xc[3];
        camera_point(P.R, P.t, (double)pts3d[3 * ii], (double)pts3d[3 * ii + 1], (double)pts3d[3 * ii + 2], Xc);
        const double z = Xc[2];
        if (!(z > 0.0)) continue;
        const double iz = 1.0 / z, xz = Xc[0] * iz, yz = Xc[1] * iz;
        const double rx = (k.fx * xz + k.cx) - (double)pts2d[2 * ii], ry = (k.fy * yz + k.cy) - (double)pts2d[2 * ii + 1];
        const double ax = k.fx * iz, ay = k.fy * iz, bx = -(ax * xz), by = -(ay * yz);
        const double Jx[6] = {bx * Xc[1], ax * z - bx * Xc[0], -(ax * Xc[1]), ax, 0.0, bx};
        const double Jy[6] = {by * Xc[1] - ay * z, -(by * Xc[0]), ay * Xc[0], 0.0, ay, by};
        double xi = Jx[0], xj = Jx[0], yi = Jy[0], yj = Jy[0];
#pragma unroll
        for (int s = 1; s < 6; ++s) {
            xi = ei == s ? Jx[s] : xi; yi = ei == s ? Jy[s] : yi;
            xj = ej == s ? Jx[s] : xj; yj = ej == s ? Jy[s] : yj;
        }
        double u;
        if (e < 21) u = xi * xj + yi * yj;
        else if (e < PNP_COST) u = xi * rx + yi * ry;
        else if (e == PNP_COST) u = rx * rx + ry * ry;
        else u = 1.0;
        acc = acc + u;
    }
    part[t] = acc;
}

inline dim3 blocks_for(long long n, int per) { return dim3((unsigned)((n + per - 1) / per)); }

// the two point arrays of a call, on the device
struct Points {
    ScratchCache::Lease buf;
    const float *p3 = nullptr, *p2 = nullptr;
    hipError_t upload(const float *h3, const float *h2, int m, ScratchCache &cache, hipStream_t st)
    {
        const size_t n3 = 3 * (size_t)m, n2 = 2 * (size_t)m;
        hipError_t e = cache.lease(buf, sizeof(float) * (n3 + n2));
        if (e != hipSuccess) return e;
        float *d = buf.get<float>();
        p3 = d;
        p2 = d + n3;
        e = hipMemcpyAsync(d, h3, sizeof(float) * n3, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        return hipMemcpyAsync(d + n3, h2, sizeof(float) * n2, hipMemcpyHostToDevice, st);
    }
};

// scratch of the refit passes and inlier passes of one call
struct Work {
    ScratchCache::Lease part, total, count;
    hipError_t reserve(int m, ScratchCache &cache)
    {
        const size_t n_blocks = ((size_t)m + AMVS_PNP_BLOCK - 1) / AMVS_PNP_BLOCK;
        hipError_t e = cache.lease(part, sizeof(double) * PNP_SUMS * n_blocks);
        if (e == hipSuccess) e = cache.lease(total, sizeof(double) * 64);
        if (e == hipSuccess) e = cache.lease(count, sizeof(int) * 2);
        return e;
    }
};

Pose pose_of(const double R[9], const double t[3])
{
    Pose P;
    std::memcpy(P.R, R, sizeof(P.R));
    std::memcpy(P.t, t, sizeof(P.t));
    return P;
}

// the 29 SUMs of a pass under (R, t) over the set mask_d (NULL: all)
hipError_t refit_pass(const double R[9], const double t[3], const Intr &k, const Points &P, const unsigned char *mask_d, int m, Work &w,
                      double out[PNP_SUMS], hipStream_t st)
{
    const int n_blocks = (m + AMVS_PNP_BLOCK - 1) / AMVS_PNP_BLOCK;
    hipLaunchKernelGGL(pnp_partials_kernel, blocks_for((long long)n_blocks * PNP_SUMS, 256), dim3(256), 0, st, pose_of(R, t), k, P.p3, P.p2,
                       mask_d, m, n_blocks, w.part.get<double>());
    PCHK(hipGetLastError());
    hipLaunchKernelGGL(fmat_total_kernel, dim3(1), dim3(64), 0, st, (const double *)w.part.get(), n_blocks, PNP_SUMS, w.total.get<double>());
    PCHK(hipGetLastError());
    PCHK(hipMemcpyAsync(out, w.total.get(), sizeof(double) * PNP_SUMS, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

// the header's refit of (R, t), in place
hipError_t refit(double R[9], double t[3], const Intr &k, const Points &P, const unsigned char *mask_d, int m, Work &w, int *steps,
                 double *cost, hipStream_t st)
{
    double sums[PNP_SUMS], next[PNP_SUMS], Rn[9], tn[3];
    PCHK(refit_pass(R, t, k, P, mask_d, m, w, sums, st));
    int taken = 0;
    for (int it = 0; it < AMVS_PNP_REFINE_STEPS; ++it) {
        if (!pnp_gn_step(sums, R, t, Rn, tn)) break;
        PCHK(refit_pass(Rn, tn, k, P, mask_d, m, w, next, st));
        if (!(next[PNP_COST] <= sums[PNP_COST] && next[PNP_FRONT] >= sums[PNP_FRONT])) break;
        std::memcpy(R, Rn, sizeof(Rn));
        std::memcpy(t, tn, sizeof(tn));
        std::memcpy(sums, next, sizeof(next));
        taken += 1;
    }
    *steps = taken;
    *cost = sums[PNP_COST];
    return hipSuccess;
}

// mask_d[i] and the count of the inliers of (R, t)
hipError_t inliers_dev(const double R[9], const double t[3], const Intr &k, const Points &P, int m, double t2, unsigned char *mask_d,
                       Work &w, long long *count, hipStream_t st)
{
    PCHK(hipMemsetAsync(w.count.get(), 0, sizeof(int), st));
    hipLaunchKernelGGL(pnp_inliers_kernel, blocks_for(m, 256), dim3(256), 0, st, pose_of(R, t), P.p3, P.p2, m, k, t2, mask_d,
                       w.count.get<int>());
    PCHK(hipGetLastError());
    int c = 0;
    PCHK(hipMemcpyAsync(&c, w.count.get(), sizeof(int), hipMemcpyDeviceToHost, st));
    PCHK(hipStreamSynchronize(st));
    *count = c;
    return hipSuccess;
}

void launch_hypotheses(const Points &P, int m, const Intr &k, uint64_t seed, int first, int count, int *idx_d, double *R_d, double *t_d,
                       hipStream_t st)
{
    hipLaunchKernelGGL(pnp_hypotheses_kernel, blocks_for(count, 64), dim3(64), 0, st, P.p3, P.p2, m, k, (unsigned long long)seed, first,
                       count, idx_d, R_d, t_d);
}

void launch_score(const double *R_d, const double *t_d, int n, const Points &P, int m, const Intr &k, double t2, int *counts_d,
                  hipStream_t st)
{
    hipLaunchKernelGGL(pnp_score_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)((n + HYP_TILE - 1) / HYP_TILE)), dim3(256), 0, st,
                       R_d, t_d, n, P.p3, P.p2, m, k, t2, counts_d);
}

}  // namespace

hipError_t pnp_hypotheses(const float *pts3d_h, const float *pts2d_h, int m, const double *K, uint64_t seed, int first, int count,
                          int *idx_h, double *R_h, double *t_h, ScratchCache &cache, hipStream_t st)
{
    Points P;
    ScratchCache::Lease idx, R, t;
    PCHK(P.upload(pts3d_h, pts2d_h, m, cache, st));
    PCHK(cache.lease(idx, sizeof(int) * 6 * (size_t)count));
    PCHK(cache.lease(R, sizeof(double) * 9 * (size_t)count));
    PCHK(cache.lease(t, sizeof(double) * 3 * (size_t)count));
    launch_hypotheses(P, m, intrinsics_of(K), seed, first, count, idx.get<int>(), R.get<double>(), t.get<double>(), st);
    PCHK(hipGetLastError());
    PCHK(hipMemcpyAsync(idx_h, idx.get(), sizeof(int) * 6 * (size_t)count, hipMemcpyDeviceToHost, st));
    PCHK(hipMemcpyAsync(R_h, R.get(), sizeof(double) * 9 * (size_t)count, hipMemcpyDeviceToHost, st));
    PCHK(hipMemcpyAsync(t_h, t.get(), sizeof(double) * 3 * (size_t)count, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t pnp_score(const double *R_h, const double *t_h, int n, const float *pts3d_h, const float *pts2d_h, int m, const double *K,
                     double threshold, int *counts_h, ScratchCache &cache, hipStream_t st)
{
    Points P;
    ScratchCache::Lease R, t, counts;
    PCHK(P.upload(pts3d_h, pts2d_h, m, cache, st));
    PCHK(cache.lease(R, sizeof(double) * 9 * (size_t)n));
    PCHK(cache.lease(t, sizeof(double) * 3 * (size_t)n));
    PCHK(cache.lease(counts, sizeof(int) * (size_t)n));
    PCHK(hipMemcpyAsync(R.get(), R_h, sizeof(double) * 9 * (size_t)n, hipMemcpyHostToDevice, st));
    PCHK(hipMemcpyAsync(t.get(), t_h, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, st));
    PCHK(hipMemsetAsync(counts.get(), 0, sizeof(int) * (size_t)n, st));
    launch_score(R.get<double>(), t.get<double>(), n, P, m, intrinsics_of(K), threshold * threshold, counts.get<int>(), st);
    PCHK(hipGetLastError());
    PCHK(hipMemcpyAsync(counts_h, counts.get(), sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t pnp_inliers(const double R[9], const double t[3], const float *pts3d_h, const float *pts2d_h, int m, const double *K,
                       double threshold, unsigned char *mask_h, long long *count, ScratchCache &cache, hipStream_t st)
{
    Points P;
    Work w;
    ScratchCache::Lease mask;
    PCHK(P.upload(pts3d_h, pts2d_h, m, cache, st));
    PCHK(w.reserve(m, cache));
    PCHK(cache.lease(mask, (size_t)m));
    PCHK(inliers_dev(R, t, intrinsics_of(K), P, m, threshold * threshold, mask.get<unsigned char>(), w, count, st));
    PCHK(hipMemcpyAsync(mask_h, mask.get(), (size_t)m, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t pnp_refine(const float *pts3d_h, const float *pts2d_h, int m, const double *K, const double R_in[9], const double t_in[3],
                      const unsigned char *mask_h, double R_out[9], double t_out[3], int *steps, double *cost, ScratchCache &cache,
                      hipStream_t st)
{
    Points P;
    Work w;
    ScratchCache::Lease mask;
    PCHK(P.upload(pts3d_h, pts2d_h, m, cache, st));
    PCHK(w.reserve(m, cache));
    if (mask_h) {
        PCHK(cache.lease(mask, (size_t)m));
        PCHK(hipMemcpyAsync(mask.get(), mask_h, (size_t)m, hipMemcpyHostToDevice, st));
    }
    double R[9], t[3];
    std::memcpy(R, R_in, sizeof(R));
    std::memcpy(t, t_in, sizeof(t));
    PCHK(refit(R, t, intrinsics_of(K), P, mask_h ? mask.get<unsigned char>() : nullptr, m, w, steps, cost, st));
    std::memcpy(R_out, R, sizeof(R));
    std::memcpy(t_out, t, sizeof(t));
    return hipSuccess;
}

hipError_t pnp_ransac(const float *pts3d_h, const float *pts2d_h, int m, const double *K, double threshold, double confidence,
                      int max_hypotheses, uint64_t seed, double R_out[9], double t_out[3], unsigned char *mask_h, long long *n_inliers,
                      int info[3], ScratchCache &cache, hipStream_t st)
{
    const double t2 = threshold * threshold;
    const Intr k = intrinsics_of(K);
    Points P;
    Work w;
    ScratchCache::Lease idx, R, t, counts, best2, mask_a, mask_b;
    PCHK(P.upload(pts3d_h, pts2d_h, m, cache, st));
    PCHK(w.reserve(m, cache));
    PCHK(cache.lease(idx, sizeof(int) * 6 * AMVS_PNP_BATCH));
    PCHK(cache.lease(R, sizeof(double) * 9 * AMVS_PNP_BATCH));
    PCHK(cache.lease(t, sizeof(double) * 3 * AMVS_PNP_BATCH));
    PCHK(cache.lease(counts, sizeof(int) * AMVS_PNP_BATCH));
    PCHK(cache.lease(best2, sizeof(int) * 2));
    PCHK(cache.lease(mask_a, (size_t)m));
    PCHK(cache.lease(mask_b, (size_t)m));

    int done = 0, best = -1, best_h = 0;
    for (;;) {
        const int nb = max_hypotheses - done < AMVS_PNP_BATCH ? max_hypotheses - done : AMVS_PNP_BATCH;
        launch_hypotheses(P, m, k, seed, done, nb, idx.get<int>(), R.get<double>(), t.get<double>(), st);
        PCHK(hipGetLastError());
        PCHK(hipMemsetAsync(counts.get(), 0, sizeof(int) * (size_t)nb, st));
        launch_score(R.get<double>(), t.get<double>(), nb, P, m, k, t2, counts.get<int>(), st);
        PCHK(hipGetLastError());
        hipLaunchKernelGGL(fmat_argmax_kernel, dim3(1), dim3(1024), 0, st, (const int *)counts.get(), nb, done, best2.get<int>());
        PCHK(hipGetLastError());
        int got[2] = {0, 0};
        PCHK(hipMemcpyAsync(got, best2.get(), sizeof(got), hipMemcpyDeviceToHost, st));
        PCHK(hipStreamSynchronize(st));
        if (got[0] > best) { best = got[0]; best_h = got[1]; }     // (a later batch wins only with a larger count)
        done += nb;
        const double wr = (double)best / (double)m, w2 = wr * wr, p = (w2 * w2) * w2;
        double N;
        if (p >= 1.0) N = 0.0;
        else if (1.0 - p == 1.0) N = (double)max_hypotheses;
        else N = std::ceil(std::log(1.0 - confidence) / std::log(1.0 - p));
        if ((double)done >= N || done == max_hypotheses) break;
    }
    info[0] = done; info[1] = best_h; info[2] = best;

    for (int e = 0; e < 9; ++e) R_out[e] = 0.0;
    for (int e = 0; e < 3; ++e) t_out[e] = 0.0;
    std::memset(mask_h, 0, (size_t)m);
    *n_inliers = 0;
    if (best < 6) return hipSuccess;

    // the best hypothesis' pose again (the sampler is a function of h), its inliers, and the two refits
    double R1[9], t1[3], R2[9], t2v[3], cost = 0.0;
    int steps = 0;
    launch_hypotheses(P, m, k, seed, best_h, 1, idx.get<int>(), R.get<double>(), t.get<double>(), st);
    PCHK(hipGetLastError());
    PCHK(hipMemcpyAsync(R1, R.get(), sizeof(R1), hipMemcpyDeviceToHost, st));
    PCHK(hipMemcpyAsync(t1, t.get(), sizeof(t1), hipMemcpyDeviceToHost, st));
    PCHK(hipStreamSynchronize(st));
    long long n0 = 0, n1 = 0, n2 = 0;
    unsigned char *ma = mask_a.get<unsigned char>(), *mb = mask_b.get<unsigned char>();
    PCHK(inliers_dev(R1, t1, k, P, m, t2, ma, w, &n0, st));
    if (n0 < 6) return hipSuccess;                      // (n0 == best >= 6: unreachable, kept as the refit's precondition)
    PCHK(refit(R1, t1, k, P, ma, m, w, &steps, &cost, st));
    PCHK(inliers_dev(R1, t1, k, P, m, t2, mb, w, &n1, st));
    if (n1 < 6) return hipSuccess;
    std::memcpy(R2, R1, sizeof(R2));
    std::memcpy(t2v, t1, sizeof(t2v));
    PCHK(refit(R2, t2v, k, P, mb, m, w, &steps, &cost, st));
    PCHK(inliers_dev(R2, t2v, k, P, m, t2, ma, w, &n2, st));
    const bool second = n2 >= n1;
    std::memcpy(R_out, second ? R2 : R1, sizeof(double) * 9);
    std::memcpy(t_out, second ? t2v : t1, sizeof(double) * 3);
    *n_inliers = second ? n2 : n1;
    PCHK(hipMemcpyAsync(mask_h, second ? ma : mb, (size_t)m, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

}  // namespace amvs

AMVS_CHECK_TU(pnp)
