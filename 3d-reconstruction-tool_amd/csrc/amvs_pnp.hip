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
// pnp_partials_kernel / ransac_total_kernel: the 29 sums of a refit pass, one lane per (block of 64 correspondences,
//     entry), then one lane per entry adding the partials in ascending order.  The 6 x 6 solve and the rotation update of
//     a step run on the host (amvs_pnp_step.h).
// Shared with amvs_fmat.hip: jacobi<N>(), the sampler, the wave's tally, the scoring tile and Points
// (amvs_ransac_common.h); ransac_total_kernel, ransac_argmax_kernel, Work, the halves of a pass and the RANSAC itself,
// ransac_run, to which PnpModel below gives what is the resection's own (amvs_ransac_run.h).
//
// -ffp-contract=off (Makefile): a * b + c below is two roundings, on the device and on the host.
#define AMVS_TU_ID 23
#include "amvs_check.h"
#include "amvs_pnp_host.h"
#include "amvs_pnp_step.h"
#include "amvs_pose.h"
#include "amvs_ransac_run.h"
#include "../../include/amvs_resection.h"

#include <cmath>
#include <cstring>

namespace amvs {

namespace {

using Tile = ScoreTile<32>;           // poses a scoring workgroup walks
using Points32 = Points<3, 2>;        // a: the points in space, b: their observations in the image
constexpr int N_TRI = 78;             // entries of the upper triangle of the 12 x 12 M
constexpr double ROOT3 = 1.7320508075688772;

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

    int idx[6];
    sample<6>(seed, h, m, idx);
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int r = idx[s];
        idx_out[6 * (size_t)j + s] = r;
        idx[s] = AMVS_IDX(r, m);
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
    const int h1 = Tile::end(n);
    for (int h = Tile::begin(); h < h1; ++h)                        // (wave-uniform pose)
        tally_wave(live && pnp_is_inlier(R + 9 * (size_t)h, t + 3 * (size_t)h, k.fx, k.fy, X, Y, Z, cu, cv, t2), counts, h);
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
    tally_wave(in, count);
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

inline int n_blocks_of(int m) { return (m + AMVS_PNP_BLOCK - 1) / AMVS_PNP_BLOCK; }

// the 29 SUMs of a pass under (R, t) over the set mask_d (NULL: all)
hipError_t refit_pass(const double R[9], const double t[3], const Intr &k, const Points32 &P, const unsigned char *mask_d, int m, Work &w,
                      double out[PNP_SUMS], hipStream_t st)
{
    const int n_blocks = n_blocks_of(m);
    hipLaunchKernelGGL(pnp_partials_kernel, blocks_for((long long)n_blocks * PNP_SUMS, 256), dim3(256), 0, st, pose_of(R, t), k, P.a, P.b,
                       mask_d, m, n_blocks, w.part.get<double>());
    STCHK(hipGetLastError());
    return pass_totals(w, n_blocks, PNP_SUMS, out, st);
}

// the header's refit of (R, t), in place
hipError_t refit_dev(double R[9], double t[3], const Intr &k, const Points32 &P, const unsigned char *mask_d, int m, Work &w, int *steps,
                 double *cost, hipStream_t st)
{
    double sums[PNP_SUMS], next[PNP_SUMS], Rn[9], tn[3];
    STCHK(refit_pass(R, t, k, P, mask_d, m, w, sums, st));
    int taken = 0;
    for (int it = 0; it < AMVS_PNP_REFINE_STEPS; ++it) {
        if (!pnp_gn_step(sums, R, t, Rn, tn)) break;
        STCHK(refit_pass(Rn, tn, k, P, mask_d, m, w, next, st));
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
hipError_t inliers_dev(const double R[9], const double t[3], const Intr &k, const Points32 &P, int m, double t2, unsigned char *mask_d,
                       Work &w, long long *count, hipStream_t st)
{
    return count_inliers(w, count, st, [&](int *count_d) {
        hipLaunchKernelGGL(pnp_inliers_kernel, blocks_for(m, 256), dim3(256), 0, st, pose_of(R, t), P.a, P.b, m, k, t2, mask_d, count_d);
    });
}

void launch_hypotheses(const Points32 &P, int m, const Intr &k, uint64_t seed, int first, int count, int *idx_d, double *R_d, double *t_d,
                       hipStream_t st)
{
    hipLaunchKernelGGL(pnp_hypotheses_kernel, blocks_for(count, 64), dim3(64), 0, st, P.a, P.b, m, k, (unsigned long long)seed, first,
                       count, idx_d, R_d, t_d);
}

void launch_score(const double *R_d, const double *t_d, int n, const Points32 &P, int m, const Intr &k, double t2, int *counts_d,
                  hipStream_t st)
{
    hipLaunchKernelGGL(pnp_score_kernel, Tile::grid(m, n), dim3(256), 0, st, R_d, t_d, n, P.a, P.b, m, k, t2, counts_d);
}

// what ransac_run asks of a model (amvs_ransac_run.h): the pose, from samples of six correspondences
struct PnpModel {
    static constexpr int SAMPLE = 6, BATCH = AMVS_PNP_BATCH;
    using Estimate = Pose;
    const float *pts3d_h, *pts2d_h;
    int m;
    Intr k;
    double t2;
    uint64_t seed;
    Points32 P;
    Work w;
    ScratchCache::Lease idx, R, t;

    hipError_t prepare(ScratchCache &cache, hipStream_t st)
    {
        STCHK(P.upload(pts3d_h, pts2d_h, m, cache, st));
        STCHK(w.reserve(PNP_SUMS, n_blocks_of(m), cache));
        STCHK(cache.lease(idx, sizeof(int) * 6 * BATCH));
        STCHK(cache.lease(R, sizeof(double) * 9 * BATCH));
        return cache.lease(t, sizeof(double) * 3 * BATCH);
    }
    void hypotheses(int first, int count, hipStream_t st)
    {
        launch_hypotheses(P, m, k, seed, first, count, idx.get<int>(), R.get<double>(), t.get<double>(), st);
    }
    void score(int n, int *counts_d, hipStream_t st) { launch_score(R.get<double>(), t.get<double>(), n, P, m, k, t2, counts_d, st); }
    hipError_t fetch(Pose &e, hipStream_t st)
    {
        STCHK(hipMemcpyAsync(e.R, R.get(), sizeof(e.R), hipMemcpyDeviceToHost, st));
        return hipMemcpyAsync(e.t, t.get(), sizeof(e.t), hipMemcpyDeviceToHost, st);
    }
    hipError_t inliers(const Pose &e, unsigned char *mask_d, long long *count, hipStream_t st)
    {
        return inliers_dev(e.R, e.t, k, P, m, t2, mask_d, w, count, st);
    }
    hipError_t refit(Pose &e, const unsigned char *mask_d, long long, hipStream_t st)
    {
        int steps = 0;
        double cost = 0.0;
        return refit_dev(e.R, e.t, k, P, mask_d, m, w, &steps, &cost, st);
    }
    static double all_inliers(double wr) { const double w2 = wr * wr; return (w2 * w2) * w2; }              // the header's (w^2 w^2) w^2
};

}  // namespace

hipError_t pnp_hypotheses(const float *pts3d_h, const float *pts2d_h, int m, const double *K, uint64_t seed, int first, int count,
                          int *idx_h, double *R_h, double *t_h, ScratchCache &cache, hipStream_t st)
{
    Points32 P;
    ScratchCache::Lease idx, R, t;
    STCHK(P.upload(pts3d_h, pts2d_h, m, cache, st));
    STCHK(cache.lease(idx, sizeof(int) * 6 * (size_t)count));
    STCHK(cache.lease(R, sizeof(double) * 9 * (size_t)count));
    STCHK(cache.lease(t, sizeof(double) * 3 * (size_t)count));
    launch_hypotheses(P, m, intrinsics_of(K), seed, first, count, idx.get<int>(), R.get<double>(), t.get<double>(), st);
    STCHK(hipGetLastError());
    STCHK(hipMemcpyAsync(idx_h, idx.get(), sizeof(int) * 6 * (size_t)count, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(R_h, R.get(), sizeof(double) * 9 * (size_t)count, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(t_h, t.get(), sizeof(double) * 3 * (size_t)count, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t pnp_score(const double *R_h, const double *t_h, int n, const float *pts3d_h, const float *pts2d_h, int m, const double *K,
                     double threshold, int *counts_h, ScratchCache &cache, hipStream_t st)
{
    Points32 P;
    ScratchCache::Lease R, t, counts;
    STCHK(P.upload(pts3d_h, pts2d_h, m, cache, st));
    STCHK(cache.lease(R, sizeof(double) * 9 * (size_t)n));
    STCHK(cache.lease(t, sizeof(double) * 3 * (size_t)n));
    STCHK(cache.lease(counts, sizeof(int) * (size_t)n));
    STCHK(hipMemcpyAsync(R.get(), R_h, sizeof(double) * 9 * (size_t)n, hipMemcpyHostToDevice, st));
    STCHK(hipMemcpyAsync(t.get(), t_h, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, st));
    STCHK(hipMemsetAsync(counts.get(), 0, sizeof(int) * (size_t)n, st));
    launch_score(R.get<double>(), t.get<double>(), n, P, m, intrinsics_of(K), threshold * threshold, counts.get<int>(), st);
    STCHK(hipGetLastError());
    STCHK(hipMemcpyAsync(counts_h, counts.get(), sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t pnp_inliers(const double R[9], const double t[3], const float *pts3d_h, const float *pts2d_h, int m, const double *K,
                       double threshold, unsigned char *mask_h, long long *count, ScratchCache &cache, hipStream_t st)
{
    Points32 P;
    Work w;
    ScratchCache::Lease mask;
    STCHK(P.upload(pts3d_h, pts2d_h, m, cache, st));
    STCHK(w.reserve(PNP_SUMS, n_blocks_of(m), cache));
    STCHK(cache.lease(mask, (size_t)m));
    STCHK(inliers_dev(R, t, intrinsics_of(K), P, m, threshold * threshold, mask.get<unsigned char>(), w, count, st));
    STCHK(hipMemcpyAsync(mask_h, mask.get(), (size_t)m, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t pnp_refine(const float *pts3d_h, const float *pts2d_h, int m, const double *K, const double R_in[9], const double t_in[3],
                      const unsigned char *mask_h, double R_out[9], double t_out[3], int *steps, double *cost, ScratchCache &cache,
                      hipStream_t st)
{
    Points32 P;
    Work w;
    ScratchCache::Lease mask;
    STCHK(P.upload(pts3d_h, pts2d_h, m, cache, st));
    STCHK(w.reserve(PNP_SUMS, n_blocks_of(m), cache));
    if (mask_h) {
        STCHK(cache.lease(mask, (size_t)m));
        STCHK(hipMemcpyAsync(mask.get(), mask_h, (size_t)m, hipMemcpyHostToDevice, st));
    }
    double R[9], t[3];
    std::memcpy(R, R_in, sizeof(R));
    std::memcpy(t, t_in, sizeof(t));
    STCHK(refit_dev(R, t, intrinsics_of(K), P, mask_h ? mask.get<unsigned char>() : nullptr, m, w, steps, cost, st));
    std::memcpy(R_out, R, sizeof(R));
    std::memcpy(t_out, t, sizeof(t));
    return hipSuccess;
}

hipError_t pnp_ransac(const float *pts3d_h, const float *pts2d_h, int m, const double *K, double threshold, double confidence,
                      int max_hypotheses, uint64_t seed, double R_out[9], double t_out[3], unsigned char *mask_h, long long *n_inliers,
                      int info[3], ScratchCache &cache, hipStream_t st)
{
    PnpModel model{pts3d_h, pts2d_h, m, intrinsics_of(K), threshold * threshold, seed};
    Pose best{};
    const hipError_t e = ransac_run(model, m, confidence, max_hypotheses, &best, mask_h, n_inliers, info, cache, st);
    std::memcpy(R_out, best.R, sizeof(best.R));
    std::memcpy(t_out, best.t, sizeof(best.t));
    return e;
}

}  // namespace amvs

AMVS_CHECK_TU(pnp)
