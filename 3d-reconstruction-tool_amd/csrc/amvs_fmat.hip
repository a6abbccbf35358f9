// amvs_fmat.hip -- a fundamental matrix fitted to the matches of two views by RANSAC (include/amvs_epipolar.h; the
// definition is the header's, the judge tests/epipolar_restatement.py, bit for bit).
//
// fmat_hypotheses_kernel: one hypothesis per lane, one wave per workgroup.  The 45 + 81 doubles of the Jacobi state (the
//     upper triangle of M, and V) live in LDS laid out [entry][lane], so the 64 lanes of a wave read 64 consecutive
//     doubles per access (ds_read_b64 / ds_write_b64 without a bank conflict) and every (p, q) pair is a compile-time
//     constant: all LDS offsets are immediates.  63 KiB a wave, so two waves a CU; a batch of 1024 hypotheses is 16
//     waves on 256 CUs and the kernel is latency-bound whatever its occupancy.
// fmat_score_kernel: the hot path, hypotheses x matches.  A lane holds one match (four doubles), a wave walks a tile of
//     hypotheses whose nine doubles are wave-uniform (read through the scalar cache), the inlier predicate goes through
//     a ballot and a population count, and lane 0 adds the count to the hypothesis' counter (no add for a zero).
//     Integers only: any grid shape gives the same counts.
// fmat_partials_kernel / ransac_total_kernel: the sums of the refit, one lane per (block of 64 matches, entry), then one
//     lane per entry adding the partials in ascending order.  The 9 x 9 Jacobi of the refit runs once, on the host,
//     through the same jacobi<N>() the hypothesis kernel compiles.
// Shared with amvs_pnp.hip: jacobi<N>(), the sampler, the wave's tally, the scoring tile and Points
// (amvs_ransac_common.h); ransac_total_kernel, ransac_argmax_kernel, Work, the halves of a pass and the RANSAC itself,
// ransac_run, to which FmatModel below gives what is the fundamental matrix's own (amvs_ransac_run.h).
//
// -ffp-contract=off (Makefile): a * b + c below is two roundings, on the device and on the host.
#define AMVS_TU_ID 21
#include "amvs_check.h"
#include "amvs_fmat_host.h"
#include "amvs_ransac_run.h"
#include "../../include/amvs_epipolar.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace amvs {

namespace {

using Tile = ScoreTile<32>;           // hypotheses a scoring workgroup walks
using Points2 = Points<2, 2>;         // a: the matches' points in the first view, b: in the second
constexpr int N_TRI = 45;             // entries of the upper triangle of the 9 x 9 M
constexpr double ROOT2 = 1.4142135623730951;

struct Norm { double cx1, cy1, s1, cx2, cy2, s2; };

// the header's row a of a match under the normalisation
__host__ __device__ __forceinline__ void fmat_row(const Norm &n, double x1, double y1, double x2, double y2, double a[9])
{
    const double x1n = (x1 - n.cx1) * n.s1, y1n = (y1 - n.cy1) * n.s1;
    const double x2n = (x2 - n.cx2) * n.s2, y2n = (y2 - n.cy2) * n.s2;
    a[0] = x2n * x1n; a[1] = x2n * y1n; a[2] = x2n;
    a[3] = y2n * x1n; a[4] = y2n * y1n; a[5] = y2n;
    a[6] = x1n; a[7] = y1n; a[8] = 1.0;
}

// step 6 of the fit
__host__ __device__ __forceinline__ void fmat_denormalise(const double f[9], const Norm &n, double F[9])
{
    double G[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        G[3 * r] = f[3 * r] * n.s1;
        G[3 * r + 1] = f[3 * r + 1] * n.s1;
        G[3 * r + 2] = (f[3 * r + 2] - G[3 * r] * n.cx1) - G[3 * r + 1] * n.cy1;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        F[c] = n.s2 * G[c];
        F[3 + c] = n.s2 * G[3 + c];
        F[6 + c] = (G[6 + c] - F[c] * n.cx2) - F[3 + c] * n.cy2;
    }
}

struct FMat { double f[9]; };

__host__ __device__ __forceinline__ bool fmat_is_inlier(const double *F, double x1, double y1, double x2, double y2, double t2)
{
    const double l20 = (F[0] * x1 + F[1] * y1) + F[2], l21 = (F[3] * x1 + F[4] * y1) + F[5], l22 = (F[6] * x1 + F[7] * y1) + F[8];
    const double l10 = (F[0] * x2 + F[3] * y2) + F[6], l11 = (F[1] * x2 + F[4] * y2) + F[7];
    const double e = (x2 * l20 + y2 * l21) + l22, dd = e * e;
    const double n2 = l20 * l20 + l21 * l21, n1 = l10 * l10 + l11 * l11;
    return n1 > 0.0 && n2 > 0.0 && dd <= t2 * n2 && dd <= t2 * n1 && dd < INFINITY;
}

// One hypothesis per lane, one wave per workgroup: sample, 8-point fit without the rank-2 step, denormalised F.
__global__ __launch_bounds__(64) void fmat_hypotheses_kernel(const float *__restrict__ pts1, const float *__restrict__ pts2, int m,
                                                             unsigned long long seed, int first, int count,
                                                             int *__restrict__ idx_out, double *__restrict__ F_out)
{
    __shared__ double lds[(N_TRI + 81) * 64];
    const int j = (int)(blockIdx.x * 64 + threadIdx.x);
    if (j >= count) return;                     // (no barrier below: a lane touches its own LDS column only)
    const unsigned long long h = (unsigned long long)first + (unsigned long long)j;

    int idx[8];
    sample<8>(seed, h, m, idx);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int r = idx[k];
        idx_out[8 * (size_t)j + k] = r;
        idx[k] = AMVS_IDX(r, m);
    }

    double x1[8], y1[8], x2[8], y2[8];
    double sx1 = 0.0, sy1 = 0.0, sx2 = 0.0, sy2 = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        x1[k] = (double)pts1[2 * idx[k]]; y1[k] = (double)pts1[2 * idx[k] + 1];
        x2[k] = (double)pts2[2 * idx[k]]; y2[k] = (double)pts2[2 * idx[k] + 1];
        sx1 = sx1 + x1[k]; sy1 = sy1 + y1[k]; sx2 = sx2 + x2[k]; sy2 = sy2 + y2[k];
    }
    Norm n;
    n.cx1 = sx1 / 8.0; n.cy1 = sy1 / 8.0; n.cx2 = sx2 / 8.0; n.cy2 = sy2 / 8.0;
    double sd1 = 0.0, sd2 = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double u1 = x1[k] - n.cx1, v1 = y1[k] - n.cy1, u2 = x2[k] - n.cx2, v2 = y2[k] - n.cy2;
        sd1 = sd1 + sqrt(u1 * u1 + v1 * v1);
        sd2 = sd2 + sqrt(u2 * u2 + v2 * v2);
    }
    n.s1 = ROOT2 / (sd1 / 8.0);
    n.s2 = ROOT2 / (sd2 / 8.0);

    const JacobiState<9, 64> S{lds + threadIdx.x, lds + N_TRI * 64 + threadIdx.x};
    // M a row at a time: nine accumulators, the rows a recomputed per match (cheaper than 72 doubles of them)
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        double acc[9];
#pragma unroll
        for (int c = i; c < 9; ++c) acc[c] = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            double a[9];
            fmat_row(n, x1[k], y1[k], x2[k], y2[k], a);
#pragma unroll
            for (int c = i; c < 9; ++c) acc[c] = acc[c] + a[i] * a[c];
        }
#pragma unroll
        for (int c = i; c < 9; ++c) S.M(i, c) = acc[c];
    }
    double f[9], F[9];
    jacobi<9, 64>(S, f);
    fmat_denormalise(f, n, F);
#pragma unroll
    for (int e = 0; e < 9; ++e) F_out[9 * (size_t)j + e] = F[e];
}

// counts[h] += inliers of F[h] among this workgroup's 256 matches, for the HYP_TILE hypotheses of blockIdx.y
__global__ __launch_bounds__(256) void fmat_score_kernel(const double *__restrict__ F, int n, const float *__restrict__ pts1,
                                                         const float *__restrict__ pts2, int m, double t2, int *__restrict__ counts)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    const bool live = i < m;
    const int ii = live ? i : 0;
    const double x1 = (double)pts1[2 * ii], y1 = (double)pts1[2 * ii + 1];
    const double x2 = (double)pts2[2 * ii], y2 = (double)pts2[2 * ii + 1];
    const int h1 = Tile::end(n);
    for (int h = Tile::begin(); h < h1; ++h) {
        const double *Fh = F + 9 * (size_t)h;                       // wave-uniform: scalar loads
        tally_wave(live && fmat_is_inlier(Fh, x1, y1, x2, y2, t2), counts, h);
    }
}

// mask[i] and *count for one F
__global__ __launch_bounds__(256) void fmat_inliers_kernel(const FMat F, const float *__restrict__ pts1, const float *__restrict__ pts2,
                                                           int m, double t2, unsigned char *__restrict__ mask, int *__restrict__ count)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    bool in = false;
    if (i < m) {
        in = fmat_is_inlier(F.f, (double)pts1[2 * i], (double)pts1[2 * i + 1], (double)pts2[2 * i], (double)pts2[2 * i + 1], t2);
        mask[i] = in ? 1 : 0;
    }
    tally_wave(in, count);
}

// The block partials of the refit's sums.  pass 0: x1, y1, x2, y2 (4 entries); pass 1: the two distances to the
// centroids (2); pass 2: the upper triangle of M (45).  One lane per (block of 64 matches, entry); part[block][entry].
__global__ __launch_bounds__(256) void fmat_partials_kernel(int pass, int entries, const Norm nrm, const float *__restrict__ pts1,
                                                            const float *__restrict__ pts2, const unsigned char *__restrict__ mask,
                                                            int m, int n_blocks, double *__restrict__ part)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n_blocks * entries) return;
    const int b = (int)(t / entries), e = (int)(t % entries);
    int ei = 0, ej = e;                         // pass 2: entry e is M[ei][ej]
    if (pass == 2)
        while (ej >= 9 - ei) { ej -= 9 - ei; ei += 1; }
    ej += ei;
    const int i1 = (b + 1) * AMVS_FMAT_BLOCK < m ? (b + 1) * AMVS_FMAT_BLOCK : m;
    double acc = 0.0;
    for (int i = b * AMVS_FMAT_BLOCK; i < i1; ++i) {
        if (mask && !mask[i]) continue;
        const double x1 = (double)pts1[2 * i], y1 = (double)pts1[2 * i + 1], x2 = (double)pts2[2 * i], y2 = (double)pts2[2 * i + 1];
        double u;
        if (pass == 0) {
            u = e == 0 ? x1 : e == 1 ? y1 : e == 2 ? x2 : y2;
        } else if (pass == 1) {
            const double du = e == 0 ? x1 - nrm.cx1 : x2 - nrm.cx2, dv = e == 0 ? y1 - nrm.cy1 : y2 - nrm.cy2;
            u = sqrt(du * du + dv * dv);
        } else {
            double a[9];
            fmat_row(nrm, x1, y1, x2, y2, a);
            double ai = a[0], aj = a[0];
#pragma unroll
            for (int k = 1; k < 9; ++k) { ai = ei == k ? a[k] : ai; aj = ej == k ? a[k] : aj; }
            u = ai * aj;
        }
        acc = acc + u;
    }
    part[t] = acc;
}

inline int n_blocks_of(int m) { return (m + AMVS_FMAT_BLOCK - 1) / AMVS_FMAT_BLOCK; }

// SUM of one pass over the set into out[entries]
hipError_t sum_pass(int pass, int entries, const Norm &nrm, const Points2 &P, const unsigned char *mask_d, int m, Work &w, double *out,
                    hipStream_t st)
{
    const int n_blocks = n_blocks_of(m);
    hipLaunchKernelGGL(fmat_partials_kernel, blocks_for((long long)n_blocks * entries, 256), dim3(256), 0, st, pass, entries, nrm, P.a, P.b,
                       mask_d, m, n_blocks, w.part.get<double>());
    STCHK(hipGetLastError());
    return pass_totals(w, n_blocks, entries, out, st);
}

// the refit (steps 1-7 of the header) to the set mask_d (NULL: all) of n_set members
hipError_t refit_dev(const Points2 &P, const unsigned char *mask_d, int m, long long n_set, Work &w, double F[9], hipStream_t st)
{
    const double N = (double)n_set;
    Norm nrm{};
    double s[N_TRI];
    STCHK(sum_pass(0, 4, nrm, P, mask_d, m, w, s, st));
    nrm.cx1 = s[0] / N; nrm.cy1 = s[1] / N; nrm.cx2 = s[2] / N; nrm.cy2 = s[3] / N;
    STCHK(sum_pass(1, 2, nrm, P, mask_d, m, w, s, st));
    nrm.s1 = ROOT2 / (s[0] / N);
    nrm.s2 = ROOT2 / (s[1] / N);
    double tri[N_TRI], V[81], f[9];
    STCHK(sum_pass(2, N_TRI, nrm, P, mask_d, m, w, tri, st));
    jacobi<9, 1>(JacobiState<9, 1>{tri, V}, f);
    // rank 2
    double A[6], VA[9], v[3];
    const JacobiState<3, 1> SA{A, VA};
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) SA.M(i, j) = (f[i] * f[j] + f[3 + i] * f[3 + j]) + f[6 + i] * f[6 + j];
    jacobi<3, 1>(SA, v);
    for (int r = 0; r < 3; ++r) {
        const double wr = (f[3 * r] * v[0] + f[3 * r + 1] * v[1]) + f[3 * r + 2] * v[2];
        for (int c = 0; c < 3; ++c) f[3 * r + c] = f[3 * r + c] - wr * v[c];
    }
    fmat_denormalise(f, nrm, F);
    double q = F[0] * F[0];
    for (int e = 1; e < 9; ++e) q = q + F[e] * F[e];
    const double norm = std::sqrt(q);
    for (int e = 0; e < 9; ++e) F[e] = F[e] / norm;
    int k = 0;
    for (int e = 1; e < 9; ++e)
        if (std::fabs(F[e]) > std::fabs(F[k])) k = e;
    if (F[k] < 0.0)
        for (int e = 0; e < 9; ++e) F[e] = -F[e];
    return hipSuccess;
}

// mask_d[i] and the count of the inliers of F
hipError_t inliers_dev(const double F[9], const Points2 &P, int m, double t2, unsigned char *mask_d, Work &w, long long *count,
                       hipStream_t st)
{
    FMat a;
    std::memcpy(a.f, F, sizeof(a.f));
    return count_inliers(w, count, st, [&](int *count_d) {
        hipLaunchKernelGGL(fmat_inliers_kernel, blocks_for(m, 256), dim3(256), 0, st, a, P.a, P.b, m, t2, mask_d, count_d);
    });
}

void launch_hypotheses(const Points2 &P, int m, uint64_t seed, int first, int count, int *idx_d, double *F_d, hipStream_t st)
{
    hipLaunchKernelGGL(fmat_hypotheses_kernel, blocks_for(count, 64), dim3(64), 0, st, P.a, P.b, m, (unsigned long long)seed, first, count,
                       idx_d, F_d);
}

void launch_score(const double *F_d, int n, const Points2 &P, int m, double t2, int *counts_d, hipStream_t st)
{
    hipLaunchKernelGGL(fmat_score_kernel, Tile::grid(m, n), dim3(256), 0, st, F_d, n, P.a, P.b, m, t2, counts_d);
}

// what ransac_run asks of a model (amvs_ransac_run.h): the fundamental matrix, from samples of eight matches
struct FmatModel {
    static constexpr int SAMPLE = 8, BATCH = AMVS_FMAT_BATCH;
    using Estimate = FMat;
    const float *pts1_h, *pts2_h;
    int m;
    double t2;
    uint64_t seed;
    Points2 P;
    Work w;
    ScratchCache::Lease idx, F;

    hipError_t prepare(ScratchCache &cache, hipStream_t st)
    {
        STCHK(P.upload(pts1_h, pts2_h, m, cache, st));
        STCHK(w.reserve(N_TRI, n_blocks_of(m), cache));
        STCHK(cache.lease(idx, sizeof(int) * 8 * BATCH));
        return cache.lease(F, sizeof(double) * 9 * BATCH);
    }
    void hypotheses(int first, int count, hipStream_t st) { launch_hypotheses(P, m, seed, first, count, idx.get<int>(), F.get<double>(), st); }
    void score(int n, int *counts_d, hipStream_t st) { launch_score(F.get<double>(), n, P, m, t2, counts_d, st); }
    hipError_t fetch(FMat &e, hipStream_t st) { return hipMemcpyAsync(e.f, F.get(), sizeof(e.f), hipMemcpyDeviceToHost, st); }
    hipError_t inliers(const FMat &e, unsigned char *mask, long long *n, hipStream_t st) { return inliers_dev(e.f, P, m, t2, mask, w, n, st); }
    hipError_t refit(FMat &e, const unsigned char *mask, long long n_set, hipStream_t st) { return refit_dev(P, mask, m, n_set, w, e.f, st); }
    static double all_inliers(double wr) { const double w2 = wr * wr, w4 = w2 * w2; return w4 * w4; }     // the header's ((w w)^2)^2
};

}  // namespace

hipError_t fmat_hypotheses(const float *pts1_h, const float *pts2_h, int m, uint64_t seed, int first, int count, int *idx_h,
                           double *F_h, ScratchCache &cache, hipStream_t st)
{
    Points2 P;
    ScratchCache::Lease idx, F;
    STCHK(P.upload(pts1_h, pts2_h, m, cache, st));
    STCHK(cache.lease(idx, sizeof(int) * 8 * (size_t)count));
    STCHK(cache.lease(F, sizeof(double) * 9 * (size_t)count));
    launch_hypotheses(P, m, seed, first, count, idx.get<int>(), F.get<double>(), st);
    STCHK(hipGetLastError());
    STCHK(hipMemcpyAsync(idx_h, idx.get(), sizeof(int) * 8 * (size_t)count, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(F_h, F.get(), sizeof(double) * 9 * (size_t)count, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t fmat_score(const double *F_h, int n, const float *pts1_h, const float *pts2_h, int m, double threshold, int *counts_h,
                      ScratchCache &cache, hipStream_t st)
{
    Points2 P;
    ScratchCache::Lease F, counts;
    STCHK(P.upload(pts1_h, pts2_h, m, cache, st));
    STCHK(cache.lease(F, sizeof(double) * 9 * (size_t)n));
    STCHK(cache.lease(counts, sizeof(int) * (size_t)n));
    STCHK(hipMemcpyAsync(F.get(), F_h, sizeof(double) * 9 * (size_t)n, hipMemcpyHostToDevice, st));
    STCHK(hipMemsetAsync(counts.get(), 0, sizeof(int) * (size_t)n, st));
    launch_score(F.get<double>(), n, P, m, threshold * threshold, counts.get<int>(), st);
    STCHK(hipGetLastError());
    STCHK(hipMemcpyAsync(counts_h, counts.get(), sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t fmat_inliers(const double F[9], const float *pts1_h, const float *pts2_h, int m, double threshold,
                        unsigned char *mask_h, long long *count, ScratchCache &cache, hipStream_t st)
{
    Points2 P;
    Work w;
    ScratchCache::Lease mask;
    STCHK(P.upload(pts1_h, pts2_h, m, cache, st));
    STCHK(w.reserve(N_TRI, n_blocks_of(m), cache));
    STCHK(cache.lease(mask, (size_t)m));
    STCHK(inliers_dev(F, P, m, threshold * threshold, mask.get<unsigned char>(), w, count, st));
    STCHK(hipMemcpyAsync(mask_h, mask.get(), (size_t)m, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t fmat_fit(const float *pts1_h, const float *pts2_h, const unsigned char *mask_h, int m, long long n_set, double F_out[9],
                    ScratchCache &cache, hipStream_t st)
{
    Points2 P;
    Work w;
    ScratchCache::Lease mask;
    STCHK(P.upload(pts1_h, pts2_h, m, cache, st));
    STCHK(w.reserve(N_TRI, n_blocks_of(m), cache));
    if (mask_h) {
        STCHK(cache.lease(mask, (size_t)m));
        STCHK(hipMemcpyAsync(mask.get(), mask_h, (size_t)m, hipMemcpyHostToDevice, st));
    }
    return refit_dev(P, mask_h ? mask.get<unsigned char>() : nullptr, m, n_set, w, F_out, st);
}

hipError_t fmat_ransac(const float *pts1_h, const float *pts2_h, int m, double threshold, double confidence, int max_hypotheses,
                       uint64_t seed, double F_out[9], unsigned char *mask_h, long long *n_inliers, int info[3],
                       ScratchCache &cache, hipStream_t st)
{
    FmatModel model{pts1_h, pts2_h, m, threshold * threshold, seed};
    FMat best{};
    const hipError_t e = ransac_run(model, m, confidence, max_hypotheses, &best, mask_h, n_inliers, info, cache, st);
    std::memcpy(F_out, best.f, sizeof(best.f));
    return e;
}

}  // namespace amvs

AMVS_CHECK_TU(fmat)
