// amvs_ransac_common.h -- what the units with hypothesis and scoring kernels share (amvs_fmat.hip, amvs_pnp.hip; the
// scoring pieces, Points and blocks_for also amvs_twoview.hip): the fixed-sweep cyclic Jacobi of include/amvs_match.h
// step 3 on an N x N symmetric matrix, for the device (state in LDS, one column a lane) and the host (state in plain
// arrays); the counter-based sampler of include/amvs_epipolar.h; the tile of a scoring launch and the wave's tally of a
// predicate; the two point arrays of a call on the device.  Private to the library.  No kernel is defined here (the two
// the RANSAC units share are in amvs_ransac_run.h), and no global-memory access with a data-dependent index is made:
// the sampler returns its draw and the kernel that gathers with it checks it (amvs_check.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/amvs_match.h"
#include "amvs_buffer.h"

namespace amvs {

// the symmetric matrix (upper triangle) and the eigenvector matrix of a Jacobi iteration, element e at base[e * STRIDE]
template <int N, int STRIDE>
struct JacobiState {
    double *m, *v;
    __host__ __device__ __forceinline__ double &M(int i, int j) const
    {
        const int a = i < j ? i : j, b = i < j ? j : i;
        return m[(a * N - a * (a - 1) / 2 + (b - a)) * STRIDE];
    }
    __host__ __device__ __forceinline__ double &V(int r, int c) const { return v[(r * N + c) * STRIDE]; }
};

// amvs_match.h step 3 on N x N: the sweeps, then the column of the smallest diagonal entry into f
template <int N, int STRIDE>
__host__ __device__ __forceinline__ void jacobi(const JacobiState<N, STRIDE> &S, double *f)
{
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) S.V(r, c) = r == c ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < AMVS_JACOBI_SWEEPS; ++sweep) {
        // (every pair a compile-time constant, so that every LDS offset is an immediate: at 12 x 12 the unrolled sweep is
        // above the compiler's default limit for a pragma, which the Makefile raises for amvs_pnp.o)
#pragma unroll
        for (int p = 0; p < N - 1; ++p)
#pragma unroll
            for (int q = p + 1; q < N; ++q) {
                const double g = S.M(p, q);
                if (g == 0.0) continue;
                const double theta = (S.M(q, q) - S.M(p, p)) / (2.0 * g);
                double t;
                if (fabs(theta) > 1e150) t = 0.5 / theta;
                else t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                S.M(p, p) = S.M(p, p) - t * g;
                S.M(q, q) = S.M(q, q) + t * g;
                S.M(p, q) = 0.0;
#pragma unroll
                for (int r = 0; r < N; ++r) {
                    if (r == p || r == q) continue;
                    const double x = S.M(r, p), y = S.M(r, q);
                    S.M(r, p) = c * x - s * y;
                    S.M(r, q) = s * x + c * y;
                }
#pragma unroll
                for (int r = 0; r < N; ++r) {
                    const double x = S.V(r, p), y = S.V(r, q);
                    S.V(r, p) = c * x - s * y;
                    S.V(r, q) = s * x + c * y;
                }
            }
    }
    double best = S.M(0, 0);
    int at = 0;
#pragma unroll
    for (int k = 1; k < N; ++k)
        if (S.M(k, k) < best) { best = S.M(k, k); at = k; }
#pragma unroll
    for (int r = 0; r < N; ++r) f[r] = S.V(r, at);
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The sampler: draw[0 .. K) = the K distinct indices of [0, m) of hypothesis h in the order drawn -- member k a draw from
// the m - k indices left, shifted past the kept ones.  The kernel that gathers with them checks them (amvs_check.h).
template <int K>
__device__ __forceinline__ void sample(unsigned long long seed, unsigned long long h, int m, int *draw)
{
    int sorted[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int r = (int)(mix64(seed ^ mix64((unsigned long long)K * h + (unsigned long long)k)) % (unsigned long long)(m - k));
#pragma unroll
        for (int i = 0; i < k; ++i)
            if (r >= sorted[i]) r += 1;
        draw[k] = r;
        int v = r;                              // insert into the ascending list
#pragma unroll
        for (int i = 0; i < k; ++i)
            if (v < sorted[i]) { const int tmp = sorted[i]; sorted[i] = v; v = tmp; }
        sorted[k] = v;
    }
}

// counters[at] += the lanes of this wave with `in` set (every lane of the wave calls; no add for a zero).  The index
// comes separately so that the address is formed where it is used, after the count: formed by the caller, it moves an
// instruction of twoview_score_kernel.
__device__ __forceinline__ void tally_wave(bool in, int *counters, size_t at = 0)
{
    const int c = __popcll(__ballot(in));
    if (c != 0 && (threadIdx.x & 63) == 0) atomicAdd(&counters[at], c);
}

// A scoring launch: workgroups of 256 correspondences in x, TILE hypotheses a workgroup in y.  The kernel walks
// [begin(), end(n)) and its launch takes grid(m, n), so the two cannot disagree on TILE.
template <int TILE>
struct ScoreTile {
    __device__ static __forceinline__ int begin() { return (int)blockIdx.y * TILE; }
    __device__ static __forceinline__ int end(int n) { const int h0 = begin(); return h0 + TILE < n ? h0 + TILE : n; }
    static dim3 grid(int m, int n) { return dim3((unsigned)((m + 255) / 256), (unsigned)((n + TILE - 1) / TILE)); }
};

// workgroups of `per` for n items
inline dim3 blocks_for(long long n, int per) { return dim3((unsigned)((n + per - 1) / per)); }

// the two point arrays of a call, m x D1 and m x D2 floats, on the device in one lease
template <int D1, int D2>
struct Points {
    ScratchCache::Lease buf;
    const float *a = nullptr, *b = nullptr;
    hipError_t upload(const float *ha, const float *hb, int m, ScratchCache &cache, hipStream_t st)
    {
        const size_t na = D1 * (size_t)m, nb = D2 * (size_t)m;
        hipError_t e = cache.lease(buf, sizeof(float) * (na + nb));
        if (e != hipSuccess) return e;
        float *d = buf.get<float>();
        a = d;
        b = d + na;
        e = hipMemcpyAsync(d, ha, sizeof(float) * na, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        return hipMemcpyAsync(d + na, hb, sizeof(float) * nb, hipMemcpyHostToDevice, st);
    }
};

}  // namespace amvs
