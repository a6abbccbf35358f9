// amvs_ransac_common.h -- what the RANSAC units share (amvs_fmat.hip, amvs_pnp.hip): the fixed-sweep cyclic Jacobi of
// include/amvs_match.h step 3 on an N x N symmetric matrix, for the device (state in LDS, one column a lane) and the
// host (state in plain arrays); the mix() of the counter-based sampler of include/amvs_epipolar.h; the kernel that adds
// block partials in ascending order and the one that finds the best count of a batch.  Private to the library.  The
// kernels are static: each unit that launches them compiles its own.  No data-dependent global-memory index is formed
// here, so nothing goes through amvs_check.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/amvs_match.h"

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

// out[0] = count, out[1] = hypothesis of the best of counts[0 .. n): count descending, index ascending.  One workgroup.
static __global__ __launch_bounds__(1024) void fmat_argmax_kernel(const int *__restrict__ counts, int n, int first, int *__restrict__ out)
{
    __shared__ unsigned long long sh[1024];
    unsigned long long best = 0ull;
    for (int j = (int)threadIdx.x; j < n; j += 1024) {
        const unsigned long long key = ((unsigned long long)(unsigned)counts[j] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)j);
        if (key > best) best = key;
    }
    sh[threadIdx.x] = best;
    __syncthreads();
    for (int step = 512; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step && sh[threadIdx.x + step] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (int)(sh[0] >> 32);
        out[1] = first + (int)(0xFFFFFFFFu - (unsigned)(sh[0] & 0xFFFFFFFFull));
    }
}

// total[e] = the partials of entry e added in ascending block order, from +0.0
static __global__ __launch_bounds__(64) void fmat_total_kernel(const double *__restrict__ part, int n_blocks, int entries, double *__restrict__ total)
{
    const int e = (int)threadIdx.x;
    if (e >= entries) return;
    double acc = 0.0;
    for (int b = 0; b < n_blocks; ++b) acc = acc + part[(size_t)b * entries + e];
    total[e] = acc;
}

}  // namespace amvs
