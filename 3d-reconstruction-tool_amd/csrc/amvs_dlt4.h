// amvs_dlt4.h -- the per-candidate two-view DLT of include/amvs_match.h steps 1 to 4 for the device: the four rows of A,
// M = A^T A, the fixed-sweep cyclic Jacobi iteration with M and V in registers (the (p, q) pairs are template arguments,
// so every index is a constant) and the column of the smallest diagonal entry.  Shared by amvs_triangulate.hip
// (amvs_pair_triangulate) and amvs_twoview.hip (include/amvs_twoview.h).  Private to the library.  No data-dependent
// index is formed here, so nothing goes through amvs_check.h.
//
// -ffp-contract=off (Makefile): a * b + c below is two roundings.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/amvs_match.h"

namespace amvs {

// one Jacobi rotation of the header's step 3 on the pair (P, Q)
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&M)[4][4], double (&V)[4][4])
{
    const double g = M[P][Q];
    if (g == 0.0) return;
    const double theta = (M[Q][Q] - M[P][P]) / (2.0 * g);
    double t;
    if (fabs(theta) > 1e150) t = 0.5 / theta;
    else t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    M[P][P] = M[P][P] - t * g;
    M[Q][Q] = M[Q][Q] + t * g;
    M[P][Q] = 0.0;
    M[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r == P || r == Q) continue;
        const double x = M[r][P], y = M[r][Q];
        M[r][P] = M[P][r] = c * x - s * y;
        M[r][Q] = M[Q][r] = s * x + c * y;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double x = V[r][P], y = V[r][Q];
        V[r][P] = c * x - s * y;
        V[r][Q] = s * x + c * y;
    }
}

// steps 1 to 3 for the match (x1, y1), (x2, y2) under the row-major 3 x 4 matrices P1, P2: v = the column of V that
// belongs to the smallest diagonal entry (step 4 divides it by v[3])
__device__ __forceinline__ void dlt4_null_vector(const double *P1, const double *P2, double x1, double y1, double x2, double y2,
                                                 double v[4])
{
    double A[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        A[0][c] = x1 * P1[8 + c] - P1[c];
        A[1][c] = y1 * P1[8 + c] - P1[4 + c];
        A[2][c] = x2 * P2[8 + c] - P2[c];
        A[3][c] = y2 * P2[8 + c] - P2[4 + c];
    }
    double M[4][4], V[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = r; c < 4; ++c) {
            const double e = ((A[0][r] * A[0][c] + A[1][r] * A[1][c]) + A[2][r] * A[2][c]) + A[3][r] * A[3][c];
            M[r][c] = e;
            M[c][r] = e;
        }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < AMVS_JACOBI_SWEEPS; ++sweep) {
        jacobi_rotate<0, 1>(M, V); jacobi_rotate<0, 2>(M, V); jacobi_rotate<0, 3>(M, V);
        jacobi_rotate<1, 2>(M, V); jacobi_rotate<1, 3>(M, V); jacobi_rotate<2, 3>(M, V);
    }
    double best = M[0][0];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = V[r][0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (M[k][k] < best) {
            best = M[k][k];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = V[r][k];
        }
}

}  // namespace amvs
