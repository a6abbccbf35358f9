// amvs_twoview_host.h -- the host arithmetic of include/amvs_twoview.h: the 3 x 3 Jacobi iteration, the decomposition of
// F into the four pose candidates, and the projection matrices and camera centres of a triangulation call -- in the
// header's order.  The checks on K are those of amvs_pnp_step.h.  Plain C++ without the HIP runtime, so that it also
// compiles into a stand-alone host program (tools/twoview_host_check.cpp).  Built with -ffp-contract=off like everything
// else: a * b + c is two roundings.
#pragma once
#include <cmath>

#include "amvs_pnp_step.h"

namespace amvs {

constexpr int TWOVIEW_JACOBI_SWEEPS = 10;      // AMVS_JACOBI_SWEEPS of include/amvs_match.h (asserted in amvs_twoview.hip)

// JACOBI3 of the header: G becomes (nearly) diagonal, V its eigenvectors by columns
inline void twoview_jacobi3(double G[3][3], double V[3][3])
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) V[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < TWOVIEW_JACOBI_SWEEPS; ++sweep)
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double g = G[p][q];
                if (g == 0.0) continue;
                const double theta = (G[q][q] - G[p][p]) / (2.0 * g);
                double t;
                if (std::fabs(theta) > 1e150) t = 0.5 / theta;
                else t = (theta < 0.0 ? -1.0 : 1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                G[p][p] = G[p][p] - t * g;
                G[q][q] = G[q][q] + t * g;
                G[p][q] = 0.0;
                G[q][p] = 0.0;
                for (int r = 0; r < 3; ++r) {
                    if (r == p || r == q) continue;
                    const double x = G[r][p], y = G[r][q];
                    G[r][p] = G[p][r] = c * x - s * y;
                    G[r][q] = G[q][r] = s * x + c * y;
                }
                for (int r = 0; r < 3; ++r) {
                    const double x = V[r][p], y = V[r][q];
                    V[r][p] = c * x - s * y;
                    V[r][q] = s * x + c * y;
                }
            }
}

inline void twoview_cross(const double a[3], const double b[3], double out[3])
{
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// E = K^T F K of the header, row-major
inline void twoview_essential(const double F[9], const double K[9], double E[3][3])
{
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    double T[3][3];
    for (int r = 0; r < 3; ++r) {
        T[r][0] = F[3 * r] * fx;
        T[r][1] = F[3 * r + 1] * fy;
        T[r][2] = (F[3 * r] * cx + F[3 * r + 1] * cy) + F[3 * r + 2];
    }
    for (int c = 0; c < 3; ++c) {
        E[0][c] = fx * T[0][c];
        E[1][c] = fy * T[1][c];
        E[2][c] = (cx * T[0][c] + cy * T[1][c]) + T[2][c];
    }
}

// amvs_twoview_decompose: Ra, Rb (R[0 .. 8], R[9 .. 17]), t and w = (w[k1], w[k2], w[k3]); false and zeros: no model
inline bool twoview_decompose(const double F[9], const double K[9], double R[18], double t[3], double w_out[3])
{
    for (int e = 0; e < 18; ++e) R[e] = 0.0;
    for (int e = 0; e < 3; ++e) t[e] = w_out[e] = 0.0;
    double E[3][3], G[3][3], V[3][3];
    twoview_essential(F, K, E);
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) G[i][j] = G[j][i] = (E[0][i] * E[0][j] + E[1][i] * E[1][j]) + E[2][i] * E[2][j];
    twoview_jacobi3(G, V);
    const double w[3] = {G[0][0], G[1][1], G[2][2]};
    int k3 = 0;
    if (w[1] < w[k3]) k3 = 1;
    if (w[2] < w[k3]) k3 = 2;
    const int a = k3 == 0 ? 1 : 0, b = k3 == 2 ? 1 : 2;
    int k1 = a, k2 = b;
    if (w[b] > w[a]) { k1 = b; k2 = a; }
    if (!(w[k2] > 0.0 && w[k2] < INFINITY)) return false;
    double v1[3], v2[3], v3[3], u1[3], u2[3], u3[3];
    for (int r = 0; r < 3; ++r) { v1[r] = V[r][k1]; v2[r] = V[r][k2]; }
    twoview_cross(v1, v2, v3);
    const double s1 = std::sqrt(w[k1]), s2 = std::sqrt(w[k2]);
    for (int r = 0; r < 3; ++r) {
        u1[r] = ((E[r][0] * v1[0] + E[r][1] * v1[1]) + E[r][2] * v1[2]) / s1;
        u2[r] = ((E[r][0] * v2[0] + E[r][1] * v2[1]) + E[r][2] * v2[2]) / s2;
    }
    twoview_cross(u1, u2, u3);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            R[3 * r + c] = (u2[r] * v1[c] - u1[r] * v2[c]) + u3[r] * v3[c];
            R[9 + 3 * r + c] = (u1[r] * v2[c] - u2[r] * v1[c]) + u3[r] * v3[c];
        }
        t[r] = u3[r];
    }
    w_out[0] = w[k1]; w_out[1] = w[k2]; w_out[2] = w[k3];
    return true;
}

// candidate j = 0 .. 3 of the header's order: (Ra, t) (Rb, t) (Ra, -t) (Rb, -t)
inline void twoview_candidate(const double R[18], const double t[3], int j, double Rj[9], double tj[3])
{
    for (int e = 0; e < 9; ++e) Rj[e] = R[9 * (j & 1) + e];
    for (int e = 0; e < 3; ++e) tj[e] = j < 2 ? t[e] : -t[e];
}

// P = K [R | t] (row-major 3 x 4) and the camera centre C of include/amvs_match.h
inline void twoview_projection(const double K[9], const double R[9], const double t[3], double P[12], double C[3])
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            const double rt0 = c < 3 ? R[c] : t[0], rt1 = c < 3 ? R[3 + c] : t[1], rt2 = c < 3 ? R[6 + c] : t[2];
            P[4 * r + c] = (K[3 * r] * rt0 + K[3 * r + 1] * rt1) + K[3 * r + 2] * rt2;
        }
    for (int i = 0; i < 3; ++i) C[i] = -((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]);
}

}  // namespace amvs
