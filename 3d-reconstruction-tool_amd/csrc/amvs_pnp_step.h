// amvs_pnp_step.h -- the host arithmetic of the resection (include/amvs_resection.h): the parameter checks on K and the
// Gauss-Newton STEP of the refit -- the 6 x 6 Cholesky solve and the trig-free rotation update -- in the header's order.
// Plain C++ without the HIP runtime, so that it also compiles into a stand-alone host program (tools/pnp_step_check.cpp).
// Built with -ffp-contract=off like everything else: a * b + c is two roundings.
#pragma once
#include <cmath>

// (the rotation update also runs inside the bundle adjustment's kernels, amvs_bundle.hip)
#ifdef __HIPCC__
#define AMVS_PNP_HD __host__ __device__
#else
#define AMVS_PNP_HD
#endif

namespace amvs {

constexpr int PNP_SUMS = 29;          // the SUMs of a refit pass: H (21), g (6), cost, front
constexpr int PNP_COST = 27, PNP_FRONT = 28;

// the header's errors of K; NULL = fine
inline const char *pnp_intrinsics_error(const double *K)
{
    if (!K) return "NULL K";
    if (!std::isfinite(K[0]) || !(K[0] > 0.0) || !std::isfinite(K[4]) || !(K[4] > 0.0)) return "fx and fy must be positive and finite";
    if (!std::isfinite(K[2]) || !std::isfinite(K[5])) return "cx and cy must be finite";
    if (K[1] != 0.0) return "K must have no skew";
    return nullptr;
}

// the pose update of a STEP: (Rn, tn) from (R, t) and the solution x = (om, dt)
AMVS_PNP_HD inline void pnp_pose_update(const double x[6], const double R[9], const double t[3], double Rn[9], double tn[3])
{
    const double hx = 0.5 * x[0], hy = 0.5 * x[1], hz = 0.5 * x[2];
    const double n = std::sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
    const double qw = 1.0 / n, qx = hx / n, qy = hy / n, qz = hz / n;
    const double Q[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qz * qw), 2.0 * (qx * qz + qy * qw),
                         2.0 * (qx * qy + qz * qw), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qx * qw),
                         2.0 * (qx * qz - qy * qw), 2.0 * (qy * qz + qx * qw), 1.0 - 2.0 * (qx * qx + qy * qy)};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Rn[3 * r + c] = (Q[3 * r] * R[c] + Q[3 * r + 1] * R[3 + c]) + Q[3 * r + 2] * R[6 + c];
        tn[r] = ((Q[3 * r] * t[0] + Q[3 * r + 1] * t[1]) + Q[3 * r + 2] * t[2]) + x[3 + r];
    }
}

// STEP from the sums of a pass: (Rn, tn) from (R, t); false when a pivot is not positive and finite (no step)
inline bool pnp_gn_step(const double sums[PNP_SUMS], const double R[9], const double t[3], double Rn[9], double tn[3])
{
    double H[6][6], L[6][6], y[6], x[6];
    int e = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) H[i][j] = sums[e++];
    const double *g = sums + 21;
    for (int j = 0; j < 6; ++j) {
        double s = H[j][j];
        for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
        if (!(s > 0.0 && s < INFINITY)) return false;
        L[j][j] = std::sqrt(s);
        for (int i = j + 1; i < 6; ++i) {
            double v = H[j][i];
            for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    for (int i = 0; i < 6; ++i) {
        double s = -g[i];
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    pnp_pose_update(x, R, t, Rn, tn);
    return true;
}

}  // namespace amvs
