// twoview_host_check.cpp -- the host arithmetic of the two-view start (csrc/amvs_twoview_host.h: the checks on K, the 3 x 3
// Jacobi iteration, the decomposition of F into the four pose candidates, the projection matrices) as a stand-alone host
// program, so that it can run under the host sanitizers without the library, Python or a GPU:
//
//     clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I 3d-reconstruction-tool_amd/csrc tools/twoview_host_check.cpp -o /tmp/twoview_host_check && /tmp/twoview_host_check
//
// (and the same line with g++).  It plants a pose (12 degrees about an axis near y, a unit baseline), forms the exact F,
// decomposes it and looks for the planted pose among the four candidates; then it feeds the F that must give no model:
// zero, rank 1, NaN and infinite entries.  Exit status 0 and "ok" when everything holds.
#include "amvs_twoview_host.h"

#include <cstdio>
#include <initializer_list>
#include <limits>

using namespace amvs;

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

static const double K[9] = {1500.0, 0.0, 960.0, 0.0, 1500.0, 540.0, 0.0, 0.0, 1.0};

static void mul3(const double A[9], const double B[9], double C[9])
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}

static double max_diff(const double *a, const double *b, int n)
{
    double d = 0.0;
    for (int e = 0; e < n; ++e) d = std::fmax(d, std::fabs(a[e] - b[e]));
    return d;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // the checks on K
    REQUIRE(pnp_intrinsics_error(K) == nullptr && pnp_intrinsics_error(nullptr) != nullptr);
    const struct { int at; double v; } bad[] = {{0, 0.0}, {0, -1.0}, {0, inf}, {0, nan}, {4, 0.0}, {4, nan}, {2, inf}, {5, nan}, {1, 0.5}};
    for (const auto &b : bad) {
        double Kb[9];
        for (int e = 0; e < 9; ++e) Kb[e] = K[e];
        Kb[b.at] = b.v;
        REQUIRE(pnp_intrinsics_error(Kb) != nullptr);
    }

    // the 3 x 3 Jacobi iteration on a matrix with known eigenvalues: Q diag(5, 2, -1) Q^T, Q a rotation
    const double th = 0.7, c = std::cos(th), s = std::sin(th);
    const double Qz[9] = {c, -s, 0, s, c, 0, 0, 0, 1}, Qx[9] = {1, 0, 0, 0, c, -s, 0, s, c};
    double Q[9];
    mul3(Qz, Qx, Q);
    const double lam[3] = {5.0, 2.0, -1.0};
    double G[3][3], V[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) G[i][j] = Q[3 * i] * lam[0] * Q[3 * j] + Q[3 * i + 1] * lam[1] * Q[3 * j + 1] + Q[3 * i + 2] * lam[2] * Q[3 * j + 2];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < i; ++j) G[i][j] = G[j][i];
    double G0[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) G0[i][j] = G[i][j];
    twoview_jacobi3(G, V);
    double trace = 0.0;
    for (int k = 0; k < 3; ++k) {
        trace += G[k][k];
        double best = 1e300;
        for (int e = 0; e < 3; ++e) best = std::fmin(best, std::fabs(G[k][k] - lam[e]));
        REQUIRE(best < 1e-12);
        for (int r = 0; r < 3; ++r) {                                        // G0 v = w v
            const double gv = G0[r][0] * V[0][k] + G0[r][1] * V[1][k] + G0[r][2] * V[2][k];
            REQUIRE(std::fabs(gv - G[k][k] * V[r][k]) < 1e-12);
        }
    }
    REQUIRE(std::fabs(trace - 6.0) < 1e-12 && G[0][1] == 0.0 && G[0][2] == 0.0 && G[1][2] == 0.0);
    double Z[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};                     // a zero matrix: every pair is skipped
    twoview_jacobi3(Z, V);
    REQUIRE(V[0][0] == 1.0 && V[1][1] == 1.0 && V[2][2] == 1.0 && V[0][1] == 0.0 && Z[0][0] == 0.0);
    double N[3][3] = {{nan, 1, 0}, {1, inf, 2}, {0, 2, 1}};                 // NaN and infinity go through without a trap
    twoview_jacobi3(N, V);

    // a planted pose: Rodrigues about (0.1, 1, 0.05) by 12 degrees, centre (1, 0.05, 0.1) normalised
    double ax[3] = {0.1, 1.0, 0.05}, C[3] = {1.0, 0.05, 0.1};
    const double an = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]), cn = std::sqrt(C[0] * C[0] + C[1] * C[1] + C[2] * C[2]);
    for (int e = 0; e < 3; ++e) { ax[e] /= an; C[e] /= cn; }
    const double a12 = 12.0 * 3.14159265358979323846 / 180.0, ca = std::cos(a12), sa = std::sin(a12);
    const double Kx[9] = {0, -ax[2], ax[1], ax[2], 0, -ax[0], -ax[1], ax[0], 0};
    double Kx2[9], R[9], t[3];
    mul3(Kx, Kx, Kx2);
    for (int e = 0; e < 9; ++e) R[e] = (e % 4 == 0 ? 1.0 : 0.0) + sa * Kx[e] + (1.0 - ca) * Kx2[e];
    for (int r = 0; r < 3; ++r) t[r] = -(R[3 * r] * C[0] + R[3 * r + 1] * C[1] + R[3 * r + 2] * C[2]);
    // F = K^-T [t]x R K^-1
    const double Ki[9] = {1.0 / K[0], 0.0, -K[2] / K[0], 0.0, 1.0 / K[4], -K[5] / K[4], 0.0, 0.0, 1.0};
    const double KiT[9] = {Ki[0], 0.0, 0.0, 0.0, Ki[4], 0.0, Ki[2], Ki[5], 1.0};
    const double Tx[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
    double TR[9], TRK[9], F[9];
    mul3(Tx, R, TR);
    mul3(TR, Ki, TRK);
    mul3(KiT, TRK, F);
    double E[3][3], Ex[9];
    twoview_essential(F, K, E);
    for (int r = 0; r < 3; ++r)
        for (int cc = 0; cc < 3; ++cc) Ex[3 * r + cc] = E[r][cc];
    REQUIRE(max_diff(Ex, TR, 9) < 1e-12);                                    // K^T F K is [t]x R again

    double R2[18], td[3], w[3];
    REQUIRE(twoview_decompose(F, K, R2, td, w));
    REQUIRE(w[0] >= w[1] && w[1] > 0.0 && std::fabs(w[0] - 1.0) < 1e-12 && std::fabs(w[1] - 1.0) < 1e-12 && std::fabs(w[2]) < 1e-12);
    int hits = 0;
    double dR = 1e300, dt = 1e300;
    for (int j = 0; j < 4; ++j) {
        double Rj[9], tj[3];
        twoview_candidate(R2, td, j, Rj, tj);
        const double a = max_diff(Rj, R, 9), b = max_diff(tj, t, 3);
        if (a < 1e-9 && b < 1e-9) hits += 1;
        dR = std::fmin(dR, a);
        dt = std::fmin(dt, b);
        for (int p = 0; p < 3; ++p)
            for (int q = 0; q < 3; ++q) {
                const double d = Rj[p] * Rj[q] + Rj[3 + p] * Rj[3 + q] + Rj[6 + p] * Rj[6 + q];
                REQUIRE(std::fabs(d - (p == q ? 1.0 : 0.0)) < 1e-12);
            }
        REQUIRE(std::signbit(tj[0]) == (j < 2 ? std::signbit(td[0]) : !std::signbit(td[0])));
    }
    std::printf("planted pose among the four candidates: %d, nearest differs by %.3e in R and %.3e in t\n", hits, dR, dt);
    REQUIRE(hits == 1);

    // the projection matrices: the first camera gives K [I | 0] and a centre of zeros
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero3[3] = {0, 0, 0};
    double P[12], Cc[3];
    twoview_projection(K, I, zero3, P, Cc);
    for (int r = 0; r < 3; ++r) {
        for (int cc = 0; cc < 3; ++cc) REQUIRE(P[4 * r + cc] == K[3 * r + cc]);
        REQUIRE(P[4 * r + 3] == 0.0 && Cc[r] == 0.0);
    }
    twoview_projection(K, R, t, P, Cc);
    REQUIRE(max_diff(Cc, C, 3) < 1e-12);

    // F without a model: zero, rank 1, NaN, infinite; the outputs are zero
    double F0[9] = {0}, F1[9], Fn[9], Fi[9];
    const double u[3] = {0.3, -0.2, 1.0}, v[3] = {-0.1, 0.4, 1.0};
    for (int e = 0; e < 9; ++e) { F1[e] = 1e-6 * u[e / 3] * v[e % 3]; Fn[e] = F[e]; Fi[e] = F[e]; }
    Fn[4] = nan;
    Fi[2] = inf;
    for (const double *Fx : {(const double *)F0, (const double *)F1, (const double *)Fn, (const double *)Fi}) {
        for (int e = 0; e < 18; ++e) R2[e] = 7.0;
        REQUIRE(!twoview_decompose(Fx, K, R2, td, w));
        for (int e = 0; e < 18; ++e) REQUIRE(R2[e] == 0.0);
        for (int e = 0; e < 3; ++e) REQUIRE(td[e] == 0.0 && w[e] == 0.0);
    }
    for (int e = 0; e < 9; ++e) Fi[e] = inf;                                 // all infinite, all NaN: no trap, no model
    REQUIRE(!twoview_decompose(Fi, K, R2, td, w));
    for (int e = 0; e < 9; ++e) Fn[e] = nan;
    REQUIRE(!twoview_decompose(Fn, K, R2, td, w));
    std::printf("ok\n");
    return 0;
}
