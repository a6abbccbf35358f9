// amvs_bundle.hip -- bundle adjustment: Levenberg-Marquardt over all free poses and all points through the Schur
// complement on the camera block (include/amvs_bundle.h; the definition is the header's, the judge
// tests/bundle_restatement.py, bit for bit).  The host builds three integer lists once per call (amvs_bundle_host.h);
// the state, the sums, S and the step stay on the device, and a trial of amvs_ba_solve reads back three doubles.
//
// Every kernel forms the terms of an observation again from the state (obs_terms: about 60 operations) instead of
// reading 40 stored doubles per observation.
// ba_point_kernel: one lane per point, serial over its observations: V, gp, the count, the 3 x 3 factor, held.
// ba_cam_partials_kernel / ba_cam_total_kernel: the 29 sums per camera, one lane per (block of 64 list positions,
//     entry), then one lane per (camera, entry) adding the partials in ascending order (as pnp_partials_kernel does).
// ba_schur_partials_kernel / ba_schur_assemble_kernel: the same shape over the pair segments, one lane per (block, row of
//     the 6 x 6 term): Y_k[i] once, then six entries and the right-hand side; the assembly, one lane per (segment, entry),
//     subtracts the totals from U', mirrors, and writes the right-hand side.
// ba_chol_diag_kernel / ba_chol_rows_kernel / ba_chol_update_kernel: right-looking Cholesky in panels of 32 columns, in
//     place in the lower triangle.  Every entry still subtracts its products in ascending k: the update of a panel
//     subtracts the 32 products of that panel in order, and panels follow each other in order.  Every dependency is a
//     kernel boundary: one workgroup factors the diagonal block of a panel in LDS; the next launch solves one row below
//     it per lane and only reads the block; the third updates the trailing triangle and only reads the panel.
// ba_solve_kernel: the two triangular solves, one workgroup, the vector in LDS, column-oriented by panels.
// ba_point_step_kernel / ba_pose_step_kernel: the back-substitution and the candidate state.
// No atomics on floating-point values, no grid-wide barrier, no cooperative launch.
//
//
// AMVS_BA_TIMES=<file> in the environment makes amvs_ba_solve append one line per trial to that file: the sizes and the
// milliseconds of each kernel family between HIP events (tools/bundle_time.py reads it).  Unset, no event is created.
//
// -ffp-contract=off (Makefile): a * b + c below is two roundings.
#define AMVS_TU_ID 25
#include "amvs_check.h"
#include "amvs_bundle_dev.h"
#include "amvs_bundle_host.h"
#include "amvs_handles.h"
#include "amvs_pose.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace amvs {

namespace {

constexpr int NB = 32;                // columns of a Cholesky panel, and the side of an update tile

// the device arrays of a problem and of one state
struct Prob {
    const int *cam, *pt;
    const float *uv;
    int C, P, N;
    Intr k;
};
struct State { double *R, *t, *X; };

struct Obs {
    bool active;
    double rx, ry, Jx[6], Jy[6], Px[3], Py[3];
};

// the header's terms of an observation of point X by camera (R, t) at (u, v)
__device__ __forceinline__ void obs_terms(const double *__restrict__ R, const double *__restrict__ t, const double *__restrict__ X,
                                          double u, double v, const Intr &k, Obs &o)
{
    double Xc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) Xc[r] = ((R[3 * r] * X[0] + R[3 * r + 1] * X[1]) + R[3 * r + 2] * X[2]) + t[r];
    const double z = Xc[2];
    o.active = z > 0.0;
    const double iz = 1.0 / z, xz = Xc[0] * iz, yz = Xc[1] * iz;
    o.rx = (k.fx * xz + k.cx) - u;
    o.ry = (k.fy * yz + k.cy) - v;
    const double ax = k.fx * iz, ay = k.fy * iz, bx = -(ax * xz), by = -(ay * yz);
    o.Jx[0] = bx * Xc[1]; o.Jx[1] = ax * z - bx * Xc[0]; o.Jx[2] = -(ax * Xc[1]); o.Jx[3] = ax; o.Jx[4] = 0.0; o.Jx[5] = bx;
    o.Jy[0] = by * Xc[1] - ay * z; o.Jy[1] = -(by * Xc[0]); o.Jy[2] = ay * Xc[0]; o.Jy[3] = 0.0; o.Jy[4] = ay; o.Jy[5] = by;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        o.Px[j] = ax * R[j] + bx * R[6 + j];
        o.Py[j] = ay * R[3 + j] + by * R[6 + j];
    }
}

// the terms of observation k of the problem under a state
__device__ __forceinline__ void obs_of(const Prob &q, const State &s, int k, Obs &o)
{
    const int c = AMVS_IDX(q.cam[k], q.C), p = AMVS_IDX(q.pt[k], q.P);
    obs_terms(s.R + 9 * (size_t)c, s.t + 3 * (size_t)c, s.X + 3 * (size_t)p, (double)q.uv[2 * (size_t)k], (double)q.uv[2 * (size_t)k + 1], q.k, o);
}

// a[i] without a dynamic index into registers
__device__ __forceinline__ double pick6(const double a[6], int i)
{
    double v = a[0];
#pragma unroll
    for (int s = 1; s < 6; ++s) v = i == s ? a[s] : v;
    return v;
}

// solve3 of the header with the factor Lp = [L00, L10, L11, L20, L21, L22]
__device__ __forceinline__ void solve3(const double *__restrict__ Lp, const double b[3], double x[3])
{
    const double y0 = b[0] / Lp[0];
    const double y1 = (b[1] - Lp[1] * y0) / Lp[2];
    const double y2 = ((b[2] - Lp[3] * y0) - Lp[4] * y1) / Lp[5];
    x[2] = y2 / Lp[5];
    x[1] = (y1 - Lp[4] * x[2]) / Lp[2];
    x[0] = ((y0 - Lp[1] * x[1]) - Lp[3] * x[2]) / Lp[0];
}

__device__ __forceinline__ bool pivot_ok(double s) { return s > 0.0 && s < INFINITY; }

// err2[k] = the squared pixel error of an active observation, -1.0 of an inactive one
__global__ __launch_bounds__(256) void ba_err_kernel(const Prob q, const State s, double *__restrict__ err2)
{
    const int k = (int)(blockIdx.x * 256 + threadIdx.x);
    if (k >= q.N) return;
    Obs o;
    obs_of(q, s, k, o);
    err2[k] = o.active ? o.rx * o.rx + o.ry * o.ry : -1.0;
}

// One lane per point: V [P][6], gp [P][3], cnt [P]; with Lp != NULL also the factor of V' under lambda and held [P].
__global__ __launch_bounds__(256) void ba_point_kernel(const Prob q, const State s, const int *__restrict__ pt_start, double lambda,
                                                       int refine_points, double *__restrict__ V, double *__restrict__ gp,
                                                       int *__restrict__ cnt, double *__restrict__ Lp, unsigned char *__restrict__ held)
{
    const int p = (int)(blockIdx.x * 256 + threadIdx.x);
    if (p >= q.P) return;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
    int n = 0;
    for (int k = pt_start[p]; k < pt_start[p + 1]; ++k) {
        Obs o;
        obs_of(q, s, AMVS_IDX(k, q.N), o);
        if (!o.active) continue;
        v[0] = v[0] + (o.Px[0] * o.Px[0] + o.Py[0] * o.Py[0]);
        v[1] = v[1] + (o.Px[0] * o.Px[1] + o.Py[0] * o.Py[1]);
        v[2] = v[2] + (o.Px[0] * o.Px[2] + o.Py[0] * o.Py[2]);
        v[3] = v[3] + (o.Px[1] * o.Px[1] + o.Py[1] * o.Py[1]);
        v[4] = v[4] + (o.Px[1] * o.Px[2] + o.Py[1] * o.Py[2]);
        v[5] = v[5] + (o.Px[2] * o.Px[2] + o.Py[2] * o.Py[2]);
#pragma unroll
        for (int i = 0; i < 3; ++i) g[i] = g[i] + (o.Px[i] * o.rx + o.Py[i] * o.ry);
        n += 1;
    }
#pragma unroll
    for (int e = 0; e < 6; ++e) V[6 * (size_t)p + e] = v[e];
#pragma unroll
    for (int i = 0; i < 3; ++i) gp[3 * (size_t)p + i] = g[i];
    cnt[p] = n;
    if (!Lp) return;
    bool ok = refine_points != 0 && n >= 2;
    double L[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double d0 = v[0] + lambda * v[0], d1 = v[3] + lambda * v[3], d2 = v[5] + lambda * v[5];
    double sp = d0;
    ok = ok && pivot_ok(sp);
    L[0] = sqrt(sp);
    L[1] = v[1] / L[0];
    L[3] = v[2] / L[0];
    sp = d1 - L[1] * L[1];
    ok = ok && pivot_ok(sp);
    L[2] = sqrt(sp);
    L[4] = (v[4] - L[3] * L[1]) / L[2];
    sp = (d2 - L[3] * L[3]) - L[4] * L[4];
    ok = ok && pivot_ok(sp);
    L[5] = sqrt(sp);
#pragma unroll
    for (int e = 0; e < 6; ++e) Lp[6 * (size_t)p + e] = L[e];
    held[p] = ok ? 0 : 1;
}

// The block partials of the per-camera sums: entries 0 .. 20 U, 21 .. 26 gc, 27 the cost, 28 the active count.  One lane
// per (block of the camera lists, entry); part[block][entry].
__global__ __launch_bounds__(256) void ba_cam_partials_kernel(const Prob q, const State s, const int *__restrict__ cam_list,
                                                              const int *__restrict__ blk, int n_blocks, double *__restrict__ part)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n_blocks * BA_CAM_SUMS) return;
    const int b = (int)(t / BA_CAM_SUMS), e = (int)(t % BA_CAM_SUMS);
    int ei = 0, ej = 0;                         // e < 21: entry e is U[ei][ej]; 21 <= e < 27: gc[ei]
    if (e < 21) {
        ej = e;
        while (ej >= 6 - ei) { ej -= 6 - ei; ei += 1; }
        ej += ei;
    } else if (e < 27) {
        ei = e - 21;
    }
    double acc = 0.0;
    for (int pos = blk[AMVS_IDX(3 * b + 1, 3 * n_blocks)]; pos < blk[AMVS_IDX(3 * b + 2, 3 * n_blocks)]; ++pos) {
        Obs o;
        obs_of(q, s, AMVS_IDX(cam_list[AMVS_IDX(pos, q.N)], q.N), o);
        if (!o.active) continue;
        const double xi = pick6(o.Jx, ei), yi = pick6(o.Jy, ei), xj = pick6(o.Jx, ej), yj = pick6(o.Jy, ej);
        double u;
        if (e < 21) u = xi * xj + yi * yj;
        else if (e < 27) u = xi * o.rx + yi * o.ry;
        else if (e == 27) u = o.rx * o.rx + o.ry * o.ry;
        else u = 1.0;
        acc = acc + u;
    }
    part[t] = acc;
}

// total[list][e] = the partials of the blocks blk0[list] .. blk0[list + 1] - 1 added in ascending order, from +0.0
__global__ __launch_bounds__(256) void ba_total_kernel(const double *__restrict__ part, const int *__restrict__ blk0, int n_lists,
                                                       int entries, double *__restrict__ total)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n_lists * entries) return;
    const int l = (int)(t / entries), e = (int)(t % entries);
    double acc = 0.0;
    for (int b = blk0[l]; b < blk0[l + 1]; ++b) acc = acc + part[(size_t)b * entries + e];
    total[t] = acc;
}

// out[0] = cost, out[1] = act over cameras 0 .. C-1 in ascending order; out[2] = the no-step flag, for the one read-back
__global__ void ba_cost_total_kernel(const double *__restrict__ camsum, int C, const int *__restrict__ bad, double *__restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double cost = 0.0, act = 0.0;
    for (int c = 0; c < C; ++c) {
        cost = cost + camsum[(size_t)c * BA_CAM_SUMS + 27];
        act = act + camsum[(size_t)c * BA_CAM_SUMS + 28];
    }
    out[0] = cost;
    out[1] = act;
    out[2] = bad ? (double)bad[0] : 0.0;
}

// The block partials of the Schur terms: one lane per (block of a pair segment, row i of the 6 x 6 term).  The lane forms
// Y_k[i] once per pair and adds the six entries T(k, k')[i][0..5] and, on a diagonal segment, the right-hand side's
// Y_k[i] gp; part[block][e] with e = 6 i + j for the entries and e = 36 + i for the right-hand side.
__global__ __launch_bounds__(256) void ba_schur_partials_kernel(const Prob q, const State s, const int *__restrict__ pair_k,
                                                                const int *__restrict__ pair_k2, long long n_pairs,
                                                                const int *__restrict__ blk, int n_blocks,
                                                                const double *__restrict__ Lp, const unsigned char *__restrict__ held,
                                                                const double *__restrict__ gp, double *__restrict__ part)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n_blocks * 6) return;
    const int b = (int)(t / 6), i = (int)(t % 6);
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int p0 = blk[AMVS_IDX(3 * b + 1, 3 * n_blocks)], p1 = blk[AMVS_IDX(3 * b + 2, 3 * n_blocks)];
    for (int pos = p0; pos < p1; ++pos) {
        const int k = AMVS_IDX(pair_k[AMVS_IDX(pos, n_pairs)], q.N), k2 = AMVS_IDX(pair_k2[AMVS_IDX(pos, n_pairs)], q.N);
        const int p = AMVS_IDX(q.pt[k], q.P);
        if (held[p]) continue;
        Obs o1, o2;
        obs_of(q, s, k, o1);
        if (!o1.active) continue;
        obs_of(q, s, k2, o2);                                 // (k2 == k on a diagonal segment: the same terms again)
        if (!o2.active) continue;
        const double xi = pick6(o1.Jx, i), yi = pick6(o1.Jy, i);
        const double w[3] = {xi * o1.Px[0] + yi * o1.Py[0], xi * o1.Px[1] + yi * o1.Py[1], xi * o1.Px[2] + yi * o1.Py[2]};
        double Y[3];
        solve3(Lp + 6 * (size_t)p, w, Y);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const double w0 = o2.Jx[j] * o2.Px[0] + o2.Jy[j] * o2.Py[0], w1 = o2.Jx[j] * o2.Px[1] + o2.Jy[j] * o2.Py[1];
            const double w2 = o2.Jx[j] * o2.Px[2] + o2.Jy[j] * o2.Py[2];
            acc[j] = acc[j] + ((Y[0] * w0 + Y[1] * w1) + Y[2] * w2);
        }
        if (k == k2) {
            const double *g = gp + 3 * (size_t)p;
            acc[6] = acc[6] + ((Y[0] * g[0] + Y[1] * g[1]) + Y[2] * g[2]);
        }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) part[(size_t)b * BA_SEG_SUMS + 6 * i + j] = acc[j];
    part[(size_t)b * BA_SEG_SUMS + 36 + i] = acc[6];
}

// S and rhs from the segment totals.  One lane per (segment, entry).  S was set to +0.0 before.
__global__ __launch_bounds__(256) void ba_schur_assemble_kernel(const double *__restrict__ part, const int *__restrict__ seg_ab,
                                                                const int *__restrict__ seg_blk0, int n_seg,
                                                                const int *__restrict__ cam_of_slot, const double *__restrict__ camsum,
                                                                double lambda, int n, double *__restrict__ S, double *__restrict__ rhs)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n_seg * BA_SEG_SUMS) return;
    const int g = (int)(t / BA_SEG_SUMS), e = (int)(t % BA_SEG_SUMS);
    const int a = seg_ab[2 * g], b = seg_ab[2 * g + 1];
    if (e >= 36 && a != b) return;
    double tot = 0.0;
    for (int k = seg_blk0[g]; k < seg_blk0[g + 1]; ++k) tot = tot + part[(size_t)k * BA_SEG_SUMS + e];
    const int i = e < 36 ? e / 6 : e - 36, j = e < 36 ? e % 6 : 0;
    if (a != b) {
        const double v = 0.0 - tot;
        S[(size_t)AMVS_IDX(6 * a + i, n) * n + AMVS_IDX(6 * b + j, n)] = v;
        S[(size_t)(6 * b + j) * n + (6 * a + i)] = v;
        return;
    }
    const double *cs = camsum + (size_t)cam_of_slot[a] * BA_CAM_SUMS;
    const bool idle = cs[28] == 0.0;
    if (e >= 36) {
        rhs[AMVS_IDX(6 * a + i, n)] = idle ? 0.0 : -(cs[21 + i]) + tot;
        return;
    }
    if (i > j) return;
    double v;
    if (idle) {
        v = i == j ? 1.0 : 0.0;
    } else {
        const double u = cs[i * 6 - i * (i - 1) / 2 + (j - i)];
        v = (i == j ? u + lambda * u : u) - tot;
    }
    S[(size_t)AMVS_IDX(6 * a + i, n) * n + AMVS_IDX(6 * a + j, n)] = v;
    S[(size_t)(6 * a + j) * n + (6 * a + i)] = v;
}

// element (i, j) of the n x n matrix A, checked in the index-checked build
#define A_AT(i, j) A[AMVS_IDX((size_t)(i) * (size_t)n + (size_t)(j), (size_t)n * (size_t)n)]

// The diagonal block of the panel of columns j0 .. j0 + nb - 1 (nb = min(NB, n - j0)), factored in place by ONE workgroup
// in LDS.  bad[0] = 1 on a pivot that is not positive and finite.  The rows below it are solved by the next launch
// (ba_chol_rows_kernel), which only reads this block: no workgroup reads what another one of its launch writes.
__global__ __launch_bounds__(256) void ba_chol_diag_kernel(double *__restrict__ A, int n, int j0, int *__restrict__ bad)
{
    __shared__ double D[NB][NB + 1];
    const int tid = (int)threadIdx.x;
    const int nb = n - j0 < NB ? n - j0 : NB;
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e / NB, c = e % NB;
        D[r][c] = (r < nb && c <= r) ? A_AT(j0 + r, j0 + c) : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
        if (tid == 0) {
            const double sp = D[j][j];
            if (!pivot_ok(sp)) bad[0] = 1;
            D[j][j] = sqrt(sp);
        }
        __syncthreads();
        if (tid > j && tid < nb) D[tid][j] = D[tid][j] / D[j][j];
        __syncthreads();
        for (int e = tid; e < NB * NB; e += 256) {
            const int r = e / NB, c = e % NB;
            if (c > j && r >= c && r < nb) D[r][c] = D[r][c] - D[r][j] * D[c][j];
        }
        __syncthreads();
    }
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e / NB, c = e % NB;
        if (r < nb && c <= r) A_AT(j0 + r, j0 + c) = D[r][c];
    }
}

// The rows j0 + NB .. n - 1 of a full panel, one per lane, against the factored diagonal block (read into LDS by every
// workgroup, written by none): L[i][c] = (A[i][c] - L[i][0]*L[c][0] - ... ) / L[c][c] in ascending c and k.
__global__ __launch_bounds__(256) void ba_chol_rows_kernel(double *__restrict__ A, int n, int j0)
{
    __shared__ double D[NB][NB + 1];
    const int tid = (int)threadIdx.x;
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e / NB, c = e % NB;
        D[r][c] = c <= r ? A_AT(j0 + r, j0 + c) : 0.0;
    }
    __syncthreads();
    const int i = j0 + NB + (int)blockIdx.x * 256 + tid;
    if (i >= n) return;
    double l[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        double v = A_AT(i, j0 + c);
#pragma unroll
        for (int k = 0; k < c; ++k) v = v - l[k] * D[c][k];
        l[c] = v / D[c][c];
    }
#pragma unroll
    for (int c = 0; c < NB; ++c) A_AT(i, j0 + c) = l[c];
}

// A[i][j] -= L[i][k] * L[j][k] for the NB columns k of the panel at j0, in ascending k, for j1 = j0 + NB <= j <= i < n.
// One workgroup per 32 x 32 tile of the lower triangle.
__global__ __launch_bounds__(256) void ba_chol_update_kernel(double *__restrict__ A, int n, int j0)
{
    if (blockIdx.y > blockIdx.x) return;
    __shared__ double Li[NB][NB + 1], Lj[NB][NB + 1];
    const int tid = (int)threadIdx.x, j1 = j0 + NB;
    const int ibase = j1 + (int)blockIdx.x * NB, jbase = j1 + (int)blockIdx.y * NB;
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e / NB, k = e % NB;
        Li[r][k] = ibase + r < n ? A_AT(ibase + r, j0 + k) : 0.0;
        Lj[r][k] = jbase + r < n ? A_AT(jbase + r, j0 + k) : 0.0;
    }
    __syncthreads();
    const int c = tid % NB;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int r = tid / NB + 8 * m;
        const int i = ibase + r, j = jbase + c;
        if (i >= n || j > i) continue;
        double acc = A_AT(i, j);
#pragma unroll
        for (int k = 0; k < NB; ++k) acc = acc - Li[r][k] * Lj[c][k];
        A_AT(i, j) = acc;
    }
}

// x = the solution of L L^T x = rhs with L in the lower triangle of A: forward in ascending k, back in descending k.
// One workgroup; the vector lives in LDS (n <= 6 * AMVS_BA_MAX_CAMERAS).
__global__ __launch_bounds__(1024) void ba_solve_kernel(const double *__restrict__ A, int n, const double *__restrict__ rhs,
                                                        double *__restrict__ x)
{
    __shared__ double v[6 * AMVS_BA_MAX_CAMERAS];
    __shared__ double D[NB][NB + 1];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < n; i += 1024) v[i] = rhs[i];
    for (int j0 = 0; j0 < n; j0 += NB) {
        const int nb = n - j0 < NB ? n - j0 : NB;
        __syncthreads();
        {
            const int r = tid / NB, c = tid % NB;
            D[r][c] = (r < nb && c <= r) ? A_AT(j0 + r, j0 + c) : 0.0;
        }
        __syncthreads();
        for (int j = 0; j < nb; ++j) {
            if (tid == 0) v[j0 + j] = v[j0 + j] / D[j][j];
            __syncthreads();
            if (tid > j && tid < nb) v[j0 + tid] = v[j0 + tid] - D[tid][j] * v[j0 + j];
            __syncthreads();
        }
        for (int i = j0 + nb + tid; i < n; i += 1024) {
            double acc = v[i];
            for (int k = 0; k < nb; ++k) acc = acc - A_AT(i, j0 + k) * v[j0 + k];
            v[i] = acc;
        }
    }
    for (int j0 = ((n - 1) / NB) * NB; j0 >= 0; j0 -= NB) {
        const int nb = n - j0 < NB ? n - j0 : NB;
        __syncthreads();
        {
            const int r = tid / NB, c = tid % NB;
            D[r][c] = (r < nb && c <= r) ? A_AT(j0 + r, j0 + c) : 0.0;
        }
        __syncthreads();
        for (int j = nb - 1; j >= 0; --j) {
            if (tid == 0) v[j0 + j] = v[j0 + j] / D[j][j];
            __syncthreads();
            if (tid < j) v[j0 + tid] = v[j0 + tid] - D[j][tid] * v[j0 + j];
            __syncthreads();
        }
        for (int i = tid; i < j0; i += 1024) {
            double acc = v[i];
            for (int k = nb - 1; k >= 0; --k) acc = acc - A_AT(j0 + k, i) * v[j0 + k];
            v[i] = acc;
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += 1024) x[i] = v[i];
}

// One lane per camera: dc [C][6] and the candidate pose; all +0.0 when there is no step.
__global__ __launch_bounds__(64) void ba_pose_step_kernel(const State s, int C, const int *__restrict__ slot, const double *__restrict__ x,
                                                          const int *__restrict__ bad, double *__restrict__ dc, const State cand)
{
    const int c = (int)(blockIdx.x * 64 + threadIdx.x);
    if (c >= C) return;
    double d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, Rn[9], tn[3];
    const double *R = s.R + 9 * (size_t)c, *t = s.t + 3 * (size_t)c;
    const int a = slot[c];
    if (bad[0]) {
#pragma unroll
        for (int e = 0; e < 9; ++e) Rn[e] = 0.0;
#pragma unroll
        for (int e = 0; e < 3; ++e) tn[e] = 0.0;
    } else if (a < 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) Rn[e] = R[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) tn[e] = t[e];
    } else {
#pragma unroll
        for (int e = 0; e < 6; ++e) d[e] = x[6 * (size_t)a + e];
        pnp_pose_update(d, R, t, Rn, tn);
    }
#pragma unroll
    for (int e = 0; e < 6; ++e) dc[6 * (size_t)c + e] = d[e];
#pragma unroll
    for (int e = 0; e < 9; ++e) cand.R[9 * (size_t)c + e] = Rn[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) cand.t[3 * (size_t)c + e] = tn[e];
}

// One lane per point: dp [P][3] and the candidate point; all +0.0 when there is no step.  dc is read, so this runs after
// ba_pose_step_kernel.
__global__ __launch_bounds__(256) void ba_point_step_kernel(const Prob q, const State s, const int *__restrict__ pt_start,
                                                            const int *__restrict__ slot, const double *__restrict__ dc,
                                                            const double *__restrict__ Lp, const unsigned char *__restrict__ held,
                                                            const double *__restrict__ gp, const int *__restrict__ bad,
                                                            double *__restrict__ dp, double *__restrict__ Xc)
{
    const int p = (int)(blockIdx.x * 256 + threadIdx.x);
    if (p >= q.P) return;
    double d[3] = {0.0, 0.0, 0.0}, Xn[3];
    const double *X = s.X + 3 * (size_t)p;
    if (bad[0]) {
        Xn[0] = Xn[1] = Xn[2] = 0.0;
    } else if (held[p]) {
        Xn[0] = X[0]; Xn[1] = X[1]; Xn[2] = X[2];
    } else {
        double b[3] = {-(gp[3 * (size_t)p]), -(gp[3 * (size_t)p + 1]), -(gp[3 * (size_t)p + 2])};
        for (int k = pt_start[p]; k < pt_start[p + 1]; ++k) {
            const int c = AMVS_IDX(q.cam[AMVS_IDX(k, q.N)], q.C);
            if (slot[c] < 0) continue;
            Obs o;
            obs_of(q, s, k, o);
            if (!o.active) continue;
            const double *dcc = dc + 6 * (size_t)c;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double w = (o.Jx[0] * o.Px[j] + o.Jy[0] * o.Py[j]) * dcc[0];
#pragma unroll
                for (int i = 1; i < 6; ++i) w = w + (o.Jx[i] * o.Px[j] + o.Jy[i] * o.Py[j]) * dcc[i];
                b[j] = b[j] - w;
            }
        }
        solve3(Lp + 6 * (size_t)p, b, d);
#pragma unroll
        for (int r = 0; r < 3; ++r) Xn[r] = X[r] + d[r];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        dp[3 * (size_t)p + r] = d[r];
        Xc[3 * (size_t)p + r] = Xn[r];
    }
}

inline dim3 blocks_for(long long n, int per) { return dim3((unsigned)((n + per - 1) / per > 0 ? (n + per - 1) / per : 1)); }

// The times of one trial, split by kernel family, when AMVS_BA_TIMES names a file.
struct TrialTimer {
    static constexpr int MAX = 12;
    const char *path = nullptr;                     // set by enable(): only amvs_ba_solve looks at the environment
    void enable() { path = std::getenv("AMVS_BA_TIMES"); }
    EventPool ev{true};
    const char *name[MAX];
    int n = 0;
    void begin(hipStream_t st) { n = 0; mark("start", st); }
    void mark(const char *what, hipStream_t st)
    {
        if (!path || n >= MAX || ev.reserve((size_t)n + 1) != hipSuccess) return;
        name[n] = what;
        (void)hipEventRecord(ev[(size_t)n++], st);
    }
    // after the stream was synchronised
    void flush(int n_sys, int N, int P, long long pairs)
    {
        if (!path || n < 2) return;
        std::FILE *f = std::fopen(path, "a");
        if (!f) return;
        std::fprintf(f, "n %d N %d P %d pairs %lld", n_sys, N, P, pairs);
        for (int i = 1; i < n; ++i) {
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, ev[(size_t)i - 1], ev[(size_t)i]);
            std::fprintf(f, " %s %.6f", name[i], ms);
        }
        std::fprintf(f, "\n");
        std::fclose(f);
    }
};

// everything a call keeps on the device
struct Device {
    TrialTimer timer;
    ScratchCache::Lease ints, uvb, state[2], V, gp, cnt, Lp, held, cpart, camsum[2], costact, spart, S, rhs, x, bad, dc, dp, err2;
    Prob q;
    State s[2];
    const int *pt_start, *cam_list, *cam_blk0, *cam_blk, *slot, *cam_of_slot, *pair_k, *pair_k2, *seg_ab, *seg_blk0, *seg_blk;
    int n_cblk = 0, n_sblk = 0, n_seg = 0, F = 0, n = 0;
    long long n_pairs = 0;
};

// with_system: S, rhs and x are wanted (the lists then hold the pairs); with_step: a candidate state, dc and dp too
hipError_t upload(const BaProblem &h, const BaLists &L, bool with_system, bool with_step, Device &d, ScratchCache &cache, hipStream_t st)
{
    const int C = h.C, P = h.P, N = h.N;
    std::vector<int> cam_of_slot((size_t)(L.F > 0 ? L.F : 1), 0);
    for (int c = 0; c < C; ++c)
        if (L.slot[c] >= 0) cam_of_slot[L.slot[c]] = c;
    const std::vector<int> cam_v(h.cam, h.cam + N), pt_v(h.pt, h.pt + N);
    const std::vector<int> *parts[] = {&cam_v, &pt_v, &L.pt_start, &L.cam_list, &L.cam_blk0, &L.cam_blk, &L.slot, &cam_of_slot,
                                       &L.pair_k, &L.pair_k2, &L.seg_ab, &L.seg_blk0, &L.seg_blk};
    size_t off[14] = {0};
    for (int i = 0; i < 13; ++i) off[i + 1] = off[i] + ((parts[i]->size() + 63) & ~size_t(63));     // (each list on a 256-byte boundary)
    STCHK(cache.lease(d.ints, sizeof(int) * off[13]));
    int *base = d.ints.get<int>();
    for (int i = 0; i < 13; ++i)
        if (!parts[i]->empty())
            STCHK(hipMemcpyAsync(base + off[i], parts[i]->data(), sizeof(int) * parts[i]->size(), hipMemcpyHostToDevice, st));
    STCHK(hipStreamSynchronize(st));                 // (cam_v, pt_v and cam_of_slot are locals)
    d.pt_start = base + off[2]; d.cam_list = base + off[3]; d.cam_blk0 = base + off[4]; d.cam_blk = base + off[5];
    d.slot = base + off[6]; d.cam_of_slot = base + off[7]; d.pair_k = base + off[8]; d.pair_k2 = base + off[9];
    d.seg_ab = base + off[10]; d.seg_blk0 = base + off[11]; d.seg_blk = base + off[12];
    d.n_cblk = (int)(L.cam_blk.size() / 3);
    d.n_sblk = (int)(L.seg_blk.size() / 3);
    d.n_seg = (int)(L.seg_ab.size() / 2);
    d.n_pairs = (long long)L.pair_k.size();
    d.F = L.F;
    d.n = with_system ? L.n : 0;
    STCHK(cache.lease(d.uvb, sizeof(float) * 2 * (size_t)N));
    STCHK(hipMemcpyAsync(d.uvb.get(), h.uv, sizeof(float) * 2 * (size_t)N, hipMemcpyHostToDevice, st));
    d.q = Prob{base + off[0], base + off[1], d.uvb.get<float>(), C, P, N, intrinsics_of(h.K)};
    const size_t n_state = 12 * (size_t)C + 3 * (size_t)P;
    for (int i = 0; i < (with_step ? 2 : 1); ++i) {
        STCHK(cache.lease(d.state[i], sizeof(double) * n_state));
        double *b = d.state[i].get<double>();
        d.s[i] = State{b, b + 9 * (size_t)C, b + 12 * (size_t)C};
        STCHK(cache.lease(d.camsum[i], sizeof(double) * BA_CAM_SUMS * (size_t)C));
    }
    STCHK(hipMemcpyAsync(d.s[0].R, h.R, sizeof(double) * 9 * (size_t)C, hipMemcpyHostToDevice, st));
    STCHK(hipMemcpyAsync(d.s[0].t, h.t, sizeof(double) * 3 * (size_t)C, hipMemcpyHostToDevice, st));
    STCHK(hipMemcpyAsync(d.s[0].X, h.X, sizeof(double) * 3 * (size_t)P, hipMemcpyHostToDevice, st));
    STCHK(cache.lease(d.cpart, sizeof(double) * BA_CAM_SUMS * (size_t)(d.n_cblk > 0 ? d.n_cblk : 1)));
    STCHK(cache.lease(d.costact, sizeof(double) * 4));
    STCHK(cache.lease(d.V, sizeof(double) * 6 * (size_t)P));
    STCHK(cache.lease(d.gp, sizeof(double) * 3 * (size_t)P));
    STCHK(cache.lease(d.cnt, sizeof(int) * (size_t)P));
    STCHK(cache.lease(d.Lp, sizeof(double) * 6 * (size_t)P));
    STCHK(cache.lease(d.held, (size_t)P));
    STCHK(cache.lease(d.bad, sizeof(int) * 2));
    STCHK(hipMemsetAsync(d.bad.get(), 0, sizeof(int) * 2, st));
    if (d.n > 0) {
        STCHK(cache.lease(d.spart, sizeof(double) * BA_SEG_SUMS * (size_t)(d.n_sblk > 0 ? d.n_sblk : 1)));
        STCHK(cache.lease(d.S, sizeof(double) * (size_t)d.n * (size_t)d.n));
        STCHK(cache.lease(d.rhs, sizeof(double) * (size_t)d.n));
        STCHK(cache.lease(d.x, sizeof(double) * (size_t)d.n));
    }
    if (with_step) {
        STCHK(cache.lease(d.dc, sizeof(double) * 6 * (size_t)C));
        STCHK(cache.lease(d.dp, sizeof(double) * 3 * (size_t)P));
    }
    return hipSuccess;
}

// the 29 sums of every camera under state i into camsum[i], and (cost, act, no-step flag) into costact
hipError_t cam_pass(Device &d, int i, hipStream_t st)
{
    if (d.n_cblk > 0) {
        hipLaunchKernelGGL(ba_cam_partials_kernel, blocks_for((long long)d.n_cblk * BA_CAM_SUMS, 256), dim3(256), 0, st, d.q, d.s[i],
                           d.cam_list, d.cam_blk, d.n_cblk, d.cpart.get<double>());
        STCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(ba_total_kernel, blocks_for((long long)d.q.C * BA_CAM_SUMS, 256), dim3(256), 0, st, (const double *)d.cpart.get(),
                       d.cam_blk0, d.q.C, BA_CAM_SUMS, d.camsum[i].get<double>());
    STCHK(hipGetLastError());
    hipLaunchKernelGGL(ba_cost_total_kernel, dim3(1), dim3(64), 0, st, (const double *)d.camsum[i].get(), d.q.C, (const int *)d.bad.get(),
                       d.costact.get<double>());
    return hipGetLastError();
}

hipError_t point_pass(Device &d, int i, double lambda, int refine_points, bool factor, hipStream_t st)
{
    hipLaunchKernelGGL(ba_point_kernel, blocks_for(d.q.P, 256), dim3(256), 0, st, d.q, d.s[i], d.pt_start, lambda, refine_points,
                       d.V.get<double>(), d.gp.get<double>(), d.cnt.get<int>(), factor ? d.Lp.get<double>() : (double *)nullptr,
                       d.held.get<unsigned char>());
    return hipGetLastError();
}

// S and rhs of state i under lambda; camsum[i] holds the state's sums
hipError_t schur(Device &d, int i, double lambda, int refine_points, hipStream_t st)
{
    STCHK(point_pass(d, i, lambda, refine_points, true, st));
    d.timer.mark("points", st);
    if (d.n_sblk > 0) {
        hipLaunchKernelGGL(ba_schur_partials_kernel, blocks_for((long long)d.n_sblk * 6, 256), dim3(256), 0, st, d.q, d.s[i],
                           d.pair_k, d.pair_k2, d.n_pairs, d.seg_blk, d.n_sblk, (const double *)d.Lp.get(),
                           (const unsigned char *)d.held.get(), (const double *)d.gp.get(), d.spart.get<double>());
        STCHK(hipGetLastError());
    }
    d.timer.mark("schur_partials", st);
    STCHK(hipMemsetAsync(d.S.get(), 0, sizeof(double) * (size_t)d.n * (size_t)d.n, st));
    hipLaunchKernelGGL(ba_schur_assemble_kernel, blocks_for((long long)d.n_seg * BA_SEG_SUMS, 256), dim3(256), 0, st,
                       (const double *)d.spart.get(), d.seg_ab, d.seg_blk0, d.n_seg, d.cam_of_slot, (const double *)d.camsum[i].get(), lambda,
                       d.n, d.S.get<double>(), d.rhs.get<double>());
    d.timer.mark("schur_assemble", st);
    return hipGetLastError();
}

// the candidate of state i under lambda into state 1 - i, with dc, dp and the no-step flag
hipError_t step(Device &d, int i, double lambda, int refine_points, hipStream_t st)
{
    STCHK(schur(d, i, lambda, refine_points, st));
    STCHK(hipMemsetAsync(d.bad.get(), 0, sizeof(int), st));
    const int n = d.n;
    double *A = d.S.get<double>();
    for (int j0 = 0; j0 < n; j0 += NB) {
        const int below = n - j0 - NB;
        hipLaunchKernelGGL(ba_chol_diag_kernel, dim3(1), dim3(256), 0, st, A, n, j0, d.bad.get<int>());
        STCHK(hipGetLastError());
        if (below > 0) {
            hipLaunchKernelGGL(ba_chol_rows_kernel, blocks_for(below, 256), dim3(256), 0, st, A, n, j0);
            STCHK(hipGetLastError());
            const unsigned nt = (unsigned)((below + NB - 1) / NB);
            hipLaunchKernelGGL(ba_chol_update_kernel, dim3(nt, nt), dim3(256), 0, st, A, n, j0);
            STCHK(hipGetLastError());
        }
    }
    d.timer.mark("cholesky", st);
    hipLaunchKernelGGL(ba_solve_kernel, dim3(1), dim3(1024), 0, st, (const double *)A, n, (const double *)d.rhs.get(), d.x.get<double>());
    STCHK(hipGetLastError());
    d.timer.mark("solve", st);
    hipLaunchKernelGGL(ba_pose_step_kernel, blocks_for(d.q.C, 64), dim3(64), 0, st, d.s[i], d.q.C, d.slot, (const double *)d.x.get(),
                       (const int *)d.bad.get(), d.dc.get<double>(), d.s[1 - i]);
    STCHK(hipGetLastError());
    hipLaunchKernelGGL(ba_point_step_kernel, blocks_for(d.q.P, 256), dim3(256), 0, st, d.q, d.s[i], d.pt_start, d.slot,
                       (const double *)d.dc.get(), (const double *)d.Lp.get(), (const unsigned char *)d.held.get(),
                       (const double *)d.gp.get(), (const int *)d.bad.get(), d.dp.get<double>(), d.s[1 - i].X);
    d.timer.mark("update", st);
    return hipGetLastError();
}

hipError_t fetch_state(const Device &d, int i, double *R, double *t, double *X, hipStream_t st)
{
    STCHK(hipMemcpyAsync(R, d.s[i].R, sizeof(double) * 9 * (size_t)d.q.C, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(t, d.s[i].t, sizeof(double) * 3 * (size_t)d.q.C, hipMemcpyDeviceToHost, st));
    return hipMemcpyAsync(X, d.s[i].X, sizeof(double) * 3 * (size_t)d.q.P, hipMemcpyDeviceToHost, st);
}

}  // namespace

hipError_t ba_cost(const BaProblem &h, double *cost, long long *active, double *err2, ScratchCache &cache, hipStream_t st)
{
    BaLists L;
    ba_build_lists(h, false, L);
    Device d;
    STCHK(upload(h, L, false, false, d, cache, st));
    STCHK(cache.lease(d.err2, sizeof(double) * (size_t)h.N));
    hipLaunchKernelGGL(ba_err_kernel, blocks_for(h.N, 256), dim3(256), 0, st, d.q, d.s[0], d.err2.get<double>());
    STCHK(hipGetLastError());
    STCHK(cam_pass(d, 0, st));
    double ca[3];
    STCHK(hipMemcpyAsync(ca, d.costact.get(), sizeof(ca), hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(err2, d.err2.get(), sizeof(double) * (size_t)h.N, hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
    *cost = ca[0];
    *active = (long long)ca[1];
    return hipSuccess;
}

hipError_t ba_normal(const BaProblem &h, double *U, double *gc, double *V, double *gp, int *counts, ScratchCache &cache, hipStream_t st)
{
    BaLists L;
    ba_build_lists(h, false, L);
    Device d;
    STCHK(upload(h, L, false, false, d, cache, st));
    STCHK(point_pass(d, 0, 0.0, 1, false, st));
    STCHK(cam_pass(d, 0, st));
    std::vector<double> sums((size_t)h.C * BA_CAM_SUMS);
    STCHK(hipMemcpyAsync(sums.data(), d.camsum[0].get(), sizeof(double) * sums.size(), hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(V, d.V.get(), sizeof(double) * 6 * (size_t)h.P, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(gp, d.gp.get(), sizeof(double) * 3 * (size_t)h.P, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(counts, d.cnt.get(), sizeof(int) * (size_t)h.P, hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
    for (int c = 0; c < h.C; ++c) {
        std::memcpy(U + 21 * (size_t)c, sums.data() + (size_t)c * BA_CAM_SUMS, sizeof(double) * 21);
        std::memcpy(gc + 6 * (size_t)c, sums.data() + (size_t)c * BA_CAM_SUMS + 21, sizeof(double) * 6);
    }
    return hipSuccess;
}

hipError_t ba_schur(const BaProblem &h, int refine_points, double lambda, double *S, double *rhs, int *slot, unsigned char *held,
                    ScratchCache &cache, hipStream_t st)
{
    BaLists L;
    ba_build_lists(h, true, L);
    Device d;
    STCHK(upload(h, L, true, false, d, cache, st));
    STCHK(cam_pass(d, 0, st));
    STCHK(schur(d, 0, lambda, refine_points, st));
    STCHK(hipMemcpyAsync(S, d.S.get(), sizeof(double) * (size_t)d.n * (size_t)d.n, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(rhs, d.rhs.get(), sizeof(double) * (size_t)d.n, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(held, d.held.get(), (size_t)h.P, hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
    std::memcpy(slot, L.slot.data(), sizeof(int) * (size_t)h.C);
    return hipSuccess;
}

hipError_t ba_step(const BaProblem &h, int refine_points, double lambda, int *ok, double *dc, double *dp, double *R_out, double *t_out,
                   double *X_out, ScratchCache &cache, hipStream_t st)
{
    BaLists L;
    ba_build_lists(h, true, L);
    Device d;
    STCHK(upload(h, L, true, true, d, cache, st));
    STCHK(cam_pass(d, 0, st));
    STCHK(step(d, 0, lambda, refine_points, st));
    int bad = 0;
    STCHK(hipMemcpyAsync(&bad, d.bad.get(), sizeof(int), hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(dc, d.dc.get(), sizeof(double) * 6 * (size_t)h.C, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(dp, d.dp.get(), sizeof(double) * 3 * (size_t)h.P, hipMemcpyDeviceToHost, st));
    STCHK(fetch_state(d, 1, R_out, t_out, X_out, st));
    STCHK(hipStreamSynchronize(st));
    *ok = bad ? 0 : 1;
    return hipSuccess;
}

hipError_t ba_solve(const BaProblem &h, int refine_points, double lambda0, double ftol, int max_trials, double *R_out, double *t_out,
                    double *X_out, double info[6], ScratchCache &cache, hipStream_t st)
{
    BaLists L;
    ba_build_lists(h, true, L);
    Device d;
    STCHK(upload(h, L, true, true, d, cache, st));
    d.timer.enable();
    int cur = 0, trials = 0, kept = 0;
    double ca[3], lambda = lambda0;
    STCHK(cam_pass(d, cur, st));
    STCHK(hipMemcpyAsync(ca, d.costact.get(), sizeof(ca), hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
    double cost = ca[0], act = ca[1];
    const double first = cost;
    while (trials < max_trials) {
        trials += 1;
        d.timer.begin(st);
        STCHK(step(d, cur, lambda, refine_points, st));
        STCHK(cam_pass(d, 1 - cur, st));             // (without a step the candidate is all zero: nothing active, and not looked at)
        d.timer.mark("pass", st);
        STCHK(hipMemcpyAsync(ca, d.costact.get(), sizeof(ca), hipMemcpyDeviceToHost, st));
        STCHK(hipStreamSynchronize(st));
        d.timer.flush(d.n, h.N, h.P, d.n_pairs);
        const bool have = ca[2] == 0.0;
        if (have && ca[0] <= cost && ca[1] >= act) {
            const double dcost = cost - ca[0], old = cost;
            cur = 1 - cur;
            cost = ca[0];
            act = ca[1];
            kept += 1;
            lambda = lambda / 10.0 > AMVS_BA_LAMBDA_MIN ? lambda / 10.0 : AMVS_BA_LAMBDA_MIN;
            if (dcost <= ftol * old) break;
        } else {
            lambda = lambda * 10.0;
            if (lambda > AMVS_BA_LAMBDA_MAX) break;
        }
    }
    STCHK(fetch_state(d, cur, R_out, t_out, X_out, st));
    STCHK(hipStreamSynchronize(st));
    info[0] = (double)trials; info[1] = (double)kept; info[2] = lambda; info[3] = first; info[4] = cost; info[5] = act;
    return hipSuccess;
}

}  // namespace amvs

AMVS_CHECK_TU(bundle)
