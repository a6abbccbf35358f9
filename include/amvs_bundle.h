/* amvs_bundle.h -- bundle adjustment in libamvs.so: Levenberg-Marquardt on the reprojection error over all free camera
 * poses and all points together, solved through the Schur complement on the camera block (csrc/amvs_bundle.hip).  The
 * reference's bundle_adjustment_light refines each camera against points it never moves; that motion-only pass is the
 * mode refine_points = 0 of the same code, batched over all cameras.
 *
 * Why a header of its own: existing tests hold include/amvs.h to 92 entry points and every other header to its own count,
 * and existing tests do not change.  What is declared here is bound from a ninth table, _lib.BA_SIGNATURES; _lib.load()
 * binds all nine.  The library, the context and the error codes are those of amvs.h.
 *
 * As in amvs_resection.h the text below IS the definition: it is judged against tests/bundle_restatement.py, written from
 * this text alone, bit for bit.
 *
 * How this differs from the reference and from Ceres-style solvers, on purpose: points move (the reference's do not); the
 * rotation update is the trig-free quaternion of amvs_resection.h, not a Rodrigues vector; the damping is Marquardt's
 * (the diagonal scaled by 1 + lambda) with a fixed factor of 10, not a trust region; there is no robust loss (a caller
 * filters outliers by amvs_ba_cost and calls again); intrinsics are shared and not refined; every sum has a fixed order,
 * so the result is a function of the inputs alone.  Parity with OpenCV / scipy is UNPINNED (DESIGN.md sections 14, 16).
 *
 * ---- inputs -------------------------------------------------------------------------------------------------------------
 * C cameras: R double[C][9] row-major, t double[C][3], Xc = R X + t.  P points: X double[P][3].  N observations:
 * cam int32[N], pt int32[N], uv float32[N][2] promoted to float64; observation k says that camera cam[k] sees point pt[k]
 * at pixel (u, v) = uv[k].  The observations are STRICTLY ASCENDING in (pt, cam): pt[k-1] < pt[k], or pt[k-1] == pt[k] and
 * cam[k-1] < cam[k].  So the observations of a point are contiguous and no camera sees a point twice.  A point may have
 * no observation.  K double[9]: read and checked exactly as in amvs_resection.h (fx = K[0], fy = K[4], cx = K[2],
 * cy = K[5], K[1] must be 0); shared by all cameras, not refined, no distortion.  fixed uint8[C]: camera c is FIXED when
 * fixed[c] != 0, else FREE; fixed == NULL means that camera 0 alone is fixed.  refine_points: 0 is the motion-only mode.
 *
 * ---- arithmetic ---------------------------------------------------------------------------------------------------------
 * That of amvs_resection.h: float64, one rounding per operation, nothing contracted, in exactly the written order; only
 * + - * / and sqrt; -(a) flips the sign bit; a + b + c means (a + b) + c; every comparison with a NaN is false.
 *
 * ---- per observation k = (c, p) under a state (R, t, X) -----------------------------------------------------------------
 * Xc and z = Xc[2] as in the inlier test of amvs_resection.h with (R, t) of camera c and (X, Y, Z) of point p.  The
 * observation is ACTIVE iff z > 0; an inactive one contributes to nothing.  An active one has iz, xz, yz, rx, ry, ax, ay,
 * bx, by, Jx[0..5], Jy[0..5] exactly as in the refit of amvs_resection.h, and with R the rotation of camera c
 *     Px[j] = ax*R[0][j] + bx*R[2][j],   Py[j] = ay*R[1][j] + by*R[2][j]      for j = 0 .. 2
 *     W[i][j] = Jx[i]*Px[j] + Jy[i]*Py[j]                                     for i = 0 .. 5, j = 0 .. 2.
 *
 * ---- sums and their orders ----------------------------------------------------------------------------------------------
 * Per point p, serial: each starts from +0.0 and adds the term of the point's active observations in ascending k:
 *     V[e] += Px[i]*Px[j] + Py[i]*Py[j]     e = 0 .. 5 for (i, j) = (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
 *     gp[i] += Px[i]*rx + Py[i]*ry          i = 0 .. 2
 *     count = the number of its active observations (an integer).
 * Per camera c: its LIST is the observations with cam[k] == c in ascending k.  SUM over the list is the blocked SUM of
 * amvs_resection.h by list POSITION with AMVS_BA_BLOCK = 64: the positions are cut into blocks of 64 consecutive
 * positions; the partial of a block starts from +0.0 and adds the term of the qualifying members of the block in
 * ascending position (others are skipped, not added as zeros); the sum starts from +0.0 and adds the partials of all
 * blocks in ascending order.  Here a member qualifies when it is active:
 *     U[0..20]  = SUM(Jx[i]*Jx[j] + Jy[i]*Jy[j]), the upper triangle row by row as H in amvs_resection.h
 *     gc[0..5]  = SUM(Jx[i]*rx + Jy[i]*ry)
 *     cost_c    = SUM(rx*rx + ry*ry),     act_c = SUM(1.0).
 * cost = the cost_c of cameras 0 .. C-1 added in ascending order from +0.0, fixed cameras included; act likewise.
 *
 * ---- held and idle ------------------------------------------------------------------------------------------------------
 * Under a damping lambda, V' is V with V'[i][i] = V[i][i] + lambda*V[i][i], other entries unchanged.  Its Cholesky factor
 * Lp (3 x 3) is formed by the formulas of the STEP of amvs_resection.h with 3 in place of 6.  A point is HELD when
 * refine_points == 0, or its count < 2, or that factorisation meets a pivot s that is not (s > 0 and s < +infinity).
 * A held point does not move and contributes nothing to the reduced system; its observations still count in U, gc, cost.
 * solve3(b), for a point that is not held: y[i] = (b[i] - Lp[i][0]*y[0] - ... - Lp[i][i-1]*y[i-1]) / Lp[i][i] for i = 0, 1, 2;
 * x[i] = (y[i] - Lp[i+1][i]*x[i+1] - ... - Lp[2][i]*x[2]) / Lp[i][i] for i = 2, 1, 0 (ascending, as in amvs_resection.h).
 * A free camera with act_c == 0 is IDLE.
 *
 * ---- the reduced system -------------------------------------------------------------------------------------------------
 * Free cameras get slots 0 .. F-1 in ascending camera index; n = 6F.  For a point p that is not held and an active
 * observation k of it, Y_k (6 x 3) has row i = solve3(W_k[i][0..2]).  A product term of two observations k, k' of the
 * same point is the 6 x 6 matrix T(k, k')[i][j] = Y_k[i][0]*W_k'[j][0] + Y_k[i][1]*W_k'[j][1] + Y_k[i][2]*W_k'[j][2]: three
 * products added left to right.  U' is U damped like V' (its six diagonal entries).
 *   Diagonal block of slot a, camera c, not idle:  S[6a+i][6a+j] = U'[i][j] - SUM over c's list of T(k, k)[i][j] for i <= j,
 *     mirrored below the diagonal; a member qualifies when it is active and its point is not held.
 *     rhs[6a+i] = -(gc[i]) + SUM over c's list of (Y_k[i][0]*gp[0] + Y_k[i][1]*gp[1] + Y_k[i][2]*gp[2]), gp of the member's point.
 *   Idle: the diagonal block is the 6 x 6 identity and rhs[6a+i] = +0.0.
 *   Block (a, b), a < b, cameras c < c':  the list is the points observed by both cameras, in ascending p, k the
 *     observation of p by c and k' that by c'; S[6a+i][6b+j] = 0.0 - SUM over that list of T(k, k')[i][j] for all i, j,
 *     blocked by list position in the same way; a member qualifies when k and k' are active and p is not held.
 *     S[6b+j][6a+i] is the same number.  Two cameras that share no point have a block of +0.0.
 *
 * ---- the dense solve ----------------------------------------------------------------------------------------------------
 * Cholesky S = L L^T by the formulas of amvs_resection.h for general n: for j = 0 .. n-1:
 * s = S[j][j] - L[j][0]*L[j][0] - ... - L[j][j-1]*L[j][j-1]; unless s > 0 and s < +infinity there is NO STEP;
 * L[j][j] = sqrt(s); L[i][j] = (S[j][i] - L[i][0]*L[j][0] - ... - L[i][j-1]*L[j][j-1]) / L[j][j] for i > j: every entry
 * subtracts its products in ascending k.  y[i] = (rhs[i] - L[i][0]*y[0] - ... - L[i][i-1]*y[i-1]) / L[i][i], ascending k.
 * The back solve subtracts in DESCENDING k:  x[i] = (y[i] - L[n-1][i]*x[n-1] - ... - L[i+1][i]*x[i+1]) / L[i][i]  for
 * i = n-1 .. 0.  This is the opposite of the 6 x 6 of amvs_resection.h on purpose: a column-oriented schedule on the
 * device (x[k] known, every row above it updated) reproduces it.
 *
 * ---- the step -----------------------------------------------------------------------------------------------------------
 * dc of the camera of slot a is x[6a .. 6a+5]; dc of a fixed camera is +0.0.  For a point p that is not held:
 *     b[j] = -(gp[j]);  for every active observation k of p whose camera c is free, in ascending k:
 *         b[j] = b[j] - (W_k[0][j]*dc_c[0] + W_k[1][j]*dc_c[1] + ... + W_k[5][j]*dc_c[5])      (left to right)
 *     dp = solve3(b);  the candidate point is X[r] + dp[r].
 * A held point has dp = +0.0 and its candidate is X itself.  The candidate pose of a free camera (idle ones too) is the
 * quaternion update of the STEP of amvs_resection.h with om = dc[0..2], dt = dc[3..5] (from "hx = 0.5*om[0]" on; the code
 * is that of csrc/amvs_pnp_step.h); the candidate pose of a fixed camera is its pose.
 *
 * ---- the iteration (amvs_ba_solve) --------------------------------------------------------------------------------------
 * lambda = lambda0, trials = kept = 0; a pass over the input state gives cost and act (first cost = this cost).
 * Repeat while trials < max_trials:
 *     trials += 1; form the step under lambda from the current state.
 *     If there is a step: a pass over the candidate gives cost', act'; it is KEPT iff cost' <= cost and act' >= act.
 *     When kept, in this order: d = cost - cost'; the candidate becomes current (cost = cost', act = act'), kept += 1;
 *         lambda = max(lambda / 10.0, AMVS_BA_LAMBDA_MIN); stop if d <= ftol * (the old cost).
 *     Otherwise (no step, or not kept): lambda = lambda * 10.0; stop if lambda > AMVS_BA_LAMBDA_MAX.
 * A NaN cost therefore never gets a step kept.  That is no error.
 * info_out = [trials, kept, the final lambda, the first cost, the final cost, the final act] as doubles.
 *
 * ---- the entry points ---------------------------------------------------------------------------------------------------
 * amvs_ba_cost: *cost, *active = (int64) act, err2_out[k] = rx*rx + ry*ry of an active observation, -1.0 of an inactive
 *   one: what a caller filters outliers by.  fixed is not among its parameters: it needs no free camera.
 * amvs_ba_normal: U_out [C][21], gc_out [C][6], V_out [P][6], gp_out [P][3], counts_out [P].
 * amvs_ba_schur: under lambda: S_out [n][n] full and symmetric, rhs_out [n], slot_out [C] (-1 for a fixed camera),
 *   held_out [P] (1 held, 0 not).
 * amvs_ba_step: under lambda: *ok = 1 and dc_out [C][6], dp_out [P][3], the candidate R_out, t_out, X_out; when there is
 *   NO STEP, *ok = 0 and all five arrays are +0.0.
 * amvs_ba_solve: the iteration; R_out, t_out, X_out the final state.
 *
 * Errors.  AMVS_EINVAL (-1) for a NULL context before anything else; AMVS_EINVAL before anything is allocated for: the K
 * errors of amvs_resection.h; any NULL other than fixed; C outside 1 .. AMVS_BA_MAX_CAMERAS, P outside
 * 1 .. AMVS_BA_MAX_POINTS, N outside 1 .. AMVS_BA_MAX_OBS; cam[k] outside 0 .. C-1 or pt[k] outside 0 .. P-1; (pt, cam) not
 * strictly ascending; no free camera (all but amvs_ba_cost); lambda or lambda0 not finite or < 0; ftol not finite or < 0;
 * max_trials < 1; more than AMVS_BA_MAX_PAIRS pairs (k <= k') of observations of one point by free cameras.  The
 * index-checked build returns AMVS_EINDEX as amvs.h describes.  Values that are not finite in R, t, X or uv are no
 * errors.  An entry point that fails leaves its outputs untouched.  */
#ifndef AMVS_BUNDLE_H
#define AMVS_BUNDLE_H

#include "amvs_resection.h"

#define AMVS_BA_BLOCK        64
#define AMVS_BA_MAX_CAMERAS  256
#define AMVS_BA_MAX_POINTS   (1 << 22)
#define AMVS_BA_MAX_OBS      (1 << 24)
#define AMVS_BA_MAX_PAIRS    (1 << 25)
#define AMVS_BA_LAMBDA_MIN   1e-12
#define AMVS_BA_LAMBDA_MAX   1e12

#ifdef __cplusplus
extern "C" {
#endif

int amvs_ba_cost(amvs_ctx *ctx, const double *R, const double *t, int C, const double *X, int P, const int32_t *cam,
                 const int32_t *pt, const float *uv, int N, const double K[9], double *cost, int64_t *active,
                 double *err2_out);

int amvs_ba_normal(amvs_ctx *ctx, const double *R, const double *t, int C, const double *X, int P, const int32_t *cam,
                   const int32_t *pt, const float *uv, int N, const double K[9], const uint8_t *fixed, double *U_out,
                   double *gc_out, double *V_out, double *gp_out, int32_t *counts_out);

int amvs_ba_schur(amvs_ctx *ctx, const double *R, const double *t, int C, const double *X, int P, const int32_t *cam,
                  const int32_t *pt, const float *uv, int N, const double K[9], const uint8_t *fixed, int refine_points,
                  double lambda, double *S_out, double *rhs_out, int32_t *slot_out, uint8_t *held_out);

int amvs_ba_step(amvs_ctx *ctx, const double *R, const double *t, int C, const double *X, int P, const int32_t *cam,
                 const int32_t *pt, const float *uv, int N, const double K[9], const uint8_t *fixed, int refine_points,
                 double lambda, int32_t *ok, double *dc_out, double *dp_out, double *R_out, double *t_out, double *X_out);

int amvs_ba_solve(amvs_ctx *ctx, const double *R, const double *t, int C, const double *X, int P, const int32_t *cam,
                  const int32_t *pt, const float *uv, int N, const double K[9], const uint8_t *fixed, int refine_points,
                  double lambda0, double ftol, int max_trials, double *R_out, double *t_out, double *X_out,
                  double info_out[6]);

#ifdef __cplusplus
}
#endif

#endif
