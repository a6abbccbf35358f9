/* amvs_resection.h -- camera resection in libamvs.so: the pose (R, t) of a view with known intrinsics from 2D-3D
 * correspondences by RANSAC, and the Gauss-Newton polish of a pose (csrc/amvs_pnp.hip).  It is the numerical core of the
 * reference's SfMPipeline.register_image (cv.solvePnPRansac, then cv.solvePnP(useExtrinsicGuess, SOLVEPNP_ITERATIVE)) and
 * of the per-camera step of its bundle_adjustment_light (the same polish).
 *
 * Why a header of its own: existing tests hold include/amvs.h to 92 entry points, amvs_depth.h to one, amvs_lens.h to two,
 * amvs_match.h to nine, amvs_epipolar.h to five and amvs_step.h to three, and existing tests do not change.  What is
 * declared here is bound from a seventh table, _lib.PNP_SIGNATURES; _lib.load() binds all seven.  The library, the context
 * and the error codes are those of amvs.h.
 *
 * As in amvs_epipolar.h the text below IS the definition: it is judged against tests/resection_restatement.py, written
 * from this text alone, bit for bit.
 *
 * How this differs from cv.solvePnPRansac, on purpose: a hypothesis is the 6-point DLT of 6 correspondences followed by
 * the nearest rotation (OpenCV draws 4 or 5 and runs EPnP, P3P or its iterative solver); the inlier test also asks for a
 * positive depth (OpenCV's does not); hypotheses are drawn and scored in batches of AMVS_PNP_BATCH, so the stopping rule
 * is looked at once per batch; the best hypothesis is polished on its inliers twice; the polish is a plain Gauss-Newton
 * with a trig-free rotation update, not OpenCV's Levenberg-Marquardt on a Rodrigues vector; the sampler is the
 * counter-based one of amvs_epipolar.h.  Parity with cv2 is UNPINNED: the pose and the inlier set
 * agree with OpenCV's only as two RANSAC runs with different random samples agree.
 *
 * The 6-point DLT IS DEGENERATE ON A PLANAR POINT SET: a sample of coplanar points (and so every sample of a planar
 * scene) has a two-dimensional null space and yields a pose that scores few or no inliers.  That is no error.  A planar
 * scene needs a different minimal solver, which is not here.
 *
 * Every entry point returns AMVS_EINVAL (-1) for a NULL context before anything else, AMVS_EINVAL for its other parameter
 * errors before anything is allocated, and AMVS_EINDEX from the index-checked build as amvs.h describes.  Errors common to
 * all five: m < 6 or m > AMVS_PNP_MAX_POINTS; a NULL pts3d / pts2d / K / output; fx or fy not finite or <= 0; cx or cy not
 * finite; a skew K[1] != 0.  Where there is a threshold: not finite or <= 0.
 *
 * ---- arithmetic -------------------------------------------------------------------------------------------------------
 * pts3d: [m][3] float32, pts2d: [m][2] float32 on the host, correspondence i = the point (X, Y, Z) of the cloud seen at
 * pixel (u, v); promoted to float64.  K: double[9] row-major, of which fx = K[0], fy = K[4], cx = K[2], cy = K[5] are read
 * (and K[1] checked); there is no distortion.  R is double[9] row-major, t double[3]: Xc = R X + t.
 * Everything below is float64: one rounding per operation, nothing contracted, in exactly the written order; the only
 * operations are + - * / and sqrt; division and square root are correctly rounded; -(a) flips the sign bit.
 * a + b + c means (a + b) + c.  Every comparison with a NaN is false.  The sampler is integers only.
 *
 * SUM over a set S of correspondences of a term u(i) is the SUM of amvs_epipolar.h with AMVS_PNP_BLOCK = 64: the indices
 * are cut into blocks of 64 consecutive indices; the partial of a block starts from +0.0 and adds u(i) for the members of
 * S in the block in ascending i (others are skipped, not added as zeros); the sum starts from +0.0 and adds the partials
 * of ALL blocks 0 .. ceil(m / 64) - 1 in ascending order.  The 6 correspondences of a sample are ONE block visited in
 * draw order, whatever their indices.
 *
 * ---- sampler -----------------------------------------------------------------------------------------------------------
 * mix(z) is that of amvs_epipolar.h.  Hypothesis h (h >= 0) draws 6 distinct indices, k = 0 .. 5:
 *     r = mix(seed ^ mix(6 h + k)) mod (m - k)
 *     for every index c chosen so far, visited in ascending order of c:  if r >= c then r = r + 1
 *     index k of the sample is r.
 * The sample keeps draw order.  There is no rejection; m = 6 always yields all six.
 *
 * ---- hypothesis: the pose of a sample -----------------------------------------------------------------------------------
 *  1. xn = (u - cx) / fx,  yn = (v - cy) / fy.
 *  2. c = (SUM(X) / 6.0, SUM(Y) / 6.0, SUM(Z) / 6.0);  dx = X - c[0], dy = Y - c[1], dz = Z - c[2],
 *     dist = sqrt(dx*dx + dy*dy + dz*dz);  d = SUM(dist) / 6.0;  s = R3 / d with R3 = 1.7320508075688772 (sqrt(3) rounded
 *     to float64);  P = [dx*s, dy*s, dz*s, 1.0].
 *  3. gx[j] = -(xn * P[j]),  gy[j] = -(yn * P[j])  for j = 0 .. 3: the two rows of the DLT system of a correspondence are
 *     [P, 0 0 0 0, gx] and [0 0 0 0, P, gy].
 *  4. the 12 x 12 matrix M of the normal equations, by blocks (i, j = 0 .. 3), each entry one SUM:
 *         M[i][j]     = M[4+i][4+j] = SUM(P[i] * P[j])                        for i <= j
 *         M[i][4+j]   = +0.0
 *         M[i][8+j]   = SUM(P[i] * gx[j]),   M[4+i][8+j] = SUM(P[i] * gy[j])  for all i, j
 *         M[8+i][8+j] = SUM(gx[i]*gx[j] + gy[i]*gy[j])                        for i <= j
 *     and M[b][a] = M[a][b].  Cyclic Jacobi on M with V = identity: exactly the rotation of amvs_match.h step 3 (with r
 *     running over 0 .. 11), AMVS_JACOBI_SWEEPS sweeps, each visiting (p, q), p < q, in lexicographic order; no early
 *     exit; a pair with g == 0 is skipped.  The diagonal entry taken is the smallest M[i][i], the lowest i on a tie (a NaN
 *     entry is never taken over entry 0); p = column i of V, read as the row-major 3 x 4 matrix (row r is p[4r .. 4r+3]).
 *  5. undo the scaling:  for r = 0 .. 2:  A[r][c] = p[4r+c] * s for c = 0, 1, 2;
 *         b[r] = p[4r+3] - A[r][0]*c[0] - A[r][1]*c[1] - A[r][2]*c[2]      (left to right)
 *  6. det = A[0][0]*(A[1][1]*A[2][2] - A[1][2]*A[2][1]) - A[0][1]*(A[1][0]*A[2][2] - A[1][2]*A[2][0])
 *           + A[0][2]*(A[1][0]*A[2][1] - A[1][1]*A[2][0]);   if det < 0 every entry of A and b is negated.
 *  7. the nearest rotation:  G[i][j] = A[0][i]*A[0][j] + A[1][i]*A[1][j] + A[2][i]*A[2][j] for i <= j, mirrored; the same
 *     Jacobi on the 3 x 3 G (pairs (0,1) (0,2) (1,2), the same sweep count) leaves w[k] = G[k][k] and V.  Then
 *         sw[k] = sqrt(w[k]);   B[r][k] = A[r][0]*V[0][k] + A[r][1]*V[1][k] + A[r][2]*V[2][k];   C[r][k] = B[r][k] / sw[k]
 *         R[r][c] = C[r][0]*V[c][0] + C[r][1]*V[c][1] + C[r][2]*V[c][2]
 *         sc = (sw[0] + sw[1] + sw[2]) / 3.0;   t[r] = b[r] / sc.
 * A degenerate sample (coplanar or repeated points, d == 0, a w that is not positive, NaN) is no error: it yields a pose,
 * possibly with entries that are not finite, that scores few or no inliers.
 *
 * ---- inlier test of correspondence i under (R, t), threshold thr ---------------------------------------------------------
 *     Xc[r] = R[r][0]*X + R[r][1]*Y + R[r][2]*Z + t[r]   for r = 0, 1, 2;      z = Xc[2]
 *     ex = fx*Xc[0] + (cx - u)*z;    ey = fy*Xc[1] + (cy - v)*z;    ee = ex*ex + ey*ey;    t2 = thr*thr
 *     inlier  iff  z > 0 and ee <= t2*(z*z) and ee < +infinity.
 * This is a reprojection error of at most thr pixels, without the division, AND a positive depth; cv.solvePnPRansac does
 * not test the depth.  A zero pose, or one with an entry that is not finite, has no inliers.
 *
 * ---- refit of a pose (R, t) to a set S, |S| >= 6 -------------------------------------------------------------------------
 * Gauss-Newton on the 6 parameters (om[0..2], dt[0..2]) of the left perturbation Xc <- Xc + om x Xc + dt, residuals in
 * pixels.  One PASS over S under a pose gives 29 SUMs.  A member with z > 0 (Xc, z as in the inlier test) contributes
 *     iz = 1.0 / z;  xz = Xc[0]*iz;  yz = Xc[1]*iz;  rx = fx*xz + cx - u;  ry = fy*yz + cy - v
 *     ax = fx*iz;  ay = fy*iz;  bx = -(ax*xz);  by = -(ay*yz)
 *     Jx = [bx*Xc[1],  ax*z - bx*Xc[0],  -(ax*Xc[1]),  ax,  0.0,  bx]
 *     Jy = [by*Xc[1] - ay*z,  -(by*Xc[0]),  ay*Xc[0],  0.0,  ay,  by]
 *     H[i][j] += Jx[i]*Jx[j] + Jy[i]*Jy[j]  for i <= j   (entries 0 .. 20, the upper triangle row by row; the products
 *                                                         with the two 0.0 are formed like the others)
 *     g[i]    += Jx[i]*rx + Jy[i]*ry                     (entries 21 .. 26)
 *     cost    += rx*rx + ry*ry                           (entry 27)
 *     front   += 1.0                                     (entry 28: the members in front of the camera, an exact count)
 * and a member that fails z > 0 contributes to none of them.
 * STEP from the sums of a pass, on the host:
 *   Cholesky, H = L L^T, for j = 0 .. 5:  s = H[j][j] - L[j][0]*L[j][0] - ... - L[j][j-1]*L[j][j-1] (left to right);  unless
 *   s > 0 and s < +infinity there is NO step;  L[j][j] = sqrt(s);  for i = j+1 .. 5:
 *   L[i][j] = (H[j][i] - L[i][0]*L[j][0] - ... - L[i][j-1]*L[j][j-1]) / L[j][j].
 *   y[i] = (-(g[i]) - L[i][0]*y[0] - ... - L[i][i-1]*y[i-1]) / L[i][i]  for i = 0 .. 5;
 *   x[i] = (y[i] - L[i+1][i]*x[i+1] - ... - L[5][i]*x[5]) / L[i][i]     for i = 5 .. 0;     om = x[0..2], dt = x[3..5].
 *   hx = 0.5*om[0], hy = 0.5*om[1], hz = 0.5*om[2];  n = sqrt(1.0 + hx*hx + hy*hy + hz*hz);
 *   qw = 1.0/n, qx = hx/n, qy = hy/n, qz = hz/n;  Q =
 *       [1.0 - 2.0*(qy*qy + qz*qz),   2.0*(qx*qy - qz*qw),         2.0*(qx*qz + qy*qw)      ]
 *       [2.0*(qx*qy + qz*qw),         1.0 - 2.0*(qx*qx + qz*qz),   2.0*(qy*qz - qx*qw)      ]
 *       [2.0*(qx*qz - qy*qw),         2.0*(qy*qz + qx*qw),         1.0 - 2.0*(qx*qx + qy*qy)]
 *   R'[r][c] = Q[r][0]*R[0][c] + Q[r][1]*R[1][c] + Q[r][2]*R[2][c];   t'[r] = Q[r][0]*t[0] + Q[r][1]*t[1] + Q[r][2]*t[2] + dt[r].
 * The iteration: steps = 0; the pass under the input pose gives the current sums.  Repeat at most AMVS_PNP_REFINE_STEPS
 * times: form the step from the current sums (no step: stop); pass under (R', t'); the step is KEPT iff
 * cost' <= cost and front' >= front, and then (R', t') and its sums become current and steps = steps + 1; otherwise it is
 * undone and the iteration stops.  The outputs are the current pose, steps and the current cost.
 *
 * ---- the entry points ---------------------------------------------------------------------------------------------------
 * amvs_pnp_hypotheses: hypotheses first .. first + count - 1: idx_out[j][k] the sample of hypothesis first + j in draw
 * order, R_out[j], t_out[j] its pose.  Errors: first < 0; count outside 1 .. AMVS_PNP_MAX_HYP.
 *
 * amvs_pnp_score: counts_out[j] = number of inliers of (R[j], t[j]), j < n.  Errors: n outside 1 .. AMVS_PNP_MAX_HYP.
 *
 * amvs_pnp_inliers: mask_out[i] = 1 for an inlier of (R, t) else 0, *count their number.
 *
 * amvs_pnp_refine: the refit of (R_in, t_in) to the correspondences whose mask byte is non-zero (mask NULL: all m);
 * *n_used = |S|.  Errors: fewer than 6 members.
 *
 * amvs_pnp_ransac.  Errors: a confidence not inside (0, 1); max_hypotheses outside 1 .. AMVS_PNP_MAX_HYP.
 *   The loop of amvs_fmat_ransac with batches of AMVS_PNP_BATCH and the exponent 6: after a batch, with
 *   w = (double)best / (double)m, w2 = w*w, p = w2*w2*w2:  N = 0 when p >= 1;  N = max_hypotheses when 1 - p == 1;
 *   otherwise N = ceil(log(1 - confidence) / log(1 - p)) (the C library's log).  Stop when done >= N or
 *   done == max_hypotheses.  The best hypothesis is the one with the largest count, the lowest h on a tie.
 *   info_out = [done, best hypothesis, its count].
 *   best < 6: no model -- AMVS_OK, R_out, t_out and mask_out all zero, *n_inliers = 0.  Otherwise S0 = the inliers of the
 *   best hypothesis' pose;  (R1, t1) = refit(that pose, S0), S1 = inliers(R1, t1);  |S1| < 6: no model.
 *   (R2, t2) = refit((R1, t1), S1), S2 = inliers(R2, t2); the result is (R2, t2, S2) when |S2| >= |S1|, else (R1, t1, S1).
 *   mask_out is exactly what amvs_pnp_inliers gives for the returned pose and *n_inliers its size.  The result depends on
 *   the points, K, the threshold, the confidence, max_hypotheses and the seed only.  */
#ifndef AMVS_RESECTION_H
#define AMVS_RESECTION_H

#include "amvs_epipolar.h"

#define AMVS_PNP_BATCH         1024
#define AMVS_PNP_BLOCK         64
#define AMVS_PNP_REFINE_STEPS  10
#define AMVS_PNP_MAX_POINTS    1048576
#define AMVS_PNP_MAX_HYP       1048576

#ifdef __cplusplus
extern "C" {
#endif

int amvs_pnp_hypotheses(amvs_ctx *ctx, const float *pts3d, const float *pts2d, int m, const double K[9], uint64_t seed,
                        int first, int count, int32_t *idx_out, double *R_out, double *t_out);

int amvs_pnp_score(amvs_ctx *ctx, const double *R, const double *t, int n, const float *pts3d, const float *pts2d, int m,
                   const double K[9], double threshold, int32_t *counts_out);

int amvs_pnp_inliers(amvs_ctx *ctx, const double R[9], const double t[3], const float *pts3d, const float *pts2d, int m,
                     const double K[9], double threshold, uint8_t *mask_out, int64_t *count);

int amvs_pnp_refine(amvs_ctx *ctx, const float *pts3d, const float *pts2d, int m, const double K[9], const double R_in[9],
                    const double t_in[3], const uint8_t *mask, double R_out[9], double t_out[3], int32_t *steps,
                    double *cost, int64_t *n_used);

int amvs_pnp_ransac(amvs_ctx *ctx, const float *pts3d, const float *pts2d, int m, const double K[9], double threshold,
                    double confidence, int max_hypotheses, uint64_t seed, double R_out[9], double t_out[3],
                    uint8_t *mask_out, int64_t *n_inliers, int32_t info_out[3]);

#ifdef __cplusplus
}
#endif

#endif
