/* amvs_twoview.h -- the start of a reconstruction from two views in libamvs.so: the relative pose of two views from their
 * fundamental matrix (decomposition of the essential matrix, the cheirality vote over the four candidates) and the
 * triangulation of their matches with every candidate's point, validity and parallax returned to the host
 * (csrc/amvs_twoview.hip, csrc/amvs_twoview_host.h).  It is the numerical core of the reference's src/core/geometry.py
 * (compute_essential_matrix, decompose_essential = cv.recoverPose, triangulate_points = cv.triangulatePoints followed by
 * validate_triangulation) as its SfMPipeline.find_best_initial_pair, initialize and triangulate_new_points call it.
 *
 * Why a header of its own: existing tests hold include/amvs.h to 92 entry points, amvs_depth.h to one, amvs_lens.h to two,
 * amvs_match.h to nine, amvs_epipolar.h to five, amvs_resection.h to five and amvs_step.h to three, and existing tests do
 * not change.  What is declared here is bound from an eighth table, _lib.TWOVIEW_SIGNATURES; _lib.load() binds all eight.
 * The library, the context and the error codes are those of amvs.h.
 *
 * As in amvs_epipolar.h and amvs_resection.h the text below IS the definition: it is judged against
 * tests/twoview_restatement.py, written from this text alone, bit for bit.
 *
 * How this differs from cv.recoverPose and cv.triangulatePoints, on purpose.  Parity with cv2 is UNPINNED (DESIGN.md
 * section 15):
 *   - the singular vectors of E come from the fixed-sweep Jacobi iteration on E^T E, not from an SVD of E; U and V get
 *     their third columns from cross products, so det U = det V = +1 without a sign fix-up, and the SIGN of the returned
 *     unit translation and which of the two rotations is called Ra are this text's, not OpenCV's (the SET of four
 *     candidates is the same);
 *   - the null vector of the 4 x 4 DLT system comes from the Jacobi iteration on A^T A (amvs_match.h), not from an SVD
 *     of A;
 *   - the vote counts a match for a candidate when BOTH depths are inside (0, max_depth); OpenCV applies the same four
 *     comparisons in float64 on its own triangulation; ties between candidates go to the lowest index here;
 *   - the mask is one byte 0 / 1 per match, not 0 / 255, and it is recomputed for the returned pose;
 *   - a candidate point of amvs_twoview_triangulate is valid only when every comparison below is TRUE.  The reference's
 *     validate_triangulation drops a point when a comparison of the opposite sense is true, which lets a NaN point (every
 *     comparison false) through as valid; here a NaN point is never valid.
 *
 * Every entry point returns AMVS_EINVAL (-1) for a NULL context before anything else, AMVS_EINVAL for its other parameter
 * errors before anything is allocated, and AMVS_EINDEX from the index-checked build as amvs.h describes.  Errors wherever
 * the argument exists: a NULL F / K / R / t / pts1 / pts2 / output (the point and per-match output arrays may be NULL when
 * m = 0, which only amvs_twoview_triangulate allows); fx or fy not finite or <= 0; cx or cy not finite; a skew K[1] != 0
 * (the checks of amvs_resection.h); m < 1 (amvs_twoview_triangulate: m < 0) or m > AMVS_TWOVIEW_MAX_MATCHES; n < 1 or
 * n > AMVS_TWOVIEW_MAX_POSES; max_depth NaN or <= 0 (+infinity is allowed); a threshold of amvs_twoview_triangulate
 * that is NaN.
 *
 * ---- conventions and arithmetic ---------------------------------------------------------------------------------------
 * pts1, pts2: [m][2] float32 on the host, match i = pixel (u1, v1) of the first view and (u2, v2) of the second; promoted
 * to float64.  K: double[9] row-major.  F: double[9] row-major, used as in amvs_epipolar.h: x2^T F x1 = 0.  A pose is R
 * double[9] row-major and t double[3]: Xc = R X + t; the first camera of a relative pose is [I | 0].
 * Everything below is float64: one rounding per operation, nothing contracted, in exactly the written order; the only
 * operations are + - * / and sqrt; division and square root are correctly rounded; -(a) flips the sign bit.
 * a + b + c means (a + b) + c.  Every comparison with a NaN is false.
 *
 * JACOBI3 on a symmetric 3 x 3 matrix G is the iteration of amvs_match.h step 3 with V = identity, the pairs (0,1) (0,2)
 * (1,2) in that order, AMVS_JACOBI_SWEEPS sweeps, no early exit, a pair with G[p][q] == 0 skipped, r running over 0 .. 2.
 * It leaves w[k] = G[k][k] and V.
 *
 * DLT of one match under two 3 x 4 matrices P_1, P_2 and image coordinates (x1, y1), (x2, y2) is amvs_match.h steps 1 to 4
 * verbatim: the four rows, M = A^T A, the 4 x 4 Jacobi iteration, the column v of the smallest diagonal entry (lowest
 * index on a tie, a NaN entry never taken over entry 0), X[i] = v[i] / v[3].
 *
 * ---- amvs_twoview_decompose: the four pose candidates of F -----------------------------------------------------------
 * With fx = K[0], fy = K[4], cx = K[2], cy = K[5] (the other entries of K are not read), E = K^T F K written out:
 *     T[r][0] = F[r][0]*fx;   T[r][1] = F[r][1]*fy;   T[r][2] = F[r][0]*cx + F[r][1]*cy + F[r][2]          r = 0, 1, 2
 *     E[0][c] = fx*T[0][c];   E[1][c] = fy*T[1][c];   E[2][c] = cx*T[0][c] + cy*T[1][c] + T[2][c]          c = 0, 1, 2
 *     G[i][j] = E[0][i]*E[0][j] + E[1][i]*E[1][j] + E[2][i]*E[2][j]  for i <= j, G[j][i] = G[i][j];   (w, V) = JACOBI3(G)
 *     k3 = 0;  if w[1] < w[k3] then k3 = 1;  if w[2] < w[k3] then k3 = 2          (the smallest, the lowest index on a tie)
 *     a < b the two other indices:  k1 = a, k2 = b;  if w[b] > w[a] then k1 = b, k2 = a       (the larger first)
 * NO MODEL unless w[k2] > 0 and w[k2] < +infinity: *ok = 0, every output entry +0.0, AMVS_OK.  (A zero F and an F with a NaN
 * entry have no model; a rank-1 F has none unless rounding leaves a positive w[k2], and its candidates then count next to
 * nothing below.  w[k1] is not tested: candidates that are not finite count nothing either.)  Otherwise *ok = 1 and
 *     v1[r] = V[r][k1], v2[r] = V[r][k2];   v3 = v1 x v2:  v3[0] = v1[1]*v2[2] - v1[2]*v2[1],
 *                                                          v3[1] = v1[2]*v2[0] - v1[0]*v2[2],  v3[2] = v1[0]*v2[1] - v1[1]*v2[0]
 *     s1 = sqrt(w[k1]), s2 = sqrt(w[k2]);
 *     u1[r] = (E[r][0]*v1[0] + E[r][1]*v1[1] + E[r][2]*v1[2]) / s1;   u2[r] likewise with v2 and s2;   u3 = u1 x u2 (as v3)
 *     Ra[r][c] = u2[r]*v1[c] - u1[r]*v2[c] + u3[r]*v3[c]         (U W V^T with W = [0 -1 0; 1 0 0; 0 0 1], entry by entry)
 *     Rb[r][c] = u1[r]*v2[c] - u2[r]*v1[c] + u3[r]*v3[c]         (U W^T V^T)
 *     t[r] = u3[r]
 * R_out[0] = Ra, R_out[1] = Rb, t_out = t, w_out = (w[k1], w[k2], w[k3]) (the squared singular values of E, descending).
 * The four candidates are, in this order, (Ra, t) (Rb, t) (Ra, -t) (Rb, -t).  This entry point is host arithmetic.
 *
 * ---- the cheirality test of match i under a pose (R, t), limit max_depth ------------------------------------------------
 *     xn1 = (u1 - cx) / fx,  yn1 = (v1 - cy) / fy,  xn2 = (u2 - cx) / fx,  yn2 = (v2 - cy) / fy
 *     Q = DLT with P_1 = [1 0 0 0; 0 1 0 0; 0 0 1 0], P_2 = [R | t], (x1, y1) = (xn1, yn1), (x2, y2) = (xn2, yn2);
 *         the products with the zeros and ones of P_1 are formed like the others (xn1 * 0.0 is -0.0 for a negative xn1,
 *         NaN for an infinite one)
 *     z1 = Q[2];    z2 = R[2][0]*Q[0] + R[2][1]*Q[1] + R[2][2]*Q[2] + t[2]
 *     in front  iff  z1 > 0 and z1 < max_depth and z2 > 0 and z2 < max_depth.
 * Depths are in units of the baseline when t has unit length; cv.recoverPose uses 50.  A point at infinity (v[3] == 0)
 * gives an infinite or NaN Q, a pose with a NaN entry a NaN z2: both fail the test.  The zero pose counts nothing either
 * (z2 == 0).
 *
 * amvs_twoview_score: counts_out[j] = the number of matches in front under (R[j], t[j]), j < n.  Integers: no launch shape
 * enters the result (a workgroup holds 256 matches and walks AMVS_TWOVIEW_POSE_TILE poses; stated because the tests aim at
 * its edges).
 *
 * amvs_twoview_front: mask_out[i] = 1 for a match in front under (R, t) else 0, *count their number.
 *
 * amvs_twoview_pose: the whole of cv.recoverPose.  Decompose F; no model: every output zero, AMVS_OK.  Score the four
 * candidates in the order above (-t flips the three sign bits); the best is the one with the largest count, the lowest
 * index on a tie; a best count of 0 is no model as well.  Otherwise R_out, t_out = the best candidate, mask_out and
 * *n_front exactly what amvs_twoview_front gives for it, info_out = [best index, count 0, count 1, count 2, count 3].
 *
 * ---- amvs_twoview_triangulate ------------------------------------------------------------------------------------------
 * P_k, C_k (k = 1, 2) are formed from K (all nine entries), R_k, t_k once per call on the host as amvs_match.h writes them.
 * Per candidate i, in pixels: X = DLT with P_1, P_2, (x1, y1) = (u1, v1), (x2, y2) = (u2, v2); z_k of amvs_match.h step 5,
 * cs of step 6, e_k of step 7.  X_out[i] = X and cos_out[i] = cs for EVERY candidate, whatever the tests decide, and
 *     valid_out[i] = 1  iff  z_1 > depth_min and z_2 > depth_min and z_1 <= depth_max and z_2 <= depth_max
 *                            and cs <= cos_max_parallax and e_1 <= max_reproj and e_2 <= max_reproj,     else 0;
 * *n_valid their number.  These are the comparisons of the reference's validate_triangulation (0.01, 200 baselines,
 * 1 degree, 4 px; the host passes the cosine, so no acos runs on the device) stated positively, with its inclusive sides;
 * a NaN anywhere makes the candidate invalid.  m = 0 is not an error and writes nothing but *n_valid = 0.  */
#ifndef AMVS_TWOVIEW_H
#define AMVS_TWOVIEW_H

#include "amvs_match.h"

#define AMVS_TWOVIEW_MAX_MATCHES       1048576
#define AMVS_TWOVIEW_MAX_POSES         1048576
#define AMVS_TWOVIEW_POSE_TILE         32
/* the defaults of the Python layer (the reference's constants; the C entry points take every value as an argument) */
#define AMVS_TWOVIEW_MAX_DEPTH         50.0
#define AMVS_TWOVIEW_DEPTH_MIN         0.01
#define AMVS_TWOVIEW_DEPTH_BASELINES   200.0
#define AMVS_TWOVIEW_MIN_PARALLAX_DEG  1.0
#define AMVS_TWOVIEW_MAX_REPROJ        4.0

#ifdef __cplusplus
extern "C" {
#endif

int amvs_twoview_decompose(amvs_ctx *ctx, const double F[9], const double K[9], double R_out[2][9], double t_out[3],
                           double w_out[3], int32_t *ok);

int amvs_twoview_score(amvs_ctx *ctx, const double *R, const double *t, int n, const float *pts1, const float *pts2, int m,
                       const double K[9], double max_depth, int32_t *counts_out);

int amvs_twoview_front(amvs_ctx *ctx, const double R[9], const double t[3], const float *pts1, const float *pts2, int m,
                       const double K[9], double max_depth, uint8_t *mask_out, int64_t *count);

int amvs_twoview_pose(amvs_ctx *ctx, const double F[9], const double K[9], const float *pts1, const float *pts2, int m,
                      double max_depth, double R_out[9], double t_out[3], uint8_t *mask_out, int64_t *n_front,
                      int32_t info_out[5]);

int amvs_twoview_triangulate(amvs_ctx *ctx, const double K[9], const double R1[9], const double t1[3], const double R2[9],
                             const double t2[3], const float *pts1, const float *pts2, int m, double depth_min,
                             double depth_max, double cos_max_parallax, double max_reproj, double *X_out,
                             uint8_t *valid_out, double *cos_out, int64_t *n_valid);

#ifdef __cplusplus
}
#endif

#endif
