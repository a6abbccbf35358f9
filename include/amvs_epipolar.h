/* amvs_epipolar.h -- geometric verification of matches in libamvs.so: a fundamental matrix fitted to the matches of two
 * views by RANSAC, and the inliers it keeps (csrc/amvs_fmat.hip).  It is the second half of the reference's
 * FeatureMatcher (match_pair_geometric: cv.findFundamentalMat(pts1, pts2, cv.FM_RANSAC, 2.0, 0.999)); the first half is
 * amvs_match.h.
 *
 * Why a header of its own: existing tests hold include/amvs.h to 92 entry points, amvs_depth.h to one, amvs_lens.h to
 * two and amvs_match.h to nine, and existing tests do not change.  What is declared here is bound from a fifth table,
 * _lib.EPIPOLAR_SIGNATURES; _lib.load() binds all five.  The library, the context and the error codes are those of
 * amvs.h.
 *
 * As in amvs_lens.h and amvs_match.h the text below IS the definition: it is judged against
 * tests/epipolar_restatement.py, written from this text alone, bit for bit.
 *
 * How this differs from cv.findFundamentalMat, on purpose: a hypothesis is the 8-point fit of 8 matches (OpenCV draws 7
 * and solves a cubic); a hypothesis is NOT forced to rank 2 (only the refits are); hypotheses are drawn and scored in
 * batches of AMVS_FMAT_BATCH, so the stopping rule is looked at once per batch; the best hypothesis is refitted to its
 * inliers twice (OpenCV once); the sampler is the counter-based one below.  The inlier test is OpenCV's.  Parity with
 * cv2 is UNPINNED: F and the inlier set agree with OpenCV's only as two RANSAC runs with
 * different random samples agree.
 *
 * Every entry point returns AMVS_EINVAL (-1) for a NULL context before anything else, AMVS_EINVAL for its other parameter
 * errors before anything is allocated, and AMVS_EINDEX from the index-checked build as amvs.h describes.  Errors common to
 * all five: m < 8 or m > AMVS_FMAT_MAX_MATCHES; a NULL pts1 / pts2 / output; a threshold that is not finite or <= 0; a
 * confidence that is not inside (0, 1).
 *
 * ---- arithmetic -------------------------------------------------------------------------------------------------------
 * pts1, pts2: [m][2] float32 on the host, match i = (x1, y1) in the first image and (x2, y2) in the second, in pixels;
 * promoted to float64.  Everything below is float64: one rounding per operation, nothing contracted, in exactly the
 * written order; division and square root are correctly rounded.  a + b + c means (a + b) + c.  Every comparison with a
 * NaN is false.  The sampler is integers only.
 *
 * SUM over a set S of matches of a term u(i): the match indices are cut into blocks of AMVS_FMAT_BLOCK = 64 consecutive
 * indices (block b holds 64 b .. 64 b + 63).  The partial of a block starts from +0.0 and adds u(i) for the members of S
 * in the block in ascending i (matches outside S are skipped, not added as zeros).  The sum starts from +0.0 and adds the
 * partials of ALL blocks 0 .. ceil(m / 64) - 1 in ascending b (an empty block adds its +0.0).  The 8 matches of a
 * sample are ONE block visited in draw order, whatever their indices.
 *
 * ---- sampler -----------------------------------------------------------------------------------------------------------
 * mix(z), all modulo 2^64 (the finaliser of splitmix64):
 *     z = z + 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *     return z ^ (z >> 31)
 * Hypothesis h (h >= 0) draws 8 distinct match indices, k = 0 .. 7:
 *     r = mix(seed ^ mix(8 h + k)) mod (m - k)
 *     for every index c chosen so far, visited in ascending order of c:  if r >= c then r = r + 1
 *     index k of the sample is r.
 * The sample keeps draw order.  There is no rejection; m = 8 always yields all eight matches.
 *
 * ---- fit of F to a set S (n = |S| >= 1 matches; N = (double)n) --------------------------------------------------------
 *  1. per image j = 1, 2:  cxj = SUM(xj) / N,  cyj = SUM(yj) / N.
 *  2. per image:  u = xj - cxj, v = yj - cyj, dist(i) = sqrt(u*u + v*v);  dj = SUM(dist) / N;  sj = R2 / dj with
 *     R2 = 1.4142135623730951 (sqrt(2) rounded to float64).
 *  3. per match:  xjn = (xj - cxj) * sj,  yjn = (yj - cyj) * sj, and the row
 *         a = [x2n*x1n, x2n*y1n, x2n, y2n*x1n, y2n*y1n, y2n, x1n, y1n, 1].
 *     M[i][j] = SUM(a[i] * a[j]) for i <= j (each product rounded before it is added), M[j][i] = M[i][j].
 *  4. cyclic Jacobi on the 9 x 9 M with V = identity: exactly the rotation of amvs_match.h step 3 (with r running over
 *     0 .. 8), AMVS_JACOBI_SWEEPS sweeps, each visiting (p, q), p < q, in lexicographic order (0,1) (0,2) ... (0,8) (1,2)
 *     ... (7,8); no early exit; a pair with g == 0 is skipped.  The diagonal entry taken is the smallest M[i][i], the
 *     lowest i on a tie (a NaN entry is never taken over entry 0); f = column i of V, f[r] = V[r][i], read as the
 *     row-major 3 x 3 matrix Fn (Fn[r][c] = f[3 r + c]).
 *  5. (the REFIT only; a hypothesis skips this step)  rank 2:  A[i][j] = f[i]*f[j] + f[3+i]*f[3+j] + f[6+i]*f[6+j] for
 *     i <= j < 3, mirrored; the same Jacobi on the 3 x 3 A (pairs (0,1) (0,2) (1,2), the same sweep count, the same
 *     choice of the smallest diagonal entry) gives v = that column of V.  Then for r = 0 .. 2:
 *         w = f[3r]*v[0] + f[3r+1]*v[1] + f[3r+2]*v[2];    f[3r+c] = f[3r+c] - w*v[c]  for c = 0, 1, 2.
 *  6. denormalise, F = T2^T Fn T1 with Tj = [sj 0 -sj cxj; 0 sj -sj cyj; 0 0 1], written out:
 *         for r = 0 .. 2:  G[r][0] = f[3r]*s1;  G[r][1] = f[3r+1]*s1;  G[r][2] = (f[3r+2] - G[r][0]*cx1) - G[r][1]*cy1
 *         for c = 0 .. 2:  F[0][c] = s2*G[0][c];  F[1][c] = s2*G[1][c];  F[2][c] = (G[2][c] - F[0][c]*cx2) - F[1][c]*cy2
 *  7. (the REFIT only)  q = F[0][0]*F[0][0] + F[0][1]*F[0][1] + ... + F[2][2]*F[2][2] (row-major, sequential);
 *     nrm = sqrt(q); every entry becomes F / nrm.  Then k is the row-major index of the entry of largest |F| (the first
 *     entry, replaced only by a strictly larger one); if F[k] < 0 every entry is negated.
 * A degenerate set (d == 0, collinear points, NaN) is no error: it yields an F that scores few or no inliers.
 *
 * ---- inlier test of match i under F, threshold thr ----------------------------------------------------------------------
 *     l2[r] = F[r][0]*x1 + F[r][1]*y1 + F[r][2]   for r = 0, 1, 2           (F x1)
 *     l1[c] = F[0][c]*x2 + F[1][c]*y2 + F[2][c]   for c = 0, 1              (F^T x2)
 *     e = x2*l2[0] + y2*l2[1] + l2[2];   dd = e*e
 *     n2 = l2[0]*l2[0] + l2[1]*l2[1];    n1 = l1[0]*l1[0] + l1[1]*l1[1];    t2 = thr*thr
 *     inlier  iff  n1 > 0 and n2 > 0 and dd <= t2*n2 and dd <= t2*n1 and dd < +infinity.
 * This is OpenCV's test (the larger of the two squared distances to the epipolar lines against thr^2) without the
 * divisions.  A zero F or one with an entry that is not finite has no inliers: a zero F fails n > 0, a NaN fails every
 * comparison, and an infinite entry makes dd infinite (or NaN) -- the last condition is there for it, since n1 and n2
 * can then be infinite as well and infinity <= infinity holds.
 *
 * ---- the entry points ---------------------------------------------------------------------------------------------------
 * amvs_fmat_hypotheses: hypotheses first .. first + count - 1: idx_out[j][k] the sample of hypothesis first + j in draw
 * order, F_out[j] its F (steps 1-4 and 6 on the sample), row-major.  Errors: first < 0; count outside 1 .. 2^20.
 *
 * amvs_fmat_score: counts_out[j] = number of inliers of F[j] among the m matches, j < n.  Errors: n outside 1 .. 2^20.
 *
 * amvs_fmat_inliers: mask_out[i] = 1 for an inlier of F else 0, *count their number.
 *
 * amvs_fmat_fit: the refit (steps 1-7) to the matches whose mask byte is non-zero (mask NULL: all m); *n_used = |S|.
 * Errors: fewer than 8 members.
 *
 * amvs_fmat_ransac.  Errors: max_hypotheses outside 1 .. 2^20.
 *   done = 0, best = -1.  Repeat: the next batch is hypotheses done .. done + nb - 1 with
 *   nb = min(AMVS_FMAT_BATCH, max_hypotheses - done); every one is scored on all m matches; the best hypothesis so far is
 *   the one with the largest count, the lowest h on a tie; done = done + nb.  Then with w = (double)best / (double)m,
 *   p = w*w, p = p*p, p = p*p:  N = 0 when p >= 1;  N = max_hypotheses when 1 - p == 1;  otherwise
 *   N = ceil(log(1 - confidence) / log(1 - p)) (the C library's log, float64).  Stop when done >= N or
 *   done == max_hypotheses.  info_out = [done, best hypothesis, its count].
 *   best < 8: no model -- AMVS_OK, F_out all zero, mask_out all zero, *n_inliers = 0.  Otherwise S0 = the inliers of the
 *   best hypothesis' F;  F1 = refit(S0), S1 = inliers(F1);  |S1| < 8: no model.  F2 = refit(S1), S2 = inliers(F2); the
 *   result is (F2, S2) when |S2| >= |S1|, else (F1, S1).  F_out is that F, mask_out its inlier set (so mask_out is
 *   exactly what amvs_fmat_inliers gives for F_out) and *n_inliers its size.  The result depends on the points, the
 *   threshold, the confidence, max_hypotheses and the seed only: counts are integers, so no launch shape enters.  */
#ifndef AMVS_EPIPOLAR_H
#define AMVS_EPIPOLAR_H

#include "amvs_match.h"

#define AMVS_FMAT_BATCH        1024
#define AMVS_FMAT_BLOCK        64
#define AMVS_FMAT_MAX_MATCHES  1048576
#define AMVS_FMAT_MAX_HYP      1048576

#ifdef __cplusplus
extern "C" {
#endif

int amvs_fmat_hypotheses(amvs_ctx *ctx, const float *pts1, const float *pts2, int m, uint64_t seed, int first, int count,
                         int32_t *idx_out, double *F_out);

int amvs_fmat_score(amvs_ctx *ctx, const double *F, int n, const float *pts1, const float *pts2, int m, double threshold,
                    int32_t *counts_out);

int amvs_fmat_inliers(amvs_ctx *ctx, const double F[9], const float *pts1, const float *pts2, int m, double threshold,
                      uint8_t *mask_out, int64_t *count);

int amvs_fmat_fit(amvs_ctx *ctx, const float *pts1, const float *pts2, const uint8_t *mask, int m, double F_out[9],
                  int64_t *n_used);

int amvs_fmat_ransac(amvs_ctx *ctx, const float *pts1, const float *pts2, int m, double threshold, double confidence,
                     int max_hypotheses, uint64_t seed, double F_out[9], uint8_t *mask_out, int64_t *n_inliers,
                     int32_t info_out[3]);

#ifdef __cplusplus
}
#endif

#endif
