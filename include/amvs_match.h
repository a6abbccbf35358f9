/* amvs_match.h -- the dense-SIFT mode of libamvs.so: exact descriptor matching on the matrix cores (csrc/amvs_match.hip),
 * two-view triangulation into an accumulating cloud (csrc/amvs_triangulate.hip) and the cloud steps anchored at the
 * cloud's minimum (bounds, grid voxel de-duplication).
 *
 * Why a header of its own: existing tests hold include/amvs.h to the 92 entry points of _lib.SIGNATURES, amvs_depth.h to
 * one and amvs_lens.h to two, and existing tests do not change.  What is declared here is bound from a fourth table,
 * _lib.MATCH_SIGNATURES; _lib.load() binds all four.  The library, the context and the error codes are those of amvs.h.
 *
 * As in amvs_lens.h the text below IS the definition: it is judged against tests/match_restatement.py, written from
 * this text alone, bit for bit.  It restates what the reference's dense mode does after its feature extractor
 * (matching, ratio test, DLT triangulation with three filters, the cloud filter's voxel grid); the extractor stays
 * OpenCV's and is no part of this library.
 *
 * Every entry point returns AMVS_EINVAL (-1) for a NULL context before anything else, AMVS_EINVAL for its other parameter
 * errors before anything is allocated, and AMVS_EINDEX from the index-checked build as amvs.h describes.
 *
 * ---- descriptors ----------------------------------------------------------------------------------------------------
 * A descriptor is 128 integers in 0 .. 255 (SIFT as OpenCV stores it).  The distance of two descriptors a and b is
 *     s(a, b) = sum over the 128 dimensions of (a - b)^2,
 * an exact integer of at most 128 * 255^2 = 8 323 200.  The library subtracts 128 from every byte, multiplies signed
 * bytes with 32-bit integer accumulation and forms s = |a|^2 + |b|^2 - 2 a.b; nothing in that rounds, so s is exact
 * whatever the tiling.  The search is EXACT: every train row is compared with every query row.  The reference's FLANN
 * index (trees = 5, checks = 100) is approximate, so its match set is not this one; at equal descriptors this is the set
 * FLANN approximates.  Parity with cv2 is UNPINNED.
 *
 * amvs_desc_set: uploads desc_u8, [n][d] uint8 row-major, into the resident slot `slot` of the context, replacing what
 * the slot held (a slot set again with fewer rows holds the new rows only).  Errors: d != 128; n < 0 or
 * n > AMVS_DESC_MAX_ROWS; slot outside 0 .. AMVS_DESC_MAX_SLOTS - 1; desc_u8 NULL with n > 0.  n = 0 is an empty slot.
 *
 * amvs_desc_knn2: for every row i of slot_q the two rows of slot_t that are smallest under the order (s, j): s the
 * distance to row i, j the train index.  Ties in s go to the lower index; the second entry is the next row in that order
 * and may have the same s.  idx_out[i][0], dist2_out[i][0] are the best row and its s, [i][1] the second; both arrays are
 * int32 [n_q][2] on the host.  The result does not depend on tiling, on how the train set is split across workgroups or
 * on launch shape: every partial result is a pair of (s, j) and pairs are merged by the same order.  Errors: a slot that
 * was never set; fewer than 2 train rows; a NULL output with n_q > 0.  n_q = 0 writes nothing.
 *
 * amvs_desc_match: Lowe's ratio test on top of amvs_desc_knn2, compacted on the device in query order.  Query i with
 * best (s1, j1) and second (s2, j2) is kept when
 *     (double)s1 < ((double)ratio * (double)ratio) * (double)s2
 * with ratio a float32, every operation in float64 rounded once and nothing contracted.  The reference compares
 * m.distance < ratio * n.distance on the float32 square roots of s1 and s2; the two tests can differ only at a rounding
 * tie (where sqrt(s1) and ratio * sqrt(s2) round to neighbouring or equal float32 values).  With cross_check != 0 a
 * match (i, j1) survives only if the search of slot_t against slot_q, under the same ratio test, keeps row j1 with best
 * index i (the symmetric filter of the reference's FeatureMatcher.match).  Outputs, host, capacity n_q each: q_idx_out
 * (ascending), t_idx_out, dist2_out (s1), and *n_matches.  Errors: as amvs_desc_knn2, in both directions with
 * cross_check (so n_q >= 2 then); ratio not finite or <= 0; NULL n_matches; a NULL output array with n_q > 0.
 *
 * Launch shape (stated because the tests aim at its edges; it is no part of the result): a matrix instruction covers
 * AMVS_DESC_TILE = 32 train rows x 32 queries; a workgroup holds AMVS_DESC_QUERY_BLOCK = 512 queries (four waves of four
 * query tiles each); the running best pair is kept in 32-bit keys over a chunk of AMVS_DESC_CHUNK = 256 train rows and widened to (s, j) after each chunk;
 * the chunks are dealt to `splits` workgroups per query block, splits = ceil(chunks / ceil(chunks / want)) with
 * want = max(1, min(chunks, 2048 / query blocks)), and the partial pairs are merged by a second kernel.
 *
 * ---- triangulation into the accumulating cloud -------------------------------------------------------------------------
 * amvs_pair_cloud_begin empties the accumulating cloud of the context.  amvs_pair_triangulate triangulates the m
 * candidates of one pair of views, appends the accepted points and their colours in candidate order and returns their
 * number in *n_accepted.  amvs_pair_cloud_finish makes the accumulated cloud the context's resident cloud (the one of
 * amvs_cloud_knn_mean_distance, amvs_cloud_take, amvs_fetch_cloud, amvs_cloud_normals ...), returns its size in *total and
 * leaves the accumulator empty and closed.  Points do not visit the host in between.  triangulate and finish without a
 * begin are errors.
 *
 * Inputs of amvs_pair_triangulate: K[9], R1[9], t1[3], R2[9], t2[3] float64, row-major (x_cam = R X + t); pts1, pts2:
 * [m][2] float32, the matched keypoints (x, y) in pixels; rgb: [m][3] uint8, the caller's colour of EVERY candidate;
 * depth_min, depth_max, cos_min_parallax, max_reproj: float64 (the reference: 0.1, 50, cos(0.3 degrees), 6).
 * Errors: NULL pointers with m > 0; m < 0 or m > 2^24; a threshold that is NaN.  m = 0 appends nothing.
 *
 * Arithmetic.  All float64: one rounding per operation, nothing contracted, in exactly the written order; division and
 * square root are correctly rounded (amvs_match_selftest_sqrt lets a test verify the latter).  Sums written a + b + c
 * mean (a + b) + c.
 *
 * Per view k (on the host, once per call):
 *     P_k[r][c] = K[r][0]*Rt[0][c] + K[r][1]*Rt[1][c] + K[r][2]*Rt[2][c]       with Rt = [R_k | t_k], r = 0..2, c = 0..3
 *     C_k[i]    = -(R_k[0][i]*t_k[0] + R_k[1][i]*t_k[1] + R_k[2][i]*t_k[2])    the camera centre, i = 0..2
 * Per candidate, with (x1, y1) = pts1 and (x2, y2) = pts2 promoted to float64:
 *  1. the rows of A (what cv.triangulatePoints solves), for c = 0..3:
 *         a0[c] = x1*P_1[2][c] - P_1[0][c]      a1[c] = y1*P_1[2][c] - P_1[1][c]
 *         a2[c] = x2*P_2[2][c] - P_2[0][c]      a3[c] = y2*P_2[2][c] - P_2[1][c]
 *  2. M = A^T A:  M[i][j] = a0[i]*a0[j] + a1[i]*a1[j] + a2[i]*a2[j] + a3[i]*a3[j]  for i <= j, M[j][i] = M[i][j].
 *  3. cyclic Jacobi on M, V = identity: AMVS_JACOBI_SWEEPS = 10 sweeps, each visiting (p, q) in the order
 *     (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); there is no early exit.  A pair with g = M[p][q] == 0 is skipped.  Otherwise
 *         theta = (M[q][q] - M[p][p]) / (2*g)
 *         t = 0.5 / theta                                               if |theta| > 1e150   (theta^2 would overflow)
 *         t = sgn(theta) / (|theta| + sqrt(theta*theta + 1))            otherwise, sgn(0) = +1
 *         c = 1 / sqrt(t*t + 1)        s = t*c
 *         M[p][p] = M[p][p] - t*g      M[q][q] = M[q][q] + t*g      M[p][q] = M[q][p] = 0
 *         for r other than p, q, ascending:  x = M[r][p], y = M[r][q]:
 *             M[r][p] = M[p][r] = c*x - s*y        M[r][q] = M[q][r] = s*x + c*y
 *         for r = 0..3:  x = V[r][p], y = V[r][q]:  V[r][p] = c*x - s*y      V[r][q] = s*x + c*y
 *     At the end the diagonal entry taken is the smallest M[i][i], the lowest i on a tie (a comparison with NaN is false,
 *     so a NaN entry is never taken over entry 0); v = column i of V.
 *  4. X[i] = v[i] / v[3], i = 0..2.
 *  5. depth test: z_k = R_k[2][0]*X[0] + R_k[2][1]*X[1] + R_k[2][2]*X[2] + t_k[2]; keep when
 *     z_1 > depth_min and z_1 < depth_max and z_2 > depth_min and z_2 < depth_max.
 *  6. parallax test: w_k = X - C_k; dot = w_1[0]*w_2[0] + w_1[1]*w_2[1] + w_1[2]*w_2[2];
 *     n_k = sqrt(w_k[0]*w_k[0] + w_k[1]*w_k[1] + w_k[2]*w_k[2]); cs = dot / (n_1*n_2 + 1e-8); keep when
 *     cs < cos_min_parallax.  The host passes cos(0.3 degrees), so no acos runs on the device; this equals the reference's
 *     degrees(arccos(clip(cs, -1, 1))) > 0.3 up to the rounding of arccos, degrees and cos.
 *  7. reprojection test, per view: pc[r] = R_k[r][0]*X[0] + R_k[r][1]*X[1] + R_k[r][2]*X[2] + t_k[r];
 *     h[r] = K[r][0]*pc[0] + K[r][1]*pc[1] + K[r][2]*pc[2]; u = h[0]/h[2], v = h[1]/h[2]; du = u - x_k, dv = v - y_k;
 *     e_k = sqrt(du*du + dv*dv); keep when e_1 < max_reproj and e_2 < max_reproj.
 * The filters apply in that order; every comparison with NaN is false, so such a candidate is dropped.  A survivor
 * appends X and its rgb.  The normal-matrix route agrees with an SVD of A to about 5e-12 relative in X at the
 * reference's parallax floor.
 *
 * ---- bounds and the voxel grid anchored at a point ----------------------------------------------------------------------
 * amvs_cloud_bounds: per-axis minimum and maximum of the resident cloud's points whose keep_mask byte is non-zero
 * (keep_mask: host, one byte per point, NULL = all); of two zeros -0 is the smaller, so the result does not depend on the order
 * the points are visited in; NaN coordinates are passed over.  Errors: no resident cloud; no kept point; NULL outputs.
 *
 * amvs_cloud_voxel_downsample_grid: the voxel de-duplication of the reference's dense mode.  For every kept point p the
 * voxel index is, per axis a, iv[a] = (int64)floor((p[a] - origin[a]) / voxel_size) in float64.  The first kept point
 * (lowest point index) of every occupied voxel is kept; the survivors leave in lexicographic (iv[0], iv[1], iv[2])
 * order with their colours (np.unique of the index rows with return_index).  The resident cloud is replaced; *count is
 * its new size.  amvs_cloud_voxel_downsample of amvs.h (voxels anchored at 0, another key) stays as it is; the stable
 * sort and the compaction are shared with it.  Errors: no resident cloud; voxel_size not finite or <= 0; origin NULL or
 * not finite; NULL count; kept points that are not finite, or whose voxel indices span more than 2^62 voxels in all
 * (AMVS_EINVAL after the bounds pass, the resident cloud unchanged).  No kept point leaves an empty cloud.
 *
 * amvs_match_selftest_sqrt is a TEST HOOK, not a supported interface (it may change or go without notice): out[i] = sqrt(in[i]) in float64 on the device for n <= 2^24 host values: the square root
 * the triangulation uses, for a test to compare with a correctly rounded one.                                          */
#ifndef AMVS_MATCH_H
#define AMVS_MATCH_H

#include "amvs.h"

#define AMVS_DESC_DIM          128
#define AMVS_DESC_MAX_ROWS     1048576
#define AMVS_DESC_MAX_SLOTS    65536
#define AMVS_DESC_TILE         32
#define AMVS_DESC_CHUNK        256
#define AMVS_DESC_QUERY_BLOCK  512
#define AMVS_JACOBI_SWEEPS     10

#ifdef __cplusplus
extern "C" {
#endif

int amvs_desc_set(amvs_ctx *ctx, int slot, const uint8_t *desc_u8, int n, int d);

int amvs_desc_knn2(amvs_ctx *ctx, int slot_q, int slot_t, int32_t *idx_out, int32_t *dist2_out);

int amvs_desc_match(amvs_ctx *ctx, int slot_q, int slot_t, float ratio, int cross_check,
                    int32_t *q_idx_out, int32_t *t_idx_out, int32_t *dist2_out, int64_t *n_matches);

int amvs_pair_cloud_begin(amvs_ctx *ctx);

int amvs_pair_triangulate(amvs_ctx *ctx, const double K[9], const double R1[9], const double t1[3],
                          const double R2[9], const double t2[3], const float *pts1, const float *pts2,
                          const uint8_t *rgb, int m, double depth_min, double depth_max,
                          double cos_min_parallax, double max_reproj, int64_t *n_accepted);

int amvs_pair_cloud_finish(amvs_ctx *ctx, int64_t *total);

int amvs_cloud_bounds(amvs_ctx *ctx, const uint8_t *keep_mask, double min_out[3], double max_out[3]);

int amvs_cloud_voxel_downsample_grid(amvs_ctx *ctx, const uint8_t *keep_mask, const double origin[3],
                                     double voxel_size, int64_t *count);

int amvs_match_selftest_sqrt(amvs_ctx *ctx, const double *in, int n, double *out);

#ifdef __cplusplus
}
#endif

#endif
