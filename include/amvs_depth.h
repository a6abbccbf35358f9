/* amvs_depth.h -- the cross-view depth-map filter of libamvs.so (csrc/amvs_depth_filter.hip).
 *
 * Why a header of its own: tests/test_cloud_normals_cpu.py holds include/amvs.h to exactly the 92 entry points of
 * _lib.SIGNATURES, and existing tests do not change.  What is added to the C ABI after that test is declared here and bound
 * from a second table, _lib.DEPTH_SIGNATURES; _lib.load() binds both.  The library, the context and the error codes are
 * those of amvs.h.
 *
 * ---- the filter ---------------------------------------------------------------------------------------------------------
 * Per pixel of every map: the number of OTHER maps whose own depth agrees after forward-backward reprojection, and the
 * mean of the agreeing depths.  The reference never checks its depth maps against each other; no counterpart, hence no
 * parity: judged against tests/depth_filter_restatement.py, written from the text below, bit for bit (DESIGN.md section
 * 10).  It is separate from amvs_xpm_consistency, which is a step of the extended mode: that one reads the extended
 * mode's job table and cost maps, computes in float32 and returns a count, never a depth.  The output is a pair of maps
 * (depth, count) that amvs_fuse_filter*, amvs_stereo_backproject*, amvs_tsdf_integrate, amvs_depth_normals and
 * amvs_cloud_normals consume as they consume (depth, confidence), with min_consistent as their threshold.
 *
 * Arithmetic.  All arithmetic below is float64: one rounding per operation, nothing contracted, in exactly the written
 * order.  Integers are converted exactly.
 *
 * Inputs.  n_maps maps depth, conf, each [n_maps][H][W] float32 at the context's size; maps_where as in
 * amvs_depth_normals: 0 host arrays, 1 device pointers, 2 the resident maps of the last amvs_plane_sweep_batch (depth and
 * conf are then ignored).  K[9] and K_inv[9], float64, row-major.  poses, n_maps x 12 float64: R row-major, then t, with
 * X_cam = R X_world + t.  neighbours, either NULL or [n_maps][n_nbr] int32: an entry is a map index or -1 for none; NULL
 * means every other map in ascending index (n_nbr is then ignored).  min_confidence (float32).  max_px and max_rel
 * (float32, positive and finite).  min_consistent (>= 1).  refine (0 or 1).
 *
 * Validity.  A pixel is VALID iff, in float32, depth > 0, depth <= FLT_MAX and conf >= min_confidence.  NaN fails each
 * comparison.  (The rule of amvs_depth_normals.)
 *
 * Per pixel.  Take a valid pixel (x, y) of map j with d = (double)depth.  Start with cnt = 0 and s = d.  Visit the
 * neighbours i of row j in stored order, skipping -1.  R_j, t_j are the pose of map j, R_i, t_i that of map i.
 *   1. r_c = (K_inv[c][0]*x + K_inv[c][1]*y) + K_inv[c][2] and P_c = r_c * d, for c = 0, 1, 2.
 *   2. Q_c = P_c - t_j[c], then Xw_c = (R_j[0][c]*Q_0 + R_j[1][c]*Q_1) + R_j[2][c]*Q_2.
 *   3. Xi_c = ((R_i[c][0]*Xw_0 + R_i[c][1]*Xw_1) + R_i[c][2]*Xw_2) + t_i[c].  Skip unless Xi_2 > 0.
 *   4. uvw_c = (K[c][0]*Xi_0 + K[c][1]*Xi_1) + K[c][2]*Xi_2.  Skip unless uvw_2 > 0.
 *      px = floor(uvw_0/uvw_2 + 0.5) and py = floor(uvw_1/uvw_2 + 0.5).
 *      Skip unless 0 <= px < W and 0 <= py < H, compared in float64 before any integer conversion (NaN fails).
 *   5. Skip unless pixel (px, py) of map i is VALID.  di is its depth, widened to float64.
 *   6. Steps 1 to 3 with the roles swapped: from the integer pixel (px, py) with depth di through pose i into camera j.
 *      This gives Y_c.  Skip unless Y_2 > 0.
 *   7. Step 4 on Y without the rounding: skip unless uvw_2 > 0; u = uvw_0/uvw_2, v = uvw_1/uvw_2.
 *      eu = u - x, ev = v - y and e2 = eu*eu + ev*ev.
 *   8. The neighbour is CONSISTENT iff e2 <= (double)max_px*(double)max_px and fabs(Y_2 - d) <= (double)max_rel * d.
 *      If so, cnt += 1 and s += Y_2.
 *
 * Outputs.  count_out[j][y][x] = (float)cnt; 0 for an invalid pixel.  depth_out[j][y][x] = 0 if the pixel is invalid or
 * cnt < min_consistent; the input depth if refine == 0; otherwise (float)(s / (double)(cnt + 1)).  counts[0] = the number
 * of valid input pixels, counts[1] = the number of pixels kept (valid and cnt >= min_consistent).
 * The sums live in registers with a fixed neighbour order; there are no atomics on them.  The outputs never alias the
 * inputs while a pixel is being read (out_where = 2 below).
 *
 * out_where: 0 host arrays; 1 device pointers, which must not overlap the inputs; 2 replace the resident plane-sweep maps
 * (depth by depth_out, confidence by count_out; allowed only with maps_where = 2; depth_out and count_out are ignored):
 * the step computes into scratch blocks of the context's cache and copies them back in stream order, so that
 * amvs_stereo_backproject_views, amvs_fetch_sweep_maps and maps_where = 2 of the normals then read the filtered maps.
 * Nothing else is kept on the device: the outputs are the interface.  Synchronises.
 *
 * Errors (AMVS_EINVAL before anything is allocated): a NULL required pointer (ctx, K, K_inv, poses, counts; the maps
 * unless maps_where = 2; the outputs unless out_where = 2); n_maps < 1; maps_where or out_where outside 0 .. 2; out_where
 * = 2 without maps_where = 2; device outputs that overlap device inputs; max_px or max_rel not positive and finite;
 * min_consistent < 1; n_nbr < 1 with a non-NULL list; a neighbour entry outside -1 .. n_maps - 1, equal to its own row, or
 * repeated within a row; more than 2^31 - 1 pixels; maps_where = 2 without a resident sweep batch of n_maps maps.         */
#ifndef AMVS_DEPTH_H
#define AMVS_DEPTH_H

#include "amvs.h"

#ifdef __cplusplus
extern "C" {
#endif

int amvs_depth_filter(amvs_ctx *ctx, int n_maps, const void *depth, const void *conf, int maps_where,
                      const double K[9], const double K_inv[9], const double *poses,
                      const int32_t *neighbours, int n_nbr,
                      float min_confidence, float max_px, float max_rel, int min_consistent, int refine,
                      void *depth_out, void *count_out, int out_where, int64_t counts[2]);

#ifdef __cplusplus
}
#endif

#endif
