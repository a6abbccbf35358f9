/* amvs_sfm.h -- the track state of an incremental reconstruction, resident in a context of libamvs.so: which keypoint of
 * which view observes which point, which views are registered, the points themselves, and the integer rules that select the
 * next view, collect its 2-D / 3-D correspondences, make new points from its verified matches, list the observations for a
 * bundle adjustment and take observations away again (csrc/amvs_sfm.hip, csrc/amvs_capi_sfm.hip, csrc/amvs_sfm_state.h).
 * It is the bookkeeping of the reference's src/core/sfm_pipeline.py (point_observations, camera_poses, find_next_image,
 * the correspondence loop of register_image, triangulate_new_points) around the numerical stages of amvs_epipolar.h,
 * amvs_resection.h, amvs_twoview.h and amvs_bundle.h.
 *
 * Why a header of its own: existing tests hold include/amvs.h to 92 entry points, amvs_depth.h to one, amvs_lens.h to two,
 * amvs_match.h to nine, amvs_epipolar.h, amvs_resection.h, amvs_twoview.h and amvs_bundle.h to five each and amvs_step.h to
 * three, and existing tests do not change.  What is declared here is bound from a tenth table, _lib.SFM_SIGNATURES;
 * _lib.load() binds all ten.  The library, the context and the error codes are those of amvs.h.
 *
 * As in amvs_twoview.h the text below IS the definition: it is judged against tests/sfm_state_restatement.py, written from
 * this text alone -- integers exactly, points bit for bit.
 *
 * How this differs from the reference's bookkeeping, on purpose.  Parity with it is UNPINNED:
 *   - amvs_sfm_scores counts the DISTINCT keypoints of a view that a match ties to an observed point; find_next_image
 *     counts match rows, so a keypoint matched into three registered views counts three times there and once here;
 *   - amvs_sfm_correspondences resolves conflicts by rank, in parallel (stages A and B below).  The reference takes, per
 *     inlier, the first registered view and match in dictionary order, and tests/sfm_chain.py the first claim in its
 *     sequential walk.  The rule here and the sequential first-come rule differ only when a keypoint has candidates
 *     from two different points: first-come then lets a keypoint that lost its first candidate go on to its second,
 *     here it gets nothing;
 *   - the reference finds a match's keypoint by comparing pixel coordinates with np.allclose; here a match row names its
 *     two keypoints by index and nothing is compared;
 *   - a point is valid only when every comparison of amvs_twoview_triangulate is TRUE (a NaN point is never valid);
 *   - point ids are never reused, and a point that dies takes its observations with it.
 *
 * Every entry point returns AMVS_EINVAL (-1) for a NULL context before anything else, AMVS_EINVAL for its other parameter
 * errors before anything is allocated or changed, and AMVS_EINDEX from the index-checked build as amvs.h describes.  Every
 * entry point but amvs_sfm_begin is an error before the first successful amvs_sfm_begin.  A NULL array is an error wherever
 * the argument exists, except that an array of length 0 may be NULL.
 *
 * ---- the state ---------------------------------------------------------------------------------------------------------
 * V views; view v has n_v keypoints; off_0 = 0, off_(v+1) = off_v + n_v, G = off_V.  Keypoint k of view v has the GLOBAL
 * index g = off_v + k and the float32 pixel kp[g] = (u, v).
 * P verified pairs (i_p, j_p) with i_p < j_p, strictly ascending in (i, j).  The match rows of pair p are
 * rows[pair_start[p] .. pair_start[p+1] - 1], a row is (k_i, k_j) int32: keypoint k_i of view i_p matches keypoint k_j of
 * view j_p.  M = pair_start[P].  The RANK of row m is m itself.  Within one pair no k_i and no k_j appears twice.
 * owner[g] int32: the id of the point keypoint g observes, or -1 (un-owned).  registered[v].  A pose (R double[9] row-major,
 * t double[3], Xc = R X + t) per registered view, kept on the host.  Points X[id] (three float64) and alive[id] for
 * id < n_points; ids ascend in the order the points are made and are never reused.
 * INVARIANTS, kept by every entry point and relied on by all of them:
 *   (I1) every keypoint of an unregistered view is un-owned;
 *   (I2) no owner is the id of a dead point;
 *   (I3) no two keypoints of one view have the same owner.
 * An OBSERVATION is a keypoint g with owner[g] >= 0: (view of g, owner[g], kp[g]).
 *
 * Limits: V <= AMVS_SFM_MAX_VIEWS, G and M <= AMVS_SFM_MAX_KEYPOINTS / AMVS_SFM_MAX_ROWS, n_points <= AMVS_SFM_MAX_POINTS
 * (= AMVS_BA_MAX_POINTS of amvs_bundle.h).
 *
 * Launch shapes, stated because the tests aim at their edges (no result depends on them: every result is an integer decided
 * by comparisons and minima, or the bits of the triangulation of amvs_twoview.h): every kernel runs workgroups of
 * AMVS_SFM_BLOCK = 256 lanes, one lane per match row or per keypoint or per point.  The rows a call walks are the rows of a
 * list of pairs laid end to end, so a workgroup can hold rows of several pairs.
 *
 * ---- amvs_sfm_begin ------------------------------------------------------------------------------------------------------
 * n_kp[V] int32, kp [G][2] float32, pair_views [P][2] int32, pair_start [P+1] int32, rows [M][2] int32.  Errors: V < 1 or
 * above the limit; an n_v < 0; G, P or M above its limit (P <= V (V - 1) / 2 follows from the order); a pair with i >= j, i < 0
 * or j >= V; pairs not strictly ascending in (i, j); pair_start[0] != 0 or pair_start descending; a row index outside its
 * view's keypoints; a keypoint twice on one side of a pair.  Then the state is replaced whole: no view registered, every
 * keypoint un-owned, no point.  P = 0 and M = 0 are allowed.
 *
 * ---- amvs_sfm_register ---------------------------------------------------------------------------------------------------
 * Marks `view` registered with the pose (R, t) and, for every i < m with mask[i] != 0 (a NULL mask: every i), sets
 * owner[off_view + kp[i]] = pid[i] unless point pid[i] is dead; *n_set = the number of owners set.  Errors: view out of
 * range or already registered; m < 0; among the rows the mask keeps, a kp outside [0, n_view), a pid outside [0, n_points),
 * a kp twice or a pid twice.  m = 0 is how the two initial views enter.
 *
 * ---- amvs_sfm_scores -----------------------------------------------------------------------------------------------------
 * scores_out[v] = -1 for a registered view; for an unregistered view v the number of its keypoints k for which SOME row of
 * SOME pair of v with a registered view r ties k to a keypoint of r that is owned.  Distinct keypoints, not rows.
 *
 * ---- amvs_sfm_correspondences --------------------------------------------------------------------------------------------
 * For an unregistered `view` (a registered or out-of-range view is an error).  A row is a CANDIDATE of keypoint k of `view`
 * when it belongs to a pair of `view` with a registered view r, names k on the side of `view`, and its keypoint of r is
 * owned; the candidate's point is that owner.
 *   Stage A: a(k) = the lowest rank among the candidates of k, p(k) = that candidate's point.  No candidate: k gets nothing.
 *   Stage B: b(p) = the lowest a(k) among the keypoints k with p(k) = p.
 *   k is kept iff a(k) = b(p(k)).  A keypoint that loses gets nothing, even if it had another candidate.
 * Output, in ascending k, *m rows: kp_out = k, pid_out = p(k), X_out = the float64 point p(k) rounded once to float32
 * (three values), x_out = the pixel of k.  The arrays hold n_view rows.  The kept keypoints are distinct and so are their
 * points.
 *
 * ---- amvs_sfm_triangulate ------------------------------------------------------------------------------------------------
 * For a registered `view` (else an error).  Errors also: the checks of amvs_resection.h on K; a threshold that is NaN;
 * n_points + n_view > AMVS_SFM_MAX_POINTS (every new point takes one keypoint of `view`, so this bounds the call).
 * For each OTHER registered view r in ascending order for which the pair (lo, hi) = (min(view, r), max(view, r)) exists,
 * with the pose (R_1, t_1) of lo and (R_2, t_2) of hi:
 *     C_k[i] = -((R_k[0][i]*t_k[0] + R_k[1][i]*t_k[1]) + R_k[2][i]*t_k[2])    (the centre as amvs_match.h forms it)
 *     d = C_2 - C_1;  baseline = sqrt((d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]);  depth_max = baseline * depth_baselines
 *   in float64 on the host, one rounding per operation.  The rows of that pair whose two keypoints are BOTH un-owned, in rank
 *   order, are the candidates; each is triangulated exactly as amvs_twoview_triangulate does it with (K, R_1, t_1, R_2, t_2),
 *   pts1 = the pixel of k_i, pts2 = the pixel of k_j, depth_min, this depth_max, cos_max_parallax, max_reproj: the same
 *   DLT, the same seven comparisons.  Every VALID candidate becomes a point: ids ascend in rank order and continue from
 *   n_points; X[id] = the candidate's X, alive[id] = 1, both keypoints become owned by id.  new_per_view[r] = their number.
 *   The pair of r' > r sees the owners the pair of r made: a keypoint of `view` that made a point with r is no candidate
 *   with r'.  This is the one sequential dependence, carried by stream order.
 * new_per_view[v] = 0 for every other v; *n_new = their sum.
 *
 * ---- amvs_sfm_counts -----------------------------------------------------------------------------------------------------
 * *n_points (dead ones included), *n_alive, *n_obs = the number of observations.
 *
 * ---- amvs_sfm_observations -----------------------------------------------------------------------------------------------
 * Every observation as cam[i] = view, pt[i] = id, uv[i] = pixel, strictly ascending in (id, view) -- the order amvs_bundle.h
 * demands; (I3) makes it strict.  *n = their number; capacity < *n is an error (ask amvs_sfm_counts first).
 *
 * ---- amvs_sfm_points_get / amvs_sfm_points_set / amvs_sfm_pose_set -------------------------------------------------------
 * amvs_sfm_points_get copies X [n_points][3] float64 and alive [n_points] bytes 0 / 1 out (capacity < n_points: an error).
 * amvs_sfm_points_set replaces both (n != n_points: an error); a point may die (alive 1 -> 0) but not come back (0 -> nonzero:
 * an error); every keypoint whose owner died becomes un-owned (I2).  amvs_sfm_pose_set replaces the pose of a registered
 * view (else an error).
 *
 * ---- amvs_sfm_drop -------------------------------------------------------------------------------------------------------
 * (cam[i], pt[i]), i < n, name observations; errors: n < 0, min_obs < 0, a cam outside [0, V), a pt outside [0, n_points).
 * Step 1: every keypoint g of view cam[i] with owner[g] = pt[i] becomes un-owned; *obs_dropped = the number of keypoints
 * un-owned by this step (a pair named twice, or one that is no observation, adds nothing).  Step 2: every live point with
 * fewer than min_obs observations left dies, *points_dropped their number, and its remaining keypoints become un-owned.
 * A later amvs_sfm_triangulate may make new points from those keypoints.  */
#ifndef AMVS_SFM_H
#define AMVS_SFM_H

#include "amvs_bundle.h"

#define AMVS_SFM_BLOCK          256
#define AMVS_SFM_MAX_VIEWS      4096
#define AMVS_SFM_MAX_KEYPOINTS  (1 << 28)
#define AMVS_SFM_MAX_ROWS       (1 << 28)
#define AMVS_SFM_MAX_POINTS     AMVS_BA_MAX_POINTS
/* the defaults of the Python layer (the reference's constants) */
#define AMVS_SFM_MIN_SCORE      12
#define AMVS_SFM_MIN_OBS        2

#ifdef __cplusplus
extern "C" {
#endif

int amvs_sfm_begin(amvs_ctx *ctx, int V, const int32_t *n_kp, const float *kp, int P, const int32_t *pair_views,
                   const int32_t *pair_start, const int32_t *rows);

int amvs_sfm_register(amvs_ctx *ctx, int view, const double R[9], const double t[3], const int32_t *kp, const int32_t *pid,
                      const uint8_t *mask, int m, int64_t *n_set);

int amvs_sfm_scores(amvs_ctx *ctx, int32_t *scores_out);

int amvs_sfm_correspondences(amvs_ctx *ctx, int view, int32_t *kp_out, int32_t *pid_out, float *X_out, float *x_out,
                             int64_t *m);

int amvs_sfm_triangulate(amvs_ctx *ctx, int view, const double K[9], double depth_min, double depth_baselines,
                         double cos_max_parallax, double max_reproj, int64_t *n_new, int32_t *new_per_view);

int amvs_sfm_counts(amvs_ctx *ctx, int64_t *n_points, int64_t *n_alive, int64_t *n_obs);

int amvs_sfm_observations(amvs_ctx *ctx, int32_t *cam, int32_t *pt, float *uv, int64_t capacity, int64_t *n);

int amvs_sfm_points_get(amvs_ctx *ctx, double *X, uint8_t *alive, int64_t capacity);

int amvs_sfm_points_set(amvs_ctx *ctx, const double *X, const uint8_t *alive, int64_t n);

int amvs_sfm_pose_set(amvs_ctx *ctx, int view, const double R[9], const double t[3]);

int amvs_sfm_drop(amvs_ctx *ctx, const int32_t *cam, const int32_t *pt, int n, int min_obs, int64_t *obs_dropped,
                  int64_t *points_dropped);

#ifdef __cplusplus
}
#endif

#endif
