/*
 * amvs.h -- C ABI of the MI355X-native dense-reconstruction backend.
 *
 * The reference (dackey-wav/3d-reconstruction-tool) has no FFI: its dense path is a
 * Python class surface that runs stock torch ops.  These entry points are what a
 * ctypes binding of that surface needs; each cites the reference interface it
 * replaces (file:line under the reference's src/core/).  Plain pointers and
 * sizes only, no C++ or torch types.  Every call returns 0 on success or a
 * negative AMVS_E* code; amvs_last_error() returns a description.
 *
 * Conventions:
 *   - images are float32 gray maps in [0,1], row-major (H,W), one size per context
 *     (mvs_patchmatch.py:183-189 'gray'); all views share one K (camera.py:111-139)
 *   - poses are world->camera, X_c = R X_w + t, R row-major (camera.py:78-103)
 *   - depth/cost/confidence maps are float32 (H,W); normal maps float32 (H,W,3)
 *     interleaved xyz (mvs_patchmatch.py:30-35 DepthNormalMap)
 *   - host buffers are caller-owned and C-contiguous; *_device variants take
 *     device pointers (e.g. torch tensor .data_ptr()) and enqueue on the
 *     context's stream without synchronising.
 */
#ifndef AMVS_H
#define AMVS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMVS_MAX_SRC 6      /* PatchMatch uses 4 (mvs_patchmatch.py:108), plane sweep 6 (dense_stereo.py:109) */

#define AMVS_OK            0
#define AMVS_EINVAL       -1   /* bad argument                                  */
#define AMVS_EHIP         -2   /* HIP runtime error (no device, OOM, launch)    */
#define AMVS_EINDEX       -4   /* index-checked build only: a kernel formed an out-of-range index (amvs_index_check) */
#define AMVS_EUNSUPPORTED -3   /* patch size (even, or above 31) / source count outside [2, 6] / k of the kNN */

typedef struct amvs_ctx amvs_ctx;

/* Arithmetic of the sweep kernels (SURVEY.md section 8b proposed a `mode` parameter).
 *   AMVS_MODE_EXACT  every float32 operation of the reference's torch chain reproduced in order
 *                    (mvs_patchmatch.py:341-411): bit-identical to the exact mode of the tests' CPU checker,
 *                    which matches torch-CPU bit for bit up to the box filter's summation order.
 *   AMVS_MODE_FAST   the same algorithm with the projection precomposed per source, one
 *                    reciprocal per projection and 8-bit code arithmetic:
 *                    bit-identical to the fast mode of the tests' CPU checker, which is pinned against the
 *                    reference's golden vectors within the tolerances DESIGN.md states (cost
 *                    mean 2e-6; >= 98 % of depths within 1e-3 relative end to end).  Needs 8-bit
 *                    images (every view exactly code/255); otherwise the call fails with
 *                    AMVS_EUNSUPPORTED.
 * AMVS_MODE_DEFAULT in amvs_pm_params.mode means "the context's mode" (amvs_set_mode).          */
#define AMVS_MODE_DEFAULT 0
#define AMVS_MODE_EXACT   1
#define AMVS_MODE_FAST    2

/* PatchMatchMVS constructor parameters that reach the device path
 * (mvs_patchmatch.py:43-50) plus the depth range of _estimate_depth_range
 * (:141-165).  log_depth_scale / log_depth_min are (float)(ln dmax - ln dmin)
 * and (float)ln dmin formed in double by the host, as :268-271 does.           */
typedef struct {
    int32_t patch_size;       /* any odd size in 3..31 (mvs_patchmatch.py:45 takes any); 3, 5, ..., 29 run
                                 kernels specialised at compile time, 31 the run-time-k kernels
                                 (csrc/amvs_generic.hip: same results contract, classic schedule, slower)  */
    int32_t num_iterations;
    int32_t num_samples;
    int32_t tile_rows;        /* rows per wave strip; 0 = choose automatically    */
    int32_t views_per_launch; /* views swept together (cache residency); 0 = auto  */
    float   depth_min, depth_max;
    float   log_depth_scale, log_depth_min;
    int32_t mode;             /* AMVS_MODE_DEFAULT / _EXACT / _FAST                    */
    int32_t schedule;         /* AMVS_SCHEDULE_*: 0 = automatic, 1 = view-major strips, 2 = band-major
                                 strips, 3 = split (fast mode only: sampling kernel + window kernel,
                                 pipelined over view groups).  Performance only; results do not
                                 depend on it.                                          */
    int32_t first_iteration;  /* 0: a new sweep (random initialisation, mvs_patchmatch.py:268-284).
                                 k > 0: CONTINUE the sweep of the previous PatchMatch call of this context
                                 -- same batch, sources, patch, samples, seed, depth range -- with
                                 iterations k .. k + num_iterations - 1 of the schedule (:287-308); k must
                                 equal the iterations already run.  A sweep run one iteration per call
                                 returns the maps of one call bit for bit; the outputs of every call are
                                 the maps as they stand (what a per-iteration exchange gathers).   */
    int32_t flags;            /* AMVS_PM_NO_CONFIDENCE: skip the confidence pass (conf output untouched) */
} amvs_pm_params;

#define AMVS_PM_NO_CONFIDENCE 1

#define AMVS_SCHEDULE_AUTO        0
#define AMVS_SCHEDULE_VIEW_MAJOR  1
#define AMVS_SCHEDULE_BAND_MAJOR  2
#define AMVS_SCHEDULE_SPLIT       3
#define AMVS_SCHEDULE_PAIRED      4   /* specialised patch sizes 3 .. 11, up to 4 sources, 8-bit images (the fast mode, and the
                                         exact mode on its packed maps): 2 x 2 strips per workgroup, vertically adjacent bands
                                         walk towards each other and exchange their boundary samples through LDS (K/2 halo
                                         rows per strip instead of K - 1); elsewhere it runs as view-major.
                                         AMVS_SCHEDULE_AUTO chooses it for patches of 5x5 and 7x7 (measured faster there;
                                         9x9 / 11x11: measured equal or slower).  The maps do not depend on the schedule.   */

/* Per-call device timing of the sweep kernels (HIP events on the context
 * stream; used by bench.py for the roofline figure).                            */
typedef struct {
    double  init_ms;          /* initialisation launch                             */
    double  sweep_ms;         /* propagation + refinement launches (pm_step)       */
    double  confidence_ms;    /* confidence launch                                 */
    int64_t sweep_launches;   /* number of pm_step launches inside sweep_ms        */
    int64_t pixel_hypotheses; /* n_ref * H * W * iters * (2 + samples)            */
} amvs_timing;

const char *amvs_version(void);
const char *amvs_last_error(const amvs_ctx *ctx);   /* ctx may be NULL: error of a failed amvs_create */

/* A context owns all device memory for one scene: n_views gray images of H x W
 * with shared intrinsics K (row-major 3x3) and K_inv (the reference forms it with
 * torch.inverse in float32, mvs_patchmatch.py:237-238; the caller passes it).   */
int amvs_create(int device_id, int H, int W, int n_views,
                const float K[9], const float K_inv[9], amvs_ctx **out);
int amvs_destroy(amvs_ctx *ctx);
int amvs_set_stream(amvs_ctx *ctx, void *hip_stream);     /* NULL = context's own stream */
int amvs_sync(amvs_ctx *ctx);

/* Upload one view once per scene (the reference re-uploads every view for every
 * reference view, mvs_patchmatch.py:235-257).  amvs_set_view returns when the host buffer
 * has been consumed.  amvs_set_view_device only ORDERS the copy on the context's stream: the
 * device buffer must be complete before the call (as seen from that stream) and stay unchanged
 * until the stream has passed it (amvs_sync, or any synchronising call).                        */
int amvs_set_view(amvs_ctx *ctx, int view, const float *gray_host,
                  const float R[9], const float t[3]);
int amvs_set_view_device(amvs_ctx *ctx, int view, const void *gray_device,
                         const float R[9], const float t[3]);

/* _prepare_images (mvs_patchmatch.py:167-191, dense_stereo.py:156-176) of one view on the device: the
 * undistorted 8-bit BGR image (src_h x src_w x 3, host; sfm_pipeline.py:114-120) is uploaded as it is
 * (3 B/pixel), resized to the context's H x W with cv.resize's INTER_LINEAR fixed-point arithmetic,
 * converted with cvtColor(BGR2GRAY)'s and divided by 255; the packed 8-bit map the sweeps sample is
 * built from it directly.  scaled_bgr_out (optional, H x W x 3) receives the resized colour image the
 * fusion takes its colours from.  The context must have been created with H = int(src_h * scale),
 * W = int(src_w * scale).  OpenCV is absent from the build container: the arithmetic restates its
 * published source and equals core/imageprep.py bit for bit.  It is pinned to an independent per-pixel
 * restatement (tests/view_upload_restatement.py) and, through it, to a derived bound around float64
 * bilinear interpolation; parity with cv2 itself is still unpinned.
 * STATED TOLERANCE against cv2 (a5): bit equality of the resized colour image and of the gray codes is
 * expected for OpenCV 4.x's generic code path; an OpenCV build that dispatches the 8-bit resize to IPP
 * or another HAL, or OpenCV 3.x's 14-bit gray coefficients, may differ by at most +-1 gray code (1/255)
 * on isolated pixels.  tests/test_host_logic.py::test_image_preparation_equals_cv2_when_present checks
 * the bit equality wherever cv2 is importable; the Python classes use cv2 itself there by default.   */
int amvs_set_view_bgr8(amvs_ctx *ctx, int view, const uint8_t *bgr_host, int src_h, int src_w,
                       const float R[9], const float t[3], uint8_t *scaled_bgr_out);

/* PatchMatchMVS._patchmatch_cuda (mvs_patchmatch.py:225-321) for n_ref reference
 * views in one batch.  src_ids is [n_ref][n_src].  Outputs are [n_ref][H][W]
 * (depth, confidence) and [n_ref][H][W][3] (normal).  The RNG stream of a view is
 * (seed, ref_ids[i]); see amvs_rng_fill.                                          */
int amvs_patchmatch(amvs_ctx *ctx, int n_ref, const int *ref_ids, const int *src_ids,
                    int n_src, const amvs_pm_params *p, uint64_t seed,
                    float *depth_out, float *normal_out, float *conf_out);
int amvs_patchmatch_device(amvs_ctx *ctx, int n_ref, const int *ref_ids, const int *src_ids,
                           int n_src, const amvs_pm_params *p, uint64_t seed,
                           void *depth_dev, void *normal_dev, void *conf_dev);
int amvs_get_timing(const amvs_ctx *ctx, amvs_timing *out);
/* 1 if the sweeps sample the packed 8-bit row-pair maps (every uploaded view is exactly
 * code/255, as cvtColor(...).astype(float32)/255 yields, mvs_patchmatch.py:177), 0 if they
 * sample the float32 maps.  In exact mode both give bit-identical results;
 * amvs_set_sampling(ctx, 1) selects the float32 path unconditionally (A/B tests).           */
int amvs_sampling_mode(const amvs_ctx *ctx);
int amvs_set_sampling(amvs_ctx *ctx, int force_f32);
/* Arithmetic mode of every later sweep call of this context (PatchMatch with
 * amvs_pm_params.mode == AMVS_MODE_DEFAULT, plane sweep, the single-step entry points).
 * A new context is in AMVS_MODE_EXACT.                                                       */
int amvs_set_mode(amvs_ctx *ctx, int mode);
int amvs_get_mode(const amvs_ctx *ctx);
/* Plane-sweep launch shape: rows per wave strip (1..64; more than 32 only for the compiled patch sizes and at most
 * 32 planes per wave -- the strip's running best then uses 8-bit keys) and planes per wave; 0 = automatic.   */
int amvs_set_sweep_tuning(amvs_ctx *ctx, int tile_rows, int planes_per_wave);
/* Launch shape of the PatchMatch sweep steps by iteration (performance only; the maps do not depend
 * on it -- tests/test_hip_fullsize_parity.py): tile_rows / wgs_per_cu are [n_iterations][2] tables,
 * column 0 = the two propagation launches of an iteration (mvs_patchmatch.py:415-457), column 1 = its
 * refinement launches (:459-491); an entry 0 = automatic, iterations beyond the table use its last
 * row, n_iterations = 0 clears it.  wgs_per_cu caps the resident workgroups (4 waves each) per CU.
 * amvs_pm_params.tile_rows > 0 overrides the row entries.                                      */
int amvs_set_step_tuning(amvs_ctx *ctx, int n_iterations, const int32_t *tile_rows, const int32_t *wgs_per_cu);
/* Per-launch device times of the sweep steps of the LAST PatchMatch call (HIP events on the context
 * stream, recorded when enabled; view groups concatenated, schedule order within a group).      */
int amvs_set_step_timing(amvs_ctx *ctx, int enable);
int amvs_get_step_times(amvs_ctx *ctx, float *ms_out, int capacity, int *n_out);
/* Dispatch order of the PatchMatch sweep steps (performance only; the maps do not depend on it --
 * tests/test_hip_launch_order.py).  edge_first: 1 = inside the contiguous range of strips every XCD receives, each
 * view's bands run from the image edge towards its centre -- the part in the upper half downwards, then the part
 * in the lower half upwards -- so that the slow edge bands start first and do not form the tail of the launch;
 * 0 = top to bottom.  group_overlap: the view groups of a batch (views_per_launch) run 0 = one after the other
 * on the context's stream, 1 = dealt to two streams of equal priority, 2 = dealt to a high / low priority pair;
 * the streams fork from the context's stream and join it before the call returns.  -1 = the library's default:
 * two equal streams, and edge-first exactly in the calls whose groups overlap (measured: DESIGN.md section 5).
 * With overlapping groups amvs_get_timing reports, for init_ms, sweep_ms and confidence_ms, the UNION of the
 * groups' intervals (chip time, as on one stream; sweep_launches stays the launch count), and amvs_get_step_times
 * keeps working per stream: a launch's time is then that of a launch sharing the chip with the other stream.   */
int amvs_set_launch_order(amvs_ctx *ctx, int edge_first, int group_overlap);
/* The strips of every wave of a sweep step launch as the kernels decode them (the host copy of the same function,
 * csrc/amvs_strip_order.h; no GPU involved, ctx-free; test infrastructure): out is [n_blocks][4 waves][5] =
 * (job, strip row, strip column, walks up, has a partner band), -1 for a wave without a strip; block b runs on
 * XCD b % 8 and an XCD starts its blocks in ascending order.  Writes as many whole records as `capacity` int32
 * values hold; *n_blocks is the grid of the launch.                                                           */
int amvs_sweep_order(int n_jobs, int tiles_x, int tiles_y, int band_major, int paired, int edge_first,
                     int64_t capacity, int32_t *out, int32_t *n_blocks);
/* (The same kind of view of the launch PLAN -- views per launch, strip rows, schedule, plane chunks; ctx-free, no GPU, test
 * infrastructure -- is declared in amvs_plan.h: this header stays at its ninety-two entry points.)                      */
/* Workgroup timeline of the sweep launches of the LAST PatchMatch call, from a library built with
 * -DAMVS_STEP_TRACE (amvs_version() then ends in "+step-trace"; tools/step_timeline.py): out is
 * [n_launches][blocks_per_launch][4] = (100 MHz wall clock at entry, before exit, XCC id,
 * job << 40 | strip row << 20 | strip column) of wave 0 of every workgroup, zeros beyond a launch's grid;
 * launches in issue order (view groups concatenated).  The shipped build records nothing: *n_launches = 0.
 * Nothing is copied when `capacity` (in values) is too small.                                                  */
int amvs_fetch_step_trace(amvs_ctx *ctx, uint64_t *out, int64_t capacity, int64_t *n_launches, int64_t *blocks_per_launch);
/* Split schedule (AMVS_SCHEDULE_SPLIT): number of view groups pipelined against each other (1..8),
 * rows per strip of the sampling kernel, and bytes of unused LDS per sampling workgroup (caps how
 * many of them a CU holds, which leaves room for the window kernel); 0 = automatic.              */
int amvs_set_split_tuning(amvs_ctx *ctx, int groups, int sample_rows, int sample_lds_bytes);
/* Rows per wave strip the last sweep used (amvs_pm_params.tile_rows, or the automatic choice). */
int amvs_last_tile_rows(const amvs_ctx *ctx);
/* Views per launch group the last PatchMatch call used (amvs_pm_params.views_per_launch or auto). */
int amvs_last_views_per_launch(const amvs_ctx *ctx);

/* DenseStereoReconstructor._plane_sweep_torch (dense_stereo.py:222-316) for one
 * reference view: D depth planes, votes (ncc > thresh) & (z > 0.1) over n_nbr
 * neighbours, first maximal plane wins.                                          */
int amvs_plane_sweep(amvs_ctx *ctx, int ref, const int *nbr_ids, int n_nbr,
                     const float *depths, int D, int patch_size, float thresh,
                     float *depth_out, float *conf_out);
int amvs_plane_sweep_device(amvs_ctx *ctx, int n_ref, const int *ref_ids, const int *nbr_ids,
                            int n_nbr, const float *depths, int D, int patch_size,
                            float thresh, void *depth_dev, void *conf_dev);

/* The reconstruct loop of DenseStereoReconstructor (dense_stereo.py:105-130) as ONE batched sweep
 * whose maps stay in the context: [n_ref][H][W] depth and vote count.  amvs_fetch_sweep_maps copies
 * maps first .. first+count-1 to the host (tests; the multi-rank gather).                        */
int amvs_plane_sweep_batch(amvs_ctx *ctx, int n_ref, const int *ref_ids, const int *nbr_ids, int n_nbr,
                           const float *depths, int D, int patch_size, float thresh);
int amvs_fetch_sweep_maps(amvs_ctx *ctx, int first, int count, float *depth_out, float *conf_out);

/* DenseStereoReconstructor._backproject (dense_stereo.py:407-437) for n_maps reference views at once,
 * in float64 and in the reference's order (view by view, row-major): pixels with confidence >=
 * min_confidence and depth > 0 -> world points + RGB colours, kept on the device (amvs_fetch_cloud).
 * maps_where: 0 = depth / conf are host arrays, 1 = device pointers, 2 = the resident maps of the last
 * amvs_plane_sweep_batch (depth / conf ignored).  per_map_counts (optional, n_maps) receives the points
 * of every view -- the numbers of the reference's progress lines (:129).                           */
int amvs_stereo_backproject(amvs_ctx *ctx, int n_maps, const void *depth, const void *conf, int maps_where,
                            const uint8_t *colors_bgr_host, const double K_inv[9], const double *poses,
                            float min_confidence, int64_t *per_map_counts, int64_t *total);
/* The same for the resident plane-sweep batch and resident colour images (amvs_set_view_bgr8): map j
 * belongs to view view_ids[j]; nothing is uploaded.                                              */
int amvs_stereo_backproject_views(amvs_ctx *ctx, int n_maps, const int *view_ids, const double K_inv[9],
                                  const double *poses, float min_confidence, int64_t *per_map_counts,
                                  int64_t *total);
/* amvs_knn_mean_distance on the context's resident cloud (the result of amvs_stereo_backproject /
 * amvs_fuse_filter): the statistic of _filter_outliers without a host round trip of the points.     */
int amvs_cloud_knn_mean_distance(amvs_ctx *ctx, int k, double *mean_out);
/* DenseStereoReconstructor._voxel_down_sample (dense_stereo.py:475-492) of the resident cloud, after an
 * optional keep mask (one byte per point: the outlier filter's selection, computed by the caller as
 * the reference does with numpy): first point of every voxel in key order.  The cloud is replaced.  */
int amvs_cloud_voxel_downsample(amvs_ctx *ctx, const uint8_t *keep_mask, double voxel_size, int64_t *count);
/* The reference's random sub-sample of clouds above 500 000 points, points[chosen] / colors[chosen]
 * (dense_stereo.py:449-455), on the resident cloud: it is replaced by its rows indices[0 .. m) in that order.  The
 * caller draws the indices (the reference uses the unseeded np.random.choice; the Python class does the same), so
 * the cloud need not travel to the host for the outlier statistic and the voxel grid that follow.                */
int amvs_cloud_take(amvs_ctx *ctx, const int64_t *indices_host, int64_t m);
/* 1 if amvs_knn_mean_distance is compiled for this neighbour count.                                */
int amvs_knn_supported(int k);

/* The k-nearest-neighbour statistic of DenseStereoReconstructor._filter_outliers
 * (dense_stereo.py:456-460: NearestNeighbors(n_neighbors=k).fit(p).kneighbors(p), then
 * np.mean(distances[:, 1:], axis=1)) for n points (host, n x 3 float64) on the device: mean_out[i]
 * = mean distance from point i to its k-1 nearest other points, bit-identical to scikit-learn +
 * numpy (same float64 distance expression, same summation order) wherever scikit-learn uses its
 * KD-tree (k < n / 2; for smaller clouds it switches to a brute-force kernel whose rounding differs
 * by a few ulps).  k in {8, 10, 16, 20, 32}, n >= k.  The threshold mean + 2 sigma and the selection stay on the host (numpy), as there.    */
int amvs_knn_mean_distance(amvs_ctx *ctx, const double *points, int64_t n, int k, double *mean_out);

/* PatchMatchMVS._fuse_depth_maps + _filter_points (mvs_patchmatch.py:536-588) on the device, in
 * float64 and in the reference's order: pixels with confidence >= min_views of n_maps maps
 * ([n_maps][H][W] float32, host or device memory) are back-projected with the float64 K_inv and
 * poses (n_maps x 12 doubles: R row-major then t); colours come from BGR uint8 images
 * ([n_maps][H][W][3], host) and leave as RGB.  With do_filter: 95th-percentile radius cut around
 * the per-axis median, then 1 cm voxel de-duplication keeping the first point of each voxel in
 * key order.  counts[0] = fused points, counts[1] = points kept; amvs_fetch_cloud copies the
 * counts[1] x 3 points (float64) and colours (uint8) to the host.  An empty result (no pixel
 * selected, or the strict cut removed every point, as it does for one point and for two at equal
 * distance) leaves no resident cloud: counts[1] = 0.  Depths, confidences, K_inv and poses must be
 * finite; what a NaN or an infinite depth of a selected pixel does to the median, the percentile
 * and the voxel keys is not defined.                                                            */
int amvs_fuse_filter(amvs_ctx *ctx, int n_maps, const void *depth, const void *conf, int maps_on_device,
                     const uint8_t *colors_bgr_host, const double K_inv[9], const double *poses,
                     float min_views, int do_filter, int64_t counts[2]);
/* Colour image (H x W x 3 uint8 BGR, at the context's size, host) of a view whose gray map was
 * uploaded with amvs_set_view[_device]: kept on the device for the *_views entry points below.
 * (amvs_set_view_bgr8 leaves the image it prepared there by itself; a later amvs_set_view[_device] of
 * the same view drops it.)                                                                        */
int amvs_set_view_colors(amvs_ctx *ctx, int view, const uint8_t *bgr_host);
/* The same fusion + filter for maps resident on the device whose colour images are resident too:
 * map j belongs to view view_ids[j], whose prepared BGR image amvs_set_view_bgr8 left on the device
 * (no host colour array: 3 B/pixel of upload per map saved).  Same results as amvs_fuse_filter.   */
int amvs_fuse_filter_views(amvs_ctx *ctx, int n_maps, const int *view_ids, const void *depth_dev, const void *conf_dev,
                           const double K_inv[9], const double *poses, float min_views, int do_filter,
                           int64_t counts[2]);
int amvs_fetch_cloud(amvs_ctx *ctx, double *points_out, uint8_t *colors_out);

/* ---- oriented normals for the cloud, fitted from the depth maps (csrc/amvs_cloud_normals.hip) ---------------------
 * The reference's cloud has no normals; no counterpart, hence no parity: judged against tests/cloud_normals_restatement.py,
 * written from the text below, bit for bit, and against the analytic normals of a synthetic height field (DESIGN.md
 * section 9).  Per view a least-squares plane is fitted to the INVERSE depths of a small window -- inverse depth is linear
 * in the pixel coordinates on a plane, so the fit is a 3 x 3 system with an integer matrix, solved in closed form: no
 * eigen-decomposition, no iteration, and a normal that faces its camera by construction.  Each cloud point then collects
 * the normals of the views that see it.
 *
 * All arithmetic below is float64 unless stated: one rounding per operation, nothing contracted, in exactly the written
 * order; an integer that meets a float64 is converted first (exactly: every integer here is below 2^53).
 *
 * Pixel validity.  Pixel p of map j is VALID iff, in float32, depth > 0, depth <= FLT_MAX and conf >= min_confidence.
 * NaN fails each comparison.
 *
 * Window fit.  Parameters: radius r in 1 .. 4, jump (float32, positive and finite), min_points (>= 3).  A valid centre
 * pixel (x0, y0) has float32 depth dc.  Walk dy = -r .. r in the outer loop and dx = -r .. r in the inner loop; skip
 * positions outside the image.  A neighbour with depth dn is USED iff it is valid and
 *     fabs((double)dn - (double)dc) <= (double)jump * (double)dc.
 * The centre always uses itself.  Over the used neighbours accumulate
 *     exact integers:            n, sx = sum dx, sy = sum dy, sxx = sum dx*dx, sxy = sum dx*dy, syy = sum dy*dy;
 *     float64, in walk order:    q = 1.0 / (double)dn;  Sq += q;  Sxq += (double)dx * q;  Syq += (double)dy * q.
 * M = [[sxx, sxy, sx], [sxy, syy, sy], [sx, sy, n]].  Its determinant det and its adjugate C (symmetric) are computed in
 * 64-bit integers:
 *     C00 = syy*n - sy*sy    C01 = sx*sy - sxy*n     C02 = sxy*sy - sx*syy
 *     C11 = sxx*n - sx*sx    C12 = sxy*sx - sxx*sy   C22 = sxx*syy - sxy*sxy      det = sxx*C00 + sxy*C01 + sx*C02.
 * The pixel has NO NORMAL if n < min_points or det == 0 (exactly collinear used points).  Otherwise M is a Gram matrix,
 * det > 0, and the numerators of the solution need no division:
 *     a = (C00*Sxq + C01*Syq) + C02*Sq
 *     b = (C01*Sxq + C11*Syq) + C12*Sq
 *     c = (C02*Sxq + C12*Syq) + C22*Sq
 * The pixel has no normal unless c > 0 (the fitted inverse depth at the centre is positive).  Then, with K row-major:
 *     c' = (c - a*(double)x0) - b*(double)y0
 *     m_i = (K[0][i]*a + K[1][i]*b) + K[2][i]*c'            i = 0, 1, 2
 *     len = sqrt((m0*m0 + m1*m1) + m2*m2)
 * The pixel has no normal unless len > 0 and len is finite.  The camera-frame normal is n_cam_i = (-m_i) / len; it faces
 * the camera: n_cam . P < 0 for the pixel's point P.  With world != 0:
 *     n_w[i] = (R[0][i]*n0 + R[1][i]*n1) + R[2][i]*n2
 * where R comes from poses[j] in the fusion's layout (12 doubles: R row-major, then t; X_cam = R X_world + t).  Each
 * component is rounded once to float32 and stored in [n_maps][H][W][3]; a pixel with no normal stores (0, 0, 0).
 *
 * Cloud normals.  Each resident cloud point X (float64) visits the maps in ascending j, using WORLD-frame normal maps:
 *   1. Xc_i = ((R[i][0]*X0 + R[i][1]*X1) + R[i][2]*X2) + t_i.
 *   2. uvw_i = (K[i][0]*Xc0 + K[i][1]*Xc1) + K[i][2]*Xc2.  Skip the map unless uvw2 > 0 and Xc2 > 0.
 *   3. px = floor(uvw0/uvw2 + 0.5), py = floor(uvw1/uvw2 + 0.5).  Skip unless 0 <= px < W and 0 <= py < H, compared in
 *      float64 before any integer conversion (NaN fails).
 *   4. Skip unless the stored normal n (float32, widened) at the pixel has a non-zero component.
 *   5. Skip unless fabs((double)d - Xc2) <= (double)depth_tolerance * (double)d, d the pixel's float32 depth.
 *   6. nc_i = (R[i][0]*n0 + R[i][1]*n1) + R[i][2]*n2 and
 *      w = (-((nc0*Xc0 + nc1*Xc1) + nc2*Xc2)) / sqrt((Xc0*Xc0 + Xc1*Xc1) + Xc2*Xc2).  Skip unless w > 0.
 *   7. s_i = s_i + w*n_i (i = 0, 1, 2) and seen += 1.
 * After the last map, with L = sqrt((s0*s0 + s1*s1) + s2*s2): the point's normal is s_i / L, each rounded to float32, iff
 * seen >= min_views (>= 1) and L > 0; otherwise it is (0, 0, 0).  seen (int32) is kept either way.  The sums live in
 * registers with a fixed map order; there are no atomics on them.
 *
 * Lifetime.  The normals belong to the resident cloud they were computed for: every step that makes a cloud
 * (amvs_fuse_filter*, amvs_stereo_backproject*, amvs_cloud_voxel_downsample, amvs_cloud_take, amvs_cloud_set) drops them,
 * and amvs_fetch_cloud_normals then returns AMVS_EINVAL until amvs_cloud_normals ran again.
 *
 * Errors (AMVS_EINVAL before anything is allocated): radius outside 1 .. 4, min_points < 3, jump or depth_tolerance not
 * positive and finite, min_views < 1, NULL K or poses, more than 2^31 - 1 pixels; amvs_cloud_normals without a resident
 * cloud.
 *
 * amvs_depth_normals: maps_where as in amvs_stereo_backproject (0 host arrays, 1 device pointers, 2 the resident maps of
 * the last amvs_plane_sweep_batch).  The normal maps stay on the device in a grow-only buffer of the context, which the
 * next amvs_depth_normals or amvs_cloud_normals overwrites; *n_normals = pixels with a normal.                          */
int amvs_depth_normals(amvs_ctx *ctx, int n_maps, const void *depth, const void *conf, int maps_where, const double K[9],
                       const double *poses, float min_confidence, int radius, float jump, int min_points, int world,
                       int64_t *n_normals);
/* maps first .. first + count - 1 of the last amvs_depth_normals / amvs_cloud_normals: out is [count][H][W][3] float32. */
int amvs_fetch_depth_normals(amvs_ctx *ctx, int first, int count, float *out);
/* The fit with world = 1, then the cloud normals of the resident cloud.  counts[0] = pixels with a normal, counts[1] =
 * points with a normal.                                                                                                 */
int amvs_cloud_normals(amvs_ctx *ctx, int n_maps, const void *depth, const void *conf, int maps_where, const double K[9],
                       const double *poses, float min_confidence, int radius, float jump, int min_points,
                       float depth_tolerance, int min_views, int64_t counts[2]);
/* normals: [n][3] float32, seen: [n] int32 for the n points of the resident cloud; either may be NULL.                  */
int amvs_fetch_cloud_normals(amvs_ctx *ctx, float *normals, int32_t *seen);
/* Test hook in the spirit of amvs_tsdf_set_volume and amvs_mesh_set: replaces the resident cloud by host arrays (copies
 * only; n x 3 float64 points, n x 3 uint8 RGB colours).  n = 0 leaves no resident cloud.                                */
int amvs_cloud_set(amvs_ctx *ctx, const double *points, const uint8_t *colors_rgb, int64_t n);

/* ---- surface mesh: TSDF fusion + marching tetrahedra (csrc/amvs_mesh.hip) ------------------------
 * The reference stops at the point cloud; no counterpart, hence no parity: judged against synthetic ground
 * truth and a NumPy restatement of the same float32 operations (tests/mesh_restatement.py).
 * The volume is a dense grid of dims[0] x dims[1] x dims[2] points (x fastest); point (i,j,k) sits at
 * origin + (i,j,k) * voxel.  At most AMVS_TSDF_MAX_POINTS points (about 20 B each for the volume, 30 B with the
 * extraction's scans; 512^3 = 2^27 fits); a larger request fails with AMVS_EINVAL before anything is allocated.
 * The volume and the mesh belong to the context (freed by amvs_destroy) and are replaced by the next call.  */
#define AMVS_TSDF_MAX_POINTS (1ll << 27)
/* Truncated signed distance fusion of n_maps depth maps ([n_maps][H][W] float32 at the context's size, host
 * arrays or, with maps_on_device, device pointers, like amvs_fuse_filter) with the float32 intrinsics K and
 * poses (n_maps x 12 float32: R row-major, then t; world -> camera).  Per grid point and map, in map order: project
 * with R X + t then K, skip the map if z <= 0, take the nearest pixel floorf(u + 0.5f), skip it if outside the
 * image, if depth <= 0 or confidence < min_views, or if sdf = depth - z < -trunc; otherwise add min(1, sdf / trunc)
 * with weight 1 and the pixel's colour.  tsdf = mean (weight 0: unobserved).  Colours come from the resident
 * prepared images of views view_ids[j] (amvs_set_view_bgr8 / amvs_set_view_colors) or from colors_bgr_host
 * ([n_maps][H][W][3] uint8 BGR): exactly one of the two is non-NULL.  Synchronises.                      */
int amvs_tsdf_integrate(amvs_ctx *ctx, int n_maps, const void *depth, const void *conf, int maps_on_device,
                        const int *view_ids, const uint8_t *colors_bgr_host, const float K[9], const float *poses,
                        float min_views, const float origin[3], float voxel, const int32_t dims[3], float trunc);
/* Zero level set of the last integrated volume by marching tetrahedra on the Kuhn subdivision (6 tetrahedra per
 * cube around its main diagonal; a tetrahedron with an unobserved corner is skipped): one vertex per lattice edge
 * whose observed ends change sign and that a face uses, ids in point order then edge direction order; faces in cube,
 * tetrahedron and table order, wound so that normals point toward increasing TSDF (free space, toward the cameras). */
int amvs_tsdf_extract(amvs_ctx *ctx, int64_t *n_vertices, int64_t *n_faces);
/* The mesh of the last amvs_tsdf_extract: n_vertices x 3 float32 positions, n_faces x 3 int32 vertex ids,
 * n_vertices x 3 uint8 RGB colours (the two edge ends' mean colours, interpolated).  NULL skips an output.  */
int amvs_fetch_mesh(amvs_ctx *ctx, float *vertices, int32_t *faces, uint8_t *colors_rgb);
/* Test hook: the last integrated volume, dims[2] x dims[1] x dims[0] float32 tsdf and weight (views counted) and
 * x 3 float32 RGB colour sums.  NULL skips an output.                                                      */
int amvs_tsdf_fetch_volume(amvs_ctx *ctx, float *tsdf, float *weight, float *color_sum);
/* Test hook: replace the context's volume by host arrays in the layout amvs_tsdf_fetch_volume returns (tsdf and
 * weight dims[2] x dims[1] x dims[0] float32, color_sum x 3 float32 RGB) on the grid origin / voxel / dims, validated
 * as in amvs_tsdf_integrate (finite origin, positive finite voxel, every dimension >= 2, AMVS_TSDF_MAX_POINTS).  Drops
 * any mesh; amvs_tsdf_extract then behaves as after an integration.  Copies only, no kernel.  A point with weight
 * <= 0 is unobserved and its tsdf and colour sums are never used; at observed points the values must be finite,
 * which is NOT checked.  Synchronises.                                                                      */
int amvs_tsdf_set_volume(amvs_ctx *ctx, const float *tsdf, const float *weight, const float *color_sum,
                         const float origin[3], float voxel, const int32_t dims[3]);
/* Hole filling (csrc/amvs_mesh_fill.hip): grow the signed distance of the context's current volume -- the one
 * amvs_tsdf_integrate or amvs_tsdf_set_volume made -- from its observed grid points into the unobserved ones next to
 * them, `steps` layers deep, so that amvs_tsdf_extract closes the holes the unobserved points left.  Judged against
 * tests/mesh_fill_restatement.py, bit for bit (DESIGN.md section 8 "Hole filling").
 *
 * Every call starts with a generation per grid point, gen (uint8, the layout of weight): 1 where weight > 0, else 0.
 * Then the steps s = 1 .. steps run.  A point is KNOWN AT STEP s if 1 <= gen <= s.  For every point p with
 * gen[p] == 0, decided from the state before the step (all points of a step at once):
 *  1. its in-grid neighbours are visited in the fixed order (i-1), (i+1), (j-1), (j+1), (k-1), (k+1); c is the number
 *     of those known at step s;
 *  2. if c >= min_neighbours:
 *       tsdf[p] = acc / (float)c, where acc starts at +0.0f and takes acc = acc + tsdf[q] over the known neighbours q
 *       in that order;
 *       color_sum[3p + ch] = cacc_ch / (float)c with cacc_ch = cacc_ch + color_sum[3q + ch] / weight[q], from +0.0f,
 *       over the same neighbours in the same order (the mean of their mean colours);
 *       weight[p] = 1.0f and gen[p] = s + 1.
 * All arithmetic is float32, every operation rounded on its own, every division IEEE.  Nothing of a neighbour that is
 * not known is read but its generation: its tsdf and colour sums may be NaN or garbage.  A point once filled never
 * changes, an observed point never changes, and a point with fewer than min_neighbours known neighbours stays
 * unobserved and may be filled by a later step.  Because acc starts at +0.0f, a single neighbour of -0.0f gives +0.0f,
 * which amvs_tsdf_extract takes for outside.
 *
 * All `steps` steps run, without a read-back between them.  filled_per_step[s - 1] (may be NULL) is the number of
 * points step s filled, *n_filled (may be NULL) their sum.  steps outside 1 .. AMVS_FILL_MAX_STEPS or min_neighbours
 * outside 1 .. 6: AMVS_EINVAL before any work; without a current volume: AMVS_EINVAL, as amvs_tsdf_extract.  Drops
 * the mesh and every attribute of it, as amvs_tsdf_set_volume does.  Synchronises.
 *
 * Afterwards the volume is the filled one (amvs_tsdf_fetch_volume: a filled point has weight 1 and its colour sums are
 * its mean colour), and a second call takes the points the first filled for observed.  Hence amvs_tsdf_fill(a) followed
 * by amvs_tsdf_fill(b) leaves the same tsdf, weight and colour sums as one amvs_tsdf_fill(a + b) with the same
 * min_neighbours (the generations differ: those of the second call count from its start).                     */
#define AMVS_FILL_MAX_STEPS 64
int amvs_tsdf_fill(amvs_ctx *ctx, int steps, int min_neighbours, int64_t *filled_per_step /* [steps], may be NULL */,
                   int64_t *n_filled);
/* Test hook: the generations of the last amvs_tsdf_fill on the current volume, dims[2] x dims[1] x dims[0] uint8 (0: still
 * unobserved, 1: observed before the call, s + 1: filled by step s).  AMVS_EINVAL if there was no amvs_tsdf_fill since
 * the volume was made.                                                                                       */
int amvs_tsdf_fetch_fill(amvs_ctx *ctx, uint8_t *gen /* dims[2] x dims[1] x dims[0] */);

/* ---- mesh clean-up: components, Taubin smoothing, vertex normals, decimation (csrc/amvs_mesh_clean.hip) ------
 * No reference counterpart (the reference has no mesh): judged against a NumPy restatement of the definitions below,
 * bit for bit (tests/mesh_clean_restatement.py, DESIGN.md section 8 "Clean-up").  Every call works in place on the
 * context's current mesh -- the one amvs_tsdf_extract made or amvs_mesh_set uploaded -- and synchronises;
 * amvs_fetch_mesh returns the current mesh, cleaned or not.  No float atomics: every float sum runs in a fixed order
 * over the corners c = 3 * face + k that hold the vertex, in ascending c.  Limits: int32 vertex ids and
 * 3 * n_faces <= INT32_MAX.  Labels and normals are attributes of the current mesh: amvs_tsdf_integrate,
 * amvs_tsdf_set_volume, amvs_tsdf_extract, amvs_mesh_set, amvs_mesh_decimate, amvs_mesh_decimate_quadric and
 * amvs_mesh_filter_visible drop both, amvs_mesh_filter_components drops the normals and leaves fresh labels,
 * amvs_mesh_smooth drops the normals and keeps the labels.  The rendered maps and the visibility counts (below) are
 * attributes too: every call of this list drops both, and so do amvs_mesh_filter_components and amvs_mesh_smooth,
 * which replace or move the mesh; amvs_mesh_normals keeps them, and a decimation refused for a vertex outside the
 * cluster grid changes nothing.  amvs_mesh_color_views writes colours only: positions, faces, labels, normals, the
 * maps and the counts all stay current after it; amvs_fetch_render_color changes nothing.  The texture
 * (amvs_mesh_texture, below) is an attribute as well: every call that drops the maps because it replaces or moves the
 * mesh drops it, and so does amvs_mesh_color_views, whose colours it falls back to; amvs_mesh_normals, amvs_mesh_render,
 * amvs_mesh_visibility and every fetch keep it, and amvs_mesh_texture itself leaves everything else current.       */
/* Replace the context's mesh by host arrays: n_vertices x 3 float32 positions, n_faces x 3 int32 vertex ids,
 * n_vertices x 3 uint8 RGB colours (NULL: zeros).  A test hook, and the way to clean a mesh made elsewhere.
 * Validated on the host before anything is copied -- finite positions, ids in [0, n_vertices), no face with a
 * repeated id, the size limits -- else AMVS_EINVAL.  Copies only, no kernel.                                      */
int amvs_mesh_set(amvs_ctx *ctx, const float *vertices, int64_t n_vertices, const int32_t *faces, int64_t n_faces,
                  const uint8_t *colors_rgb);
/* Connected components (vertices joined through faces; the label of a vertex is the smallest vertex id of its
 * component; a vertex no face uses is a component of 0 faces) and their filter: keep the components with at least
 * min_faces faces and, with keep_largest, only the one with the most faces (a tie goes to the smallest label).
 * Faces, then vertices and colours, are compacted in their order and the labels renamed to the new ids.
 * min_faces <= 0 without keep_largest removes nothing and only labels.  n_components counts the components BEFORE
 * the filter; n_vertices and n_faces are the mesh after it.                                                       */
int amvs_mesh_filter_components(amvs_ctx *ctx, int64_t min_faces, int keep_largest, int64_t *n_components,
                                int64_t *n_vertices, int64_t *n_faces);
/* Taubin smoothing: `iterations` (0 .. 1000) times an umbrella step with factor lambda (0 < lambda <= 1), then one with
 * factor mu (finite; skipped if 0) on ping-pong buffers.  A step moves vertex p with deg incident corners to
 * p + factor * (s / (2.0f * (float)deg) - p), s the float32 sum, in corner order, of the face's next vertex and the one
 * after it; every operation is rounded to float32.  deg == 0 copies through, and so does, with fix_boundary, a vertex
 * with an edge that exactly one face has.  Faces and colours are untouched.                                       */
int amvs_mesh_smooth(amvs_ctx *ctx, int iterations, float lambda, float mu, int fix_boundary);
/* Area-weighted vertex normals: the float32 sum, in corner order, of cross(p1 - p0, p2 - p0) of the incident faces,
 * divided by its length sqrtf((x * x + y * y) + z * z); (0, 0, 0) unless the length is > 0.  They point the way the
 * faces do (amvs_tsdf_extract: toward increasing TSDF, the cameras' side).                                        */
int amvs_mesh_normals(amvs_ctx *ctx);
/* Decimation by vertex clustering (csrc/amvs_mesh_decimate.hip; tests/mesh_decimate_restatement.py, DESIGN.md
 * section 8 "Decimation") on a grid of cubic cells of side `cell` (finite, > 0) with a cell corner at `origin` (finite).
 * All float32, every operation rounded on its own, the divisions IEEE.
 * 1. Cell of a vertex: per axis q = (p - origin) / cell, i = floorf(q).  -2^20 <= i < 2^20 must hold on every axis,
 *    otherwise the call fails with AMVS_EINVAL ("mesh_decimate: vertex ... outside the cluster grid") and the mesh,
 *    with its attributes, is exactly as before.  key = (iz + 2^20) << 42 | (iy + 2^20) << 21 | (ix + 2^20).
 * 2. Clusters: the distinct keys in ascending order (x fastest) are the provisional new vertex ids.
 * 3. Representative: position s / (float)count, s the sum of the members' positions in ascending old vertex id
 *    starting from 0; colour per channel (2 * sum + count) / (2 * count) of the integer sum (round half up).
 * 4. Faces: the three ids go through the clustering; a face with a repeated id is dropped.  The others are grouped by
 *    their unordered id triple; a face's winding is its triple rotated so that the smallest id comes first.  net = the
 *    faces of one winding minus those of the other.  net == 0: the whole group goes (two sheets back to back).
 *    Otherwise exactly one face stays, the one with the smallest face index among those of the majority winding, in
 *    its own corner order.  The faces that stay keep their relative order.
 * 5. The clusters no face uses leave the mesh as in amvs_tsdf_extract's last pass.
 * n_vertices and n_faces are the mesh after it; the empty mesh and a mesh of vertices only give 0 / 0.  Drops labels
 * and normals.                                                                                                    */
int amvs_mesh_decimate(amvs_ctx *ctx, const float origin[3], float cell, int64_t *n_vertices, int64_t *n_faces);
/* amvs_mesh_decimate with quadric placement of the clusters' vertices (Lindstrom's out-of-core simplification, stated
 * so that it runs data-parallel and compares bit for bit: tests/mesh_quadric_restatement.py, DESIGN.md section 8
 * "Quadric placement").  Steps 1, 2, 4 and 5 and the colour of step 3 are amvs_mesh_decimate's: faces, colours and
 * counts are identical, only positions differ.  `regularisation` must be finite and in (0, 1], else AMVS_EINVAL; origin
 * and cell as above; the messages are amvs_mesh_decimate's with this call's name.  All float32, every operation rounded
 * on its own (no fused multiply-add), the divisions IEEE.  The position of a cluster, on the OLD faces and positions:
 * a. m = the representative of step 3.
 * b. Face normal n = cross(p1 - p0, p2 - p0) as amvs_mesh_normals forms it (u * v - w * x per component, not normalised).
 * c. Vertex quadric of old vertex v in cluster c: Qv = nine zeros; for every corner of v in ascending corner index
 *    3 * face + k, f the corner's face: e = p[faces[3 f]] - m_c per axis, d = (n.x * e.x + n.y * e.y) + n.z * e.z, and the
 *    nine products nx nx, nx ny, nx nz, ny ny, ny nz, nz nz, d nx, d ny, d nz are added to Qv component by component.
 * d. Cluster quadric S = 0; S += Qv along the cluster's members in ascending old vertex id:
 *    (a00 a01 a02 a11 a12 a22 b0 b1 b2).  It minimises sum (n . y - d)^2 over y = x - m, weighted by area squared.
 * e. Solve, in exactly this order:
 *        t   = (a00 + a11) + a22            lam = regularisation * t
 *        m00 = a00 + lam;  m11 = a11 + lam;  m22 = a22 + lam
 *        l10 = a01 / m00;  l20 = a02 / m00
 *        d1  = m11 - l10 * a01              u12 = a12 - l20 * a01           l21 = u12 / d1
 *        d2  = (m22 - l20 * a02) - l21 * u12
 *        z1  = b1 - l10 * b0                z2  = (b2 - l20 * b0) - l21 * z1
 *        y2  = z2 / d2                      y1  = z1 / d1 - l21 * y2        y0 = (b0 / m00 - l10 * y1) - l20 * y2
 *        cand = m + y
 * f. cand is the position iff t > 0, d1 > 0 and d2 > 0, every component of cand is finite and |y_a| <= 0.5f * cell on
 *    every axis (comparisons false for NaN); otherwise the position is m.
 * The regulariser ties the null space of a flat cluster to the mean (in a plane only the normal component moves), a
 * cluster whose vertices have no faces has t = 0 and keeps the mean, and the half-cell bound keeps a near-singular
 * solve from throwing a vertex away.  n_fallback counts the clusters of step 2 that kept m, those that step 5 removes
 * included.  A vertex outside the cluster grid refuses the call as above, before anything of the mesh or its attributes
 * changes.  Drops labels and normals.                                                                              */
int amvs_mesh_decimate_quadric(amvs_ctx *ctx, const float origin[3], float cell, float regularisation, int64_t *n_vertices,
                               int64_t *n_faces, int64_t *n_fallback);
/* n_vertices x 3 float32 normals (amvs_mesh_normals) and n_vertices int32 labels (amvs_mesh_filter_components) of
 * the current mesh.  NULL skips an output; asking for one that is not current is AMVS_EINVAL.                     */
int amvs_fetch_mesh_attributes(amvs_ctx *ctx, float *normals, int32_t *labels);

/* ---- rendering and visibility: the current mesh seen from given cameras (csrc/amvs_mesh_render.hip) -----------
 * No reference counterpart (the reference has no mesh): judged against a NumPy restatement of the definitions below,
 * bit for bit (tests/mesh_render_restatement.py, DESIGN.md section 8 "Rendering and visibility").  Images are the
 * context's H x W; pixel centres sit at integer coordinates, as in amvs_tsdf_integrate (nearest pixel
 * floorf(u + 0.5f)).  No float atomics and no dependence on execution order: integer coverage, and a 64-bit integer
 * minimum per pixel.  The maps and the counts are attributes of the current mesh (the list above says what drops
 * them); all calls synchronise.                                                                                    */
/* Z-buffer rasteriser of the current mesh into n_views cameras with the float32 intrinsics K and poses (n_views x 12
 * float32: R row-major, then t; world -> camera).  All float32 unless stated, every operation rounded on its own (no
 * fused multiply-add), the divisions IEEE.
 * a. Projection of vertex X, as amvs_tsdf_integrate forms it: zc = ((P[6]*X + P[7]*Y) + P[8]*Z) + P[11], xc and yc
 *    likewise from rows 0 and 1; pu = (K0*xc + K1*yc) + K2*zc, pv and pw likewise from rows 1 and 2 of K; u = pu / pw,
 *    v = pv / pw, iz = 1.0f / zc.  The vertex is usable iff zc > near, |u| <= 2^20 and |v| <= 2^20 (comparisons false
 *    for NaN).  Its fixed-point screen position is sx = (int64)rintf(u * 256.0f), sy likewise (ties to even).
 * b. Face set-up.  A face with a vertex that is not usable is skipped whole (no clipping) and counted in
 *    n_skipped[view].  area = (x1-x0)*(y2-y0) - (y1-y0)*(x2-x0) in int64; area == 0 draws nothing; area < 0: the second
 *    and third corner are exchanged and area negated, and everything below uses the exchanged order (both windings are
 *    drawn, there is no back-face culling).
 * c. Coverage, exact in int64, at the pixels (px, py) of the face's bounding box clamped to the image, P = (256 px,
 *    256 py).  For the edges a -> b = v1 -> v2, v2 -> v0, v0 -> v1: w = (bx-ax)*(Py-ay) - (by-ay)*(Px-ax).  The pixel is
 *    inside iff for all three w > 0, or w == 0 and (dy < 0 or (dy == 0 and dx > 0)) with dx = bx-ax, dy = by-ay: a
 *    pixel centre on an edge two faces share belongs to exactly one of them.  (Coordinates <= 2^28 in magnitude,
 *    differences <= 2^29, products < 2^58.)
 * d. Depth, perspective-correct: b_i = (float)w_i / (float)area (int64 -> float32 rounds to nearest even),
 *    z = 1.0f / ((b0*iz_0 + b1*iz_1) + b2*iz_2); the pixel is dropped unless z is finite and > 0.
 * e. Resolve: key = (uint64)bits(z) << 32 | (uint32)face; the pixel keeps the minimum key over all faces (the nearest
 *    surface, equal depth going to the smallest face index).  depth = the key's upper word as float, or 0.0f where
 *    nothing was drawn; face = the key's lower word, or -1 there.
 * AMVS_EINVAL: no current mesh, n_views < 1, near not finite or <= 0, non-finite K or poses, n_views * H * W >
 * INT32_MAX.  An empty mesh renders empty maps.  n_skipped: NULL or [n_views].                                      */
int amvs_mesh_render(amvs_ctx *ctx, int n_views, const float K[9], const float *poses, float near, int64_t *n_skipped);
/* The maps of views first .. first + count - 1 of the current render: [count][H][W] float32 depth and int32 face ids.
 * NULL skips an output; AMVS_EINVAL without a current render or for views that were not rendered.                   */
int amvs_fetch_render(amvs_ctx *ctx, int first, int count, float *depth_out, int32_t *face_out);
/* Visibility counts against the current render (AMVS_EINVAL without one; depth_tolerance finite and >= 0).  For every
 * vertex and rendered view, with the projection (a) and the render's near: the vertex is seen iff zc > near,
 * fx = floorf(u + 0.5f) and fy = floorf(v + 0.5f) fall inside the image, and the rendered depth d there is 0.0f
 * (nothing drawn) or zc <= d + depth_tolerance.  counts[v] = the number of such views.  n_seen (optional): the
 * vertices with a count > 0.                                                                                       */
int amvs_mesh_visibility(amvs_ctx *ctx, float depth_tolerance, int64_t *n_seen);
/* The n_vertices int32 counts of amvs_mesh_visibility; AMVS_EINVAL unless they are current.                        */
int amvs_fetch_mesh_visibility(amvs_ctx *ctx, int32_t *counts);
/* Keeps the faces whose three vertices each have counts >= min_views (min_views >= 1; the views need not be the same
 * ones), compacted in their order; the vertices no face uses leave as in amvs_tsdf_extract's last pass.  Needs current
 * counts, else AMVS_EINVAL.  n_vertices and n_faces are the mesh after it; a mesh that loses every face gives 0 / 0.
 * Drops the maps, the counts, labels and normals.                                                                  */
int amvs_mesh_filter_visible(amvs_ctx *ctx, int min_views, int64_t *n_vertices, int64_t *n_faces);
/* Performance only, the maps do not depend on it: a face whose clamped bounding box holds more than large_face_pixels
 * pixels is drawn by a workgroup instead of by one lane (0 = automatic; < 0 is AMVS_EINVAL).                        */
int amvs_set_render_tuning(amvs_ctx *ctx, int large_face_pixels);

/* ---- colours from the views, and the render in colour (csrc/amvs_mesh_color.hip) -------------------------------
 * No reference counterpart: judged against a NumPy restatement of the definitions below, bit for bit
 * (tests/mesh_color_restatement.py, DESIGN.md section 8 "Colours from the views").  All float32, every operation
 * rounded on its own (no fused multiply-add), the divisions and sqrtf IEEE.  No float atomics and no dependence on
 * execution order: a vertex walks the views in ascending order.  Both calls synchronise.                            */
/* Recolours the vertices of the current mesh from the images of the rendered views.  Needs the current render and the
 * current normals (amvs_mesh_normals keeps the render and amvs_mesh_render keeps the normals, so either order works).
 * Image j belongs to rendered view j, for as many images as views were rendered, at the context's H x W.  Exactly one
 * of view_ids (resident prepared images, each with a colour image: amvs_set_view_bgr8) and colors_bgr_host
 * ([n][H][W][3] uint8 BGR, staged as amvs_tsdf_integrate's) is non-NULL.  For every vertex X with normal n, the rendered
 * views in ascending order:
 * a. Projection (a) of amvs_mesh_render with the render's K, poses and near, keeping xc, yc, zc, u, v.  The view is
 *    skipped unless zc > near.
 * b. Footprint: x0 = floorf(u), y0 = floorf(v); skipped unless x0 >= 0, x0 < W - 1, y0 >= 0 and y0 < H - 1 (comparisons
 *    false for NaN).  ax = u - x0, ay = v - y0.
 * c. Occlusion and silhouettes: at each of the four pixels (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), d the
 *    rendered depth there, the view is skipped unless d > 0, zc <= d + depth_tolerance and d <= zc + depth_tolerance
 *    hold at all four: an undrawn pixel shows background, a nearer surface occludes the vertex, a farther one means
 *    that the footprint straddles this surface's outline.
 * d. Weight: ncx = (P0*nx + P1*ny) + P2*nz, ncy and ncz likewise from rows 1 and 2 of R;
 *    dot = (ncx*xc + ncy*yc) + ncz*zc; len = sqrtf((xc*xc + yc*yc) + zc*zc); c = (-dot) / len.  Skipped unless
 *    c > min_cos (false for NaN; a zero normal never passes).  w = c.
 * e. Sample, for each of the B, G, R bytes, f the bytes as float with the first index x:
 *    top = f00 + ax*(f10 - f00); bot = f01 + ax*(f11 - f01); val = top + ay*(bot - top).
 * f. Combine.  best_view == 0: S_ch += w*val and Wsum += w, both from 0.0f, in view order.  Otherwise the val of the view
 *    with the largest w is kept; only a strictly greater w replaces it, so a tie goes to the lowest view index.
 * g. Write: q = S_ch / Wsum, or the best view's val; colour = floorf(q + 0.5f) clamped to 0 .. 255, written in the
 *    mesh's RGB order.  A vertex that no view reached keeps its colour.  n_colored (optional) counts the vertices
 *    written.
 * AMVS_EINVAL: no current render or no current normals; both image arguments or neither; a view id out of range or
 * without a resident colour image; depth_tolerance not finite or < 0; min_cos not finite or outside [0, 1).
 * Positions, faces, index, labels, normals, the render and the counts all stay current; a texture (amvs_mesh_texture)
 * does not, since its fall-back colours changed.                                                                    */
int amvs_mesh_color_views(amvs_ctx *ctx, const int *view_ids, const uint8_t *colors_bgr_host, float depth_tolerance,
                          float min_cos, int best_view, int64_t *n_colored);
/* The current render of views first .. first + count - 1 shaded with the current vertex colours: [count][H][W][3] uint8
 * RGB.  A pixel whose face id is -1 gives 0, 0, 0.  Otherwise the face is set up again as in (b) of amvs_mesh_render, the
 * pixel's three edge functions w_i are evaluated as in (c), b_i = (float)w_i / (float)area, z is the pixel's rendered
 * depth, and per channel q = z * ((b0*iz_0*c0 + b1*iz_1*c1) + b2*iz_2*c2) with c_i the corners' colours as float in the
 * exchanged corner order and every product taken left to right; the byte is floorf(q + 0.5f) clamped to 0 .. 255.
 * AMVS_EINVAL without a current render or for views that were not rendered.  Keeps no state: the picture is computed
 * into scratch memory and copied out.                                                                               */
int amvs_fetch_render_color(amvs_ctx *ctx, int first, int count, uint8_t *rgb_out);

/* ---- texture from the views, and the render shaded with it (csrc/amvs_mesh_texture.hip) --------------------------
 * A per-face texture atlas of the current mesh, the carrier of colour for a decimated mesh whose faces span many image
 * pixels.  No reference counterpart: judged against a NumPy restatement of the definitions below, bit for bit
 * (tests/mesh_texture_restatement.py, DESIGN.md section 8 "Texture").  All float32, every operation rounded on its own
 * (no fused multiply-add), the divisions and sqrtf IEEE.  No float atomics and nothing depends on execution order.  All
 * three calls synchronise.
 *
 * Layout.  N = texels is the number of texel intervals along a leg, 1 <= N <= AMVS_TEXTURE_MAX_TEXELS; C = N + 3.  Faces
 * 2c and 2c+1 share cell c.  With cols cells per row, cols is cells_per_row if that is positive; if it is 0, cols is the
 * smallest integer with cols*cols >= n_cells, n_cells = (F+1)/2.  rows = ceil(n_cells / cols).  The origin of cell c is
 * (cx, cy) = ((c % cols)*C, (c / cols)*C).  The atlas is Ht = rows*C by Wt = cols*C texels, uint8 RGB, row 0 on top.
 * Either side above AMVS_TEXTURE_MAX_SIDE is AMVS_EINVAL, before anything is allocated; a mesh with no faces gives a
 * 0 x 0 atlas and success.  The texel set of a face is {(i, j): 0 <= i, j <= N, i + j <= N + 1}; the diagonal
 * i + j = N + 1 is the gutter that a bilinear lookup inside the triangle can touch.  Texel (i, j) of an even face sits
 * at atlas (cx + i, cy + j), of an odd face at (cx + C-1-i, cy + C-1-j).  The two sets of a cell are disjoint, the
 * diagonal between them stays unused.  Corners 0, 1, 2 of a face are its texels (0,0), (N,0), (0,N).  Every atlas texel
 * in no set is 0, 0, 0; this includes the odd half of a last cell that has no second face.
 *
 * UVs.  [F][3][2] float32 per corner, with (X, Y) the corner's atlas texel: u = ((float)X + 0.5f) / (float)Wt,
 * v = 1.0f - ((float)Y + 0.5f) / (float)Ht (OBJ convention, v up).
 *
 * Colour of texel (i, j) of face f with corners p0, p1, p2 in the face's own order:
 * a. b1 = (float)i / (float)N, b2 = (float)j / (float)N, b0 = (1.0f - b1) - b2.  In the gutter b0 is -1/N, so the point
 *    lies just outside the face on its plane.
 * b. The point, per axis: X = (b0*x0 + b1*x1) + b2*x2.
 * c. The normal is the face's: n = cross(p1 - p0, p2 - p0) formed as amvs_mesh_normals forms it
 *    (ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx with a = p1 - p0, b = p2 - p0); l = sqrtf((nx*nx + ny*ny) + nz*nz);
 *    n / l per component if l > 0, else (0, 0, 0).  No current vertex normals are needed.
 * d. Steps a to f of amvs_mesh_color_views, word for word, for this point and this normal: projection with the render's
 *    K, poses and near, the 2 x 2 footprint, the four-depth occlusion and outline test with depth_tolerance, the cosine
 *    against min_cos, the bilinear sample, and blend or best_view.
 * e. If a view was reached, q = S_ch / Wsum or the best view's val, and the byte is floorf(q + 0.5f) clamped to 0 .. 255,
 *    in RGB order.
 * f. Otherwise the texel falls back to the vertex colours: per channel q = (b0*c0 + b1*c1) + b2*c2 of the corners'
 *    current colours as float, rounded and clamped the same way.  The atlas then has no holes.
 * g. n_texels counts the texels in some face's set, F * ((N+1)*(N+2)/2 + N); n_textured counts those of them a view
 *    reached.
 * The image arguments and their rules are amvs_mesh_color_views's.  width, height, n_texels and n_textured are optional.
 * AMVS_EINVAL: no current mesh or render; both image arguments or neither; a view id out of range or without a resident
 * colour image; depth_tolerance not finite or < 0; min_cos not finite or outside [0, 1); texels outside
 * 1 .. AMVS_TEXTURE_MAX_TEXELS; cells_per_row < 0; an atlas side above AMVS_TEXTURE_MAX_SIDE.
 * Needs the current render and nothing else, and leaves everything else current.  What keeps the texture current:
 * amvs_mesh_normals, amvs_mesh_render (the mesh may be rendered again from other cameras and shaded with the atlas),
 * amvs_mesh_visibility and every fetch.  What drops it: every operation that replaces or moves the mesh
 * (amvs_tsdf_integrate, amvs_tsdf_set_volume, amvs_tsdf_extract, amvs_mesh_set, amvs_mesh_filter_components,
 * amvs_mesh_smooth with any iteration count, amvs_mesh_decimate and amvs_mesh_decimate_quadric unless refused,
 * amvs_mesh_filter_visible), and amvs_mesh_color_views, because the fall-back colours changed.                       */
#define AMVS_TEXTURE_MAX_TEXELS 64
#define AMVS_TEXTURE_MAX_SIDE 16384
int amvs_mesh_texture(amvs_ctx *ctx, const int *view_ids, const uint8_t *colors_bgr_host, float depth_tolerance, float min_cos,
                      int best_view, int texels, int cells_per_row, int *width, int *height, int64_t *n_texels,
                      int64_t *n_textured);
/* The current texture: atlas_rgb [Ht][Wt][3] uint8 and uv [F][3][2] float32; NULL skips an output.  AMVS_EINVAL
 * without a current texture.                                                                                        */
int amvs_fetch_mesh_texture(amvs_ctx *ctx, uint8_t *atlas_rgb, float *uv);
/* The current render of views first .. first + count - 1 shaded with the atlas: [count][H][W][3] uint8 RGB.  A pixel
 * whose face id is -1 gives 0, 0, 0.  Otherwise the face is set up again as amvs_fetch_render_color does, the three edge
 * functions w_k are evaluated and b_k = (float)w_k / (float)area; z is the pixel's rendered depth.
 * g_k = z * (b_k * iz_k) in the exchanged corner order; if the set-up exchanged corners 1 and 2, g_1 and g_2 are
 * exchanged back.  x = fminf(fmaxf(g_1 * (float)N, 0.0f), (float)N), and y likewise from g_2.
 * i = min((int)floorf(x), N-1), j likewise; ax = x - (float)i, ay = y - (float)j.  If i + j >= N the pixel is on the
 * hypotenuse within rounding, and j = N - 1 - i, ay = 1.0f.  The four taps (i,j), (i+1,j), (i,j+1), (i+1,j+1) are then in
 * the face's set; per channel, f the taps' bytes as float with the first index i:
 * top = f00 + ax*(f10 - f00); bot = f01 + ax*(f11 - f01); q = top + ay*(bot - top); the byte is floorf(q + 0.5f) clamped
 * to 0 .. 255.  AMVS_EINVAL without a current render or a current texture, or for views that were not rendered.  Keeps
 * no state: the picture is computed into scratch memory and copied out.                                             */
int amvs_fetch_render_texture(amvs_ctx *ctx, int first, int count, uint8_t *rgb_out);

/* ---- extended mode: what the reference's docstring names but does not implement ----------------
 * (mvs_patchmatch.py:1-13 lists plane hypotheses with normals and VIEW propagation; its code ignores
 * the normal in the cost, :323-390, and has no view propagation.)  Slanted-plane homography cost,
 * red-black in-place propagation, view propagation from a snapshot of the other views' maps, random
 * refinement, geometric-consistency confidence.  No reference counterpart, hence no parity: judged
 * against synthetic ground truth (tests/test_extended_mode.py); off unless a caller asks for it.
 * State arrays are caller-owned DEVICE memory covering ALL views of the context: depth / cost
 * [n_views][H][W], normal [n_views][H][W][3]; a call updates the rows of ref_ids and reads the others
 * (view propagation, consistency) -- on several GPUs the caller all-gathers the rows between
 * iterations.  conf_out of amvs_xpm_consistency is [n_ref][H][W] in ref_ids order.                */
typedef struct {
    int32_t patch_size;       /* odd window side, 3..31                                  */
    int32_t window_stride;    /* sample every window_stride-th pixel of the window       */
    int32_t num_refine;       /* perturbed hypotheses per pixel and half sweep (0..6)    */
    int32_t view_propagation; /* 0 / 1                                                   */
    float   depth_min, depth_max;
    float   log_depth_scale, log_depth_min;     /* as amvs_pm_params                     */
    float   consistency_px, consistency_rel;    /* forward-backward thresholds           */
} amvs_xpm_params;
int amvs_xpm_init(amvs_ctx *ctx, int n_ref, const int *ref_ids, const int *src_ids, int n_src,
                  const amvs_xpm_params *p, uint64_t seed, void *depth_all, void *normal_all, void *cost_all);
/* One iteration = view candidates, red half sweep, black half sweep.  snapshot_depth / snapshot_normal
 * (device, same layout as depth_all / normal_all; NULL = the live maps): what the view candidates
 * read.  A caller that splits the views of one iteration over several calls (jobs with different
 * source counts) passes a copy taken before the first call, so that no call sees maps another call
 * of the same iteration already wrote -- the result then does not depend on the grouping.          */
int amvs_xpm_iterate(amvs_ctx *ctx, int n_ref, const int *ref_ids, const int *src_ids, int n_src,
                     const amvs_xpm_params *p, int iteration, uint64_t seed,
                     void *depth_all, void *normal_all, void *cost_all,
                     const void *snapshot_depth, const void *snapshot_normal);
/* The phases of an iteration one at a time (tests/test_extended_oracle.py compares each with the CPU
 * restatement oracle/xpm_oracle.py), plus a test hook: AMVS_XPM_PHASE_EVAL writes the cost of every
 * pixel's CURRENT plane to cost_out ([n_ref][H][W], device) and changes nothing.                     */
#define AMVS_XPM_PHASE_CANDIDATES 0
#define AMVS_XPM_PHASE_RED        1
#define AMVS_XPM_PHASE_BLACK      2
#define AMVS_XPM_PHASE_EVAL       3
int amvs_xpm_step(amvs_ctx *ctx, int n_ref, const int *ref_ids, const int *src_ids, int n_src,
                  const amvs_xpm_params *p, int iteration, uint64_t seed, int phase,
                  void *depth_all, void *normal_all, void *cost_all,
                  const void *snapshot_depth, const void *snapshot_normal, void *cost_out);
/* The view-propagation candidates of the last AMVS_XPM_PHASE_CANDIDATES call: depth [n_ref][H][W]
 * (0 = none), normal [n_ref][H][W][3], host arrays (test hook).                                       */
int amvs_xpm_fetch_candidates(amvs_ctx *ctx, int n_ref, float *cand_depth_out, float *cand_normal_out);
int amvs_xpm_consistency(amvs_ctx *ctx, int n_ref, const int *ref_ids, const int *src_ids, int n_src,
                         const amvs_xpm_params *p, void *depth_all, void *normal_all, void *cost_all,
                         void *conf_out);

/* ---- single-step entry points (parity tests drive these one reference call at a time) ---- */

/* _compute_patch_cost (mvs_patchmatch.py:323-390): depth map in, averaged cost out. */
int amvs_eval_cost(amvs_ctx *ctx, int ref, const int *src_ids, int n_src, int patch_size,
                   const float *depth_in, float *cost_out);
/* The stage before the box filter (mvs_patchmatch.py:341-377): every pixel projected into every
 * source at its own depth and sampled bilinearly.  sampled_out is [n_src][H][W] -- gray in exact
 * mode, 8-bit code units (gray * 255) in fast mode --, valid_out [H][W] holds bit s = source s
 * valid.  bounds: 0 = patch bounds (:362-363), 1 = image bounds (:516-517), 2 = depth test only
 * (dense_stereo.py:280,303).                                                                    */
int amvs_sample_sources(amvs_ctx *ctx, int ref, const int *src_ids, int n_src, int patch_size, int bounds,
                        const float *depth_in, float *sampled_out, uint8_t *valid_out);
/* _compute_confidence (mvs_patchmatch.py:493-534). */
int amvs_confidence(amvs_ctx *ctx, int ref, const int *src_ids, int n_src, int patch_size,
                    const float *depth_in, float *conf_out);
/* One pull step of _spatial_propagation (mvs_patchmatch.py:427-455): candidate at
 * (y,x) is the state at (y+oy, x+ox); state arrays are updated in place.          */
int amvs_propagate_step(amvs_ctx *ctx, int ref, const int *src_ids, int n_src, int patch_size,
                        float *depth, float *normal, float *cost,
                        int oy, int ox, float depth_min);
/* One sample of _random_refinement (mvs_patchmatch.py:470-489) with draw `draw`
 * of stream (seed, stream_view).                                                  */
int amvs_refine_step(amvs_ctx *ctx, int ref, const int *src_ids, int n_src, int patch_size,
                     float *depth, float *normal, float *cost,
                     uint64_t seed, uint32_t stream_view, uint32_t draw,
                     float depth_range, float normal_range,
                     float depth_min, float depth_max);
/* Initialisation (mvs_patchmatch.py:268-284) from draw 0 of stream (seed, stream_view). */
int amvs_init_state(amvs_ctx *ctx, uint64_t seed, uint32_t stream_view,
                    float log_depth_scale, float log_depth_min,
                    float *depth, float *normal, float *cost);
/* mean / variance maps of view `view` under a k x k zero-padded box filter
 * (mvs_patchmatch.py:403,406).                                                    */
int amvs_box_stats(amvs_ctx *ctx, int view, int patch_size, float *mean_out, float *var_out);
/* The counter-hash RNG that stands in for torch.rand / torch.randn
 * (mvs_patchmatch.py:271,279,280,471,475): per element one uniform (u_out, n
 * floats) and three normals (n_out, n x 3).  Either output may be NULL.           */
int amvs_rng_fill(amvs_ctx *ctx, uint64_t seed, uint32_t stream_view, uint32_t draw,
                  int64_t n, float *u_out, float *n_out);

/* ---- native exchange between ranks (amvs_comm_init / amvs_allgather_maps) ----
 * For a consumer of this ABI WITHOUT torch.distributed (the Python classes use torch's process group,
 * which issues the same RCCL calls).  One process per GPU; the reference has no counterpart (its loop
 * over views is serial, mvs_patchmatch.py:104-123).  RCCL is resolved at run time (dlopen of
 * librccl.so.1 -- the copy already in the process when a PyTorch-ROCm wheel loaded one, the system copy
 * otherwise), so libamvs.so carries no link-time dependency on it.
 *   amvs_comm_unique_id   rank 0 creates the 128-byte id; the caller sends it to the other ranks
 *                         (any transport: a file, MPI, a socket) -- ncclGetUniqueId
 *   amvs_comm_init        every rank, with the same id: ncclCommInitRank on the context's device
 *   amvs_allgather_maps   all-gather of `floats_per_rank` float32 from local_dev into full_dev
 *                         ([world][floats_per_rank], rank order), device pointers, enqueued on the
 *                         context's stream behind the sweep that produced local_dev -- ncclAllGather;
 *                         full_dev + rank * floats_per_rank may be local_dev itself (in place)
 *   amvs_comm_destroy     ncclCommDestroy (also done by amvs_destroy)                                 */
#define AMVS_COMM_ID_BYTES 128
int amvs_comm_unique_id(uint8_t id_out[AMVS_COMM_ID_BYTES]);
int amvs_comm_init(amvs_ctx *ctx, int rank, int world, const uint8_t id[AMVS_COMM_ID_BYTES]);
int amvs_allgather_maps(amvs_ctx *ctx, const void *local_dev, void *full_dev, int64_t floats_per_rank);
int amvs_comm_destroy(amvs_ctx *ctx);

/* utils.save_ply (utils.py:8-37): ASCII PLY with "%.6f %.6f %.6f %d %d %d" per vertex; the same
 * bytes as the reference writes, through one buffered native writer (no GPU involved; ctx-free).
 * points: n x 3 float64, colors: n x 3 int64 (the reference casts with .astype(int)).          */
int amvs_write_ply(const char *path, const double *points, const int64_t *colors, int64_t n);
/* The same with normals (n x 3 float32, not NULL; no reference counterpart): the header gains `property float nx`, `ny`,
 * `nz` between z and red, and each line is "x y z nx ny nz r g b" with the normals as "%.6f" of the widened float32.   */
int amvs_write_ply_normals(const char *path, const double *points, const float *normals, const int64_t *colors, int64_t n);

/* Index-checked build (csrc/amvs_check.h, -DAMVS_CHECK_INDICES; amvs_version() then ends in "+index-checks"): the
 * GPU-side substitute for an address sanitizer, which this pool does not offer for device code.  Every
 * data-dependent global index of the sweep, plane-sweep, extended, fusion, neighbour-search and mesh kernels is compared
 * with its buffer's extent before the access; a violation is counted, the first is recorded and the access
 * redirected to a safe index.  report[0] = violations since the last reset, report[1] = translation unit << 32 |
 * source line of the first, report[2] = its index, report[3] = the extent; amvs_sync, amvs_patchmatch,
 * amvs_plane_sweep, amvs_fetch_cloud and the amvs_tsdf_* / amvs_mesh_* / amvs_fetch_mesh calls return AMVS_EINDEX while a
 * violation is on record.  The shipped build
 * compiles the checks away: it reports zeros.  (The reference has no counterpart; test infrastructure of the
 * device code.)                                                                                             */
int amvs_index_check(uint64_t report[4], int reset);

/* Self test: the kernels replace the IEEE divide / sqrt expansions by v_rcp_f32 / v_rsq_f32 with
 * FMA corrections (plus an IEEE path for out-of-range operands).  Compares both against
 * 1.0f/x and sqrtf(x) on ALL 2^32 float bit patterns; mismatches[0] = reciprocal,
 * mismatches[1] = square root (both must be 0 for bit-exact parity with the tests' CPU checker).      */
int amvs_selftest_lean_math(amvs_ctx *ctx, uint64_t mismatches[2]);

#ifdef __cplusplus
}
#endif
#endif /* AMVS_H */
