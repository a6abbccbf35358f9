// amvs_kernels.h -- host-visible launch interface of the gfx950 kernels.
#pragma once
#include "amvs_strip_order.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#define AMVS_KMAX_SRC 6
#define AMVS_SWEEP_MAX_TH 32          // rows per strip with 16-bit running-best keys ...
#define AMVS_SWEEP_MAX_CHUNK 4096     // ... of up to 4096 planes per wave (12-bit plane index in its LDS keys)
#define AMVS_SWEEP_MAX_TH8 64         // rows per strip with 8-bit keys (SweepArgs::key8: the same 4 KB of LDS) ...
#define AMVS_SWEEP_MAX_CHUNK8 32      // ... of up to 32 planes per wave (5-bit plane index, 3-bit vote count)
#define AMVS_MAX_PATCH 31             // largest (odd) patch size: the run-time-k kernels' rings fit 64 KB of LDS up to here

namespace amvs {

class ScratchCache;                   // amvs_buffer.h
template <class T> class DeviceBuffer;

// One source view of a job: everything its sampling needs in one 64-byte record (a single
// s_load_dwordx16 and one wait per source instead of three load / wait rounds).
struct alignas(64) SrcEntry {
    float R[9], t[3];
    unsigned long long pairs;   // first element of the zero-bordered packed map
    unsigned long long gray;    // float32 gray map
};

// Fast (tolerance) mode: the chain back-project -> world -> source camera -> pixel of
// mvs_patchmatch.py:341-360 precomposed per (reference, source) pair in double on the host:
//   [u z, v z, z]^T = d * (M [x, y, 1]^T) + b,  M = K R_s R_ref^T K^-1,  b = K (t_s - R_s R_ref^T t_ref)
struct alignas(64) FastSrc {
    float M[9], b[3];
    unsigned long long pairs;   // first element of the zero-bordered packed map
    unsigned long long pad_;
};

// One reference view of a batch: its pose, its source views and where its state lives.
struct alignas(64) Job {
    float K[9], Kinv[9];    // shared intrinsics, copied per job so that the kernels fetch them with
                            // the same in-loop scalar loads as the poses
    float Rref[9], tref[3];
    int ref_img;
    uint32_t stream_view;   // RNG stream id (the reference view's index)
    int slot;               // state / output slot inside the batch buffers
    int n_src;
    unsigned long long ref_pairs;   // image pixel (0,0) of the reference view's packed map
    unsigned long long ref_stats;   // fast mode: float2 (mean1, var1) map of the reference view
    SrcEntry src[AMVS_KMAX_SRC];
    FastSrc fsrc[AMVS_KMAX_SRC];    // fast mode
};

enum Mode { MODE_EVAL = 0, MODE_PROP = 1, MODE_REFINE = 2, MODE_CONF = 3 };

// where the images live (common head of StepArgs and SweepArgs)
struct StepArgsBase {
    long long img_stride;                    // floats between consecutive images
    const float *images;                     // float32 gray maps [n_views][img_stride]
    const uint16_t *pairs;                   // packed 8-bit row-pair maps [n_views][pair_stride], or NULL
    long long pair_stride;
    int fast;                                // 1: fast (tolerance) arithmetic; needs `pairs`
};

struct StepArgs : StepArgsBase {
    int H, W, TH, tiles_x, tiles_y, n_jobs;
    // Strip order.  0 (view-major): strips run view by view, row by row -- an XCD's resident
    // waves cover ~19 consecutive strip rows of one view.  1 (band-major): strips run band by band
    // (a band = one strip row of EVERY view of the launch), so an XCD's resident waves walk the same
    // rows of all views together; the views' source images are each other, so the XCD's L2 holds
    // one thin row front of every image instead of a tall band of a few.
    int band_major;
    // State [slot][H*W] (normals [slot][H*W*3]).  Depth is ping-ponged on every step (halo pixels
    // of other strips read the pre-step map).  Cost is only ever touched at a lane's own pixel and
    // updated in place.  Normals never enter the cost (mvs_patchmatch.py:323-390 ignores them), so
    // they are moved only where a candidate WINS: they live in two buffers nbuf[0], nbuf[1], and the
    // SIGN BIT of a pixel's depth in the state maps names the buffer that holds its current normal
    // (depths are >= depth_min > 0, so the bit is free; it travels with the depth ping-pong at no
    // cost).  A propagation winner p (candidate = the NEIGHBOUR q's pre-step normal, :452-455) reads
    // nbuf[sign d_in[q]][q], writes the buffer p does not currently use and stores its new depth with
    // the flipped sign; a refinement winner updates its current buffer in place; losers touch no
    // normal.  No pixel reads a location another pixel writes in the same launch.  `depth_mask` strips
    // the tag from every depth read: 0x7FFFFFFF for state maps, 0xFFFFFFFF for caller-supplied maps
    // (amvs_eval_cost / amvs_confidence).  launch_resolve_state turns tagged state into plain maps.
    const float *d_in;
    float *d_out;
    float *cost;
    float *nbuf[2];
    unsigned depth_mask;
    float *aux;                              // MODE_EVAL: cost map, MODE_CONF: confidence
    const Job *jobs;
    int mode, oy, ox;
    float depth_min, depth_max, depth_range, normal_range;
    unsigned long long seed;
    unsigned draw;
    // Split schedule (fast mode): sample maps [slot][n_src][H*W] written by launch_sample_fast and
    // read by launch_step when `presampled`; the sampling kernel's own strips (64 columns, no halo).
    float *samples;
    int presampled;
    int half;                                // patch_size / 2
    int s_TH, s_tiles_x, s_tiles_y;
    int s_lds;                               // unused dynamic LDS per sampling workgroup (occupancy cap); 0 = default
    // Resident workgroups per CU of this sweep launch (enforced through unused dynamic LDS: 160 KiB /
    // wg_cap per workgroup); 0 = the default of AMVS_DEFAULT_WGS_PER_CU.  Performance only.
    int wg_cap;
    // Paired-band schedule of the fast step (pm_step_fast_kernel<..., PAIR = true>): 2 x 2 strips per
    // workgroup, vertically adjacent bands exchange their boundary samples through LDS
    int paired;
    // Dispatch order inside every XCD's range: 1 = each view's bands from the image edge towards its centre
    // (amvs_strip_order.h), 0 = top to bottom.  Performance only.
    int edge_first;
    // Fast step, compiled patch sizes up to 15 x 15 (step_fast_regs_supported).  ref_in_kernel: the reference window's
    // (mean1, var1) are formed in the kernel from the codes it carries; Job::ref_stats is not read (and may be 0).
    // depth_hist: the centre pixel's / the propagation neighbour's depth is kept from the load that sampled it.
    // Performance only: the maps are the same bit for bit.
    int ref_in_kernel, depth_hist;
    // -DAMVS_STEP_TRACE builds: [grid][4] workgroup timeline of this launch (amvs_kernel_common.h), or NULL
    unsigned long long *trace;
};

#define AMVS_DEFAULT_WGS_PER_CU 4

struct SweepArgs : StepArgsBase {
    int H, W, TH, tiles_x, tiles_y, n_jobs, D;
    int n_chunks, chunk;                     // planes are split into n_chunks groups of `chunk`
    int key8;                                // 1: 8-bit running-best keys (chunk <= 32): strips of up to 64 rows in the same LDS
    unsigned *keys;                          // [slot][H*W] running best, merged with atomicMax
    const float *depths;                     // [D] device
    float thresh;
    float *depth_out, *conf_out;             // [slot][H*W]
    const Job *jobs;
    // exact arithmetic, compiled patch sizes: mean1 / var1 maps of every view for this patch size
    // ([n_views][img_stride], launch_box_stats) -- plane-invariant, so the sweep loads them instead of
    // re-forming the reference's window sums for every plane
    const float *ref_mean, *ref_var;
};

bool patch_supported(int K);          // any odd patch size in 3 .. AMVS_MAX_PATCH
bool patch_compiled(int K);           // ... with kernels specialised at compile time (CompiledPatches, amvs_dispatch.h);
                                      // the others run the run-time-k kernels of amvs_generic.hip
// amvs_generic.hip: sweep step / plane sweep / statistics with the patch size as a launch argument (both
// arithmetic modes, classic schedule); launch_step / launch_sweep / launch_box_stats / launch_fast_stats forward
// to these for patch sizes that are not compiled in
hipError_t launch_step_generic(int K, int S, const StepArgs &a, hipStream_t st);
hipError_t launch_sweep_generic(int K, int S, const SweepArgs &a, hipStream_t st);
hipError_t launch_box_stats_generic(int K, const float *images, long long img_stride, int H, int W, int first_img, int n_img,
                                    float *mean_out, float *var_out, hipStream_t st);
hipError_t launch_fast_stats_generic(int K, const uint16_t *pairs_view, int H, int W, float2 *out, hipStream_t st);
int step_generic_waves_per_cu(int K, int S);
bool knn_supported(int k);
// scratch from the context's `cache`; synchronises `st`
hipError_t knn_mean_distance(const double *points, long long n, int k, double *mean_out, ScratchCache &cache, hipStream_t st,
                             bool points_on_device = false);
int strip_out_width(int K);
int step_waves_per_cu(int K, int S, bool u8, int wg_cap = 0);      // resident waves per CU under the cap (0 = default)
hipError_t launch_step(int K, int S, const StepArgs &a, hipStream_t st);
// launch geometry and strip decode of the step kernels on the host (amvs_strip_order.h; amvs_sweep_order)
int step_wg_waves(bool paired);
int step_grid_blocks(int n_jobs, int tiles_x, int tiles_y, bool paired);
bool strip_decode_host(int n_jobs, int tiles_x, int tiles_y, int band_major, bool paired, int edge_first, int bid, int nblk,
                       int wv, StripPos &p);
hipError_t launch_sweep(int K, int S, const SweepArgs &a, hipStream_t st);
// amvs_kernels_fast.hip: the same steps in the fast arithmetic (a.fast != 0; launch_step /
// launch_sweep forward to these)
hipError_t launch_step_fast(int K, int S, const StepArgs &a, hipStream_t st);
hipError_t launch_sample_fast(int S, const StepArgs &a, hipStream_t st);      // split schedule, first half
hipError_t launch_sweep_fast(int K, int S, const SweepArgs &a, hipStream_t st);
int step_fast_waves_per_cu(int K, int S, int wg_cap = 0);
// the paired-band schedule is compiled for this patch / source count: fast arithmetic, exact arithmetic (packed 8-bit maps)
bool step_fast_pair_supported(int K, int S);
bool step_pair_supported(int K, int S);
// StepArgs::ref_in_kernel / depth_hist are compiled for this patch size (the largest such: step_fast_regs_max_patch)
bool step_fast_regs_supported(int K);
int step_fast_regs_max_patch();
// amvs_kernels_fast_regs.hip: the launches of launch_step_fast with one of the two set (it forwards them)
hipError_t launch_step_fast_regs(int K, int S, const StepArgs &a, hipStream_t st);
// test hook: per-source samples [S][H*W] and validity bits [H*W] of job 0 at the depth map a.d_in;
// a.TH carries k/2, a.mode selects the bounds (MODE_EVAL patch bounds, MODE_CONF image bounds,
// MODE_EVAL + 100 depth test only = plane sweep)
hipError_t launch_sample_dump(int S, const StepArgs &a, float *out, unsigned char *valid_out, hipStream_t st);
hipError_t launch_sample_dump_fast(int S, const StepArgs &a, float *out, unsigned char *valid_out, hipStream_t st);
// (mean1, var1) of one view under the k x k zero-padded box filter from its packed 8-bit map:
// exact integer window sums, statistics in gray units (float2 per pixel)
hipError_t launch_fast_stats(int K, const uint16_t *pairs_view, int H, int W, float2 *out, hipStream_t st);
// the double-precision composition of FastSrc::M / b
void fast_compose(const float K[9], const float Rr[9], const float tr[3], const float Rs[9], const float ts[3],
                  float M[9], float b[3]);
hipError_t launch_sweep_finish(const SweepArgs &a, hipStream_t st);
hipError_t launch_box_stats(int K, const float *images, long long img_stride, int H, int W,
                            int first_img, int n_img, float *mean_out, float *var_out,
                            hipStream_t st);
long long pair_map_elems(int H, int W);      // ushorts of one zero-bordered packed map
long long pair_map_origin(int W);            // texel offset of image pixel (0,0) inside it
int pair_map_texel_bytes();                  // 2 (row-pair layout) or 1 (byte layout)
hipError_t launch_pack_pairs(const float *img, int H, int W, uint16_t *pairs, int *inexact,
                             hipStream_t st);
hipError_t launch_init(const Job *jobs, int n_jobs, long long HW, unsigned long long seed,
                       float log_scale, float log_min, float *depth, float *normal, float *cost,
                       hipStream_t st);
// Tagged state (StepArgs::nbuf) -> plain maps for the slots of `jobs`: depth_out[p] = |depth[p]|,
// normal_out[p] = nbuf[sign depth[p]][p].  Outputs are indexed by (slot - out_slot0); with depth_out ==
// NULL the state is resolved in place (depth untagged, current normals gathered into nbuf0).
hipError_t launch_resolve_state(const Job *jobs, int n_jobs, long long HW, float *depth, float *nbuf0, const float *nbuf1,
                                float *depth_out, float *normal_out, long long out_slot0, hipStream_t st);
hipError_t launch_lean_math_check(unsigned long long *mismatch, hipStream_t st);
hipError_t launch_rng_fill(unsigned long long seed, unsigned view, unsigned draw, long long n,
                           float *u_out, float *n_out, hipStream_t st);

// amvs_fusion.hip: fusion (+ filter) of per-view maps into a cloud.  Every post-step of amvs_fusion.hip takes its
// scratch from the context's `cache`, writes its cloud into EMPTY buffers pts_out / rgb_out (exactly the points found)
// and synchronises `st`.
hipError_t fuse_filter(const float *depth, const float *conf, const unsigned char *bgr, int n_maps, int H, int W,
                       const double *Kinv_h, const double *poses_h, float min_views, bool do_filter, ScratchCache &cache,
                       DeviceBuffer<double> &pts_out, DeviceBuffer<unsigned char> &rgb_out, long long counts[2], hipStream_t st);

// amvs_extended.hip: the extended PatchMatch mode (slanted-plane cost, red-black schedule, view
// propagation, geometric consistency); no reference counterpart
struct XArgs {
    int H, W, n_jobs, n_src;
    const Job *jobs;
    const float *images;          // float32 gray maps [n_views][img_stride]
    long long img_stride;
    const uint16_t *pairs;        // packed 8-bit row-pair maps [n_views][pair_stride] (NULL: sample `images`)
    long long pair_stride;
    float *depth, *normal, *cost; // state of ALL views: [n_views][H*W] (normal x3), indexed by Job::ref_img
    const float *snap_depth, *snap_normal;   // what the view candidates read: a snapshot of depth / normal taken
                                             // before any call of the iteration wrote a map (or the live maps)
    float *cand_d, *cand_n;       // view-propagation candidates [n_jobs][H*W] (x3), indexed by Job::slot
    const int *src_view;          // [n_jobs][n_src] view ids of the sources
    int patch, stride;            // window side, sample stride inside it
    float depth_min, depth_max;
    float rel_range, nrm_range;   // refinement ranges of this iteration
    int n_refine, with_random, colour, with_view_cand;
    unsigned long long seed;
    unsigned draw;
};

hipError_t launch_xpm_init(const XArgs &a, float log_scale, float log_min, hipStream_t st);
hipError_t launch_xpm_view_candidates(const XArgs &a, hipStream_t st);
hipError_t launch_xpm_sweep(const XArgs &a, hipStream_t st);
hipError_t launch_xpm_eval(const XArgs &a, float *cost_out, hipStream_t st);   // test hook: cost of every pixel's current plane
hipError_t launch_xpm_consistency(const XArgs &a, float *conf_out, float max_px, float max_rel, hipStream_t st);

// amvs_prep.hip: cv.resize (INTER_LINEAR, 8-bit BGR) + cvtColor(BGR2GRAY) / 255 of one view; the
// weight tables are built on the host (amvs_capi.hip, OpenCV's float32 arithmetic)
hipError_t launch_prep_bgr8(const unsigned char *src, int sh, int sw, int dh, int dw, const int *xofs,
                            const short *ialpha, const int *yofs, const short *ibeta, unsigned char *scaled,
                            float *gray, hipStream_t st);

// amvs_undistort.hip: lens undistortion of one [h][w][3] image at its own resolution (include/amvs_lens.h): K, 9 doubles
// row-major, and dist8 = k1, k2, p1, p2, k3, k4, k5, k6 on the host, validated by the caller; src and dst on the device,
// apart; n_outside NULL or a device counter the OUTSIDE pixels are added to.  Does not synchronise.
hipError_t launch_undistort_bgr8(const unsigned char *src, int h, int w, const double K[9], const double dist8[8],
                                 unsigned char *dst, unsigned long long *n_outside, hipStream_t st);

// amvs_fusion.hip: the stereo path's post-steps (dense_stereo.py:407-437, 475-492)
hipError_t stereo_backproject(const float *depth, const float *conf, const unsigned char *bgr, int n_maps, int H, int W,
                              const double *Kinv_h, const double *poses_h, float min_confidence, ScratchCache &cache,
                              DeviceBuffer<double> &pts_out, DeviceBuffer<unsigned char> &rgb_out, long long *total,
                              long long *per_map_h, hipStream_t st);
hipError_t cloud_take(const double *pts, const unsigned char *rgb, long long n, const long long *idx_h, long long m,
                      ScratchCache &cache, DeviceBuffer<double> &pts_out, DeviceBuffer<unsigned char> &rgb_out, hipStream_t st);
hipError_t voxel_downsample(const double *pts, const unsigned char *rgb, long long m, const unsigned char *keep_h,
                            double voxel, ScratchCache &cache, DeviceBuffer<double> &pts_out,
                            DeviceBuffer<unsigned char> &rgb_out, long long *m_out, hipStream_t st);
// the grid anchored at `origin` of include/amvs_match.h; lo / ext: the voxel-index box of the kept points
hipError_t voxel_downsample_grid(const double *pts, const unsigned char *rgb, long long m, const unsigned char *keep_h,
                                 const double origin[3], double voxel, const long long lo[3], const long long ext[3],
                                 ScratchCache &cache, DeviceBuffer<double> &pts_out, DeviceBuffer<unsigned char> &rgb_out,
                                 long long *m_out, hipStream_t st);

// amvs_cloud_normals.hip: per-view normal maps fitted to the inverse depths, and the normals of a cloud from them
// (include/amvs.h amvs_depth_normals, amvs_cloud_normals).  depth / conf: [n_maps][H*W] float32 on the device; K_h: 9
// doubles row-major, poses_h: n_maps x 12 doubles (host).  The caller has validated the parameters.  `normals` /
// `map_normals` ([n_maps][H*W][3]), nrm_out ([n_pts][3]) and seen_out ([n_pts]) are grown as needed.  Both synchronise.
hipError_t depth_normals(const float *depth, const float *conf, int n_maps, int H, int W, const double *K_h, const double *poses_h,
                         float min_confidence, int radius, float jump, int min_points, bool world, ScratchCache &cache,
                         DeviceBuffer<float> &normals, long long *n_normals, hipStream_t st);
// counts[0] = pixels with a normal (world frame), counts[1] = points with a normal
hipError_t cloud_normals(const double *pts, long long n_pts, const float *depth, const float *conf, int n_maps, int H, int W,
                         const double *K_h, const double *poses_h, float min_confidence, int radius, float jump, int min_points,
                         float depth_tolerance, int min_views, ScratchCache &cache, DeviceBuffer<float> &map_normals,
                         DeviceBuffer<float> &nrm_out, DeviceBuffer<int> &seen_out, long long counts[2], hipStream_t st);
// amvs_depth_filter.hip: the cross-view depth-map filter (include/amvs_depth.h amvs_depth_filter).  depth / conf and the
// two outputs: [n_maps][H*W] float32 on the device, the outputs apart from the inputs; K_h, Ki_h: 9 doubles row-major,
// poses_h: n_maps x 12 doubles, nbr_h: [n_maps][n_nbr] int32 map indices or -1 (host; n_nbr may be 0).  The caller has
// validated the parameters.  counts[0] = valid input pixels, counts[1] = pixels kept.  Synchronises.
hipError_t depth_filter(const float *depth, const float *conf, int n_maps, int H, int W, const double *K_h, const double *Ki_h,
                        const double *poses_h, const int *nbr_h, int n_nbr, float min_confidence, float max_px, float max_rel,
                        int min_consistent, bool refine, ScratchCache &cache, float *depth_out, float *count_out,
                        long long counts[2], hipStream_t st);

// amvs_mesh.hip: TSDF fusion of the per-view maps and marching-tetrahedra extraction (include/amvs.h
// amvs_tsdf_*).  The state (volume, scans, mesh) is owned by a context and freed with it; its buffers are
// allocated through the context's `cache`.
struct TsdfState;
TsdfState *tsdf_state_new();
void tsdf_state_free(TsdfState *s);
// depth / conf: [n_maps][H*W] (host or device); bgr: [bgr_images][H*W][3] BGR (host or device), map j takes
// its colours from image slots_h[j]; poses_h: [n_maps][12] float32 R row-major, t.  Synchronises.
hipError_t tsdf_integrate(TsdfState *s, ScratchCache &cache, const float *depth, const float *conf, bool maps_on_device,
                          int n_maps, int H, int W, const unsigned char *bgr, bool bgr_on_device, long long bgr_images,
                          const int *slots_h, const float K[9], const float *poses_h, float min_views, const float origin[3],
                          float voxel, const int dims[3], float trunc, hipStream_t st);
// test hook: replaces the volume by host arrays in tsdf_fetch_volume's layout (copies only).  Synchronises.
hipError_t tsdf_set_volume(TsdfState *s, ScratchCache &cache, const float *tsdf, const float *weight, const float *color_sum,
                           const float origin[3], float voxel, const int dims[3], hipStream_t st);
hipError_t tsdf_extract(TsdfState *s, ScratchCache &cache, long long *n_vertices, long long *n_faces, hipStream_t st);
bool tsdf_has_volume(const TsdfState *s);
bool tsdf_has_mesh(const TsdfState *s);
hipError_t tsdf_fetch_mesh(TsdfState *s, float *verts, int *faces, unsigned char *rgb, hipStream_t st);
hipError_t tsdf_fetch_volume(TsdfState *s, float *tsdf, float *weight, float *color_sum, hipStream_t st);

// amvs_mesh_fill.hip: hole filling in the state's current volume (include/amvs.h amvs_tsdf_fill, amvs_tsdf_fetch_fill).
// steps in 1 .. AMVS_FILL_MAX_STEPS and min_neighbours in 1 .. 6 are the caller's business.  Drops the mesh; filled_per_step
// ([steps]) and n_filled may be NULL.  Synchronises.
hipError_t tsdf_fill(TsdfState *s, ScratchCache &cache, int steps, int min_neighbours, long long *filled_per_step,
                     long long *n_filled, hipStream_t st);
bool tsdf_has_fill(const TsdfState *s);          // a fill ran on the current volume
hipError_t tsdf_fetch_fill(TsdfState *s, unsigned char *gen, hipStream_t st);

// amvs_mesh_clean.hip: clean-up of the state's current mesh in place (include/amvs.h amvs_mesh_*).  All synchronise.
// replaces the mesh by host arrays the caller has validated (copies only); rgb NULL: zeros
hipError_t mesh_set(TsdfState *s, ScratchCache &cache, const float *verts, long long nv, const int *faces, long long nf,
                    const unsigned char *rgb, hipStream_t st);
// n_components: before the filter; n_vertices, n_faces: after it
hipError_t mesh_filter_components(TsdfState *s, ScratchCache &cache, long long min_faces, bool keep_largest, long long *n_components,
                                  long long *n_vertices, long long *n_faces, hipStream_t st);
hipError_t mesh_smooth(TsdfState *s, ScratchCache &cache, int iterations, float lambda, float mu, bool fix_boundary, hipStream_t st);
hipError_t mesh_normals(TsdfState *s, ScratchCache &cache, hipStream_t st);
bool mesh_has_normals(const TsdfState *s);
bool mesh_has_labels(const TsdfState *s);
hipError_t mesh_fetch_attributes(TsdfState *s, float *normals, int *labels, hipStream_t st);
// for amvs_mesh_decimate.hip: the vertex -> corner index of the current faces (built once per topology) and the face
// normals cross(p1 - p0, p2 - p0) of the current faces and positions into the state's face_normal.  Neither synchronises.
hipError_t ensure_index(TsdfState *s, ScratchCache &cache, hipStream_t st);
hipError_t mesh_face_normals(TsdfState *s, ScratchCache &cache, hipStream_t st);

// amvs_mesh_decimate.hip: vertex clustering of the state's current mesh in place on the grid of cells of side `cell`
// at `origin` (include/amvs.h amvs_mesh_decimate).  bad_vertex: -1, or the smallest id of a vertex outside the cluster
// grid -- then nothing was changed.  Otherwise drops labels, normals and the index.  Synchronises.
hipError_t mesh_decimate(TsdfState *s, ScratchCache &cache, const float origin[3], float cell, long long *bad_vertex,
                         long long *n_vertices, long long *n_faces, hipStream_t st);
// the same with quadric placement of the clusters' vertices (include/amvs.h amvs_mesh_decimate_quadric).  n_fallback:
// the clusters that kept the mean.  Builds the index of the mesh before the decimation, after the range check.
hipError_t mesh_decimate_quadric(TsdfState *s, ScratchCache &cache, const float origin[3], float cell, float regularisation,
                                 long long *bad_vertex, long long *n_vertices, long long *n_faces, long long *n_fallback,
                                 hipStream_t st);

// amvs_mesh_render.hip: the state's current mesh drawn into views, the visibility counts and their filter
// (include/amvs.h amvs_mesh_render ...).  The maps and the counts are attributes of the current mesh.  All synchronise.
// poses_h: [n_views][12] float32 R row-major, t; n_skipped_h: NULL or [n_views].  The caller has validated the arguments.
void mesh_set_render_tuning(TsdfState *s, int large_face_pixels);
hipError_t mesh_render(TsdfState *s, ScratchCache &cache, int n_views, int H, int W, const float K[9], const float *poses_h,
                       float near, long long *n_skipped_h, hipStream_t st);
bool mesh_has_render(const TsdfState *s);
bool mesh_has_visibility(const TsdfState *s);
int mesh_render_views(const TsdfState *s);       // views of the current render, 0 without one
hipError_t mesh_fetch_render(TsdfState *s, int first, int count, float *depth, int *face, hipStream_t st);
hipError_t mesh_visibility(TsdfState *s, ScratchCache &cache, float tolerance, long long *n_seen, hipStream_t st);
hipError_t mesh_fetch_visibility(TsdfState *s, int *counts, hipStream_t st);
// drops the maps, the counts, labels, normals and the index
hipError_t mesh_filter_visible(TsdfState *s, ScratchCache &cache, int min_views, long long *n_vertices, long long *n_faces,
                               hipStream_t st);

// amvs_mesh_color.hip: the current mesh coloured from the images of the rendered views, and the current render shaded
// with the vertex colours (include/amvs.h amvs_mesh_color_views, amvs_fetch_render_color).  Both need the current render,
// the first the current normals too; the caller has validated the arguments.  Both synchronise and change no flag.
// bgr: [bgr_images][H*W][3] BGR (host or device), rendered view j takes its colours from image slots_h[j].
hipError_t mesh_color_views(TsdfState *s, ScratchCache &cache, const unsigned char *bgr, bool bgr_on_device, long long bgr_images,
                            const int *slots_h, float tolerance, float min_cos, bool best_view, long long *n_colored, hipStream_t st);
// rgb_out: [count][H][W][3] RGB on the host, computed into a leased block
hipError_t mesh_fetch_render_color(TsdfState *s, ScratchCache &cache, int first, int count, unsigned char *rgb_out, hipStream_t st);

// amvs_mesh_texture.hip: the texture atlas of the current mesh from the images of the rendered views, its UVs and the
// current render shaded with it (include/amvs.h amvs_mesh_texture, amvs_fetch_mesh_texture, amvs_fetch_render_texture).
// The caller has validated the arguments; all synchronise.
bool mesh_has_texture(const TsdfState *s);
// the layout of the current mesh's n_faces faces at `texels` intervals per leg: cells per row (cells_per_row, or the
// automatic value for 0) and the atlas's sides, which the caller compares with AMVS_TEXTURE_MAX_SIDE.  No faces: all zero.
void mesh_texture_layout(const TsdfState *s, int texels, int cells_per_row, long long *n_faces, long long *cols, long long *width,
                         long long *height);
// of the current texture
void mesh_texture_size(const TsdfState *s, int *texels, int *width, int *height);
// images as mesh_color_views; cols, width, height from mesh_texture_layout.  Sets the texture, changes no other flag.
hipError_t mesh_texture(TsdfState *s, ScratchCache &cache, const unsigned char *bgr, bool bgr_on_device, long long bgr_images,
                        const int *slots_h, float tolerance, float min_cos, bool best_view, int texels, int cols, int width,
                        int height, long long *n_textured, hipStream_t st);
// atlas_rgb: [height][width][3], uv: [n_faces][3][2] on the host; NULL skips one
hipError_t mesh_fetch_texture(TsdfState *s, unsigned char *atlas_rgb, float *uv, hipStream_t st);
// rgb_out: [count][H][W][3] RGB on the host, computed into a leased block
hipError_t mesh_fetch_render_texture(TsdfState *s, ScratchCache &cache, int first, int count, unsigned char *rgb_out, hipStream_t st);

}  // namespace amvs
