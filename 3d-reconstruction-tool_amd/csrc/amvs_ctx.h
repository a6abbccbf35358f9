// amvs_ctx.h -- private to the C ABI's translation units (amvs_context.hip, amvs_capi*.hip, amvs_comm.hip; not
// installed): the context behind include/amvs.h and the host helpers more than one of those files uses.
#pragma once
#include "../../include/amvs.h"
#include "amvs_kernels.h"
#include "amvs_buffer.h"
#include "amvs_handles.h"
#include "amvs_launch_plan.h"
#include "amvs_match_state.h"
#include "amvs_sfm_state.h"
#include "amvs_features_state.h"

#include <array>
#include <cmath>
#include <map>
#include <memory>
#include <string>
#include <vector>

// the communicator of amvs_comm.hip, the only file that sees RCCL (as rccl.h declares it)
struct ncclComm;
typedef ncclComm *ncclComm_t;

namespace amvs {
namespace host {

struct Stats {
    amvs::DeviceBuffer<float> mean, var;
    std::vector<char> done;             // empty until the maps are allocated
};

struct FastStats {
    amvs::DeviceBuffer<float2> maps;    // [n_views][H*W]
    std::vector<char> done;
};

// a point cloud on the device: float64 xyz, uint8 rgb; after amvs_cloud_normals also float32 normals and the int32 counts
// of the views that gave them.  Every step that makes a cloud assigns a fresh Cloud, so the normals never outlive the
// points they were computed for.
struct Cloud {
    amvs::DeviceBuffer<double> pts;
    amvs::DeviceBuffer<unsigned char> rgb;
    long long n = 0;
    amvs::DeviceBuffer<float> nrm;
    amvs::DeviceBuffer<int> seen;
    bool have_normals = false;
};

}  // namespace host
}  // namespace amvs

struct amvs_ctx {
    int device = 0, H = 0, W = 0, n_views = 0, n_cu = 256;
    long long stride = 0;   // floats between images (H*W rounded up + tail padding)
    float K[9], Kinv[9];
    std::vector<std::array<float, 9>> R;
    std::vector<std::array<float, 3>> t;
    std::vector<char> have;
    // every device allocation of the context goes through its cache (amvs_buffer.h), the post-steps' short-lived
    // blocks come from it
    amvs::ScratchCache cache;
    amvs::DeviceBuffer<float> d_images;
    // packed 8-bit row-pair maps (sampling fast path), valid while every uploaded view is
    // exactly code/255 (n_inexact == 0); otherwise the sweep samples the float32 maps
    amvs::DeviceBuffer<uint16_t> d_pairs;
    long long pstride = 0;              // ushorts between packed maps
    amvs::DeviceBuffer<unsigned char> d_bgr;      // [n_views][H*W*3] prepared colour images (amvs_set_view_bgr8), lazily allocated
    amvs::DeviceBuffer<unsigned char> d_prep_src; // staging of one uploaded source image + the resize tables (amvs_set_view_bgr8):
    amvs::DeviceBuffer<int> d_prep_tab;           // kept across calls -- an allocation per view cost more than the copy
    amvs::DeviceBuffer<unsigned char> d_prep_undist;   // the staged image undistorted at its own size (include/amvs_lens.h), grown only
    std::vector<char> have_bgr;
    amvs::DeviceBuffer<int> d_flag;     // [n_views] 1 = the view did not quantise to 8 bits losslessly
    mutable std::vector<char> exact8;    // host copy of !d_flag, refreshed lazily (flags_dirty)
    mutable bool flags_dirty = false;
    bool force_f32 = false;             // amvs_set_sampling: A/B switch for tests
    int mode = AMVS_MODE_EXACT;         // arithmetic of the sweeps (amvs_set_mode)
    amvs::plan::SweepTuning tuning;     // the launch policy's knobs (amvs_set_*_tuning, amvs_set_launch_order, amvs_set_step_sources)
    std::map<int, amvs::host::Stats> stats;
    std::map<int, amvs::host::FastStats> fstats;    // fast mode: (mean1, var1) maps per patch size
    // PatchMatch state of the batch slots (ensure_slots); the cost is updated in place, so it has one buffer
    amvs::DeviceBuffer<float> d_depth[2], d_cost, d_normal[2], d_aux;
    amvs::DeviceBuffer<amvs::Job> d_jobs;
    amvs::DeviceBuffer<float> d_planes;
    amvs::DeviceBuffer<unsigned> d_keys;          // plane-sweep running best, [slot][H*W]
    amvs::DeviceBuffer<float> d_xcand_d, d_xcand_n;            // extended mode: view-propagation candidates
    amvs::DeviceBuffer<int> d_xsrc;
    amvs::DeviceBuffer<float> d_sweep_depth, d_sweep_conf;     // maps of the last amvs_plane_sweep_batch
    int n_sweep = 0;
    amvs::host::Cloud cloud;             // result of the last fusion / back-projection and the steps after it
    std::map<int, amvs::DescSlot> desc;   // resident descriptors by slot (include/amvs_match.h amvs_desc_set)
    amvs::PairCloud pair_cloud;          // what amvs_pair_triangulate appends to, until amvs_pair_cloud_finish
    amvs::SfmState sfm;                  // the track state of an incremental reconstruction (include/amvs_sfm.h)
    amvs::ClaheState clahe;              // the result of the last amvs_clahe_u8 (include/amvs_features.h)
    amvs::SiftState sift;                // the scale space of the last amvs_sift_scale_space
    amvs::DeviceBuffer<float> d_depth_normals;   // [depth_normal_maps][H*W][3] of the last amvs_depth_normals / amvs_cloud_normals
    int depth_normal_maps = 0;           // (grown only; 0 = none to fetch)
    // volume, scans and mesh of amvs_tsdf_* (amvs_mesh.hip), lazily created
    std::unique_ptr<amvs::TsdfState, void (*)(amvs::TsdfState *)> tsdf{nullptr, amvs::tsdf_state_free};
    // split schedule (amvs_pm_params.schedule == AMVS_SCHEDULE_SPLIT): sample maps (its streams and token events are
    // among the handles below)
    amvs::DeviceBuffer<float> d_samples;
    hipStream_t stream = nullptr;       // own_stream, or the caller's (amvs_set_stream: borrowed, never destroyed here)
    int last_tile_rows = 0, last_views_per_launch = 0;
    // state a continuation call (amvs_pm_params.first_iteration > 0) resumes: which depth buffer is
    // current, the next iteration, and a fingerprint of the batch it belongs to
    bool pm_resumable = false;
    int pm_cur = 0, pm_next_iteration = 0;
    uint64_t pm_key = 0;
    // native exchange (amvs_comm_*): RCCL resolved with dlopen, one communicator per context
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 0;
    // amvs_set_step_timing: an event behind every sweep launch of the last PatchMatch call (ev_steps)
    bool step_timing = false;
    int n_step_events = 0;
    int timing_groups = 0;
    bool timing_overlapped = false;      // the groups of the last call ran on two streams (resolve_timing)
    bool timing_pending = false;
    // -DAMVS_STEP_TRACE: [launch][trace_stride blocks][4] workgroup timeline of the last PatchMatch call
    amvs::DeviceBuffer<unsigned long long> d_trace;
    long long trace_stride = 0, trace_launches = 0;
    amvs_timing timing{};
    std::string err;
    // The streams and events the context owns (amvs_handles.h).  Declared after every device buffer, so that they are
    // destroyed before the memory the work queued on them uses.  A pair of streams is created whole or not at all.
    amvs::Stream own_stream;
    amvs::Event ev[4];                        // start / after init / after the steps / end of the last timed call
    amvs::Stream split_streams[2];            // split schedule: [0] sampling kernels, [1] window kernels
    amvs::EventPool split_events{false};      // [0] fork, [1 + g] sampled(g), [9 + g] windowed(g)
    amvs::EventPool ev_steps{true};
    amvs::EventPool ev_groups{true};          // per view group of the last PatchMatch call: init / steps / confidence
    amvs::Stream group_streams[2][2];         // [group_overlap - 1][stream]
    amvs::Event group_fork, group_join;
};

namespace amvs {
namespace host {

// the error message of `c` (NULL: of amvs_create, read with amvs_last_error(NULL)); returns `code`
int fail(amvs_ctx *c, int code, const std::string &msg);

#define HIPCHK(c, call)                                                                   \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail((c), AMVS_EHIP,                                                   \
                        std::string(#call) + ": " + hipGetErrorString(e_));               \
    } while (0)

// amvs_context.hip (each is described at its definition)
void index_report(uint64_t out[4], bool reset);
int checked(amvs_ctx *c, int rc);
int bind_device(amvs_ctx *c);
int check_patch_src(amvs_ctx *c, int patch, int n_src);
int ensure_slots(amvs_ctx *c, int n);
int ensure_stats(amvs_ctx *c, int patch);
int ensure_fast_stats(amvs_ctx *c, int patch);
using StepRegs = amvs::plan::StepRegs;      // StepArgs::ref_in_kernel / depth_hist of the fast sweep steps of `c`
StepRegs step_regs(const amvs_ctx *c, int patch);
amvs::plan::Device plan_device(const amvs_ctx *c, bool packed_maps);
amvs::plan::Facts plan_facts(int patch, int n_src, bool fast, bool packed_maps, unsigned waves_entries);
amvs::plan::SweepTuning plan_tuning(const amvs_plan_tuning &t);
int upload_jobs(amvs_ctx *c, int n_ref, const int *ref_ids, const int *src_ids, int n_src, int fast_patch = 0,
                bool compose_only = false, bool ref_maps = true);
const uint16_t *usable_pairs(const amvs_ctx *c);
int resolve_fast(amvs_ctx *c, int requested, int *fast);
void resolve_timing(amvs_ctx *c);
int check_colour_views(amvs_ctx *c, int n, const int *view_ids);
int gather_colours(amvs_ctx *c, int n, const int *view_ids, amvs::DeviceBuffer<unsigned char> &out);
int stage_maps(amvs_ctx *c, size_t n, const float *&depth, const float *&conf, amvs::DeviceBuffer<float> (&copy)[2]);

// a threshold the entry points refuse: not positive, or not finite
inline bool bad_threshold(double t) { return !(t > 0.0) || !std::isfinite(t); }

// the non-zero bytes of mask[0 .. m)
inline long long count_set(const uint8_t *mask, int m)
{
    long long n = 0;
    for (int i = 0; i < m; ++i) n += mask[i] != 0;
    return n;
}

// n elements of host memory into `out` (a post-step's inputs)
template <class T>
int upload(amvs_ctx *c, const T *host, size_t n, amvs::DeviceBuffer<T> &out)
{
    HIPCHK(c, out.reserve(n, c->cache));
    HIPCHK(c, hipMemcpyAsync(out.get(), host, sizeof(T) * n, hipMemcpyHostToDevice, c->stream));
    return AMVS_OK;
}

}  // namespace host
}  // namespace amvs
