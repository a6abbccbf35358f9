// amvs_capi.hip -- the C ABI of include/amvs.h: view upload and the issuing of the PatchMatch sweep steps.
// (The context: amvs_context.hip; the other entry points: amvs_capi_*.hip, amvs_comm.hip.  What a call launches -- views
// per launch, strip rows, schedule -- is decided in amvs_launch_plan.h; the schedules here issue that plan.)
//
// Host-side orchestration of PatchMatchMVS._patchmatch_cuda (mvs_patchmatch.py:225-321)
// and DenseStereoReconstructor._plane_sweep_torch (dense_stereo.py:222-316): all views of
// a scene are uploaded once and stay resident; a batch of reference views is swept
// together, one kernel launch per cost-evaluation step over the whole batch.
#include "amvs_ctx.h"
#include "../../include/amvs_lens.h"
#include "../../include/amvs_step.h"

#include <cmath>
#include <cstring>
#include <utility>

using namespace amvs::host;

namespace {

using amvs::plan::PmPlan;

static_assert(amvs::plan::STEP_PROP == amvs::MODE_PROP && amvs::plan::STEP_REFINE == amvs::MODE_REFINE, "step modes out of sync");
static_assert(amvs::plan::SPLIT_MAX_GROUPS == 8, "amvs_ctx::split_events holds 1 + 2 * 8 events");

amvs::StepArgs base_args(const amvs_ctx *c, int patch, int n_jobs, int TH)
{
    amvs::StepArgs a{};
    a.H = c->H; a.W = c->W; a.TH = TH;
    a.tiles_x = amvs::plan::strip_cols(c->W, amvs::strip_out_width(patch));
    a.tiles_y = amvs::plan::ceil_div(c->H, TH);
    a.n_jobs = n_jobs;
    a.img_stride = c->stride;
    a.images = c->d_images.get();
    a.pairs = usable_pairs(c);
    a.pair_stride = c->pstride;
    a.jobs = c->d_jobs.get();
    a.aux = c->d_aux.get();
    const StepRegs regs = step_regs(c, patch);             // (read by the fast step only; upload_jobs skips the maps to match)
    a.ref_in_kernel = regs.stats ? 1 : 0;
    a.depth_hist = regs.hist ? 1 : 0;
    return a;
}

// depth buffer `cur_d` is read and cur_d^1 written on every step; cost lives in d_cost and is
// updated in place; normals: both buffers, the sign bit of the state depths names each pixel's
// current one (StepArgs::nbuf).  `tagged`: d_in is a state map (its depths carry that bit).
void set_io(amvs::StepArgs &a, const amvs_ctx *c, int cur_d, bool tagged = true)
{
    a.d_in = c->d_depth[cur_d].get();
    a.d_out = c->d_depth[cur_d ^ 1].get();
    a.cost = c->d_cost.get();
    a.nbuf[0] = c->d_normal[0].get();
    a.nbuf[1] = c->d_normal[1].get();
    a.depth_mask = tagged ? 0x7FFFFFFFu : 0xFFFFFFFFu;
}

// one launch of the plan: what it does and its shape
void apply_step(amvs::StepArgs &a, const amvs::plan::Step &st)
{
    a.mode = st.mode; a.oy = st.oy; a.ox = st.ox;
    if (st.mode == amvs::MODE_REFINE) { a.depth_range = st.depth_range; a.normal_range = st.normal_range; a.draw = st.draw; }
    a.TH = st.rows; a.tiles_y = st.tiles_y; a.wg_cap = st.wg_cap;
}

// The two streams of SweepTuning::group_overlap = 1 (equal priorities) or 2 (high / low), created once per context.
int group_streams(amvs_ctx *c, int overlap, hipStream_t out[2])
{
    amvs::Stream (&st)[2] = c->group_streams[overlap - 1];
    if (!st[0].get()) HIPCHK(c, amvs::create_stream_pair(st, overlap == 2, false));
    if (!c->group_fork.get()) {
        amvs::Event fork, join;
        HIPCHK(c, fork.create(false));
        HIPCHK(c, join.create(false));
        c->group_fork = std::move(fork); c->group_join = std::move(join);
    }
    out[0] = st[0].get(); out[1] = st[1].get();
    return AMVS_OK;
}

// The batch in the plan's groups of views, each group through the whole schedule with the fused kernel (sampling +
// window sums + selection in one launch).  One stream, or (PmPlan::overlap) the groups dealt to two streams
// that fork from the context's stream and join it again: the groups are independent (mvs_patchmatch.py:104-123) --
// their StepArgs, state slots, job entries and confidence slots are disjoint, the images and the job table are
// read-only, and the fused launches use no other scratch -- so the workgroups of one group fill the wave slots the
// tail of the other leaves empty.  Every group still runs its whole schedule in order on its stream.
int run_fused_schedule(amvs_ctx *c, int n_src, const amvs_pm_params *p, uint64_t seed, int fast, const PmPlan &plan, void *conf_dev,
                       int cur0, bool do_init, bool do_conf)
{
    const size_t hw = (size_t)c->H * c->W;
    const size_t n_groups = plan.groups.size();
    HIPCHK(c, c->ev_steps.reserve((c->step_timing ? (size_t)plan.launches : 0) + n_groups));
    c->n_step_events = 0;
    // events: [0] start, then per group: after init, after steps, after confidence
    HIPCHK(c, c->ev_groups.reserve(3 * n_groups));
    c->timing_groups = (int)n_groups;
#ifdef AMVS_STEP_TRACE
    // (cleared on the context's stream BEFORE the group streams fork from it)
    c->trace_stride = plan.trace_blocks;
    c->trace_launches = plan.launches;
    HIPCHK(c, c->d_trace.reserve((size_t)(4 * c->trace_stride * c->trace_launches) + 1, c->cache));
    HIPCHK(c, hipMemsetAsync(c->d_trace.get(), 0, sizeof(unsigned long long) * (size_t)(4 * c->trace_stride * c->trace_launches), c->stream));
#endif
    c->timing_overlapped = plan.overlap != 0;
    hipStream_t lanes[2] = {c->stream, c->stream};
    if (plan.overlap) {
        int rc = group_streams(c, plan.overlap, lanes);
        if (rc) return rc;
        HIPCHK(c, hipEventRecord(c->group_fork.get(), c->stream));
        for (hipStream_t st : lanes) HIPCHK(c, hipStreamWaitEvent(st, c->group_fork.get(), 0));
    }
    for (size_t g = 0; g < n_groups; ++g) {
        const int nj = plan.groups[g].count;
        hipStream_t stream = lanes[g % 2];
        amvs::StepArgs a = base_args(c, p->patch_size, nj, plan.TH);
        a.fast = fast;
        a.band_major = plan.band_major;
        a.paired = plan.paired ? 1 : 0;
        a.jobs = c->d_jobs.get() + plan.groups[g].first;     // slots stay global: job.slot = index in the batch
        a.depth_min = p->depth_min; a.depth_max = p->depth_max;
        a.seed = seed;
        a.edge_first = plan.edge_first;
        int cur = cur0;
        // initialisation (mvs_patchmatch.py:268-284); a continuation call resumes the context's state
        if (do_init)
            HIPCHK(c, amvs::launch_init(a.jobs, nj, (long long)hw, seed, p->log_depth_scale, p->log_depth_min,
                                        c->d_depth[cur].get(), c->d_normal[0].get(), c->d_cost.get(), stream));
        HIPCHK(c, hipEventRecord(c->ev_groups[3 * g], stream));
        if (c->step_timing) HIPCHK(c, hipEventRecord(c->ev_steps[c->n_step_events++], stream));
        for (size_t i = 0; i < plan.steps.size(); ++i) {
            const amvs::plan::Step &st = plan.steps[i];
            apply_step(a, st);
            set_io(a, c, cur);
#ifdef AMVS_STEP_TRACE
            a.trace = c->d_trace.get() + 4 * c->trace_stride * (long long)(g * plan.steps.size() + i);
#endif
            HIPCHK(c, amvs::launch_step(p->patch_size, n_src, a, stream));
            if (c->step_timing) HIPCHK(c, hipEventRecord(c->ev_steps[c->n_step_events++], stream));
            cur ^= st.flip_d;
        }
        a.TH = plan.TH;
        a.tiles_y = plan.tiles_y;
        a.wg_cap = 0;
        a.trace = nullptr;
        HIPCHK(c, hipEventRecord(c->ev_groups[3 * g + 1], stream));
        // _compute_confidence (mvs_patchmatch.py:493-534), written straight into the output
        if (do_conf) {
            a.mode = amvs::MODE_CONF;
            set_io(a, c, cur);
            a.aux = conf_dev ? (float *)conf_dev : c->d_aux.get();
            HIPCHK(c, amvs::launch_step(p->patch_size, n_src, a, stream));
        }
        HIPCHK(c, hipEventRecord(c->ev_groups[3 * g + 2], stream));
    }
    if (plan.overlap)
        for (hipStream_t st : lanes) {
            HIPCHK(c, hipEventRecord(c->group_join.get(), st));
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->group_join.get(), 0));
        }
    return AMVS_OK;
}

// Split schedule (fast mode).  A sweep step is two kernels: the SAMPLING kernel visits every pixel
// once -- no strip halo -- and is bound by the CU's L1 line rate for scattered gathers; the WINDOW
// kernel streams the sample maps (coalesced) through the box sums, NCC and selection.  They stress
// different parts of the CU, so the batch is cut into view groups (SplitPlan) and the two kernel kinds run on
// two streams (distinct priorities, so that they land on distinct hardware queues):
//     sampling stream:  sample(g0,n) sample(g1,n) sample(g0,n+1) ...   (never two of them at once)
//     window stream:    window(g,n) after sample(g,n); sample(g,n+1) after window(g,n)   (events)
// so window(g,n) runs under the sampling of the next group.  Views are independent
// (mvs_patchmatch.py:104-123), nothing else orders the groups.  Results are those of the fused kernel
// bit for bit (same arithmetic, same order of every sum).
int run_split_schedule(amvs_ctx *c, int n_ref, int n_src, const amvs_pm_params *p, uint64_t seed, const PmPlan &plan, void *conf_dev)
{
    const size_t hw = (size_t)c->H * c->W;
    const amvs::plan::SplitPlan &sp = plan.split;
    HIPCHK(c, c->d_samples.reserve((size_t)n_ref * n_src * hw, c->cache));
    if (!c->split_streams[0].get()) HIPCHK(c, amvs::create_stream_pair(c->split_streams, false, true));
    HIPCHK(c, c->split_events.reserve(1 + 2 * amvs::plan::SPLIT_MAX_GROUPS));
    HIPCHK(c, c->ev_groups.reserve(3));
    c->timing_groups = 1;
    c->n_step_events = 0;                       // (no per-launch events in this schedule: amvs_get_step_times returns none)
    hipStream_t s_smp = c->split_streams[0].get(), s_win = c->split_streams[1].get();
    hipEvent_t ev_fork = c->split_events[0];
    const hipEvent_t *ev_sampled = &c->split_events[1], *ev_windowed = &c->split_events[1 + amvs::plan::SPLIT_MAX_GROUPS];

    amvs::StepArgs all = base_args(c, p->patch_size, n_ref, sp.TH);
    all.fast = 1;
    all.depth_min = p->depth_min; all.depth_max = p->depth_max;
    all.seed = seed;
    all.samples = c->d_samples.get();
    all.half = p->patch_size / 2;
    all.s_TH = sp.s_TH;
    all.s_lds = sp.s_lds;
    all.s_tiles_x = sp.s_tiles_x;
    all.s_tiles_y = sp.s_tiles_y;
    int cur = 0;
    HIPCHK(c, amvs::launch_init(all.jobs, n_ref, (long long)hw, seed, p->log_depth_scale, p->log_depth_min,
                                c->d_depth[cur].get(), c->d_normal[0].get(), c->d_cost.get(), c->stream));
    HIPCHK(c, hipEventRecord(c->ev_groups[0], c->stream));
    HIPCHK(c, hipEventRecord(ev_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(s_smp, ev_fork, 0));
    HIPCHK(c, hipStreamWaitEvent(s_win, ev_fork, 0));
    bool first = true;
    for (const amvs::plan::Step &st : plan.steps) {
        for (size_t g = 0; g < sp.groups.size(); ++g) {
            amvs::StepArgs a = all;
            a.n_jobs = sp.groups[g].count;
            a.jobs = c->d_jobs.get() + sp.groups[g].first;
            apply_step(a, st);
            set_io(a, c, cur);
            if (!first) HIPCHK(c, hipStreamWaitEvent(s_smp, ev_windowed[g], 0));
            HIPCHK(c, amvs::launch_sample_fast(n_src, a, s_smp));
            HIPCHK(c, hipEventRecord(ev_sampled[g], s_smp));
            HIPCHK(c, hipStreamWaitEvent(s_win, ev_sampled[g], 0));
            a.presampled = 1;
            HIPCHK(c, amvs::launch_step(p->patch_size, n_src, a, s_win));
            HIPCHK(c, hipEventRecord(ev_windowed[g], s_win));
        }
        first = false;
        cur ^= st.flip_d;
    }
    // the window stream is in order, so its last event covers every group
    if (!plan.steps.empty()) HIPCHK(c, hipStreamWaitEvent(c->stream, ev_windowed[sp.groups.size() - 1], 0));
    HIPCHK(c, hipEventRecord(c->ev_groups[1], c->stream));
    // _compute_confidence (mvs_patchmatch.py:493-534): one fused launch over the whole batch
    if ((p->flags & AMVS_PM_NO_CONFIDENCE) == 0) {
        all.mode = amvs::MODE_CONF;
        set_io(all, c, cur);
        all.aux = conf_dev ? (float *)conf_dev : c->d_aux.get();
        HIPCHK(c, amvs::launch_step(p->patch_size, n_src, all, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->ev_groups[2], c->stream));
    return AMVS_OK;
}

// single-view, single-step helper for the test entry points
struct OneStep {
    amvs_ctx *c;
    amvs::StepArgs a;
    int patch, n_src;
    size_t hw;
};

int one_step_begin(amvs_ctx *c, int ref, const int *src_ids, int n_src, int patch, OneStep &o)
{
    if (!c) return AMVS_EINVAL;
    int rc = bind_device(c);
    if (rc) return rc;
    if ((rc = check_patch_src(c, patch, n_src))) return rc;
    if ((rc = ensure_slots(c, 1))) return rc;
    int fast = 0;
    if ((rc = resolve_fast(c, AMVS_MODE_DEFAULT, &fast))) return rc;
    if ((rc = upload_jobs(c, 1, &ref, src_ids, n_src, fast ? patch : 0, false, !step_regs(c, patch).stats))) return rc;
    c->pm_resumable = false;                    // the single-step entry points overwrite the state of slot 0
    o.c = c; o.patch = patch; o.n_src = n_src; o.hw = (size_t)c->H * c->W;
    const bool packed = usable_pairs(c) != nullptr;
    o.a = base_args(c, patch, 1, amvs::plan::single_step_rows(plan_device(c, packed), plan_facts(patch, n_src, fast != 0, packed, 1u), patch));
    o.a.fast = fast;
    o.a.mode = amvs::MODE_EVAL;
    set_io(o.a, c, 0, false);                   // caller-supplied depth maps: no tag to strip
    return AMVS_OK;
}

int upload_state(amvs_ctx *c, size_t hw, const float *depth, const float *normal, const float *cost)
{
    if (depth) HIPCHK(c, hipMemcpyAsync(c->d_depth[0].get(), depth, 4 * hw, hipMemcpyHostToDevice, c->stream));
    if (normal) HIPCHK(c, hipMemcpyAsync(c->d_normal[0].get(), normal, 12 * hw, hipMemcpyHostToDevice, c->stream));
    if (cost) HIPCHK(c, hipMemcpyAsync(c->d_cost.get(), cost, 4 * hw, hipMemcpyHostToDevice, c->stream));
    return AMVS_OK;
}

// state of slot 0 after a single step (tagged depths in d_depth[dbuf]) -> plain host arrays
int download_state(amvs_ctx *c, size_t hw, int dbuf, float *depth, float *normal, float *cost)
{
    HIPCHK(c, amvs::launch_resolve_state(c->d_jobs.get(), 1, (long long)hw, c->d_depth[dbuf].get(), c->d_normal[0].get(), c->d_normal[1].get(),
                                         nullptr, nullptr, 0, c->stream));
    HIPCHK(c, hipMemcpyAsync(depth, c->d_depth[dbuf].get(), 4 * hw, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(normal, c->d_normal[0].get(), 12 * hw, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cost, c->d_cost.get(), 4 * hw, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AMVS_OK;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

// The end of every upload of a view's gray image (queued on the stream): its packed 8-bit map and losslessness test
// (read back lazily, usable_pairs), its pose; its window statistics are stale.  `sync`: host buffers of the upload
// are the caller's again on return (a device buffer is only ordered on the stream).
static int view_uploaded(amvs_ctx *c, int view, const float R[9], const float t[3], bool sync)
{
    HIPCHK(c, hipMemsetAsync(c->d_flag.get() + view, 0, sizeof(int), c->stream));
    HIPCHK(c, amvs::launch_pack_pairs(c->d_images.get() + view * c->stride, c->H, c->W,
                                      c->d_pairs.get() + view * c->pstride, c->d_flag.get() + view, c->stream));
    c->flags_dirty = true;
    if (sync) HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(c->R[view].data(), R, 36);
    std::memcpy(c->t[view].data(), t, 12);
    c->have[view] = 1;
    for (auto &kv : c->stats) if (!kv.second.done.empty()) kv.second.done[view] = 0;
    for (auto &kv : c->fstats) if (!kv.second.done.empty()) kv.second.done[view] = 0;
    return AMVS_OK;
}

static int set_view_common(amvs_ctx *c, int view, const void *gray, const float R[9], const float t[3],
                           hipMemcpyKind kind)
{
    if (c) c->pm_resumable = false;             // new images / poses: a sweep cannot be continued across them
    if (!c) return AMVS_EINVAL;
    if (view < 0 || view >= c->n_views || !gray || !R || !t) return fail(c, AMVS_EINVAL, "bad view argument");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_images.get() + view * c->stride, gray, sizeof(float) * c->H * c->W, kind,
                             c->stream));
    c->have_bgr[view] = 0;
    if ((rc = view_uploaded(c, view, R, t, kind == hipMemcpyHostToDevice))) return rc;
    return checked(c, AMVS_OK);
}

// OpenCV's linear-resize tables for one axis (resize.cpp, resizeGeneric_ setup, ksize = 2): float32
// arithmetic as there; cvRound = round half to even
static void resize_axis_tables(int n_dst, int n_src, std::vector<int> &ofs, std::vector<short> &w, bool clamp_ofs)
{
    const double scale = 1.0 / ((double)n_dst / (double)n_src);
    ofs.resize(n_dst); w.resize(2 * (size_t)n_dst);
    for (int d = 0; d < n_dst; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= (float)s;
        if (clamp_ofs) {                       // columns: taps clamped into the image, weight zeroed
            if (s < 0) { f = 0.f; s = 0; }
            if (s >= n_src - 1) { f = 0.f; s = n_src - 1; }
        }
        ofs[d] = s;                            // rows: the kernel clamps the two row indices, weights stay
        const float c0 = 1.f - f, c1 = f;
        w[2 * d] = (short)std::nearbyint(c0 * 2048.f);
        w[2 * d + 1] = (short)std::nearbyint(c1 * 2048.f);
    }
}

// The lens of include/amvs_lens.h as the kernel takes it: K and k1, k2, p1, p2, k3, k4, k5, k6 (absent ones 0).
struct Lens {
    double K[9], dist8[8];
};

// the header's "Errors": NULL = fine (lens filled), else what is wrong
static const char *lens_arguments(int h, int w, const double *K, const double *dist, int n_dist, Lens &lens)
{
    if (!K || !dist) return "NULL K / dist";
    if (h < 1 || w < 1 || h > (1 << 24) || w > (1 << 24)) return "image side outside 1 .. 2^24";
    if (n_dist != 4 && n_dist != 5 && n_dist != 8) return "n_dist must be 4, 5 or 8";
    for (int k = 0; k < 9; ++k) if (!std::isfinite(K[k])) return "K is not finite";
    for (int k = 0; k < n_dist; ++k) if (!std::isfinite(dist[k])) return "a distortion coefficient is not finite";
    if (!(K[0] > 0.0) || !(K[4] > 0.0)) return "fx and fy must be positive";
    if (K[1] != 0.0 || K[3] != 0.0 || K[6] != 0.0 || K[7] != 0.0 || K[8] != 1.0) return "K must be [fx 0 cx; 0 fy cy; 0 0 1]";
    std::memcpy(lens.K, K, sizeof(lens.K));
    for (int k = 0; k < 8; ++k) lens.dist8[k] = k < n_dist ? dist[k] : 0.0;
    return nullptr;
}

// amvs_set_view_bgr8, and with `lens` amvs_set_view_bgr8_undistorted: the same copies and launches in the same order, with
// the undistortion of the staged source (into d_prep_undist, which the resize then reads) behind its upload.
static int set_view_bgr8(amvs_ctx *c, int view, const uint8_t *bgr_host, int src_h, int src_w, const Lens *lens, const float R[9],
                         const float t[3], uint8_t *scaled_bgr_out)
{
    int rc = bind_device(c);
    if (rc) return rc;
    const size_t n_src = (size_t)src_h * src_w, n_dst = (size_t)c->H * c->W;
    std::vector<int> xofs, yofs;
    std::vector<short> ialpha, ibeta;
    resize_axis_tables(c->W, src_w, xofs, ialpha, true);
    resize_axis_tables(c->H, src_h, yofs, ibeta, false);
    // the prepared colour image stays on the device (the fusion reads it there: amvs_fuse_filter_views)
    HIPCHK(c, c->d_bgr.reserve(3 * n_dst * (size_t)c->n_views, c->cache));
    unsigned char *d_scaled = c->d_bgr.get() + 3 * n_dst * (size_t)view;
    // tables: xofs [W], yofs [H] ints, then ialpha [2W], ibeta [2H] shorts
    const size_t tab_ints = (size_t)c->W + c->H, tab_shorts = 2 * ((size_t)c->W + c->H);
    HIPCHK(c, c->d_prep_src.reserve(3 * n_src, c->cache));
    HIPCHK(c, c->d_prep_tab.reserve(tab_ints + tab_shorts / 2, c->cache));
    unsigned char *d_src = c->d_prep_src.get();
    int *d_xofs = c->d_prep_tab.get(), *d_yofs = d_xofs + c->W;
    short *d_ialpha = (short *)(d_xofs + tab_ints), *d_ibeta = d_ialpha + 2 * c->W;
    HIPCHK(c, hipMemcpyAsync(d_src, bgr_host, 3 * n_src, hipMemcpyHostToDevice, c->stream));
    if (lens) {
        HIPCHK(c, c->d_prep_undist.reserve(3 * n_src, c->cache));
        HIPCHK(c, amvs::launch_undistort_bgr8(d_src, src_h, src_w, lens->K, lens->dist8, c->d_prep_undist.get(), nullptr, c->stream));
        d_src = c->d_prep_undist.get();
    }
    HIPCHK(c, hipMemcpyAsync(d_xofs, xofs.data(), 4 * (size_t)c->W, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_yofs, yofs.data(), 4 * (size_t)c->H, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_ialpha, ialpha.data(), 4 * (size_t)c->W, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_ibeta, ibeta.data(), 4 * (size_t)c->H, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, amvs::launch_prep_bgr8(d_src, src_h, src_w, c->H, c->W, d_xofs, d_ialpha, d_yofs, d_ibeta, d_scaled,
                                     c->d_images.get() + view * c->stride, c->stream));
    if (scaled_bgr_out) HIPCHK(c, hipMemcpyAsync(scaled_bgr_out, d_scaled, 3 * n_dst, hipMemcpyDeviceToHost, c->stream));
    if ((rc = view_uploaded(c, view, R, t, true))) return rc;
    c->have_bgr[view] = 1;
    return checked(c, AMVS_OK);
}

int amvs_set_view_bgr8(amvs_ctx *c, int view, const uint8_t *bgr_host, int src_h, int src_w, const float R[9],
                       const float t[3], uint8_t *scaled_bgr_out)
{
    if (c) c->pm_resumable = false;
    if (!c) return AMVS_EINVAL;
    if (view < 0 || view >= c->n_views || !bgr_host || !R || !t || src_h < 1 || src_w < 1)
        return fail(c, AMVS_EINVAL, "bad view argument");
    return set_view_bgr8(c, view, bgr_host, src_h, src_w, nullptr, R, t, scaled_bgr_out);
}

int amvs_set_view_bgr8_undistorted(amvs_ctx *c, int view, const uint8_t *bgr_host, int src_h, int src_w, const double K_src[9],
                                   const double *dist, int n_dist, const float R[9], const float t[3], uint8_t *scaled_bgr_out)
{
    if (c) c->pm_resumable = false;
    if (!c) return AMVS_EINVAL;
    if (view < 0 || view >= c->n_views || !bgr_host || !R || !t) return fail(c, AMVS_EINVAL, "bad view argument");
    Lens lens;
    if (const char *bad = lens_arguments(src_h, src_w, K_src, dist, n_dist, lens)) return fail(c, AMVS_EINVAL, bad);
    return set_view_bgr8(c, view, bgr_host, src_h, src_w, &lens, R, t, scaled_bgr_out);
}

int amvs_undistort_bgr8(amvs_ctx *c, const uint8_t *bgr_host, int h, int w, const double K[9], const double *dist, int n_dist,
                        uint8_t *out_host, int64_t *n_outside)
{
    if (!c) return AMVS_EINVAL;
    if (!bgr_host || !out_host) return fail(c, AMVS_EINVAL, "NULL image");
    Lens lens;
    if (const char *bad = lens_arguments(h, w, K, dist, n_dist, lens)) return fail(c, AMVS_EINVAL, bad);
    int rc = bind_device(c);
    if (rc) return rc;
    const size_t bytes = 3 * (size_t)h * (size_t)w;
    HIPCHK(c, c->d_prep_src.reserve(bytes, c->cache));
    HIPCHK(c, c->d_prep_undist.reserve(bytes, c->cache));
    amvs::ScratchCache::Lease counter;
    if (n_outside) HIPCHK(c, c->cache.lease(counter, sizeof(unsigned long long)));
    // amvs_get_timing after this call: init_ms = the upload (and the counter's reset), sweep_ms = the kernel,
    // confidence_ms = the download (as amvs_plane_sweep_device fills the same three)
    resolve_timing(c);
    c->timing = amvs_timing{};
    c->timing_groups = 0;
    c->n_step_events = 0;
    HIPCHK(c, hipEventRecord(c->ev[0].get(), c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_prep_src.get(), bgr_host, bytes, hipMemcpyHostToDevice, c->stream));
    if (n_outside) HIPCHK(c, hipMemsetAsync(counter.get(), 0, sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipEventRecord(c->ev[1].get(), c->stream));
    HIPCHK(c, amvs::launch_undistort_bgr8(c->d_prep_src.get(), h, w, lens.K, lens.dist8, c->d_prep_undist.get(),
                                          counter.get<unsigned long long>(), c->stream));
    HIPCHK(c, hipEventRecord(c->ev[2].get(), c->stream));
    HIPCHK(c, hipMemcpyAsync(out_host, c->d_prep_undist.get(), bytes, hipMemcpyDeviceToHost, c->stream));
    unsigned long long outside = 0;
    if (n_outside) HIPCHK(c, hipMemcpyAsync(&outside, counter.get(), sizeof(outside), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[3].get(), c->stream));
    c->timing.sweep_launches = 1;
    c->timing_pending = true;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_timing(c);
    if (n_outside) *n_outside = (int64_t)outside;
    return checked(c, AMVS_OK);
}

int amvs_set_view_colors(amvs_ctx *c, int view, const uint8_t *bgr_host)
{
    if (!c) return AMVS_EINVAL;
    if (view < 0 || view >= c->n_views || !bgr_host) return fail(c, AMVS_EINVAL, "bad view argument");
    int rc = bind_device(c);
    if (rc) return rc;
    const size_t n = (size_t)c->H * c->W;
    HIPCHK(c, c->d_bgr.reserve(3 * n * (size_t)c->n_views, c->cache));
    HIPCHK(c, hipMemcpyAsync(c->d_bgr.get() + 3 * n * (size_t)view, bgr_host, 3 * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_bgr[view] = 1;
    return checked(c, AMVS_OK);
}

int amvs_set_view(amvs_ctx *c, int view, const float *gray_host, const float R[9], const float t[3])
{
    return set_view_common(c, view, gray_host, R, t, hipMemcpyHostToDevice);
}

int amvs_set_view_device(amvs_ctx *c, int view, const void *gray_device, const float R[9], const float t[3])
{
    return set_view_common(c, view, gray_device, R, t, hipMemcpyDeviceToDevice);
}

// The sweep of a batch: state in the context's buffers (final tagged depth in d_depth[*cur], normals
// in d_normal[0 / 1] as the tags say), confidence into `conf_dev` (NULL: the context's d_aux).
static int patchmatch_core(amvs_ctx *c, int n_ref, const int *ref_ids, const int *src_ids, int n_src,
                           const amvs_pm_params *p, uint64_t seed, void *conf_dev, int *cur_out)
{
    if (!p || !ref_ids || !src_ids || n_ref <= 0) return fail(c, AMVS_EINVAL, "NULL argument / empty batch");
    if (p->num_iterations < 0 || p->num_samples < 0) return fail(c, AMVS_EINVAL, "negative iteration count");
    // (the reference takes log(depth_min), mvs_patchmatch.py:269; the state maps use the depths' sign bit)
    if (!(p->depth_min > 0.0f) || !(p->depth_max >= p->depth_min)) return fail(c, AMVS_EINVAL, "need 0 < depth_min <= depth_max");
    int rc = bind_device(c);
    if (rc) return rc;
    if ((rc = check_patch_src(c, p->patch_size, n_src))) return rc;
    if ((rc = ensure_slots(c, n_ref))) return rc;
    int fast = 0;
    if ((rc = resolve_fast(c, p->mode, &fast))) return rc;
    // (the (mean1, var1) maps only if the steps of this call read them)
    if ((rc = upload_jobs(c, n_ref, ref_ids, src_ids, n_src, fast ? p->patch_size : 0, false, !step_regs(c, p->patch_size).stats)))
        return rc;

    const size_t hw = (size_t)c->H * c->W;
    if (p->schedule < 0 || p->schedule > AMVS_SCHEDULE_PAIRED) return fail(c, AMVS_EINVAL, "unknown schedule");
    if (p->schedule == AMVS_SCHEDULE_SPLIT && !fast)
        return fail(c, AMVS_EUNSUPPORTED, "the split schedule exists in fast mode only");
    if (p->schedule == AMVS_SCHEDULE_SPLIT && !amvs::patch_compiled(p->patch_size))
        return fail(c, AMVS_EUNSUPPORTED, "the split schedule exists for the compiled patch sizes (3 ... 29) only");
    // Continuation: iterations first_iteration .. of a sweep whose earlier iterations a previous call ran
    // on the same batch; the state maps stay in the context between the calls.
    if (p->first_iteration < 0) return fail(c, AMVS_EINVAL, "negative first_iteration");
    uint64_t key = 1469598103934665603ull;
    auto mix = [&key](uint64_t v) { key = (key ^ v) * 1099511628211ull; };
    mix((uint64_t)n_ref); mix((uint64_t)n_src); mix((uint64_t)p->patch_size); mix((uint64_t)p->num_samples); mix(seed);
    mix((uint64_t)fast); mix((uint64_t)__builtin_bit_cast(uint32_t, p->depth_min)); mix((uint64_t)__builtin_bit_cast(uint32_t, p->depth_max));
    for (int i = 0; i < n_ref; ++i) mix((uint64_t)(uint32_t)ref_ids[i]);
    for (int i = 0; i < n_ref * n_src; ++i) mix((uint64_t)(uint32_t)src_ids[i]);
    const bool resume = p->first_iteration > 0;
    if (resume) {
        if (p->schedule == AMVS_SCHEDULE_SPLIT) return fail(c, AMVS_EUNSUPPORTED, "the split schedule cannot resume a sweep");
        if (!c->pm_resumable || c->pm_key != key || c->pm_next_iteration != p->first_iteration)
            return fail(c, AMVS_EINVAL, "first_iteration > 0 continues the previous call: same batch, sources, patch, samples, "
                                        "seed and depth range, and first_iteration = the iterations already run");
    }
    c->pm_resumable = false;
    resolve_timing(c);
    c->timing = amvs_timing{};
    HIPCHK(c, hipEventRecord(c->ev[0].get(), c->stream));
    // the launch plan (amvs_launch_plan.h): every decision of the call; the two schedules below only issue it
    const bool packed = usable_pairs(c) != nullptr;
    const PmPlan plan = amvs::plan::plan_patchmatch(
        plan_device(c, packed), amvs::plan::Call{n_ref, n_src, fast, *p}, c->tuning,
        plan_facts(p->patch_size, n_src, fast != 0, packed, amvs::plan::waves_entries_read(c->tuning, *p)));
    c->last_tile_rows = plan.last_tile_rows;
    const int cur0 = resume ? c->pm_cur : 0;
    const int cur = cur0 ^ plan.final_parity;                                     // final depth buffer
    if (p->schedule == AMVS_SCHEDULE_SPLIT) {
        if ((rc = run_split_schedule(c, n_ref, n_src, p, seed, plan, conf_dev))) return rc;
    } else {
        if ((rc = run_fused_schedule(c, n_src, p, seed, fast, plan, conf_dev, cur0, !resume,
                                     (p->flags & AMVS_PM_NO_CONFIDENCE) == 0))) return rc;
        c->pm_resumable = true; c->pm_cur = cur; c->pm_key = key;
        c->pm_next_iteration = p->first_iteration + p->num_iterations;
    }
    c->timing.sweep_launches = plan.launches;
    c->last_views_per_launch = plan.views_per_launch;
    // every group ran the same schedule, so the final depth buffer is the same for all
    HIPCHK(c, hipEventRecord(c->ev[3].get(), c->stream));
    *cur_out = cur;
    c->timing.pixel_hypotheses =
        (int64_t)n_ref * (int64_t)hw * p->num_iterations * (2 + p->num_samples);
    c->timing_pending = true;
    return AMVS_OK;
}

int amvs_patchmatch_device(amvs_ctx *c, int n_ref, const int *ref_ids, const int *src_ids, int n_src,
                           const amvs_pm_params *p, uint64_t seed, void *depth_dev, void *normal_dev,
                           void *conf_dev)
{
    if (!c) return AMVS_EINVAL;
    if (!depth_dev || !normal_dev || !conf_dev) return fail(c, AMVS_EINVAL, "NULL output");
    int cur = 0;
    int rc = patchmatch_core(c, n_ref, ref_ids, src_ids, n_src, p, seed, conf_dev, &cur);
    if (rc) return rc;
    const size_t hw = (size_t)c->H * c->W;
    // untagged depths and the current normal of every pixel straight into the caller's arrays
    HIPCHK(c, amvs::launch_resolve_state(c->d_jobs.get(), n_ref, (long long)hw, c->d_depth[cur].get(), c->d_normal[0].get(), c->d_normal[1].get(),
                                         (float *)depth_dev, (float *)normal_dev, 0, c->stream));
    return AMVS_OK;
}

// Host-buffer entry: the maps go from the context's own state buffers straight to the caller's
// arrays -- no per-call device allocation, one synchronisation.
int amvs_patchmatch(amvs_ctx *c, int n_ref, const int *ref_ids, const int *src_ids, int n_src,
                    const amvs_pm_params *p, uint64_t seed, float *depth_out, float *normal_out,
                    float *conf_out)
{
    if (!c) return AMVS_EINVAL;
    if (!depth_out || !normal_out || !conf_out || n_ref <= 0) return fail(c, AMVS_EINVAL, "NULL output");
    int cur = 0;
    int rc = patchmatch_core(c, n_ref, ref_ids, src_ids, n_src, p, seed, nullptr, &cur);
    if (rc) return rc;
    const size_t hw = (size_t)c->H * c->W;
    HIPCHK(c, amvs::launch_resolve_state(c->d_jobs.get(), n_ref, (long long)hw, c->d_depth[cur].get(), c->d_normal[0].get(), c->d_normal[1].get(),
                                         nullptr, nullptr, 0, c->stream));
    HIPCHK(c, hipMemcpyAsync(depth_out, c->d_depth[cur].get(), 4 * hw * n_ref, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(normal_out, c->d_normal[0].get(), 12 * hw * n_ref, hipMemcpyDeviceToHost, c->stream));
    if ((p->flags & AMVS_PM_NO_CONFIDENCE) == 0)
        HIPCHK(c, hipMemcpyAsync(conf_out, c->d_aux.get(), 4 * hw * n_ref, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_timing(c);
    return checked(c, AMVS_OK);
}

int amvs_set_split_tuning(amvs_ctx *c, int groups, int sample_rows, int sample_lds_bytes)
{
    if (!c) return AMVS_EINVAL;
    if (groups < 0 || groups > 8 || sample_rows < 0 || sample_lds_bytes < 0 || sample_lds_bytes > 64 * 1024)
        return fail(c, AMVS_EINVAL, "split tuning out of range");
    c->tuning.split_groups = groups; c->tuning.split_sample_rows = sample_rows; c->tuning.split_sample_lds = sample_lds_bytes;
    return AMVS_OK;
}

int amvs_set_step_tuning(amvs_ctx *c, int n_iterations, const int32_t *tile_rows, const int32_t *wgs_per_cu)
{
    if (!c) return AMVS_EINVAL;
    if (n_iterations < 0 || (n_iterations > 0 && !tile_rows && !wgs_per_cu)) return fail(c, AMVS_EINVAL, "bad step tuning table");
    c->tuning.tune_rows.clear(); c->tuning.tune_cap.clear();
    for (int i = 0; i < 2 * n_iterations; ++i) {
        const int r = tile_rows ? tile_rows[i] : 0, w = wgs_per_cu ? wgs_per_cu[i] : 0;
        if (r < 0 || r > (1 << 20) || w < 0 || w > 8) {
            c->tuning.tune_rows.clear(); c->tuning.tune_cap.clear();
            return fail(c, AMVS_EINVAL, "step tuning: rows >= 0, workgroups per CU in 0..8");
        }
        c->tuning.tune_rows.push_back(r); c->tuning.tune_cap.push_back(w);
    }
    return AMVS_OK;
}

int amvs_set_launch_order(amvs_ctx *c, int edge_first, int group_overlap)
{
    if (!c) return AMVS_EINVAL;
    if (edge_first < -1 || edge_first > 1 || group_overlap < -1 || group_overlap > 2)
        return fail(c, AMVS_EINVAL, "launch order: edge_first in -1..1, group_overlap in -1..2");
    c->tuning.edge_first = edge_first < 0 ? AMVS_DEFAULT_EDGE_FIRST : edge_first;
    c->tuning.group_overlap = group_overlap < 0 ? AMVS_DEFAULT_GROUP_OVERLAP : group_overlap;
    return AMVS_OK;
}

int amvs_set_step_sources(amvs_ctx *c, int ref_stats, int centre_depth)
{
    if (!c) return AMVS_EINVAL;
    if (ref_stats < -1 || ref_stats > 1 || centre_depth < -1 || centre_depth > 1)
        return fail(c, AMVS_EINVAL, "step sources: ref_stats and centre_depth in -1..1");
    c->tuning.ref_stats_source = ref_stats < 0 ? AMVS_DEFAULT_REF_STATS_SOURCE : ref_stats;
    c->tuning.depth_source = centre_depth < 0 ? AMVS_DEFAULT_DEPTH_SOURCE : centre_depth;
    return AMVS_OK;
}

int amvs_get_step_sources(amvs_ctx *c, int patch_size, int *ref_stats, int *centre_depth)
{
    if (!c) return AMVS_EINVAL;
    if (!ref_stats || !centre_depth) return fail(c, AMVS_EINVAL, "step sources: NULL output");
    const StepRegs regs = step_regs(c, patch_size);
    *ref_stats = regs.stats ? 1 : 0;
    *centre_depth = regs.hist ? 1 : 0;
    return AMVS_OK;
}

int amvs_step_sources_max_patch(void) { return amvs::step_fast_regs_max_patch(); }

int amvs_sweep_order(int n_jobs, int tiles_x, int tiles_y, int band_major, int paired, int edge_first,
                     int64_t capacity, int32_t *out, int32_t *n_blocks)
{
    if (n_jobs < 1 || tiles_x < 1 || tiles_y < 1 || !n_blocks || (capacity > 0 && !out)) return AMVS_EINVAL;
    if ((long long)n_jobs * tiles_x * tiles_y > (1ll << 28)) return AMVS_EINVAL;
    const int waves = amvs::step_wg_waves(paired != 0);
    const int nblk = amvs::step_grid_blocks(n_jobs, tiles_x, tiles_y, paired != 0);
    *n_blocks = nblk;
    for (int bid = 0; bid < nblk; ++bid)
        for (int wv = 0; wv < waves; ++wv) {
            const int64_t o = 5 * ((int64_t)bid * waves + wv);
            if (o + 5 > capacity) return AMVS_OK;
            amvs::StripPos sp{};
            const bool live = amvs::strip_decode_host(n_jobs, tiles_x, tiles_y, band_major, paired != 0, edge_first, bid, nblk, wv, sp);
            out[o] = live ? sp.job : -1; out[o + 1] = live ? sp.ty : -1; out[o + 2] = live ? sp.tx : -1;
            out[o + 3] = live ? sp.up : -1; out[o + 4] = live ? sp.paired : -1;
        }
    return AMVS_OK;
}

int amvs_plan_patchmatch(const amvs_plan_device *dev, const amvs_plan_call *call, const amvs_plan_tuning *tuning,
                         const amvs_plan_facts *facts, amvs_pm_plan *out, amvs_plan_step *steps, int32_t capacity)
{
    if (!dev || !call || !tuning || !facts || !out || (capacity > 0 && !steps)) return AMVS_EINVAL;
    const amvs_pm_params &p = call->p;
    if (dev->H < 1 || dev->W < 1 || dev->n_cu < 1 || call->n_ref < 1 || facts->out_width < 1 || p.num_iterations < 0 ||
        p.num_iterations > (1 << 16) || p.num_samples < 0 || p.num_samples > (1 << 10) || p.first_iteration < 0 || p.schedule < 0 ||
        p.schedule > AMVS_SCHEDULE_PAIRED || tuning->n_tune < 0)
        return AMVS_EINVAL;
    for (int i = 0; i < tuning->n_tune; ++i)
        if (tuning->tune_cap && (tuning->tune_cap[i] < 0 || tuning->tune_cap[i] > 8)) return AMVS_EINVAL;
    const amvs::plan::SweepTuning t = plan_tuning(*tuning);
    const unsigned read = amvs::plan::waves_entries_read(t, p);
    for (int w = 0; w <= 8; ++w)
        if ((read >> w & 1u) && facts->waves_per_cu[w] < 1) return AMVS_EINVAL;
    const PmPlan plan = amvs::plan::plan_patchmatch(*dev, *call, t, *facts);
    const amvs::plan::SplitPlan &sp = plan.split;
    const StepRegs regs = amvs::plan::step_regs(t, facts->fast_regs_supported != 0, p.patch_size);
    *out = amvs_pm_plan{plan.band_major, plan.paired, plan.views_per_launch, (int32_t)plan.groups.size(), plan.TH, plan.tiles_x, plan.tiles_y,
                        plan.overlap, plan.edge_first, (int32_t)plan.steps.size(), plan.final_parity, plan.last_tile_rows, plan.launches,
                        (int32_t)sp.groups.size(), sp.vpl, sp.TH, sp.s_TH, sp.s_lds, sp.s_tiles_x, sp.s_tiles_y, regs.stats, regs.hist,
                        facts->waves_per_cu[0] >= 1 ? amvs::plan::single_step_rows(*dev, *facts, p.patch_size) : 0};
    for (size_t i = 0; i < plan.steps.size() && (int64_t)i < capacity; ++i) steps[i] = plan.steps[i];
    return AMVS_OK;
}

int amvs_fetch_step_trace(amvs_ctx *c, uint64_t *out, int64_t capacity, int64_t *n_launches, int64_t *blocks_per_launch)
{
    if (!c) return AMVS_EINVAL;
    if (!n_launches || !blocks_per_launch || (capacity > 0 && !out)) return fail(c, AMVS_EINVAL, "NULL argument");
    int rc = bind_device(c);
    if (rc) return rc;
    *n_launches = c->trace_launches; *blocks_per_launch = c->trace_stride;
    const int64_t n = 4 * c->trace_launches * c->trace_stride;
    if (n == 0 || capacity < n) return AMVS_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->d_trace.get(), sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost));
    return AMVS_OK;
}

int amvs_set_step_timing(amvs_ctx *c, int enable)
{
    if (!c) return AMVS_EINVAL;
    c->step_timing = enable != 0;
    c->n_step_events = 0;
    return AMVS_OK;
}

int amvs_get_step_times(amvs_ctx *c, float *ms_out, int capacity, int *n_out)
{
    if (!c) return AMVS_EINVAL;
    if (!n_out || (capacity > 0 && !ms_out)) return fail(c, AMVS_EINVAL, "NULL argument");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // events: per view group one start event followed by one per launch
    const int groups = c->timing_groups > 0 ? c->timing_groups : 1;
    const int per_group = c->n_step_events / groups;          // 1 + launches
    int n = 0;
    for (int g = 0; g < groups && per_group > 1; ++g)
        for (int i = 1; i < per_group; ++i, ++n) {
            if (n >= capacity) continue;
            float ms = 0.f;
            HIPCHK(c, hipEventElapsedTime(&ms, c->ev_steps[g * per_group + i - 1], c->ev_steps[g * per_group + i]));
            ms_out[n] = ms;
        }
    *n_out = n;
    return AMVS_OK;
}

int amvs_last_tile_rows(const amvs_ctx *c) { return c ? c->last_tile_rows : 0; }

int amvs_last_views_per_launch(const amvs_ctx *c) { return c ? c->last_views_per_launch : 0; }

int amvs_eval_cost(amvs_ctx *c, int ref, const int *src_ids, int n_src, int patch_size,
                   const float *depth_in, float *cost_out)
{
    OneStep o;
    int rc = one_step_begin(c, ref, src_ids, n_src, patch_size, o);
    if (rc) return rc;
    if (!depth_in || !cost_out) return fail(c, AMVS_EINVAL, "NULL argument");
    if ((rc = upload_state(c, o.hw, depth_in, nullptr, nullptr))) return rc;
    o.a.mode = amvs::MODE_EVAL;
    HIPCHK(c, amvs::launch_step(patch_size, n_src, o.a, c->stream));
    HIPCHK(c, hipMemcpyAsync(cost_out, c->d_aux.get(), 4 * o.hw, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return checked(c, AMVS_OK);
}

int amvs_sample_sources(amvs_ctx *c, int ref, const int *src_ids, int n_src, int patch_size, int bounds,
                        const float *depth_in, float *sampled_out, uint8_t *valid_out)
{
    OneStep o;
    int rc = one_step_begin(c, ref, src_ids, n_src, patch_size, o);
    if (rc) return rc;
    if (!depth_in || !sampled_out || !valid_out || bounds < 0 || bounds > 2) return fail(c, AMVS_EINVAL, "bad argument");
    if ((rc = upload_state(c, o.hw, depth_in, nullptr, nullptr))) return rc;
    amvs::DeviceBuffer<float> ds;
    amvs::DeviceBuffer<unsigned char> dv;
    HIPCHK(c, ds.reserve(o.hw * n_src, c->cache));
    HIPCHK(c, dv.reserve(o.hw, c->cache));
    o.a.TH = patch_size / 2;
    o.a.mode = bounds == 0 ? amvs::MODE_EVAL : (bounds == 1 ? amvs::MODE_CONF : amvs::MODE_EVAL + 100);
    HIPCHK(c, amvs::launch_sample_dump(n_src, o.a, ds.get(), dv.get(), c->stream));
    HIPCHK(c, hipMemcpyAsync(sampled_out, ds.get(), 4 * o.hw * n_src, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(valid_out, dv.get(), o.hw, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return checked(c, AMVS_OK);
}

int amvs_confidence(amvs_ctx *c, int ref, const int *src_ids, int n_src, int patch_size,
                    const float *depth_in, float *conf_out)
{
    OneStep o;
    int rc = one_step_begin(c, ref, src_ids, n_src, patch_size, o);
    if (rc) return rc;
    if (!depth_in || !conf_out) return fail(c, AMVS_EINVAL, "NULL argument");
    if ((rc = upload_state(c, o.hw, depth_in, nullptr, nullptr))) return rc;
    o.a.mode = amvs::MODE_CONF;
    set_io(o.a, c, 0, false);
    HIPCHK(c, amvs::launch_step(patch_size, n_src, o.a, c->stream));
    HIPCHK(c, hipMemcpyAsync(conf_out, c->d_aux.get(), 4 * o.hw, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return checked(c, AMVS_OK);
}

int amvs_propagate_step(amvs_ctx *c, int ref, const int *src_ids, int n_src, int patch_size, float *depth,
                        float *normal, float *cost, int oy, int ox, float depth_min)
{
    OneStep o;
    int rc = one_step_begin(c, ref, src_ids, n_src, patch_size, o);
    if (rc) return rc;
    if (!depth || !normal || !cost) return fail(c, AMVS_EINVAL, "NULL argument");
    if ((rc = upload_state(c, o.hw, depth, normal, cost))) return rc;
    o.a.mode = amvs::MODE_PROP;
    set_io(o.a, c, 0);
    o.a.oy = oy; o.a.ox = ox; o.a.depth_min = depth_min;
    HIPCHK(c, amvs::launch_step(patch_size, n_src, o.a, c->stream));
    return checked(c, download_state(c, o.hw, 1, depth, normal, cost));
}

int amvs_refine_step(amvs_ctx *c, int ref, const int *src_ids, int n_src, int patch_size, float *depth,
                     float *normal, float *cost, uint64_t seed, uint32_t stream_view, uint32_t draw,
                     float depth_range, float normal_range, float depth_min, float depth_max)
{
    OneStep o;
    int rc = one_step_begin(c, ref, src_ids, n_src, patch_size, o);
    if (rc) return rc;
    if (!depth || !normal || !cost) return fail(c, AMVS_EINVAL, "NULL argument");
    if ((rc = upload_state(c, o.hw, depth, normal, cost))) return rc;
    // the job's RNG stream defaults to the reference view; tests may address another stream
    HIPCHK(c, hipMemcpyAsync(&c->d_jobs.get()->stream_view, &stream_view, sizeof(uint32_t),
                             hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    o.a.mode = amvs::MODE_REFINE;
    set_io(o.a, c, 0);
    o.a.seed = seed; o.a.draw = draw;
    o.a.depth_range = depth_range; o.a.normal_range = normal_range;
    o.a.depth_min = depth_min; o.a.depth_max = depth_max;
    HIPCHK(c, amvs::launch_step(patch_size, n_src, o.a, c->stream));
    return checked(c, download_state(c, o.hw, 1, depth, normal, cost));
}

int amvs_init_state(amvs_ctx *c, uint64_t seed, uint32_t stream_view, float log_depth_scale,
                    float log_depth_min, float *depth, float *normal, float *cost)
{
    if (!c) return AMVS_EINVAL;
    if (!depth || !normal || !cost) return fail(c, AMVS_EINVAL, "NULL argument");
    int rc = bind_device(c);
    if (rc) return rc;
    c->pm_resumable = false;
    if ((rc = ensure_slots(c, 1))) return rc;
    HIPCHK(c, c->d_jobs.reserve(1, c->cache));
    amvs::Job j;
    std::memset(&j, 0, sizeof(j));
    j.stream_view = stream_view;
    HIPCHK(c, hipMemcpyAsync(c->d_jobs.get(), &j, sizeof(j), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t hw = (size_t)c->H * c->W;
    HIPCHK(c, amvs::launch_init(c->d_jobs.get(), 1, (long long)hw, seed, log_depth_scale, log_depth_min,
                                c->d_depth[0].get(), c->d_normal[0].get(), c->d_cost.get(), c->stream));
    return checked(c, download_state(c, hw, 0, depth, normal, cost));
}

int amvs_box_stats(amvs_ctx *c, int view, int patch_size, float *mean_out, float *var_out)
{
    if (!c) return AMVS_EINVAL;
    if (view < 0 || view >= c->n_views || !c->have[view] || !mean_out || !var_out)
        return fail(c, AMVS_EINVAL, "bad view / NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    if (!amvs::patch_supported(patch_size)) return fail(c, AMVS_EUNSUPPORTED, "patch_size unsupported (odd sizes from 3 to 31)");
    if ((rc = ensure_stats(c, patch_size))) return rc;
    const Stats &s = c->stats.at(patch_size);
    const size_t hw = (size_t)c->H * c->W;
    HIPCHK(c, hipMemcpyAsync(mean_out, s.mean.get() + view * c->stride, 4 * hw, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(var_out, s.var.get() + view * c->stride, 4 * hw, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return checked(c, AMVS_OK);
}

int amvs_selftest_lean_math(amvs_ctx *c, uint64_t mismatches[2])
{
    if (!c || !mismatches) return AMVS_EINVAL;
    int rc = bind_device(c);
    if (rc) return rc;
    amvs::DeviceBuffer<unsigned long long> d;
    HIPCHK(c, d.reserve(2, c->cache));
    HIPCHK(c, hipMemsetAsync(d.get(), 0, 16, c->stream));
    HIPCHK(c, amvs::launch_lean_math_check(d.get(), c->stream));
    unsigned long long h[2] = {~0ull, ~0ull};
    HIPCHK(c, hipMemcpyAsync(h, d.get(), 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    mismatches[0] = h[0]; mismatches[1] = h[1];
    return checked(c, AMVS_OK);
}

int amvs_rng_fill(amvs_ctx *c, uint64_t seed, uint32_t stream_view, uint32_t draw, int64_t n, float *u_out,
                  float *n_out)
{
    if (!c) return AMVS_EINVAL;
    if (n < 0 || n > (1ll << 31)) return fail(c, AMVS_EINVAL, "bad n");
    int rc = bind_device(c);
    if (rc) return rc;
    amvs::DeviceBuffer<float> du, dn;
    if (u_out) HIPCHK(c, du.reserve(n ? n : 1, c->cache));
    if (n_out) HIPCHK(c, dn.reserve(3 * (size_t)(n ? n : 1), c->cache));
    HIPCHK(c, amvs::launch_rng_fill(seed, stream_view, draw, n, du.get(), dn.get(), c->stream));
    if (u_out) HIPCHK(c, hipMemcpyAsync(u_out, du.get(), 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (n_out) HIPCHK(c, hipMemcpyAsync(n_out, dn.get(), 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return checked(c, AMVS_OK);
}

}  // extern "C"
#pragma GCC visibility pop
