// amvs_capi.hip -- the C ABI of include/amvs.h: view upload and the PatchMatch step scheduling.
// (The context: amvs_context.hip; the other entry points: amvs_capi_*.hip, amvs_comm.hip.)
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

// Views swept together by one launch (the views of a batch are independent, mvs_patchmatch.py:104-123, so
// a batch can be swept in groups, each through the whole schedule).  Groups of FOUR views against the
// whole 16-view batch, measured on MI355X in round 3 (S=4, G px-hyp/s, automatic strip heights, one run
// per pair):
//     fast, 1080p:  k=3  52.0 / 49.3    k=5  46.2 / 45.0    k=7  42.1 / 41.6    k=9  36.4 / 38.3    k=11  33.8 / 35.4
//     fast, k=7:    2560x1440  36.4 / 38.8      3840x2160 (8 views: 4 / 8 per launch)  35.4 / 36.1
//     exact, 1080p, k=7:  37.0 / 38.2           fast, 1080p, k=7, 8-view rank shard:  42.2 / 40.0
// Four 1080p views are two generations of resident waves at 18-row strips and an XCD's L2 then serves the
// sources of 4 views instead of 16 (hit rate 0.81 against 0.69); a launch of two generations also has a
// relatively longer tail than one of six, which is what the wider images, the larger patches and the
// slower exact kernel lose more to than the L2 returns.  Hence groups of four exactly where they were
// measured to win, else the whole batch (capped so that the per-launch state stays in the low GB).
// Paired bands (round 3, later; bench.py, G px-hyp/s, groups of four / whole batch): 16 views 43.3 / 43.2,
// 8 views 44.2 / 42.3, k=5 47.2 / 45.9 -- the same rule holds.
int default_views_per_launch(const amvs_ctx *c, int n_ref, int patch, bool fast)
{
    if (fast && patch <= 7 && c->W <= 2048 && n_ref >= 8 && n_ref % 4 == 0) return 4;
    return n_ref < 32 ? n_ref : 32;
}

// Rows per wave strip.  A strip re-samples 2*(patch/2) halo rows, so tall strips waste less; two
// things pull the other way.  (1) The set of source rows the resident waves touch at once: measured
// on MI355X (S=4, 16 views 1080p; best strip height per patch size) k=3: 10-12 rows, k=5: 14-18, k=7:
// 20-26 (32: -3 %, 40+: -15 %), k=9: 24-32, k=11: 32-40, i.e. about 4k-4, and lower for wider images
// (8 views 4K, k=7: 12-16 rows best, 24: -6 %) -- that is the cap `tall`.  (2) Wave quantisation: the
// launch runs in generations of `slots` resident waves, and a last generation that is nearly empty
// costs as much as a full one.  Measured, k=7, 1080p, G px-hyp/s by (views per launch: strip rows):
// 16: 24 -> 40.2; 8: 24 / 20 / 16 / 12 -> 39.2 / 39.2 / 39.1 / 38.5; 4: 24 / 16 / 12 / 8 -> 36.7 / 38.4 /
// 39.9 / 37.5; 2: 24 / 16 / 12 / 8 -> 39.4 / 34.5 / 38.6 / 35.9; 1: 24 / 16 / 12 / 8 -> 26.5 / 29.0 / 35.3 / 29.1
// -- the winners are the heights whose wave count is just below a whole number of generations
// (or at least 3/4 of one).  Hence: among the heights up to `tall`, the best product of the last
// generation's fill and the strip's useful fraction rows / (rows + patch - 1).
// Paired bands (`paired`): a pair of bands samples 2 th + patch - 1 rows for 2 th output rows (an odd last
// band keeps the classic th + patch - 1), and the locality cap is lower -- measured, 16 views 1080p, k=7, ms
// per launch by band rows 12 / 14 / 16 / 18 / 20 / 22 / 24 / 27 / 30 / 36: 0.761 / 0.755 / 0.750 / 0.749 /
// 0.751 / 0.755 / 0.762 / 0.761 / 0.765 / 0.780 -> 3 * patch - 3; k=5 in groups of 4 views: 12 rows 47.2, 16 rows
// 44.0 G px-hyp/s; 2560x1440: 12 / 16 / 18 rows 40.5 / 41.1 / 41.3; 8 views 3840x2160: 38.5 / 38.4 / 38.2 (the
// reduction for wide images applies beyond 3072 columns only).
int pick_tile_rows(const amvs_ctx *c, int patch, int n_src, int n_jobs, int requested, int cap, bool fast = false,
                   int wg_cap = 0, bool paired = false)
{
    if (requested > 0) return requested < cap ? requested : cap;
    const int tiles_x = (c->W + amvs::strip_out_width(patch) - 1) / amvs::strip_out_width(patch);
    const long long slots = (long long)c->n_cu * (fast ? amvs::step_fast_waves_per_cu(patch, n_src, wg_cap)
                                                       : amvs::step_waves_per_cu(patch, n_src, usable_pairs(c) != nullptr, wg_cap));
    int tall = 4 * patch - 4 > 12 ? 4 * patch - 4 : 12;
    if (paired) tall = 3 * patch - 3 > 8 ? 3 * patch - 3 : 8;
    if (c->W > (paired ? 3072 : 2048)) tall = tall * 2 / 3 > 8 ? tall * 2 / 3 : 8;
    if (tall > cap) tall = cap;
    int best = tall < 8 ? tall : 8;
    double best_score = -1.0;
    for (int th = tall; th >= (tall < 8 ? tall : 8); th -= 2) {
        const double waves = (double)n_jobs * tiles_x * ((c->H + th - 1) / th);
        const double g = waves / (double)slots;
        const double fill = g > 1.0 ? g / std::ceil(g) : (g >= 0.75 ? 1.0 : g / 0.75);
        double useful = (double)th / (double)(th + patch - 1);
        if (paired) {
            const int bands = (c->H + th - 1) / th;
            const double sampled = (double)(bands / 2) * (2 * th + patch - 1) + (double)(bands % 2) * (th + patch - 1);
            useful = (double)c->H / sampled;
        }
        const double score = fill * useful;
        if (score > best_score + 1e-9) { best_score = score; best = th; }
    }
    return best;
}

// Band-major schedule (StepArgs::band_major): strip height such that ONE band of all views of the
// launch about fills an XCD's wave slots, i.e. every XCD walks its own band(s) of all views top to
// bottom in one generation of waves.  Few views: several adjacent bands per XCD.
int pick_band_rows(const amvs_ctx *c, int patch, int n_src, int n_jobs, bool fast)
{
    const int tiles_x = (c->W + amvs::strip_out_width(patch) - 1) / amvs::strip_out_width(patch);
    const long long slots_xcd = (long long)(c->n_cu / 8 > 0 ? c->n_cu / 8 : 1) *
                                (fast ? amvs::step_fast_waves_per_cu(patch, n_src)
                                      : amvs::step_waves_per_cu(patch, n_src, usable_pairs(c) != nullptr));
    const long long per_band = (long long)n_jobs * tiles_x;
    long long g = slots_xcd / per_band;             // bands resident together per XCD
    if (g < 1) g = 1;
    const long long bands = 8 * g;
    long long th = (c->H + bands - 1) / bands;
    const int min_th = 2 * patch > 8 ? 2 * patch : 8;
    if (th < min_th) th = min_th;
    return (int)th;
}

amvs::StepArgs base_args(const amvs_ctx *c, int patch, int n_jobs, int TH)
{
    amvs::StepArgs a{};
    a.H = c->H; a.W = c->W; a.TH = TH;
    a.tiles_x = (c->W + amvs::strip_out_width(patch) - 1) / amvs::strip_out_width(patch);
    a.tiles_y = (c->H + TH - 1) / TH;
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

// Launch shape of one sweep step.  The gathers of an early iteration are scattered over the whole
// depth range (every pixel perturbs its depth by up to depth_range / 2^it), those of a late one are
// coherent, so the best strip height / residency differ by iteration; measured table: DESIGN.md
// section 5 (round 3).  An explicit amvs_pm_params.tile_rows, then amvs_set_step_tuning, override it.
struct StepShape { int rows, wg_cap; };

StepShape step_shape(const amvs_ctx *c, const amvs_pm_params *p, int n_src, int n_jobs, int iter, bool refine, bool fast,
                     int default_rows)
{
    StepShape s{default_rows, 0};
    const size_t idx = (size_t)2 * (size_t)iter + (refine ? 1 : 0);
    const size_t last = c->tune_rows.size() >= 2 ? c->tune_rows.size() - 2 + (refine ? 1 : 0) : 0;
    int rows = 0, cap = 0;
    if (!c->tune_rows.empty()) rows = c->tune_rows[idx < c->tune_rows.size() ? idx : last];
    if (!c->tune_cap.empty()) cap = c->tune_cap[idx < c->tune_cap.size() ? idx : last];
    if (cap > 0) s.wg_cap = cap;
    if (p->tile_rows > 0) return s;                       // the caller fixed the strip height
    if (rows > 0) s.rows = rows;
    else if (cap > 0) s.rows = pick_tile_rows(c, p->patch_size, n_src, n_jobs, 0, 1 << 20, fast, cap);
    return s;
}

// The sweep schedule of one PatchMatch call as a list of launches (the same for every view).
struct SchedStep {
    int mode, oy, ox;
    float depth_range, normal_range;
    unsigned draw;
    int flip_d;                          // depth buffers ping-ponged by the step (set_io)
    int iter;
};

std::vector<SchedStep> build_schedule(const amvs_pm_params *p)
{
    std::vector<SchedStep> v;
    for (int it = p->first_iteration; it < p->first_iteration + p->num_iterations; ++it) {
        // _spatial_propagation (mvs_patchmatch.py:415-457): even iterations pull from
        // (y+1,x) then (y,x+1), odd iterations from (y-1,x) then (y,x-1)
        const int sgn = (it % 2 == 0) ? 1 : -1;
        for (int k = 0; k < 2; ++k)
            v.push_back(SchedStep{amvs::MODE_PROP, k == 0 ? sgn : 0, k == 0 ? 0 : sgn, 0.f, 0.f, 0u, 1, it});
        // _random_refinement (mvs_patchmatch.py:459-491): ranges formed in double, cast once
        const float dr = (float)(((double)p->depth_max - (double)p->depth_min) * std::pow(0.5, it));
        const float nr = (float)(0.5 * std::pow(0.5, it));
        for (int s = 0; s < p->num_samples; ++s)
            v.push_back(SchedStep{amvs::MODE_REFINE, 0, 0, dr, nr, (unsigned)(1 + it * p->num_samples + s), 1, it});
    }
    return v;
}

void apply_step(amvs::StepArgs &a, const SchedStep &st)
{
    a.mode = st.mode; a.oy = st.oy; a.ox = st.ox;
    if (st.mode == amvs::MODE_REFINE) { a.depth_range = st.depth_range; a.normal_range = st.normal_range; a.draw = st.draw; }
}

// The two streams of amvs_ctx::group_overlap = 1 (equal priorities) or 2 (high / low: distinct priorities land on
// distinct hardware queues, see run_split_schedule), created once per context.
int group_streams(amvs_ctx *c, int overlap, hipStream_t out[2])
{
    amvs::Stream *st = c->group_streams[overlap - 1];
    if (!st[0].get()) {
        int lo = 0, hi = 0;
        HIPCHK(c, hipDeviceGetStreamPriorityRange(&lo, &hi));      // (numerically: hi <= lo)
        amvs::Stream made[2];                                      // (both or neither: a failure leaves the pair empty)
        for (int i = 0; i < 2; ++i)
            HIPCHK(c, made[i].create(overlap == 2 ? (i == 0 ? hi : lo) : lo));
        for (int i = 0; i < 2; ++i) st[i] = std::move(made[i]);
    }
    if (!c->group_fork.get()) {
        amvs::Event fork, join;
        HIPCHK(c, fork.create(false));
        HIPCHK(c, join.create(false));
        c->group_fork = std::move(fork); c->group_join = std::move(join);
    }
    out[0] = st[0].get(); out[1] = st[1].get();
    return AMVS_OK;
}

// The batch in groups of `vpl` views, each group through the whole schedule with the fused kernel (sampling +
// window sums + selection in one launch).  One stream, or (amvs_ctx::group_overlap) the groups dealt to two streams
// that fork from the context's stream and join it again: the groups are independent (mvs_patchmatch.py:104-123) --
// their StepArgs, state slots, job entries and confidence slots are disjoint, the images and the job table are
// read-only, and the fused launches use no other scratch -- so the workgroups of one group fill the wave slots the
// tail of the other leaves empty.  Every group still runs its whole schedule in order on its stream.
int run_fused_schedule(amvs_ctx *c, int n_ref, int n_src, const amvs_pm_params *p, uint64_t seed, int fast,
                       const std::vector<SchedStep> &sched, void *conf_dev, int cur0, bool do_init, bool do_conf)
{
    const size_t hw = (size_t)c->H * c->W;
    // Views per launch: the views of a batch are independent, so the batch can be swept in groups of
    // `vpl` views, each group through the whole schedule (see default_views_per_launch).
    const int band_major = p->schedule == 0 ? c->default_band_major : (p->schedule == 2);
    // paired bands: asked for, or the automatic choice where they were measured faster (round 3, fast
    // arithmetic, one run per pair, G px-hyp/s paired / classic: k=7 1080p 43.3 / 41.9, k=5 47.3 / 46.2,
    // k=3 51.2 / 52.0 -- a one-row halo leaves nothing to save --, 2560x1440 41.6 / 39.3, 8 views of
    // 3840x2160 38.7 / 36.4, 32 views 43.0 / 41.7)
    // 9x9 / 11x11 (round 4: compiled, their exchange fits four workgroups per CU, bit-identical -- and measured NOT
    // faster: fast 11x11 36.2 paired at its best height (34 rows) against 36.4 classic, 9x9 38.2 against 39.2, exact
    // 35.4 / 35.7 and 30.7 / 32.3: at these sizes the k - 1 cross-lane adds of the window sums, not the sampled rows,
    // carry the launch): the automatic schedule keeps them classic
    const bool paired = (p->schedule == AMVS_SCHEDULE_PAIRED ||
                         (p->schedule == AMVS_SCHEDULE_AUTO && !band_major && p->patch_size >= 5 && p->patch_size <= 7)) &&
                        (fast ? amvs::step_fast_pair_supported(p->patch_size, n_src)
                              : (usable_pairs(c) != nullptr && amvs::step_pair_supported(p->patch_size, n_src)));
    int vpl = p->views_per_launch > 0 ? p->views_per_launch : default_views_per_launch(c, n_ref, p->patch_size, fast != 0);
    if (vpl > n_ref) vpl = n_ref;
    const int TH = p->tile_rows > 0 || !band_major
                       ? pick_tile_rows(c, p->patch_size, n_src, vpl, p->tile_rows, 1 << 20, fast != 0, 0, paired)
                       : pick_band_rows(c, p->patch_size, n_src, vpl, fast != 0);
    c->last_tile_rows = TH;
    // launch shape of every step: strip rows and resident workgroups per CU (step_shape)
    std::vector<StepShape> shapes(sched.size());
    for (size_t i = 0; i < sched.size(); ++i) {
        shapes[i] = band_major ? StepShape{TH, 0}
                               : step_shape(c, p, n_src, vpl, sched[i].iter, sched[i].mode == amvs::MODE_REFINE, fast != 0, TH);
        c->last_tile_rows = shapes[i].rows;
    }
    const int n_steps_timed = c->step_timing ? (int)sched.size() * ((n_ref + vpl - 1) / vpl) : 0;
    HIPCHK(c, c->ev_steps.reserve(n_steps_timed + (n_ref + vpl - 1) / vpl));
    c->n_step_events = 0;
    const int n_groups = (n_ref + vpl - 1) / vpl;
    // events: [0] start, then per group: after init, after steps, after confidence
    HIPCHK(c, c->ev_groups.reserve(3 * n_groups));
    c->timing_groups = n_groups;
#ifdef AMVS_STEP_TRACE
    // (cleared on the context's stream BEFORE the group streams fork from it)
    {
        long long blocks = 0;
        for (const StepShape &sh : shapes) {
            const long long b = (long long)vpl * base_args(c, p->patch_size, vpl, TH).tiles_x * ((c->H + sh.rows - 1) / sh.rows);
            blocks = b > blocks ? b : blocks;                  // (one strip per block at most: the run-time-k kernels)
        }
        c->trace_stride = blocks;
        c->trace_launches = (long long)n_groups * (long long)sched.size();
        HIPCHK(c, c->d_trace.reserve((size_t)(4 * blocks * c->trace_launches) + 1, c->cache));
        HIPCHK(c, hipMemsetAsync(c->d_trace.get(), 0, sizeof(unsigned long long) * (size_t)(4 * blocks * c->trace_launches), c->stream));
    }
#endif
    const int overlap = n_groups > 1 ? c->group_overlap : 0;
    c->timing_overlapped = overlap != 0;
    hipStream_t lanes[2] = {c->stream, c->stream};
    if (overlap) {
        int rc = group_streams(c, overlap, lanes);
        if (rc) return rc;
        HIPCHK(c, hipEventRecord(c->group_fork.get(), c->stream));
        for (hipStream_t st : lanes) HIPCHK(c, hipStreamWaitEvent(st, c->group_fork.get(), 0));
    }
    int64_t launches = 0;
    for (int g = 0; g < n_groups; ++g) {
        const int j0 = g * vpl, nj = (n_ref - j0) < vpl ? (n_ref - j0) : vpl;
        hipStream_t stream = lanes[g % 2];
        amvs::StepArgs a = base_args(c, p->patch_size, nj, TH);
        a.fast = fast;
        a.band_major = band_major;
        a.paired = paired ? 1 : 0;
        a.jobs = c->d_jobs.get() + j0;                   // slots stay global: job.slot = index in the batch
        a.depth_min = p->depth_min; a.depth_max = p->depth_max;
        a.seed = seed;
        a.edge_first = c->edge_first < 0 ? (overlap != 0) : c->edge_first;
        int cur = cur0;
        // initialisation (mvs_patchmatch.py:268-284); a continuation call resumes the context's state
        if (do_init)
            HIPCHK(c, amvs::launch_init(a.jobs, nj, (long long)hw, seed, p->log_depth_scale, p->log_depth_min,
                                        c->d_depth[cur].get(), c->d_normal[0].get(), c->d_cost.get(), stream));
        HIPCHK(c, hipEventRecord(c->ev_groups[3 * g], stream));
        if (c->step_timing) HIPCHK(c, hipEventRecord(c->ev_steps[c->n_step_events++], stream));
        for (size_t i = 0; i < sched.size(); ++i) {
            const SchedStep &st = sched[i];
            apply_step(a, st);
            a.TH = shapes[i].rows;
            a.tiles_y = (c->H + a.TH - 1) / a.TH;
            a.wg_cap = shapes[i].wg_cap;
            set_io(a, c, cur);
#ifdef AMVS_STEP_TRACE
            a.trace = c->d_trace.get() + 4 * c->trace_stride * ((long long)g * (long long)sched.size() + (long long)i);
#endif
            HIPCHK(c, amvs::launch_step(p->patch_size, n_src, a, stream));
            if (c->step_timing) HIPCHK(c, hipEventRecord(c->ev_steps[c->n_step_events++], stream));
            cur ^= st.flip_d; ++launches;
        }
        a.TH = TH;
        a.tiles_y = (c->H + TH - 1) / TH;
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
    if (overlap)
        for (hipStream_t st : lanes) {
            HIPCHK(c, hipEventRecord(c->group_join.get(), st));
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->group_join.get(), 0));
        }
    c->timing.sweep_launches = launches;
    c->last_views_per_launch = vpl;
    return AMVS_OK;
}

// Split schedule (fast mode).  A sweep step is two kernels: the SAMPLING kernel visits every pixel
// once -- no strip halo -- and is bound by the CU's L1 line rate for scattered gathers; the WINDOW
// kernel streams the sample maps (coalesced) through the box sums, NCC and selection.  They stress
// different parts of the CU, so the batch is cut into G view groups and the two kernel kinds run on
// two streams (distinct priorities, so that they land on distinct hardware queues):
//     sampling stream:  sample(g0,n) sample(g1,n) sample(g0,n+1) ...   (never two of them at once)
//     window stream:    window(g,n) after sample(g,n); sample(g,n+1) after window(g,n)   (events)
// so window(g,n) runs under the sampling of the next group.  Views are independent
// (mvs_patchmatch.py:104-123), nothing else orders the groups.  Results are those of the fused kernel
// bit for bit (same arithmetic, same order of every sum).
int run_split_schedule(amvs_ctx *c, int n_ref, int n_src, const amvs_pm_params *p, uint64_t seed,
                       const std::vector<SchedStep> &sched, void *conf_dev)
{
    const size_t hw = (size_t)c->H * c->W;
    constexpr int MAXG = 8;
    int G = p->views_per_launch > 0 ? (n_ref + p->views_per_launch - 1) / p->views_per_launch
                                    : (c->split_groups > 0 ? c->split_groups : 2);
    if (G > n_ref) G = n_ref;
    if (G > MAXG) G = MAXG;
    const int vpl = (n_ref + G - 1) / G;
    G = (n_ref + vpl - 1) / vpl;
    HIPCHK(c, c->d_samples.reserve((size_t)n_ref * n_src * hw, c->cache));
    if (!c->split_streams[0].get()) {
        int lo = 0, hi = 0;
        HIPCHK(c, hipDeviceGetStreamPriorityRange(&lo, &hi));        // lo = least urgent
        amvs::Stream made[2];                                        // (both or neither, as group_streams)
        for (int i = 0; i < 2; ++i)
            HIPCHK(c, made[i].create(i == 0 ? lo : hi));
        for (int i = 0; i < 2; ++i) c->split_streams[i] = std::move(made[i]);
    }
    HIPCHK(c, c->split_events.reserve(1 + 2 * MAXG));
    HIPCHK(c, c->ev_groups.reserve(3));
    c->timing_groups = 1;
    c->n_step_events = 0;                       // (no per-launch events in this schedule: amvs_get_step_times returns none)
    // The window kernel gathers nothing, so its strips can be tall (vertical halo 1.09 at 64 rows);
    // the sampling kernel has no halo at all and wants SHORT strips (the resident waves then touch
    // fewer source rows at once).  Measured on MI355X, 16 views 1080p, k=7, S=4, 2 groups, ms per step:
    // window rows 32 / 48 / 64 / 96: 67.4 / 67.3 / 66.5 / 68.3; sampling rows 16 / 8 / 4 / 2: 70.8 / 68.4 /
    // 65.2-66.8 / 66.5.
    const int TH = p->tile_rows > 0 ? p->tile_rows : (c->H < 64 ? c->H : 64);
    c->last_tile_rows = TH;
    const int s_TH = c->split_sample_rows > 0 ? c->split_sample_rows : 4;
    hipStream_t s_smp = c->split_streams[0].get(), s_win = c->split_streams[1].get();
    hipEvent_t ev_fork = c->split_events[0];
    const hipEvent_t *ev_sampled = &c->split_events[1], *ev_windowed = &c->split_events[1 + MAXG];

    amvs::StepArgs all = base_args(c, p->patch_size, n_ref, TH);
    all.fast = 1;
    all.depth_min = p->depth_min; all.depth_max = p->depth_max;
    all.seed = seed;
    all.samples = c->d_samples.get();
    all.half = p->patch_size / 2;
    all.s_TH = s_TH;
    all.s_lds = c->split_sample_lds;
    all.s_tiles_x = (c->W + 63) / 64;
    all.s_tiles_y = (c->H + s_TH - 1) / s_TH;
    int cur = 0;
    HIPCHK(c, amvs::launch_init(all.jobs, n_ref, (long long)hw, seed, p->log_depth_scale, p->log_depth_min,
                                c->d_depth[cur].get(), c->d_normal[0].get(), c->d_cost.get(), c->stream));
    HIPCHK(c, hipEventRecord(c->ev_groups[0], c->stream));
    HIPCHK(c, hipEventRecord(ev_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(s_smp, ev_fork, 0));
    HIPCHK(c, hipStreamWaitEvent(s_win, ev_fork, 0));
    bool first = true;
    for (const SchedStep &st : sched) {
        for (int g = 0; g < G; ++g) {
            const int j0 = g * vpl, nj = (n_ref - j0) < vpl ? (n_ref - j0) : vpl;
            amvs::StepArgs a = all;
            a.n_jobs = nj;
            a.jobs = c->d_jobs.get() + j0;
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
    if (!sched.empty()) HIPCHK(c, hipStreamWaitEvent(c->stream, ev_windowed[G - 1], 0));
    HIPCHK(c, hipEventRecord(c->ev_groups[1], c->stream));
    // _compute_confidence (mvs_patchmatch.py:493-534): one fused launch over the whole batch
    if ((p->flags & AMVS_PM_NO_CONFIDENCE) == 0) {
        all.mode = amvs::MODE_CONF;
        set_io(all, c, cur);
        all.aux = conf_dev ? (float *)conf_dev : c->d_aux.get();
        HIPCHK(c, amvs::launch_step(p->patch_size, n_src, all, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->ev_groups[2], c->stream));
    c->timing.sweep_launches = (int64_t)sched.size();     // one hypothesis of the whole batch each
    c->last_views_per_launch = n_ref;
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
    o.a = base_args(c, patch, 1, pick_tile_rows(c, patch, n_src, 1, 0, 64, fast != 0));
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
    const std::vector<SchedStep> sched = build_schedule(p);
    const int cur0 = resume ? c->pm_cur : 0;
    int cur = cur0;
    for (const SchedStep &st : sched) cur ^= st.flip_d;                           // final depth buffer
    HIPCHK(c, hipEventRecord(c->ev[0].get(), c->stream));
    if (p->schedule == AMVS_SCHEDULE_SPLIT) {
        if ((rc = run_split_schedule(c, n_ref, n_src, p, seed, sched, conf_dev))) return rc;
    } else {
        if ((rc = run_fused_schedule(c, n_ref, n_src, p, seed, fast, sched, conf_dev, cur0, !resume,
                                     (p->flags & AMVS_PM_NO_CONFIDENCE) == 0))) return rc;
        c->pm_resumable = true; c->pm_cur = cur; c->pm_key = key;
        c->pm_next_iteration = p->first_iteration + p->num_iterations;
    }
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
    c->split_groups = groups; c->split_sample_rows = sample_rows; c->split_sample_lds = sample_lds_bytes;
    return AMVS_OK;
}

int amvs_set_step_tuning(amvs_ctx *c, int n_iterations, const int32_t *tile_rows, const int32_t *wgs_per_cu)
{
    if (!c) return AMVS_EINVAL;
    if (n_iterations < 0 || (n_iterations > 0 && !tile_rows && !wgs_per_cu)) return fail(c, AMVS_EINVAL, "bad step tuning table");
    c->tune_rows.clear(); c->tune_cap.clear();
    for (int i = 0; i < 2 * n_iterations; ++i) {
        const int r = tile_rows ? tile_rows[i] : 0, w = wgs_per_cu ? wgs_per_cu[i] : 0;
        if (r < 0 || r > (1 << 20) || w < 0 || w > 8) {
            c->tune_rows.clear(); c->tune_cap.clear();
            return fail(c, AMVS_EINVAL, "step tuning: rows >= 0, workgroups per CU in 0..8");
        }
        c->tune_rows.push_back(r); c->tune_cap.push_back(w);
    }
    return AMVS_OK;
}

int amvs_set_launch_order(amvs_ctx *c, int edge_first, int group_overlap)
{
    if (!c) return AMVS_EINVAL;
    if (edge_first < -1 || edge_first > 1 || group_overlap < -1 || group_overlap > 2)
        return fail(c, AMVS_EINVAL, "launch order: edge_first in -1..1, group_overlap in -1..2");
    c->edge_first = edge_first < 0 ? AMVS_DEFAULT_EDGE_FIRST : edge_first;
    c->group_overlap = group_overlap < 0 ? AMVS_DEFAULT_GROUP_OVERLAP : group_overlap;
    return AMVS_OK;
}

int amvs_set_step_sources(amvs_ctx *c, int ref_stats, int centre_depth)
{
    if (!c) return AMVS_EINVAL;
    if (ref_stats < -1 || ref_stats > 1 || centre_depth < -1 || centre_depth > 1)
        return fail(c, AMVS_EINVAL, "step sources: ref_stats and centre_depth in -1..1");
    c->ref_stats_source = ref_stats < 0 ? AMVS_DEFAULT_REF_STATS_SOURCE : ref_stats;
    c->depth_source = centre_depth < 0 ? AMVS_DEFAULT_DEPTH_SOURCE : centre_depth;
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
