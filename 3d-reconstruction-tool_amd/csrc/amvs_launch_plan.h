// amvs_launch_plan.h -- the launch policy of the PatchMatch sweep steps and the plane sweep as pure functions: views
// per launch, strip rows per step, band-major or paired bands, the split schedule's shapes, the plane-sweep chunking
// and 8-bit keys, and the register-source table.  Plain C++17: no HIP header, no context.  What the policy cannot
// compute -- the resident waves per CU of the step kernel, which patch sizes and schedules are compiled -- comes in
// as values (amvs_plan_facts, include/amvs_plan.h), so every line below runs without a GPU: amvs_plan_patchmatch and
// amvs_plan_plane_sweep hand the same functions to tests/test_launch_plan_cpu.py.  The entry points (amvs_capi.hip,
// amvs_capi_sweep.hip) fill the inputs from the context and the kernels' launch interface, plan once, and issue.
#pragma once
#include "../../include/amvs_plan.h"

#include <cmath>
#include <cstddef>
#include <vector>

// Defaults of amvs_set_launch_order (A/B builds: ALL=1 tools/build_variant.sh NAME -DAMVS_DEFAULT_GROUP_OVERLAP=0 ...).
// Measured on MI355X, bench.py main line, ms per step, five alternating runs each:
// one stream top-to-bottom 59.65, one stream edge-first 59.86, two equal streams edge-first 58.77, top-to-bottom
// 58.95, a high / low pair 60.81.  Hence edge-first exactly where the groups overlap (-1), two equal streams.
#ifndef AMVS_DEFAULT_EDGE_FIRST
#define AMVS_DEFAULT_EDGE_FIRST -1
#endif
#ifndef AMVS_DEFAULT_GROUP_OVERLAP
#define AMVS_DEFAULT_GROUP_OVERLAP 1
#endif

// Defaults of amvs_set_step_sources (-1 = the automatic table of step_regs).
#ifndef AMVS_DEFAULT_REF_STATS_SOURCE
#define AMVS_DEFAULT_REF_STATS_SOURCE -1
#endif
#ifndef AMVS_DEFAULT_DEPTH_SOURCE
#define AMVS_DEFAULT_DEPTH_SOURCE -1
#endif

namespace amvs {
namespace plan {

using Device = amvs_plan_device;        // H, W, n_cu, packed_maps: the packed 8-bit maps are usable
using Call = amvs_plan_call;            // n_ref, n_src, fast, and the amvs_pm_params of the call
using Facts = amvs_plan_facts;          // what the kernels' launch interface says about this (patch, n_src, arithmetic)

enum { STEP_PROP = 1, STEP_REFINE = 2 };        // amvs::MODE_PROP / MODE_REFINE (amvs_kernels.h)
constexpr int SPLIT_MAX_GROUPS = 8;

// The knobs of a context (the amvs_set_* setters validate and write them).
struct SweepTuning {
    int default_band_major = 0;         // schedule of amvs_pm_params.schedule == 0 (view-major measured faster)
    // amvs_set_step_tuning: strip rows / resident workgroups per CU by [iteration][0 = propagation, 1 = refinement]
    // (0 = automatic); iterations beyond the table use its last row.  Two tables of ONE size (the setter fills both).
    std::vector<int> tune_rows, tune_cap;
    int split_groups = 0, split_sample_rows = 0, split_sample_lds = 0;      // amvs_set_split_tuning (0 = automatic)
    // Sweep-step dispatch order (amvs_set_launch_order): edge_first -- every XCD walks each view's bands from the image
    // edge to its centre (amvs_strip_order.h; -1: where the groups overlap, else top to bottom); group_overlap -- the
    // view groups of a batch dealt to two streams of the context: 0 one stream, 1 two streams of equal priority, 2 a
    // high / low pair
    int edge_first = AMVS_DEFAULT_EDGE_FIRST, group_overlap = AMVS_DEFAULT_GROUP_OVERLAP;
    int sweep_tile_rows = 0, sweep_chunk = 0;   // amvs_set_sweep_tuning (0 = automatic)
    int sweep_key8 = 1;                         // strips above 32 rows with 8-bit keys where the plane chunks allow it
    // Where the fast sweep step takes the reference window's statistics and the centre depth from (amvs_set_step_sources;
    // resolved per call by step_regs): -1 the automatic table, 0 the (mean1, var1) maps / a second load, 1 the registers
    int ref_stats_source = AMVS_DEFAULT_REF_STATS_SOURCE, depth_source = AMVS_DEFAULT_DEPTH_SOURCE;
};

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// strip columns of an image `W` wide whose strips write `out_width` columns each (strip_out_width of the patch)
inline int strip_cols(int W, int out_width) { return ceil_div(W, out_width); }

inline bool band_major(const SweepTuning &t, const amvs_pm_params &p)
{
    return p.schedule == AMVS_SCHEDULE_AUTO ? t.default_band_major != 0 : p.schedule == AMVS_SCHEDULE_BAND_MAJOR;
}

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
inline int default_views_per_launch(const Device &d, int n_ref, int patch, bool fast)
{
    if (fast && patch <= 7 && d.W <= 2048 && n_ref >= 8 && n_ref % 4 == 0) return 4;
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
// (f.waves_per_cu[wg_cap]: the resident waves per CU of this call's step kernel under that cap.)
inline int pick_tile_rows(const Device &d, const Facts &f, int patch, int n_jobs, int requested, int cap, int wg_cap = 0,
                          bool paired = false)
{
    if (requested > 0) return requested < cap ? requested : cap;
    const int tiles_x = strip_cols(d.W, f.out_width);
    const long long slots = (long long)d.n_cu * f.waves_per_cu[wg_cap];
    int tall = 4 * patch - 4 > 12 ? 4 * patch - 4 : 12;
    if (paired) tall = 3 * patch - 3 > 8 ? 3 * patch - 3 : 8;
    if (d.W > (paired ? 3072 : 2048)) tall = tall * 2 / 3 > 8 ? tall * 2 / 3 : 8;
    if (tall > cap) tall = cap;
    int best = tall < 8 ? tall : 8;
    double best_score = -1.0;
    for (int th = tall; th >= (tall < 8 ? tall : 8); th -= 2) {
        const double waves = (double)n_jobs * tiles_x * ceil_div(d.H, th);
        const double g = waves / (double)slots;
        const double fill = g > 1.0 ? g / std::ceil(g) : (g >= 0.75 ? 1.0 : g / 0.75);
        double useful = (double)th / (double)(th + patch - 1);
        if (paired) {
            const int bands = ceil_div(d.H, th);
            const double sampled = (double)(bands / 2) * (2 * th + patch - 1) + (double)(bands % 2) * (th + patch - 1);
            useful = (double)d.H / sampled;
        }
        const double score = fill * useful;
        if (score > best_score + 1e-9) { best_score = score; best = th; }
    }
    return best;
}

// the strip height of the single-step entry points (one view, one launch)
inline int single_step_rows(const Device &d, const Facts &f, int patch) { return pick_tile_rows(d, f, patch, 1, 0, 64); }

// Band-major schedule (StepArgs::band_major): strip height such that ONE band of all views of the
// launch about fills an XCD's wave slots, i.e. every XCD walks its own band(s) of all views top to
// bottom in one generation of waves.  Few views: several adjacent bands per XCD.
inline int pick_band_rows(const Device &d, const Facts &f, int patch, int n_jobs)
{
    const int tiles_x = strip_cols(d.W, f.out_width);
    const long long slots_xcd = (long long)(d.n_cu / 8 > 0 ? d.n_cu / 8 : 1) * f.waves_per_cu[0];
    const long long per_band = (long long)n_jobs * tiles_x;
    long long g = slots_xcd / per_band;             // bands resident together per XCD
    if (g < 1) g = 1;
    const long long bands = 8 * g;
    long long th = (d.H + bands - 1) / bands;
    const int min_th = 2 * patch > 8 ? 2 * patch : 8;
    if (th < min_th) th = min_th;
    return (int)th;
}

// the amvs_set_step_tuning entries of a step (0 = automatic)
struct TuneEntry { int rows, cap; };

inline TuneEntry tune_entry(const SweepTuning &t, int iter, bool refine)
{
    const size_t idx = (size_t)2 * (size_t)iter + (refine ? 1 : 0);
    const size_t last = t.tune_rows.size() >= 2 ? t.tune_rows.size() - 2 + (refine ? 1 : 0) : 0;
    TuneEntry e{0, 0};
    if (!t.tune_rows.empty()) e.rows = t.tune_rows[idx < t.tune_rows.size() ? idx : last];
    if (!t.tune_cap.empty()) e.cap = t.tune_cap[idx < t.tune_cap.size() ? idx : last];
    return e;
}

// Launch shape of one sweep step.  The gathers of an early iteration are scattered over the whole
// depth range (every pixel perturbs its depth by up to depth_range / 2^it), those of a late one are
// coherent, so the best strip height / residency differ by iteration; measured table: DESIGN.md
// section 5 (round 3).  An explicit amvs_pm_params.tile_rows, then amvs_set_step_tuning, override it.
struct StepShape { int rows, wg_cap; };

inline StepShape step_shape(const Device &d, const Facts &f, const SweepTuning &t, const amvs_pm_params &p, int n_jobs, int iter,
                            bool refine, int default_rows)
{
    StepShape s{default_rows, 0};
    const TuneEntry e = tune_entry(t, iter, refine);
    if (e.cap > 0) s.wg_cap = e.cap;
    if (p.tile_rows > 0) return s;                       // the caller fixed the strip height
    if (e.rows > 0) s.rows = e.rows;
    else if (e.cap > 0) s.rows = pick_tile_rows(d, f, p.patch_size, n_jobs, 0, 1 << 20, e.cap);
    return s;
}

// One launch of the sweep schedule of a PatchMatch call (the same for every view group), with its shape.
using Step = amvs_plan_step;

// (shapes: filled by plan_patchmatch)
inline std::vector<Step> build_schedule(const amvs_pm_params &p)
{
    std::vector<Step> v;
    for (int it = p.first_iteration; it < p.first_iteration + p.num_iterations; ++it) {
        // _spatial_propagation (mvs_patchmatch.py:415-457): even iterations pull from
        // (y+1,x) then (y,x+1), odd iterations from (y-1,x) then (y,x-1)
        const int sgn = (it % 2 == 0) ? 1 : -1;
        for (int k = 0; k < 2; ++k)
            v.push_back(Step{STEP_PROP, k == 0 ? sgn : 0, k == 0 ? 0 : sgn, 0.f, 0.f, 0u, 1, it, 0, 0, 0});
        // _random_refinement (mvs_patchmatch.py:459-491): ranges formed in double, cast once
        const float dr = (float)(((double)p.depth_max - (double)p.depth_min) * std::pow(0.5, it));
        const float nr = (float)(0.5 * std::pow(0.5, it));
        for (int s = 0; s < p.num_samples; ++s)
            v.push_back(Step{STEP_REFINE, 0, 0, dr, nr, (unsigned)(1 + it * p.num_samples + s), 1, it, 0, 0, 0});
    }
    return v;
}

// The waves_per_cu entries the plan of this call reads, bit w = the entry of wg_cap w: what the caller has to fill
// (an occupancy query each).
inline unsigned waves_entries_read(const SweepTuning &t, const amvs_pm_params &p)
{
    if (p.schedule == AMVS_SCHEDULE_SPLIT || p.tile_rows > 0) return 0u;
    unsigned mask = 1u;
    if (band_major(t, p)) return mask;
    for (const Step &st : build_schedule(p)) {
        const TuneEntry e = tune_entry(t, st.iter, st.mode == STEP_REFINE);
        if (e.rows == 0 && e.cap > 0) mask |= 1u << e.cap;
    }
    return mask;
}

struct Group { int first, count; };     // views first .. first + count - 1 of the batch

inline std::vector<Group> view_groups(int n_ref, int vpl)
{
    std::vector<Group> v;
    for (int j0 = 0; j0 < n_ref; j0 += vpl) v.push_back(Group{j0, (n_ref - j0) < vpl ? (n_ref - j0) : vpl});
    return v;
}

// Split schedule: `groups` view groups pipelined against each other, the window kernel's strips of TH rows, the
// sampling kernel's own strips (64 columns, no halo) of s_TH rows.
struct SplitPlan {
    std::vector<Group> groups;
    int vpl = 0, TH = 0, tiles_y = 0, s_TH = 0, s_lds = 0, s_tiles_x = 0, s_tiles_y = 0;
};

// The plan of a PatchMatch call.  Fused schedule: the batch in `groups` of views_per_launch views, each group through
// all `steps`.  Split schedule (`split` filled): every step sweeps the whole batch, so it counts as one group.
struct PmPlan {
    bool band_major = false, paired = false;
    int views_per_launch = 0;
    std::vector<Group> groups;
    int TH = 0, tiles_x = 0, tiles_y = 0;       // base strip rows (initialisation and confidence launches) and their grid
    int overlap = 0, edge_first = 0;            // effective: no overlap with one group; edge-first resolved
    std::vector<Step> steps;
    int final_parity = 0;                       // the depth buffers ping-pong: the final one is the first one ^ this
    long long launches = 0;                     // amvs_timing::sweep_launches
    int last_tile_rows = 0;                     // amvs_last_tile_rows
    long long trace_blocks = 0;                 // strips of the largest launch (-DAMVS_STEP_TRACE)
    SplitPlan split;
};

inline SplitPlan plan_split(const Device &d, const Call &call, const SweepTuning &t)
{
    const amvs_pm_params &p = call.p;
    const int n_ref = call.n_ref;
    SplitPlan s;
    int G = p.views_per_launch > 0 ? ceil_div(n_ref, p.views_per_launch) : (t.split_groups > 0 ? t.split_groups : 2);
    if (G > n_ref) G = n_ref;
    if (G > SPLIT_MAX_GROUPS) G = SPLIT_MAX_GROUPS;
    s.vpl = ceil_div(n_ref, G);
    s.groups = view_groups(n_ref, s.vpl);
    // The window kernel gathers nothing, so its strips can be tall (vertical halo 1.09 at 64 rows);
    // the sampling kernel has no halo at all and wants SHORT strips (the resident waves then touch
    // fewer source rows at once).  Measured on MI355X, 16 views 1080p, k=7, S=4, 2 groups, ms per step:
    // window rows 32 / 48 / 64 / 96: 67.4 / 67.3 / 66.5 / 68.3; sampling rows 16 / 8 / 4 / 2: 70.8 / 68.4 /
    // 65.2-66.8 / 66.5.
    s.TH = p.tile_rows > 0 ? p.tile_rows : (d.H < 64 ? d.H : 64);
    s.tiles_y = ceil_div(d.H, s.TH);
    s.s_TH = t.split_sample_rows > 0 ? t.split_sample_rows : 4;
    s.s_lds = t.split_sample_lds;
    s.s_tiles_x = ceil_div(d.W, 64);
    s.s_tiles_y = ceil_div(d.H, s.s_TH);
    return s;
}

inline PmPlan plan_patchmatch(const Device &d, const Call &call, const SweepTuning &t, const Facts &f)
{
    const amvs_pm_params &p = call.p;
    const int n_ref = call.n_ref;
    const bool fast = call.fast != 0;
    PmPlan plan;
    plan.steps = build_schedule(p);
    for (const Step &st : plan.steps) plan.final_parity ^= st.flip_d;
    plan.tiles_x = strip_cols(d.W, f.out_width);
    if (p.schedule == AMVS_SCHEDULE_SPLIT) {
        plan.split = plan_split(d, call, t);
        plan.TH = plan.split.TH;
        plan.tiles_y = plan.split.tiles_y;
        for (Step &st : plan.steps) { st.rows = plan.TH; st.tiles_y = plan.tiles_y; }
        plan.views_per_launch = n_ref;
        plan.groups = view_groups(n_ref, n_ref);
        plan.launches = (long long)plan.steps.size();         // one hypothesis of the whole batch each
        plan.last_tile_rows = plan.TH;
        return plan;
    }
    plan.band_major = band_major(t, p);
    // paired bands: asked for, or the automatic choice where they were measured faster (round 3, fast
    // arithmetic, one run per pair, G px-hyp/s paired / classic: k=7 1080p 43.3 / 41.9, k=5 47.3 / 46.2,
    // k=3 51.2 / 52.0 -- a one-row halo leaves nothing to save --, 2560x1440 41.6 / 39.3, 8 views of
    // 3840x2160 38.7 / 36.4, 32 views 43.0 / 41.7)
    // 9x9 / 11x11 (round 4: compiled, their exchange fits four workgroups per CU, bit-identical -- and measured NOT
    // faster: fast 11x11 36.2 paired at its best height (34 rows) against 36.4 classic, 9x9 38.2 against 39.2, exact
    // 35.4 / 35.7 and 30.7 / 32.3: at these sizes the k - 1 cross-lane adds of the window sums, not the sampled rows,
    // carry the launch): the automatic schedule keeps them classic
    plan.paired = (p.schedule == AMVS_SCHEDULE_PAIRED ||
                   (p.schedule == AMVS_SCHEDULE_AUTO && !plan.band_major && p.patch_size >= 5 && p.patch_size <= 7)) &&
                  (fast ? f.fast_pair_supported != 0 : (d.packed_maps != 0 && f.pair_supported != 0));
    int vpl = p.views_per_launch > 0 ? p.views_per_launch : default_views_per_launch(d, n_ref, p.patch_size, fast);
    if (vpl > n_ref) vpl = n_ref;
    plan.views_per_launch = vpl;
    plan.groups = view_groups(n_ref, vpl);
    plan.TH = p.tile_rows > 0 || !plan.band_major ? pick_tile_rows(d, f, p.patch_size, vpl, p.tile_rows, 1 << 20, 0, plan.paired)
                                                  : pick_band_rows(d, f, p.patch_size, vpl);
    plan.tiles_y = ceil_div(d.H, plan.TH);
    plan.last_tile_rows = plan.TH;
    // launch shape of every step: strip rows and resident workgroups per CU (step_shape)
    for (Step &st : plan.steps) {
        const StepShape sh = plan.band_major ? StepShape{plan.TH, 0}
                                             : step_shape(d, f, t, p, vpl, st.iter, st.mode == STEP_REFINE, plan.TH);
        st.rows = sh.rows; st.wg_cap = sh.wg_cap;
        st.tiles_y = ceil_div(d.H, st.rows);
        plan.last_tile_rows = st.rows;
        const long long b = (long long)vpl * plan.tiles_x * st.tiles_y;
        plan.trace_blocks = b > plan.trace_blocks ? b : plan.trace_blocks;     // (one strip per block at most: the run-time-k kernels)
    }
    plan.overlap = plan.groups.size() > 1 ? t.group_overlap : 0;
    plan.edge_first = t.edge_first < 0 ? (plan.overlap != 0) : t.edge_first;
    plan.launches = (long long)plan.groups.size() * (long long)plan.steps.size();
    return plan;
}

// The plane sweep: tall strips (little halo re-sampling); the planes are chunked so that the launch still has
// about four strips per resident wave slot.  A strip's running best lives in 4 KB of LDS: 16-bit keys for up
// to sweep_max_th = 32 rows, or -- compiled patch sizes, chunks of at most 32 planes -- 8-bit keys for up
// to 64 rows (SweepArgs::key8); the fewest bands of at most that many rows, evenly high.
struct PlaneSweepPlan { int TH, tiles_x, tiles_y, chunk, n_chunks, key8; };

inline PlaneSweepPlan plan_plane_sweep(const Device &d, const SweepTuning &t, const Facts &f, int n_ref, int D)
{
    PlaneSweepPlan a{};
    a.tiles_x = strip_cols(d.W, f.out_width);
    auto shape = [&](int max_rows) {
        const int bands = ceil_div(d.H, max_rows);
        a.TH = ceil_div(d.H, bands);
        if (t.sweep_tile_rows >= 1 && t.sweep_tile_rows <= max_rows && t.sweep_tile_rows < d.H) a.TH = t.sweep_tile_rows;
        a.tiles_y = ceil_div(d.H, a.TH);
        const long long strips = (long long)n_ref * a.tiles_x * a.tiles_y;
        const long long slots = (long long)d.n_cu * 16;        // four waves per SIMD
        // chunks for ~8 waves per slot, evenly sized (measured on MI355X, config 2, strips of 60 rows, planes per
        // wave 2 / 3 / 4 / 5 / 6 / 8 / 13: exact 51.7 / 50.0 / 51.7 / 50.7 / 49.8 / 49.2 / 46.1, fast 73.7 / 73.8 / 76.8 /
        // 74.5 / 74.0 / 72.5 / 67.8 G px-hyp/s: many short waves fill the tail of the launch, uneven last chunks lose)
        long long want = (8 * slots + strips - 1) / strips;
        if (want < 1) want = 1;
        if (want > (D + 1) / 2) want = (D + 1) / 2;              // (at least two planes per wave: a wave's set-up)
        a.chunk = (int)((D + want - 1) / want);
        a.chunk = (int)((D + (D + a.chunk - 1) / a.chunk - 1) / ((D + a.chunk - 1) / a.chunk));   // even chunks
        if (t.sweep_chunk >= 1) a.chunk = t.sweep_chunk < D ? t.sweep_chunk : D;
        if (a.chunk > f.sweep_max_chunk) a.chunk = f.sweep_max_chunk;
        a.n_chunks = (D + a.chunk - 1) / a.chunk;
    };
    a.key8 = 0;
    if (f.patch_compiled && t.sweep_key8 != 0 && (t.sweep_tile_rows == 0 || t.sweep_tile_rows > f.sweep_max_th)) {
        shape(f.sweep_max_th8);
        a.key8 = a.chunk <= f.sweep_max_chunk8 ? 1 : 0;
    }
    if (!a.key8) shape(f.sweep_max_th);
    return a;
}

// Where the fast sweep steps take the reference statistics and the centre depth from (amvs_set_step_sources).  The
// automatic choice is a table by patch size, like the `paired` rule of plan_patchmatch: the registers where they were
// measured faster by the rule of DESIGN.md section 5 (round 9; bench.py
// main line at that patch size, ms per step, medians of five alternating runs, maps and loads / statistics in the kernel
// / both): 3x3 51.24 / 47.08 / 45.64 (three runs), 5x5 54.25 / 51.35 / 49.96, 7x7 58.42 / 55.71 / 54.27 (a second
// session 58.87 / 55.61 / 54.17), 9x9 68.18 / 66.02 / 64.72, 11x11 73.76 / 72.47 / 71.16 -- and 13x13 80.85 / 82.33 /
// 80.64, 15x15 86.81 / 89.80 / 88.25: there the 2 (k - 1) more cross-lane adds cost more than the load saves.
// The statistics entry meets that rule against the maps at every size up to 11x11.  The HISTORY entry does not meet
// it as worded -- alone against the maps and loads it gains 1.2 - 1.7 %, below three parent spreads at 7x7 (2.6 -
// 3.1 %) and 3x3 (1.3 %) --: it rests on the stacked comparison, "both" against "statistics" (7x7: 2.6 % in both
// sessions against three spreads of 1.1 %, every run below every run).  Sizes other than 7x7: one session.
// 13x13 and 15x15 stay compiled although the table never picks them: they are the measurements that place the
// table's edge, and the switch lets that edge be measured again on another image size or source count with one build.
// The run-time-k kernels and patches above step_fast_regs_max_patch() always read the maps.
struct StepRegs { bool stats, hist; };      // StepArgs::ref_in_kernel / depth_hist

inline StepRegs step_regs(const SweepTuning &t, bool regs_supported, int patch)
{
    if (!regs_supported) return StepRegs{false, false};
    const bool auto_stats = patch <= 11, auto_hist = patch <= 11;
    return StepRegs{t.ref_stats_source < 0 ? auto_stats : t.ref_stats_source != 0,
                    t.depth_source < 0 ? auto_hist : t.depth_source != 0};
}

}  // namespace plan
}  // namespace amvs
