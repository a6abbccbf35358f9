// amvs_context.hip -- the context of the C ABI (include/amvs.h): creation and destruction, stream, arithmetic
// mode, and the host helpers the other entry-point files share (declared in amvs_ctx.h).
#include "amvs_ctx.h"

#include <algorithm>
#include <cstring>
#include <utility>

static_assert(AMVS_MAX_SRC == AMVS_KMAX_SRC, "source-count limits out of sync");

#ifdef AMVS_CHECK_INDICES
// index-checked build (amvs_check.h): one device-side report per kernel translation unit
namespace amvs {
void check_fetch_kernels(unsigned long long out[4], bool reset);
void check_fetch_kernels_fast(unsigned long long out[4], bool reset);
void check_fetch_sweep_fast(unsigned long long out[4], bool reset);
void check_fetch_sweep_exact(unsigned long long out[4], bool reset);
void check_fetch_generic(unsigned long long out[4], bool reset);
void check_fetch_extended(unsigned long long out[4], bool reset);
void check_fetch_fusion(unsigned long long out[4], bool reset);
void check_fetch_knn(unsigned long long out[4], bool reset);
void check_fetch_mesh(unsigned long long out[4], bool reset);
void check_fetch_mesh_clean(unsigned long long out[4], bool reset);
void check_fetch_mesh_decimate(unsigned long long out[4], bool reset);
void check_fetch_mesh_render(unsigned long long out[4], bool reset);
void check_fetch_mesh_color(unsigned long long out[4], bool reset);
void check_fetch_mesh_texture(unsigned long long out[4], bool reset);
void check_fetch_mesh_fill(unsigned long long out[4], bool reset);
void check_fetch_cloud_normals(unsigned long long out[4], bool reset);
void check_fetch_depth_filter(unsigned long long out[4], bool reset);
void check_fetch_undistort(unsigned long long out[4], bool reset);
void check_fetch_match(unsigned long long out[4], bool reset);
void check_fetch_triangulate(unsigned long long out[4], bool reset);
void check_fetch_fmat(unsigned long long out[4], bool reset);
void check_fetch_pnp(unsigned long long out[4], bool reset);
void check_fetch_twoview(unsigned long long out[4], bool reset);
void check_fetch_kernels_fast_regs(unsigned long long out[4], bool reset);
void check_fetch_bundle(unsigned long long out[4], bool reset);
void check_fetch_sfm(unsigned long long out[4], bool reset);
void check_fetch_kernels_fast_regs_packed(unsigned long long out[4], bool reset);
}  // namespace amvs
#endif

namespace amvs {
namespace host {

namespace {
std::string g_create_error;
}  // namespace

// Sum of the violations all kernels have counted since the last reset and the record of the first one found
// (out[1] = translation unit << 32 | source line: 1 amvs_kernels, 2 amvs_kernels_fast, 3 amvs_sweep_fast,
// 4 amvs_sweep_exact, 5 amvs_generic, 6 amvs_extended, 7 amvs_fusion, 8 amvs_knn, 9 amvs_mesh, 10 amvs_mesh_clean,
// 11 amvs_mesh_decimate, 12 amvs_mesh_render, 13 amvs_mesh_color, 14 amvs_mesh_texture, 15 amvs_mesh_fill,
// 16 amvs_cloud_normals, 17 amvs_depth_filter, 18 amvs_undistort, 19 amvs_match, 20 amvs_triangulate, 21 amvs_fmat,
// 22 amvs_kernels_fast_regs (lines of amvs_kernels_fast.hip), 23 amvs_pnp, 24 amvs_twoview, 25 amvs_bundle, 26 amvs_sfm,
// 27 amvs_kernels_fast_regs_packed (lines of amvs_kernels_fast.hip);
// out[2] = the index, out[3] = the extent it was compared with).  Zeros in the shipped build.
void index_report(uint64_t out[4], bool reset)
{
    out[0] = out[1] = out[2] = out[3] = 0;
#ifdef AMVS_CHECK_INDICES
    (void)hipDeviceSynchronize();
    void (*const fetch[])(unsigned long long[4], bool) = {
        amvs::check_fetch_kernels, amvs::check_fetch_kernels_fast, amvs::check_fetch_sweep_fast, amvs::check_fetch_sweep_exact,
        amvs::check_fetch_generic, amvs::check_fetch_extended, amvs::check_fetch_fusion, amvs::check_fetch_knn,
        amvs::check_fetch_mesh, amvs::check_fetch_mesh_clean, amvs::check_fetch_mesh_decimate,
        amvs::check_fetch_mesh_render, amvs::check_fetch_mesh_color, amvs::check_fetch_mesh_texture,
        amvs::check_fetch_mesh_fill, amvs::check_fetch_cloud_normals, amvs::check_fetch_depth_filter,
        amvs::check_fetch_undistort, amvs::check_fetch_match, amvs::check_fetch_triangulate,
        amvs::check_fetch_fmat, amvs::check_fetch_kernels_fast_regs, amvs::check_fetch_pnp, amvs::check_fetch_twoview,
        amvs::check_fetch_bundle, amvs::check_fetch_sfm, amvs::check_fetch_kernels_fast_regs_packed};
    for (auto f : fetch) {
        unsigned long long r[4] = {0, 0, 0, 0};
        f(r, reset);
        if (r[0] && !out[0]) { out[1] = r[1]; out[2] = r[2]; out[3] = r[3]; }
        out[0] += r[0];
    }
#else
    (void)reset;
#endif
}

int fail(amvs_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

// end of a synchronising entry point: in the index-checked build a recorded violation turns success into
// AMVS_EINDEX (the report stays until amvs_index_check resets it)
int checked(amvs_ctx *c, int rc)
{
#ifdef AMVS_CHECK_INDICES
    if (rc == AMVS_OK) {
        uint64_t r[4];
        index_report(r, false);
        if (r[0])
            return fail(c, AMVS_EINDEX, "index check: " + std::to_string(r[0]) + " out-of-range accesses; first in translation unit " +
                                            std::to_string(r[1] >> 32) + " line " + std::to_string(r[1] & 0xFFFFFFFFull) + ": index " +
                                            std::to_string((long long)r[2]) + ", extent " + std::to_string((long long)r[3]));
    }
#else
    (void)c;
#endif
    return rc;
}

int bind_device(amvs_ctx *c)
{
    HIPCHK(c, hipSetDevice(c->device));
    return AMVS_OK;
}

int check_patch_src(amvs_ctx *c, int patch, int n_src)
{
    if (!amvs::patch_supported(patch))
        return fail(c, AMVS_EUNSUPPORTED,
                    "patch_size " + std::to_string(patch) + " unsupported (odd sizes from 3 to " + std::to_string(AMVS_MAX_PATCH) + ")");
    if (n_src < 2 || n_src > AMVS_MAX_SRC)
        return fail(c, AMVS_EUNSUPPORTED,
                    "n_src " + std::to_string(n_src) + " outside [2, " + std::to_string(AMVS_MAX_SRC) + "]");
    return AMVS_OK;
}

// state buffers for n batch slots: the whole group is released before any of it is allocated again (d_aux,
// allocated last, holds the number of slots)
int ensure_slots(amvs_ctx *c, int n)
{
    const size_t hw = (size_t)c->H * c->W;
    if (hw * n <= c->d_aux.capacity()) return AMVS_OK;
    for (auto *b : {&c->d_depth[0], &c->d_cost, &c->d_normal[0], &c->d_depth[1], &c->d_normal[1], &c->d_aux}) b->release();
    for (int i = 0; i < 2; ++i) {
        HIPCHK(c, c->d_depth[i].reserve(hw * n, c->cache));
        if (i == 0) HIPCHK(c, c->d_cost.reserve(hw * n, c->cache));
        HIPCHK(c, c->d_normal[i].reserve(hw * n * 3, c->cache));
    }
    HIPCHK(c, c->d_aux.reserve(hw * n, c->cache));
    return AMVS_OK;
}

// mean1 / var1 of every uploaded view for this patch size (computed once, kept resident)
int ensure_stats(amvs_ctx *c, int patch)
{
    Stats &s = c->stats[patch];
    if (s.done.empty()) {
        HIPCHK(c, s.mean.reserve(c->stride * c->n_views, c->cache));
        HIPCHK(c, s.var.reserve(c->stride * c->n_views, c->cache));
        s.done.assign(c->n_views, 0);
    }
    for (int v = 0; v < c->n_views; ++v) {
        if (!c->have[v] || s.done[v]) continue;
        HIPCHK(c, amvs::launch_box_stats(patch, c->d_images.get(), c->stride, c->H, c->W, v, 1, s.mean.get(),
                                         s.var.get(), c->stream));
        s.done[v] = 1;
    }
    return AMVS_OK;
}

// fast mode: (mean1, var1) of every uploaded view for this patch size (exact integer window sums
// of the 8-bit codes), computed once and kept resident
int ensure_fast_stats(amvs_ctx *c, int patch)
{
    FastStats &s = c->fstats[patch];
    const size_t hw = (size_t)c->H * c->W;
    if (s.done.empty()) {
        HIPCHK(c, s.maps.reserve(hw * c->n_views, c->cache));
        s.done.assign(c->n_views, 0);
    }
    for (int v = 0; v < c->n_views; ++v) {
        if (!c->have[v] || s.done[v]) continue;
        HIPCHK(c, amvs::launch_fast_stats(patch, c->d_pairs.get() + (long long)v * c->pstride, c->H, c->W,
                                          s.maps.get() + (size_t)v * hw, c->stream));
        s.done[v] = 1;
    }
    return AMVS_OK;
}

// where the fast sweep steps of this context take the reference statistics and the centre depth from (the rule and its
// measurements: amvs_launch_plan.h)
StepRegs step_regs(const amvs_ctx *c, int patch)
{
    return amvs::plan::step_regs(c->tuning, amvs::step_fast_regs_supported(patch), patch);
}

// The launch planner's inputs (amvs_launch_plan.h).  The kernel facts of (patch, n_src) in this arithmetic: the resident
// waves per CU only for the workgroup caps named by `waves_entries` (bit w = cap w; an occupancy query each).
amvs::plan::Device plan_device(const amvs_ctx *c, bool packed_maps) { return amvs::plan::Device{c->H, c->W, c->n_cu, packed_maps ? 1 : 0}; }

amvs::plan::Facts plan_facts(int patch, int n_src, bool fast, bool packed_maps, unsigned waves_entries)
{
    amvs::plan::Facts f{};
    f.out_width = amvs::strip_out_width(patch);
    for (int w = 0; w <= 8; ++w)
        if (waves_entries >> w & 1u)
            f.waves_per_cu[w] = fast ? amvs::step_fast_waves_per_cu(patch, n_src, w) : amvs::step_waves_per_cu(patch, n_src, packed_maps, w);
    f.patch_compiled = amvs::patch_compiled(patch);
    f.pair_supported = amvs::step_pair_supported(patch, n_src);
    f.fast_pair_supported = amvs::step_fast_pair_supported(patch, n_src);
    f.fast_regs_supported = amvs::step_fast_regs_supported(patch);
    f.sweep_max_th = AMVS_SWEEP_MAX_TH; f.sweep_max_th8 = AMVS_SWEEP_MAX_TH8;
    f.sweep_max_chunk = AMVS_SWEEP_MAX_CHUNK; f.sweep_max_chunk8 = AMVS_SWEEP_MAX_CHUNK8;
    return f;
}

amvs::plan::SweepTuning plan_tuning(const amvs_plan_tuning &t)
{
    amvs::plan::SweepTuning s;
    s.default_band_major = t.default_band_major;
    for (int i = 0; i < t.n_tune; ++i) {            // (as amvs_set_step_tuning stores them: two tables of one size)
        s.tune_rows.push_back(t.tune_rows ? t.tune_rows[i] : 0);
        s.tune_cap.push_back(t.tune_cap ? t.tune_cap[i] : 0);
    }
    s.split_groups = t.split_groups; s.split_sample_rows = t.split_sample_rows; s.split_sample_lds = t.split_sample_lds;
    s.edge_first = t.edge_first; s.group_overlap = t.group_overlap;
    s.sweep_tile_rows = t.sweep_tile_rows; s.sweep_chunk = t.sweep_chunk; s.sweep_key8 = t.sweep_key8;
    s.ref_stats_source = t.ref_stats_source; s.depth_source = t.depth_source;
    return s;
}

// `fast_patch` > 0: also fill the fast-mode records (precomposed projections, ref statistics of
// that patch size -- unless `ref_maps` is false: no kernel of the call reads the maps, see step_regs)
int upload_jobs(amvs_ctx *c, int n_ref, const int *ref_ids, const int *src_ids, int n_src, int fast_patch, bool compose_only,
                bool ref_maps)
{
    if (n_ref <= 0 || !ref_ids || !src_ids) return fail(c, AMVS_EINVAL, "empty batch");
    const float2 *fmaps = nullptr;
    if (fast_patch > 0 && ref_maps) {
        int rc = ensure_fast_stats(c, fast_patch);
        if (rc) return rc;
        fmaps = c->fstats[fast_patch].maps.get();
    }
    std::vector<amvs::Job> jobs(n_ref);
    for (int i = 0; i < n_ref; ++i) {
        amvs::Job &j = jobs[i];
        std::memset(&j, 0, sizeof(j));
        const int r = ref_ids[i];
        if (r < 0 || r >= c->n_views || !c->have[r])
            return fail(c, AMVS_EINVAL, "reference view " + std::to_string(r) + " not uploaded");
        std::memcpy(j.K, c->K, 36);
        std::memcpy(j.Kinv, c->Kinv, 36);
        std::memcpy(j.Rref, c->R[r].data(), 36);
        std::memcpy(j.tref, c->t[r].data(), 12);
        j.ref_img = r;
        j.ref_pairs = (unsigned long long)(uintptr_t)(c->d_pairs.get() + (long long)r * c->pstride) +
                      (unsigned long long)(amvs::pair_map_origin(c->W) * amvs::pair_map_texel_bytes());
        j.ref_stats = fmaps ? (unsigned long long)(uintptr_t)(fmaps + (size_t)r * c->H * c->W) : 0ull;
        j.stream_view = (uint32_t)r;
        j.slot = i;
        j.n_src = n_src;
        for (int s = 0; s < n_src; ++s) {
            const int v = src_ids[i * n_src + s];
            if (v < 0 || v >= c->n_views || !c->have[v])
                return fail(c, AMVS_EINVAL, "source view " + std::to_string(v) + " not uploaded");
            j.src[s].pairs = (unsigned long long)(uintptr_t)(c->d_pairs.get() + (long long)v * c->pstride);
            j.src[s].gray = (unsigned long long)(uintptr_t)(c->d_images.get() + (long long)v * c->stride);
            std::memcpy(j.src[s].R, c->R[v].data(), 36);
            std::memcpy(j.src[s].t, c->t[v].data(), 12);
            if (fast_patch > 0 || compose_only) {
                amvs::fast_compose(c->K, c->R[r].data(), c->t[r].data(), c->R[v].data(), c->t[v].data(),
                                   j.fsrc[s].M, j.fsrc[s].b);
                j.fsrc[s].pairs = j.src[s].pairs;
            }
        }
    }
    HIPCHK(c, c->d_jobs.reserve(n_ref, c->cache));
    HIPCHK(c, hipMemcpyAsync(c->d_jobs.get(), jobs.data(), sizeof(amvs::Job) * n_ref,
                             hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // `jobs` is a stack-lifetime staging buffer
    return AMVS_OK;
}

// the packed maps can be used when every uploaded view quantised losslessly
const uint16_t *usable_pairs(const amvs_ctx *c)
{
    if (c->force_f32) return nullptr;
    if (c->flags_dirty) {
        // the uploads only queue the losslessness test; its results are read here, once
        std::vector<int> flags(c->n_views, 1);
        if (hipMemcpyAsync(flags.data(), c->d_flag.get(), sizeof(int) * c->n_views, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
            hipStreamSynchronize(c->stream) == hipSuccess) {
            for (int v = 0; v < c->n_views; ++v) c->exact8[v] = flags[v] ? 0 : 1;
            c->flags_dirty = false;
        } else {
            return nullptr;
        }
    }
    for (int v = 0; v < c->n_views; ++v)
        if (c->have[v] && !c->exact8[v]) return nullptr;
    return c->d_pairs.get();
}

// 1 when the sweeps of this call run in the fast arithmetic; fails when fast was asked for but
// some uploaded view is not 8-bit exact (the fast kernels sample the packed maps only)
int resolve_fast(amvs_ctx *c, int requested, int *fast)
{
    const int m = requested == AMVS_MODE_DEFAULT ? c->mode : requested;
    if (m != AMVS_MODE_EXACT && m != AMVS_MODE_FAST) return fail(c, AMVS_EINVAL, "unknown arithmetic mode");
    *fast = m == AMVS_MODE_FAST;
    if (*fast && !usable_pairs(c))
        return fail(c, AMVS_EUNSUPPORTED,
                    "fast mode needs 8-bit images (every uploaded view exactly code/255) and packed sampling");
    return AMVS_OK;
}

void resolve_timing(amvs_ctx *c)
{
    if (!c->timing_pending) return;
    c->timing_pending = false;
    if (hipEventSynchronize(c->ev[3].get()) != hipSuccess) return;
    if (c->timing_groups > 0 && c->timing_overlapped) {
        // Groups on two streams: the phases of different groups overlap, so each figure is the UNION of its groups'
        // intervals (chip time, as on one stream), not their sum.  Group g ran on stream g % 2, after group g - 2.
        std::vector<std::pair<float, float>> iv[3];
        for (int g = 0; g < c->timing_groups; ++g) {
            float t[4] = {0.f, 0.f, 0.f, 0.f};
            if (g >= 2) (void)hipEventElapsedTime(&t[0], c->ev[0].get(), c->ev_groups[3 * (g - 2) + 2]);
            for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&t[k + 1], c->ev[0].get(), c->ev_groups[3 * g + k]);
            for (int k = 0; k < 3; ++k) iv[k].emplace_back(t[k], t[k + 1]);
        }
        double u[3];
        for (int k = 0; k < 3; ++k) {
            std::sort(iv[k].begin(), iv[k].end());
            double sum = 0.0, end = -1.0;
            for (const auto &x : iv[k]) {
                const double lo = std::max<double>(x.first, end), hi = x.second;
                if (hi > lo) sum += hi - lo;
                end = std::max<double>(end, hi);
            }
            u[k] = sum;
        }
        c->timing.init_ms = u[0]; c->timing.sweep_ms = u[1]; c->timing.confidence_ms = u[2];
    } else if (c->timing_groups > 0) {
        // PatchMatch: per view group [start | init | steps | confidence]
        double t_init = 0, t_sweep = 0, t_conf = 0;
        hipEvent_t prev = c->ev[0].get();
        for (int g = 0; g < c->timing_groups; ++g) {
            float a = 0.f, b = 0.f, d = 0.f;
            (void)hipEventElapsedTime(&a, prev, c->ev_groups[3 * g]);
            (void)hipEventElapsedTime(&b, c->ev_groups[3 * g], c->ev_groups[3 * g + 1]);
            (void)hipEventElapsedTime(&d, c->ev_groups[3 * g + 1], c->ev_groups[3 * g + 2]);
            t_init += a; t_sweep += b; t_conf += d;
            prev = c->ev_groups[3 * g + 2];
        }
        c->timing.init_ms = t_init; c->timing.sweep_ms = t_sweep; c->timing.confidence_ms = t_conf;
    } else {
        float ms0 = 0.f, ms1 = 0.f, ms2 = 0.f;
        (void)hipEventElapsedTime(&ms0, c->ev[0].get(), c->ev[1].get());
        (void)hipEventElapsedTime(&ms1, c->ev[1].get(), c->ev[2].get());
        (void)hipEventElapsedTime(&ms2, c->ev[2].get(), c->ev[3].get());
        c->timing.init_ms = ms0; c->timing.sweep_ms = ms1; c->timing.confidence_ms = ms2;
    }
}

// every view id names a view with a resident colour image
int check_colour_views(amvs_ctx *c, int n, const int *view_ids)
{
    for (int j = 0; j < n; ++j)
        if (view_ids[j] < 0 || view_ids[j] >= c->n_views || !c->have_bgr[view_ids[j]])
            return fail(c, AMVS_EINVAL, "view " + std::to_string(view_ids[j]) + " has no resident colour image (amvs_set_view_bgr8)");
    return AMVS_OK;
}

// the resident colour images of `view_ids` in map order (device-to-device; the images of a scene are rarely in that
// order already)
int gather_colours(amvs_ctx *c, int n, const int *view_ids, amvs::DeviceBuffer<unsigned char> &out)
{
    const size_t bytes = 3 * (size_t)c->H * c->W;
    HIPCHK(c, out.reserve(bytes * n, c->cache));
    for (int j = 0; j < n; ++j)
        HIPCHK(c, hipMemcpyAsync(out.get() + bytes * j, c->d_bgr.get() + bytes * view_ids[j], bytes, hipMemcpyDeviceToDevice,
                                 c->stream));
    return AMVS_OK;
}

// host maps of a post-step (n floats each) staged on the device: `depth` / `conf` then point into the copies
int stage_maps(amvs_ctx *c, size_t n, const float *&depth, const float *&conf, amvs::DeviceBuffer<float> (&copy)[2])
{
    int rc;
    if ((rc = upload(c, depth, n, copy[0])) || (rc = upload(c, conf, n, copy[1]))) return rc;
    depth = copy[0].get();
    conf = copy[1].get();
    return AMVS_OK;
}

}  // namespace host
}  // namespace amvs

using namespace amvs::host;

#pragma GCC visibility push(default)
extern "C" {

#ifdef AMVS_CHECK_INDICES
const char *amvs_version(void) { return "amvs 0.1 (gfx950) +index-checks"; }
#else
#ifdef AMVS_STEP_TRACE
const char *amvs_version(void) { return "amvs 0.1 (gfx950) +step-trace"; }
#else
const char *amvs_version(void) { return "amvs 0.1 (gfx950)"; }
#endif
#endif

int amvs_index_check(uint64_t report[4], int reset)
{
    if (!report) return AMVS_EINVAL;
    index_report(report, reset != 0);
    return AMVS_OK;
}

const char *amvs_last_error(const amvs_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int amvs_create(int device_id, int H, int W, int n_views, const float K[9], const float K_inv[9],
                amvs_ctx **out)
{
    if (!out) return fail(nullptr, AMVS_EINVAL, "out is NULL");
    *out = nullptr;
    if (H < 2 || W < 2 || n_views < 1 || !K || !K_inv)
        return fail(nullptr, AMVS_EINVAL, "bad image size / view count / intrinsics");
    if ((long long)H * W > (1ll << 29)) return fail(nullptr, AMVS_EINVAL, "image too large (H*W must stay below 2^29: 32-bit pixel indices, 3 per normal)");
    if (H > (1 << 23) || W > (1 << 23)) return fail(nullptr, AMVS_EINVAL, "image side above 2^23 (24-bit row arithmetic)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, AMVS_EHIP, "no HIP device available (this backend has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, AMVS_EINVAL, "device_id out of range");
    std::unique_ptr<amvs_ctx, int (*)(amvs_ctx *)> c(new amvs_ctx(), amvs_destroy);
    c->device = device_id; c->H = H; c->W = W; c->n_views = n_views;
    // rows of an image are W floats; one extra 256-byte line of tail padding per image
    c->stride = (((long long)H * W + 63) / 64) * 64 + 64;
    std::memcpy(c->K, K, 36);
    std::memcpy(c->Kinv, K_inv, 36);
    c->R.resize(n_views); c->t.resize(n_views); c->have.assign(n_views, 0);
    c->exact8.assign(n_views, 0);
    c->have_bgr.assign(n_views, 0);
    c->pstride = ((amvs::pair_map_elems(H, W) + 63) / 64) * 64 + 64;
    // (a failure below destroys the partial context: amvs_destroy; its error goes to amvs_last_error(NULL))
    HIPCHK(nullptr, hipSetDevice(device_id));
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && ncu > 0)
            c->n_cu = ncu;
    }
    HIPCHK(nullptr, c->own_stream.create());
    c->stream = c->own_stream.get();
    for (auto &ev : c->ev) HIPCHK(nullptr, ev.create(true));
    HIPCHK(nullptr, c->d_images.reserve(c->stride * n_views, c->cache));
    HIPCHK(nullptr, hipMemsetAsync(c->d_images.get(), 0, sizeof(float) * c->stride * n_views, c->stream));
    HIPCHK(nullptr, c->d_pairs.reserve(c->pstride * n_views, c->cache));
    HIPCHK(nullptr, hipMemsetAsync(c->d_pairs.get(), 0, sizeof(uint16_t) * c->pstride * n_views, c->stream));
    HIPCHK(nullptr, c->d_flag.reserve(n_views, c->cache));
    HIPCHK(nullptr, hipMemsetAsync(c->d_flag.get(), 0, sizeof(int) * n_views, c->stream));
    *out = c.release();
    return AMVS_OK;
}

int amvs_destroy(amvs_ctx *c)
{
    if (!c) return AMVS_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    (void)amvs_comm_destroy(c);
    delete c;                           // streams and events first, then the device buffers and the scratch cache (amvs_ctx.h)
    return AMVS_OK;
}

int amvs_set_stream(amvs_ctx *c, void *hip_stream)
{
    if (!c) return AMVS_EINVAL;
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream.get();
    return AMVS_OK;
}

int amvs_sync(amvs_ctx *c)
{
    if (!c) return AMVS_EINVAL;
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_timing(c);
    return checked(c, AMVS_OK);
}

int amvs_get_timing(const amvs_ctx *c, amvs_timing *out)
{
    if (!c || !out) return AMVS_EINVAL;
    resolve_timing(const_cast<amvs_ctx *>(c));
    *out = c->timing;
    return AMVS_OK;
}

int amvs_sampling_mode(const amvs_ctx *c) { return c && usable_pairs(c) ? 1 : 0; }

int amvs_set_mode(amvs_ctx *c, int mode)
{
    if (!c) return AMVS_EINVAL;
    if (mode != AMVS_MODE_EXACT && mode != AMVS_MODE_FAST) return fail(c, AMVS_EINVAL, "unknown arithmetic mode");
    c->mode = mode;
    return AMVS_OK;
}

int amvs_get_mode(const amvs_ctx *c) { return c ? c->mode : AMVS_EINVAL; }

int amvs_set_sampling(amvs_ctx *c, int force_f32)
{
    if (!c) return AMVS_EINVAL;
    c->force_f32 = force_f32 != 0;
    return AMVS_OK;
}

}  // extern "C"
#pragma GCC visibility pop
