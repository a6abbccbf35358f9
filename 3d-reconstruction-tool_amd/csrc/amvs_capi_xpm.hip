// amvs_capi_xpm.hip -- the extended-mode entry points of the C ABI (include/amvs.h; kernels: amvs_extended.hip).
#include "amvs_ctx.h"

#include <algorithm>
#include <cmath>

using namespace amvs::host;

#pragma GCC visibility push(default)
extern "C" {

// ---- extended mode (csrc/amvs_extended.hip) ----
static int xpm_begin(amvs_ctx *c, int n_ref, const int *ref_ids, const int *src_ids, int n_src, const amvs_xpm_params *p,
                     void *depth_all, void *normal_all, void *cost_all, amvs::XArgs &a)
{
    if (!c) return AMVS_EINVAL;
    if (!p || !depth_all || !normal_all || !cost_all) return fail(c, AMVS_EINVAL, "NULL argument");
    if (p->patch_size < 3 || p->patch_size > 31 || (p->patch_size & 1) == 0 || p->window_stride < 1)
        return fail(c, AMVS_EINVAL, "extended mode: odd patch_size in 3..31 and window_stride >= 1");
    if (n_src < 2 || n_src > AMVS_MAX_SRC) return fail(c, AMVS_EUNSUPPORTED, "n_src outside [2, 6]");
    int rc = bind_device(c);
    if (rc) return rc;
    if ((rc = upload_jobs(c, n_ref, ref_ids, src_ids, n_src, 0, true))) return rc;
    const size_t hw = (size_t)c->H * c->W;
    HIPCHK(c, c->d_xcand_d.reserve(hw * n_ref, c->cache));
    HIPCHK(c, c->d_xcand_n.reserve(3 * hw * n_ref, c->cache));
    if ((rc = upload(c, src_ids, (size_t)n_ref * n_src, c->d_xsrc))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    a = amvs::XArgs{};
    a.H = c->H; a.W = c->W; a.n_jobs = n_ref; a.n_src = n_src;
    a.jobs = c->d_jobs.get(); a.images = c->d_images.get(); a.img_stride = c->stride;
    a.pairs = usable_pairs(c); a.pair_stride = c->pstride;
    a.depth = (float *)depth_all; a.normal = (float *)normal_all; a.cost = (float *)cost_all;
    a.snap_depth = a.depth; a.snap_normal = a.normal;
    a.cand_d = c->d_xcand_d.get(); a.cand_n = c->d_xcand_n.get(); a.src_view = c->d_xsrc.get();
    a.patch = p->patch_size; a.stride = p->window_stride;
    a.depth_min = p->depth_min; a.depth_max = p->depth_max;
    return AMVS_OK;
}

int amvs_xpm_init(amvs_ctx *c, int n_ref, const int *ref_ids, const int *src_ids, int n_src, const amvs_xpm_params *p,
                  uint64_t seed, void *depth_all, void *normal_all, void *cost_all)
{
    amvs::XArgs a;
    int rc = xpm_begin(c, n_ref, ref_ids, src_ids, n_src, p, depth_all, normal_all, cost_all, a);
    if (rc) return rc;
    a.seed = seed;
    HIPCHK(c, amvs::launch_xpm_init(a, p->log_depth_scale, p->log_depth_min, c->stream));
    return AMVS_OK;
}

// ranges / hypothesis set of one iteration (shared by amvs_xpm_iterate and amvs_xpm_step)
static void xpm_iteration_args(amvs::XArgs &a, const amvs_xpm_params *p, int iteration, uint64_t seed)
{
    a.seed = seed;
    const double shrink = std::pow(0.5, iteration);
    a.rel_range = (float)std::max(0.2 * shrink, 0.004);
    a.nrm_range = (float)std::max(0.4 * shrink, 0.01);
    a.n_refine = p->num_refine < 0 ? 0 : (p->num_refine > 6 ? 6 : p->num_refine);
    a.with_random = iteration < 2;
    a.with_view_cand = p->view_propagation ? 1 : 0;
}

static int xpm_run_phase(amvs_ctx *c, amvs::XArgs a, int n_src, int iteration, int phase, void *cost_out)
{
    if (phase == AMVS_XPM_PHASE_CANDIDATES) {
        // view propagation from a snapshot: the candidates of this iteration come from source
        // (iteration mod n_src) of every view, read from maps no call of this iteration has written
        if (a.with_view_cand) {
            a.colour = iteration % n_src;
            HIPCHK(c, amvs::launch_xpm_view_candidates(a, c->stream));
        }
    } else if (phase == AMVS_XPM_PHASE_RED || phase == AMVS_XPM_PHASE_BLACK) {
        a.colour = phase - AMVS_XPM_PHASE_RED;
        a.draw = (unsigned)(1 + 2 * iteration + a.colour);
        HIPCHK(c, amvs::launch_xpm_sweep(a, c->stream));
    } else {
        if (!cost_out) return fail(c, AMVS_EINVAL, "NULL output");
        HIPCHK(c, amvs::launch_xpm_eval(a, (float *)cost_out, c->stream));
    }
    return AMVS_OK;
}

static int xpm_phases(amvs_ctx *c, int n_ref, const int *ref_ids, const int *src_ids, int n_src, const amvs_xpm_params *p,
                      int iteration, uint64_t seed, int first_phase, int last_phase, void *depth_all, void *normal_all,
                      void *cost_all, const void *snapshot_depth, const void *snapshot_normal, void *cost_out)
{
    amvs::XArgs a;
    int rc = xpm_begin(c, n_ref, ref_ids, src_ids, n_src, p, depth_all, normal_all, cost_all, a);
    if (rc) return rc;
    if (iteration < 0) return fail(c, AMVS_EINVAL, "negative iteration");
    if ((snapshot_depth == nullptr) != (snapshot_normal == nullptr)) return fail(c, AMVS_EINVAL, "snapshot: both maps or none");
    if (snapshot_depth) { a.snap_depth = (const float *)snapshot_depth; a.snap_normal = (const float *)snapshot_normal; }
    xpm_iteration_args(a, p, iteration, seed);
    for (int phase = first_phase; phase <= last_phase; ++phase)
        if ((rc = xpm_run_phase(c, a, n_src, iteration, phase, cost_out))) return rc;
    return AMVS_OK;
}

int amvs_xpm_step(amvs_ctx *c, int n_ref, const int *ref_ids, const int *src_ids, int n_src, const amvs_xpm_params *p,
                  int iteration, uint64_t seed, int phase, void *depth_all, void *normal_all, void *cost_all,
                  const void *snapshot_depth, const void *snapshot_normal, void *cost_out)
{
    if (!c) return AMVS_EINVAL;
    if (phase < AMVS_XPM_PHASE_CANDIDATES || phase > AMVS_XPM_PHASE_EVAL) return fail(c, AMVS_EINVAL, "unknown phase");
    return xpm_phases(c, n_ref, ref_ids, src_ids, n_src, p, iteration, seed, phase, phase, depth_all, normal_all, cost_all,
                      snapshot_depth, snapshot_normal, cost_out);
}

int amvs_xpm_iterate(amvs_ctx *c, int n_ref, const int *ref_ids, const int *src_ids, int n_src, const amvs_xpm_params *p,
                     int iteration, uint64_t seed, void *depth_all, void *normal_all, void *cost_all,
                     const void *snapshot_depth, const void *snapshot_normal)
{
    if (!c) return AMVS_EINVAL;
    return xpm_phases(c, n_ref, ref_ids, src_ids, n_src, p, iteration, seed, AMVS_XPM_PHASE_CANDIDATES, AMVS_XPM_PHASE_BLACK,
                      depth_all, normal_all, cost_all, snapshot_depth, snapshot_normal, nullptr);
}

int amvs_xpm_fetch_candidates(amvs_ctx *c, int n_ref, float *cand_depth_out, float *cand_normal_out)
{
    if (!c) return AMVS_EINVAL;
    const size_t hw = (size_t)c->H * c->W;
    if (!cand_depth_out || !cand_normal_out || n_ref < 1 || hw * n_ref > c->d_xcand_d.capacity() ||
        3 * hw * n_ref > c->d_xcand_n.capacity())
        return fail(c, AMVS_EINVAL, "bad argument / no candidates");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(cand_depth_out, c->d_xcand_d.get(), 4 * hw * n_ref, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cand_normal_out, c->d_xcand_n.get(), 12 * hw * n_ref, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return checked(c, AMVS_OK);
}

int amvs_xpm_consistency(amvs_ctx *c, int n_ref, const int *ref_ids, const int *src_ids, int n_src,
                         const amvs_xpm_params *p, void *depth_all, void *normal_all, void *cost_all, void *conf_out)
{
    amvs::XArgs a;
    int rc = xpm_begin(c, n_ref, ref_ids, src_ids, n_src, p, depth_all, normal_all, cost_all, a);
    if (rc) return rc;
    if (!conf_out) return fail(c, AMVS_EINVAL, "NULL output");
    HIPCHK(c, amvs::launch_xpm_consistency(a, (float *)conf_out, p->consistency_px, p->consistency_rel, c->stream));
    return AMVS_OK;
}

}  // extern "C"
#pragma GCC visibility pop
