// amvs_capi_sweep.hip -- the plane-sweep entry points of the C ABI (include/amvs.h).
//
// Host-side orchestration of DenseStereoReconstructor._plane_sweep_torch (dense_stereo.py:222-316).
#include "amvs_ctx.h"

using namespace amvs::host;

#pragma GCC visibility push(default)
extern "C" {

int amvs_set_sweep_tuning(amvs_ctx *c, int tile_rows, int chunk)
{
    if (!c) return AMVS_EINVAL;
    if (tile_rows < 0 || tile_rows > AMVS_SWEEP_MAX_TH8 || chunk < 0)
        return fail(c, AMVS_EINVAL, "plane-sweep tuning out of range");
    c->tuning.sweep_tile_rows = tile_rows; c->tuning.sweep_chunk = chunk;
    return AMVS_OK;
}

int amvs_plan_plane_sweep(const amvs_plan_device *dev, const amvs_plan_tuning *tuning, const amvs_plan_facts *facts, int n_ref,
                          int D, amvs_sweep_plan *plan)
{
    if (!dev || !tuning || !facts || !plan || dev->H < 1 || dev->W < 1 || dev->n_cu < 1 || n_ref < 1 || D < 1 ||
        facts->out_width < 1 || facts->sweep_max_th < 1 || facts->sweep_max_th8 < 1 || facts->sweep_max_chunk < 1)
        return AMVS_EINVAL;
    const amvs::plan::PlaneSweepPlan s = amvs::plan::plan_plane_sweep(*dev, plan_tuning(*tuning), *facts, n_ref, D);
    *plan = amvs_sweep_plan{s.TH, s.tiles_x, s.tiles_y, s.chunk, s.n_chunks, s.key8};
    return AMVS_OK;
}

int amvs_plane_sweep_device(amvs_ctx *c, int n_ref, const int *ref_ids, const int *nbr_ids, int n_nbr,
                            const float *depths, int D, int patch_size, float thresh, void *depth_dev,
                            void *conf_dev)
{
    if (!c) return AMVS_EINVAL;
    if (!depths || D < 1 || D > 65535 || !depth_dev || !conf_dev) return fail(c, AMVS_EINVAL, "bad plane list / outputs");
    int rc = bind_device(c);
    if (rc) return rc;
    if ((rc = check_patch_src(c, patch_size, n_nbr))) return rc;
    int fast = 0;
    if ((rc = resolve_fast(c, AMVS_MODE_DEFAULT, &fast))) return rc;
    if ((rc = upload_jobs(c, n_ref, ref_ids, nbr_ids, n_nbr, fast ? patch_size : 0))) return rc;
    if ((rc = upload(c, depths, D, c->d_planes))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t hw = (size_t)c->H * c->W;
    HIPCHK(c, c->d_keys.reserve(hw * n_ref, c->cache));
    amvs::SweepArgs a{};
    a.H = c->H; a.W = c->W;
    a.n_jobs = n_ref; a.D = D;
    a.pairs = usable_pairs(c);
    const amvs::plan::PlaneSweepPlan plan =
        amvs::plan::plan_plane_sweep(plan_device(c, a.pairs != nullptr), c->tuning, plan_facts(patch_size, n_nbr, fast != 0, a.pairs != nullptr, 0u), n_ref, D);
    a.TH = plan.TH; a.tiles_x = plan.tiles_x; a.tiles_y = plan.tiles_y;
    a.chunk = plan.chunk; a.n_chunks = plan.n_chunks; a.key8 = plan.key8;
    c->last_tile_rows = a.TH;
    a.img_stride = c->stride;
    a.images = c->d_images.get();
    a.pair_stride = c->pstride;
    a.fast = fast;
    a.depths = c->d_planes.get();
    a.thresh = thresh;
    if (!fast && amvs::patch_compiled(patch_size)) {
        // the exact sweep loads the reference views' window statistics (plane-invariant) from the resident maps
        if ((rc = ensure_stats(c, patch_size))) return rc;
        a.ref_mean = c->stats[patch_size].mean.get();
        a.ref_var = c->stats[patch_size].var.get();
    }
    a.depth_out = (float *)depth_dev; a.conf_out = (float *)conf_dev;
    a.keys = c->d_keys.get();
    a.jobs = c->d_jobs.get();
    resolve_timing(c);
    c->timing = amvs_timing{};
    c->timing_groups = 0;
    c->n_step_events = 0;
    HIPCHK(c, hipEventRecord(c->ev[0].get(), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_keys.get(), 0, sizeof(unsigned) * hw * n_ref, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[1].get(), c->stream));
    HIPCHK(c, amvs::launch_sweep(patch_size, n_nbr, a, c->stream));
    HIPCHK(c, amvs::launch_sweep_finish(a, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[2].get(), c->stream));
    HIPCHK(c, hipEventRecord(c->ev[3].get(), c->stream));
    c->timing.sweep_launches = 1;
    c->timing.pixel_hypotheses = (int64_t)n_ref * c->H * c->W * D;
    c->timing_pending = true;
    return AMVS_OK;
}

int amvs_plane_sweep(amvs_ctx *c, int ref, const int *nbr_ids, int n_nbr, const float *depths, int D,
                     int patch_size, float thresh, float *depth_out, float *conf_out)
{
    if (!c) return AMVS_EINVAL;
    if (!depth_out || !conf_out) return fail(c, AMVS_EINVAL, "NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    if ((rc = ensure_slots(c, 1))) return rc;
    c->pm_resumable = false;                    // the maps below land in slot 0 of the PatchMatch state
    const size_t hw = (size_t)c->H * c->W;
    rc = amvs_plane_sweep_device(c, 1, &ref, nbr_ids, n_nbr, depths, D, patch_size, thresh,
                                 c->d_depth[0].get(), c->d_aux.get());
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(depth_out, c->d_depth[0].get(), 4 * hw, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(conf_out, c->d_aux.get(), 4 * hw, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_timing(c);
    return checked(c, AMVS_OK);
}

int amvs_plane_sweep_batch(amvs_ctx *c, int n_ref, const int *ref_ids, const int *nbr_ids, int n_nbr,
                           const float *depths, int D, int patch_size, float thresh)
{
    if (!c) return AMVS_EINVAL;
    if (n_ref <= 0) return fail(c, AMVS_EINVAL, "empty batch");
    int rc = bind_device(c);
    if (rc) return rc;
    const size_t hw = (size_t)c->H * c->W;
    c->n_sweep = 0;
    HIPCHK(c, c->d_sweep_depth.reserve(hw * n_ref, c->cache));
    HIPCHK(c, c->d_sweep_conf.reserve(hw * n_ref, c->cache));
    rc = amvs_plane_sweep_device(c, n_ref, ref_ids, nbr_ids, n_nbr, depths, D, patch_size, thresh,
                                 c->d_sweep_depth.get(), c->d_sweep_conf.get());
    if (rc) return rc;
    c->n_sweep = n_ref;
    return checked(c, AMVS_OK);
}

int amvs_fetch_sweep_maps(amvs_ctx *c, int first, int count, float *depth_out, float *conf_out)
{
    if (!c) return AMVS_EINVAL;
    if (first < 0 || count < 0 || first + count > c->n_sweep || !depth_out || !conf_out)
        return fail(c, AMVS_EINVAL, "sweep maps out of range (run amvs_plane_sweep_batch first)");
    int rc = bind_device(c);
    if (rc) return rc;
    const size_t hw = (size_t)c->H * c->W;
    HIPCHK(c, hipMemcpyAsync(depth_out, c->d_sweep_depth.get() + first * hw, 4 * hw * count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(conf_out, c->d_sweep_conf.get() + first * hw, 4 * hw * count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_timing(c);
    return checked(c, AMVS_OK);
}

}  // extern "C"
#pragma GCC visibility pop
