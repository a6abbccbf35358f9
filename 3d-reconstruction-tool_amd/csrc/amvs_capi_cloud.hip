// amvs_capi_cloud.hip -- the point-cloud entry points of the C ABI (include/amvs.h): back-projection, fusion, the
// steps on the resident cloud, its normals from the depth maps, the neighbour statistic and the PLY writers; and the
// cross-view depth-map filter of include/amvs_depth.h, whose maps those steps consume.
#include "amvs_ctx.h"
#include "../../include/amvs_depth.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <utility>
#include <vector>

using namespace amvs::host;

#pragma GCC visibility push(default)
extern "C" {

int amvs_stereo_backproject(amvs_ctx *c, int n_maps, const void *depth, const void *conf, int maps_where,
                            const uint8_t *colors_bgr_host, const double K_inv[9], const double *poses,
                            float min_confidence, int64_t *per_map_counts, int64_t *total)
{
    if (!c) return AMVS_EINVAL;
    if (n_maps < 1 || !colors_bgr_host || !K_inv || !poses || !total || maps_where < 0 || maps_where > 2)
        return fail(c, AMVS_EINVAL, "bad argument");
    if (maps_where == 2 ? n_maps != c->n_sweep : (!depth || !conf))
        return fail(c, AMVS_EINVAL, maps_where == 2 ? "n_maps differs from the resident plane-sweep batch" : "NULL maps");
    int rc = bind_device(c);
    if (rc) return rc;
    const size_t hw = (size_t)c->H * c->W, n = hw * (size_t)n_maps;
    c->cloud = Cloud{};
    amvs::DeviceBuffer<unsigned char> dbgr;
    amvs::DeviceBuffer<float> copy[2];
    const float *dd = maps_where == 2 ? c->d_sweep_depth.get() : (const float *)depth;
    const float *dc = maps_where == 2 ? c->d_sweep_conf.get() : (const float *)conf;
    if ((rc = upload(c, colors_bgr_host, 3 * n, dbgr))) return rc;
    if (maps_where == 0 && (rc = stage_maps(c, n, dd, dc, copy))) return rc;
    long long tot = 0;
    std::vector<long long> per(n_maps, 0);
    const hipError_t e = amvs::stereo_backproject(dd, dc, dbgr.get(), n_maps, c->H, c->W, K_inv, poses, min_confidence, c->cache,
                                                  c->cloud.pts, c->cloud.rgb, &tot, per.data(), c->stream);
    if (e != hipSuccess) return fail(c, AMVS_EHIP, std::string("stereo_backproject: ") + hipGetErrorString(e));
    c->cloud.n = tot;
    *total = tot;
    if (per_map_counts) for (int j = 0; j < n_maps; ++j) per_map_counts[j] = per[j];
    return checked(c, AMVS_OK);
}

int amvs_stereo_backproject_views(amvs_ctx *c, int n_maps, const int *view_ids, const double K_inv[9], const double *poses,
                                  float min_confidence, int64_t *per_map_counts, int64_t *total)
{
    if (!c) return AMVS_EINVAL;
    if (n_maps < 1 || !view_ids || !K_inv || !poses || !total) return fail(c, AMVS_EINVAL, "bad argument");
    if (n_maps != c->n_sweep) return fail(c, AMVS_EINVAL, "n_maps differs from the resident plane-sweep batch");
    int rc = check_colour_views(c, n_maps, view_ids);
    if (rc) return rc;
    if ((rc = bind_device(c))) return rc;
    c->cloud = Cloud{};
    amvs::DeviceBuffer<unsigned char> dbgr;
    if ((rc = gather_colours(c, n_maps, view_ids, dbgr))) return rc;
    long long tot = 0;
    std::vector<long long> per(n_maps, 0);
    const hipError_t e = amvs::stereo_backproject(c->d_sweep_depth.get(), c->d_sweep_conf.get(), dbgr.get(), n_maps, c->H, c->W,
                                                  K_inv, poses, min_confidence, c->cache, c->cloud.pts, c->cloud.rgb, &tot,
                                                  per.data(), c->stream);
    if (e != hipSuccess) return fail(c, AMVS_EHIP, std::string("stereo_backproject_views: ") + hipGetErrorString(e));
    c->cloud.n = tot;
    *total = tot;
    if (per_map_counts) for (int j = 0; j < n_maps; ++j) per_map_counts[j] = per[j];
    return checked(c, AMVS_OK);
}

int amvs_cloud_knn_mean_distance(amvs_ctx *c, int k, double *mean_out)
{
    if (!c) return AMVS_EINVAL;
    if (!mean_out || c->cloud.n < 1) return fail(c, AMVS_EINVAL, "no resident cloud / NULL output");
    if (!amvs::knn_supported(k)) return fail(c, AMVS_EUNSUPPORTED, "k not compiled in (8, 10, 16, 20, 32)");
    if (c->cloud.n < k) return fail(c, AMVS_EINVAL, "fewer points than neighbours");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::knn_mean_distance(c->cloud.pts.get(), c->cloud.n, k, mean_out, c->cache, c->stream, true));
    return checked(c, AMVS_OK);
}

int amvs_cloud_voxel_downsample(amvs_ctx *c, const uint8_t *keep_mask, double voxel_size, int64_t *count)
{
    if (!c) return AMVS_EINVAL;
    if (!count || !(voxel_size > 0.0)) return fail(c, AMVS_EINVAL, "bad argument");
    int rc = bind_device(c);
    if (rc) return rc;
    Cloud next;                         // (the resident cloud is the input: replaced once the new one is made)
    const hipError_t e = amvs::voxel_downsample(c->cloud.pts.get(), c->cloud.rgb.get(), c->cloud.n, keep_mask, voxel_size,
                                                c->cache, next.pts, next.rgb, &next.n, c->stream);
    if (e != hipSuccess) return fail(c, AMVS_EHIP, std::string("voxel_downsample: ") + hipGetErrorString(e));
    c->cloud = std::move(next);
    *count = c->cloud.n;
    return checked(c, AMVS_OK);
}

int amvs_cloud_take(amvs_ctx *c, const int64_t *indices, int64_t m)
{
    if (!c) return AMVS_EINVAL;
    if (m < 0 || (m > 0 && !indices)) return fail(c, AMVS_EINVAL, "bad argument");
    if (c->cloud.n < 1 && m > 0) return fail(c, AMVS_EINVAL, "no resident cloud");
    int rc = bind_device(c);
    if (rc) return rc;
    static_assert(sizeof(long long) == sizeof(int64_t), "index width");
    Cloud next;                         // (the resident cloud is the input: replaced once the new one is made)
    const hipError_t e = amvs::cloud_take(c->cloud.pts.get(), c->cloud.rgb.get(), c->cloud.n, (const long long *)indices, m,
                                          c->cache, next.pts, next.rgb, c->stream);
    if (e == hipErrorInvalidValue) return fail(c, AMVS_EINVAL, "cloud_take: index outside the resident cloud");
    if (e != hipSuccess) return fail(c, AMVS_EHIP, std::string("cloud_take: ") + hipGetErrorString(e));
    next.n = m;
    c->cloud = std::move(next);
    return checked(c, AMVS_OK);
}

int amvs_knn_supported(int k) { return amvs::knn_supported(k) ? 1 : 0; }

int amvs_fuse_filter(amvs_ctx *c, int n_maps, const void *depth, const void *conf, int maps_on_device,
                     const uint8_t *colors_bgr_host, const double K_inv[9], const double *poses,
                     float min_views, int do_filter, int64_t counts[2])
{
    if (!c) return AMVS_EINVAL;
    if (n_maps < 1 || !depth || !conf || !colors_bgr_host || !K_inv || !poses || !counts)
        return fail(c, AMVS_EINVAL, "bad argument");
    int rc = bind_device(c);
    if (rc) return rc;
    const size_t hw = (size_t)c->H * c->W, n = hw * (size_t)n_maps;
    c->cloud = Cloud{};
    amvs::DeviceBuffer<unsigned char> dbgr;
    amvs::DeviceBuffer<float> copy[2];
    const float *dd = (const float *)depth, *dc = (const float *)conf;
    if ((rc = upload(c, colors_bgr_host, 3 * n, dbgr))) return rc;
    if (!maps_on_device && (rc = stage_maps(c, n, dd, dc, copy))) return rc;
    long long cnt[2] = {0, 0};
    const hipError_t e = amvs::fuse_filter(dd, dc, dbgr.get(), n_maps, c->H, c->W, K_inv, poses, min_views, do_filter != 0,
                                           c->cache, c->cloud.pts, c->cloud.rgb, cnt, c->stream);
    if (e != hipSuccess) return fail(c, AMVS_EHIP, std::string("fuse_filter: ") + hipGetErrorString(e));
    counts[0] = cnt[0]; counts[1] = cnt[1];
    c->cloud.n = cnt[1];
    return checked(c, AMVS_OK);
}

int amvs_fuse_filter_views(amvs_ctx *c, int n_maps, const int *view_ids, const void *depth_dev, const void *conf_dev,
                           const double K_inv[9], const double *poses, float min_views, int do_filter,
                           int64_t counts[2])
{
    if (!c) return AMVS_EINVAL;
    if (n_maps < 1 || !view_ids || !depth_dev || !conf_dev || !K_inv || !poses || !counts)
        return fail(c, AMVS_EINVAL, "bad argument");
    int rc = check_colour_views(c, n_maps, view_ids);
    if (rc) return rc;
    if ((rc = bind_device(c))) return rc;
    c->cloud = Cloud{};
    amvs::DeviceBuffer<unsigned char> dbgr;
    if ((rc = gather_colours(c, n_maps, view_ids, dbgr))) return rc;
    long long cnt[2] = {0, 0};
    const hipError_t e = amvs::fuse_filter((const float *)depth_dev, (const float *)conf_dev, dbgr.get(), n_maps, c->H, c->W, K_inv,
                                           poses, min_views, do_filter != 0, c->cache, c->cloud.pts, c->cloud.rgb, cnt, c->stream);
    if (e != hipSuccess) return fail(c, AMVS_EHIP, std::string("fuse_filter_views: ") + hipGetErrorString(e));
    counts[0] = cnt[0]; counts[1] = cnt[1];
    c->cloud.n = cnt[1];
    return checked(c, AMVS_OK);
}

int amvs_fetch_cloud(amvs_ctx *c, double *points, uint8_t *colors)
{
    if (!c) return AMVS_EINVAL;
    if (c->cloud.n == 0) return AMVS_OK;
    if (!points || !colors) return fail(c, AMVS_EINVAL, "NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(points, c->cloud.pts.get(), sizeof(double) * 3 * c->cloud.n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(colors, c->cloud.rgb.get(), 3 * c->cloud.n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return checked(c, AMVS_OK);
}

// the parameters amvs_depth_normals and amvs_cloud_normals share, and where the maps are; NULL = fine
static const char *normal_args_error(const amvs_ctx *c, int n_maps, const void *depth, const void *conf, int maps_where,
                                     const double *K, const double *poses, int radius, float jump, int min_points)
{
    if (n_maps < 1 || maps_where < 0 || maps_where > 2) return "bad argument";
    if (!K || !poses) return "NULL K / poses";
    if (radius < 1 || radius > 4) return "radius outside 1 .. 4";
    if (min_points < 3) return "min_points below 3";
    if (!(jump > 0.0f && jump <= FLT_MAX)) return "jump must be positive and finite";
    if (maps_where == 2 ? n_maps != c->n_sweep : (!depth || !conf))
        return maps_where == 2 ? "n_maps differs from the resident plane-sweep batch" : "NULL maps";
    if ((long long)n_maps * c->H * c->W > 0x7FFFFFFFll) return "more than 2^31 - 1 pixels";
    return nullptr;
}

int amvs_depth_normals(amvs_ctx *c, int n_maps, const void *depth, const void *conf, int maps_where, const double K[9],
                       const double *poses, float min_confidence, int radius, float jump, int min_points, int world,
                       int64_t *n_normals)
{
    if (!c) return AMVS_EINVAL;
    if (!n_normals) return fail(c, AMVS_EINVAL, "NULL output");
    if (const char *why = normal_args_error(c, n_maps, depth, conf, maps_where, K, poses, radius, jump, min_points))
        return fail(c, AMVS_EINVAL, why);
    int rc = bind_device(c);
    if (rc) return rc;
    const size_t n = (size_t)c->H * c->W * (size_t)n_maps;
    amvs::DeviceBuffer<float> copy[2];
    const float *dd = maps_where == 2 ? c->d_sweep_depth.get() : (const float *)depth;
    const float *dc = maps_where == 2 ? c->d_sweep_conf.get() : (const float *)conf;
    if (maps_where == 0 && (rc = stage_maps(c, n, dd, dc, copy))) return rc;
    c->depth_normal_maps = 0;
    long long cnt = 0;
    const hipError_t e = amvs::depth_normals(dd, dc, n_maps, c->H, c->W, K, poses, min_confidence, radius, jump, min_points,
                                             world != 0, c->cache, c->d_depth_normals, &cnt, c->stream);
    if (e != hipSuccess) return fail(c, AMVS_EHIP, std::string("depth_normals: ") + hipGetErrorString(e));
    c->depth_normal_maps = n_maps;
    *n_normals = cnt;
    return checked(c, AMVS_OK);
}

int amvs_fetch_depth_normals(amvs_ctx *c, int first, int count, float *out)
{
    if (!c) return AMVS_EINVAL;
    if (!out || first < 0 || count < 1 || (long long)first + count > c->depth_normal_maps)
        return fail(c, AMVS_EINVAL, "NULL output / maps outside the last amvs_depth_normals");
    int rc = bind_device(c);
    if (rc) return rc;
    const size_t per = 3 * (size_t)c->H * c->W;
    HIPCHK(c, hipMemcpyAsync(out, c->d_depth_normals.get() + per * first, sizeof(float) * per * count, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return checked(c, AMVS_OK);
}

int amvs_cloud_normals(amvs_ctx *c, int n_maps, const void *depth, const void *conf, int maps_where, const double K[9],
                       const double *poses, float min_confidence, int radius, float jump, int min_points,
                       float depth_tolerance, int min_views, int64_t counts[2])
{
    if (!c) return AMVS_EINVAL;
    if (!counts) return fail(c, AMVS_EINVAL, "NULL output");
    if (const char *why = normal_args_error(c, n_maps, depth, conf, maps_where, K, poses, radius, jump, min_points))
        return fail(c, AMVS_EINVAL, why);
    if (!(depth_tolerance > 0.0f && depth_tolerance <= FLT_MAX)) return fail(c, AMVS_EINVAL, "depth_tolerance must be positive and finite");
    if (min_views < 1) return fail(c, AMVS_EINVAL, "min_views below 1");
    if (c->cloud.n < 1) return fail(c, AMVS_EINVAL, "no resident cloud");
    int rc = bind_device(c);
    if (rc) return rc;
    const size_t n = (size_t)c->H * c->W * (size_t)n_maps;
    amvs::DeviceBuffer<float> copy[2];
    const float *dd = maps_where == 2 ? c->d_sweep_depth.get() : (const float *)depth;
    const float *dc = maps_where == 2 ? c->d_sweep_conf.get() : (const float *)conf;
    if (maps_where == 0 && (rc = stage_maps(c, n, dd, dc, copy))) return rc;
    c->depth_normal_maps = 0;
    c->cloud.have_normals = false;
    long long cnt[2] = {0, 0};
    const hipError_t e = amvs::cloud_normals(c->cloud.pts.get(), c->cloud.n, dd, dc, n_maps, c->H, c->W, K, poses, min_confidence,
                                             radius, jump, min_points, depth_tolerance, min_views, c->cache, c->d_depth_normals,
                                             c->cloud.nrm, c->cloud.seen, cnt, c->stream);
    if (e != hipSuccess) return fail(c, AMVS_EHIP, std::string("cloud_normals: ") + hipGetErrorString(e));
    c->depth_normal_maps = n_maps;
    c->cloud.have_normals = true;
    counts[0] = cnt[0]; counts[1] = cnt[1];
    return checked(c, AMVS_OK);
}

int amvs_fetch_cloud_normals(amvs_ctx *c, float *normals, int32_t *seen)
{
    if (!c) return AMVS_EINVAL;
    if (c->cloud.n < 1 || !c->cloud.have_normals) return fail(c, AMVS_EINVAL, "the resident cloud has no normals");
    int rc = bind_device(c);
    if (rc) return rc;
    static_assert(sizeof(int) == sizeof(int32_t), "count width");
    if (normals)
        HIPCHK(c, hipMemcpyAsync(normals, c->cloud.nrm.get(), sizeof(float) * 3 * c->cloud.n, hipMemcpyDeviceToHost, c->stream));
    if (seen) HIPCHK(c, hipMemcpyAsync(seen, c->cloud.seen.get(), sizeof(int32_t) * c->cloud.n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return checked(c, AMVS_OK);
}

int amvs_cloud_set(amvs_ctx *c, const double *points, const uint8_t *colors_rgb, int64_t n)
{
    if (!c) return AMVS_EINVAL;
    if (n < 0 || n > 0x7FFFFFFFll || (n > 0 && (!points || !colors_rgb))) return fail(c, AMVS_EINVAL, "bad argument");
    int rc = bind_device(c);
    if (rc) return rc;
    Cloud next;
    if (n > 0) {
        if ((rc = upload(c, points, 3 * (size_t)n, next.pts)) || (rc = upload(c, colors_rgb, 3 * (size_t)n, next.rgb))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        next.n = n;
    }
    c->cloud = std::move(next);
    return checked(c, AMVS_OK);
}

// do the byte ranges [a, a + n) and [b, b + n) share a byte
static bool ranges_overlap(const void *a, const void *b, size_t n)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + n && y < x + n;
}

int amvs_depth_filter(amvs_ctx *c, int n_maps, const void *depth, const void *conf, int maps_where, const double K[9],
                      const double K_inv[9], const double *poses, const int32_t *neighbours, int n_nbr, float min_confidence,
                      float max_px, float max_rel, int min_consistent, int refine, void *depth_out, void *count_out,
                      int out_where, int64_t counts[2])
{
    if (!c) return AMVS_EINVAL;
    if (!counts) return fail(c, AMVS_EINVAL, "NULL output");
    if (n_maps < 1 || maps_where < 0 || maps_where > 2 || out_where < 0 || out_where > 2) return fail(c, AMVS_EINVAL, "bad argument");
    if (!K || !K_inv || !poses) return fail(c, AMVS_EINVAL, "NULL K / K_inv / poses");
    if (out_where == 2 && maps_where != 2) return fail(c, AMVS_EINVAL, "out_where 2 replaces the resident maps: it needs maps_where 2");
    if (maps_where == 2 ? n_maps != c->n_sweep : (!depth || !conf))
        return fail(c, AMVS_EINVAL, maps_where == 2 ? "n_maps differs from the resident plane-sweep batch" : "NULL maps");
    if (out_where != 2 && (!depth_out || !count_out)) return fail(c, AMVS_EINVAL, "NULL output maps");
    if (!(max_px > 0.0f && max_px <= FLT_MAX) || !(max_rel > 0.0f && max_rel <= FLT_MAX))
        return fail(c, AMVS_EINVAL, "max_px and max_rel must be positive and finite");
    if (min_consistent < 1) return fail(c, AMVS_EINVAL, "min_consistent below 1");
    if ((long long)n_maps * c->H * c->W > 0x7FFFFFFFll) return fail(c, AMVS_EINVAL, "more than 2^31 - 1 pixels");
    const size_t n = (size_t)c->H * c->W * (size_t)n_maps;
    if (maps_where == 1 && out_where == 1) {
        const void *in[2] = {depth, conf}, *out[2] = {depth_out, count_out};
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b)
                if (ranges_overlap(in[a], out[b], sizeof(float) * n)) return fail(c, AMVS_EINVAL, "the outputs overlap the inputs");
    }
    if (out_where == 1 && ranges_overlap(depth_out, count_out, sizeof(float) * n)) return fail(c, AMVS_EINVAL, "the outputs overlap");
    // the neighbour rows: the caller's, checked, or every other map in ascending index
    std::vector<int> rows;
    if (neighbours) {
        if (n_nbr < 1) return fail(c, AMVS_EINVAL, "n_nbr below 1");
        std::vector<char> seen((size_t)n_maps);
        for (int j = 0; j < n_maps; ++j) {
            std::fill(seen.begin(), seen.end(), 0);
            for (int k = 0; k < n_nbr; ++k) {
                const int i = neighbours[(size_t)j * n_nbr + k];
                if (i == -1) continue;
                if (i < 0 || i >= n_maps) return fail(c, AMVS_EINVAL, "a neighbour outside -1 .. n_maps - 1");
                if (i == j) return fail(c, AMVS_EINVAL, "a map is its own neighbour");
                if (seen[i]) return fail(c, AMVS_EINVAL, "a neighbour repeated within a row");
                seen[i] = 1;
            }
        }
        rows.assign(neighbours, neighbours + (size_t)n_maps * n_nbr);
    } else {
        n_nbr = n_maps - 1;
        rows.reserve((size_t)n_maps * n_nbr);
        for (int j = 0; j < n_maps; ++j)
            for (int i = 0; i < n_maps; ++i)
                if (i != j) rows.push_back(i);
    }
    int rc = bind_device(c);
    if (rc) return rc;
    amvs::DeviceBuffer<float> copy[2];
    const float *dd = maps_where == 2 ? c->d_sweep_depth.get() : (const float *)depth;
    const float *dc = maps_where == 2 ? c->d_sweep_conf.get() : (const float *)conf;
    if (maps_where == 0 && (rc = stage_maps(c, n, dd, dc, copy))) return rc;
    // device outputs are written where the caller wants them; host outputs and the resident maps get scratch first
    amvs::ScratchCache::Lease scratch;
    float *od = (float *)depth_out, *oc = (float *)count_out;
    if (out_where != 1) {
        HIPCHK(c, c->cache.lease(scratch, 2 * sizeof(float) * n));
        od = scratch.get<float>();
        oc = od + n;
    }
    long long cnt[2] = {0, 0};
    const hipError_t e = amvs::depth_filter(dd, dc, n_maps, c->H, c->W, K, K_inv, poses, rows.data(), n_nbr, min_confidence, max_px,
                                            max_rel, min_consistent, refine != 0, c->cache, od, oc, cnt, c->stream);
    if (e != hipSuccess) return fail(c, AMVS_EHIP, std::string("depth_filter: ") + hipGetErrorString(e));
    if (out_where != 1) {
        void *to_d = out_where == 2 ? (void *)c->d_sweep_depth.get() : depth_out;
        void *to_c = out_where == 2 ? (void *)c->d_sweep_conf.get() : count_out;
        const hipMemcpyKind kind = out_where == 2 ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        hipError_t e2 = hipMemcpyAsync(to_d, od, sizeof(float) * n, kind, c->stream);
        if (e2 == hipSuccess) e2 = hipMemcpyAsync(to_c, oc, sizeof(float) * n, kind, c->stream);
        const hipError_t e3 = hipStreamSynchronize(c->stream);      // (also on failure: the lease goes back with nothing in flight)
        if (e2 != hipSuccess || e3 != hipSuccess)
            return fail(c, AMVS_EHIP, std::string("depth_filter copy: ") + hipGetErrorString(e2 != hipSuccess ? e2 : e3));
    }
    counts[0] = cnt[0]; counts[1] = cnt[1];
    return checked(c, AMVS_OK);
}

int amvs_knn_mean_distance(amvs_ctx *c, const double *points, int64_t n, int k, double *mean_out)
{
    if (!c) return AMVS_EINVAL;
    if (!points || !mean_out || n < 1) return fail(c, AMVS_EINVAL, "NULL argument / empty cloud");
    if (!amvs::knn_supported(k)) return fail(c, AMVS_EUNSUPPORTED, "k not compiled in (8, 10, 16, 20, 32)");
    if (n < k) return fail(c, AMVS_EINVAL, "fewer points than neighbours");
    if (n > (1ll << 30)) return fail(c, AMVS_EINVAL, "cloud too large (32-bit point indices)");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::knn_mean_distance(points, (long long)n, k, mean_out, c->cache, c->stream));
    return checked(c, AMVS_OK);
}

// "%.6f" of a double, the bytes printf writes (correctly rounded decimal expansion of the exact binary value,
// ties to even -- glibc), without printf for the common case: for |x| < 1e9 the scaled value x * 1e6 splits
// into an integer n (exact as a double: below 2^53) and a residual r = fma(|x|, 1e6, -n), which is exact up to
// one rounding far below the decision margin; the sixth decimal rounds up iff r > 1/2.  A residual within 1e-9
// of 1/2 (true ties exist: 0.0078125 * 1e6 = 7812.5) and everything outside the range goes through snprintf.
// (The per-point printf was 40 % of the CLI-default run's end-to-end time: 24 of 61 ms for 56 k points.)
static inline char *put_u64(char *o, uint64_t v)
{
    char tmp[24];
    int k = 0;
    do { tmp[k++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (k) *o++ = tmp[--k];
    return o;
}

static inline char *put_f6(char *o, double x)
{
    const double ax = std::fabs(x);
    if (!(ax < 1e9)) return o + std::snprintf(o, 400, "%.6f", x);       // (also NaN / inf)
    uint64_t n = (uint64_t)(ax * 1e6);
    double r = std::fma(ax, 1e6, -(double)n);
    if (r < 0.0) { n -= 1; r += 1.0; }
    if (r >= 1.0) { n += 1; r -= 1.0; }
    if (std::fabs(r - 0.5) < 1e-9 || r < 0.0 || r >= 1.0) return o + std::snprintf(o, 400, "%.6f", x);
    if (r > 0.5) n += 1;
    if (std::signbit(x)) *o++ = '-';
    o = put_u64(o, n / 1000000u);
    *o++ = '.';
    uint32_t f = (uint32_t)(n % 1000000u);
    for (int i = 5; i >= 0; --i) { o[i] = (char)('0' + f % 10); f /= 10; }
    return o + 6;
}

static inline char *put_i64(char *o, long long v)
{
    if (v < 0) { *o++ = '-'; return put_u64(o, (uint64_t)(-(v + 1)) + 1u); }
    return put_u64(o, (uint64_t)v);
}

// utils.save_ply (utils.py:8-37): ASCII PLY, "%.6f %.6f %.6f %d %d %d" per vertex; with normals (float32, widened)
// three more "%.6f" between the position and the colour.  Host-only: formats into a 1 MiB buffer instead of one Python
// f.write per point.
static int write_ply(const char *path, const double *points, const float *normals, const int64_t *colors, int64_t n)
{
    FILE *f = std::fopen(path, "w");
    if (!f) return fail(nullptr, AMVS_EINVAL, std::string("cannot open ") + path);
    std::vector<char> buf(1 << 20);
    size_t used = (size_t)std::snprintf(buf.data(), buf.size(),
                                        "ply\nformat ascii 1.0\nelement vertex %lld\nproperty float x\n"
                                        "property float y\nproperty float z\n%sproperty uchar red\n"
                                        "property uchar green\nproperty uchar blue\nend_header\n",
                                        (long long)n, normals ? "property float nx\nproperty float ny\nproperty float nz\n" : "");
    bool ok = true;
    for (int64_t i = 0; i < n && ok; ++i) {
        if (used + 1400 > buf.size()) {              // (a "%.6f" of the largest double is 316 characters, of a float 46)
            ok = std::fwrite(buf.data(), 1, used, f) == used;
            used = 0;
        }
        char *o = buf.data() + used;
        o = put_f6(o, points[3 * i]); *o++ = ' ';
        o = put_f6(o, points[3 * i + 1]); *o++ = ' ';
        o = put_f6(o, points[3 * i + 2]); *o++ = ' ';
        if (normals)
            for (int k = 0; k < 3; ++k) { o = put_f6(o, (double)normals[3 * i + k]); *o++ = ' '; }
        o = put_i64(o, (long long)colors[3 * i]); *o++ = ' ';
        o = put_i64(o, (long long)colors[3 * i + 1]); *o++ = ' ';
        o = put_i64(o, (long long)colors[3 * i + 2]); *o++ = '\n';
        used = (size_t)(o - buf.data());
    }
    if (ok && used) ok = std::fwrite(buf.data(), 1, used, f) == used;
    ok = (std::fclose(f) == 0) && ok;
    return ok ? AMVS_OK : fail(nullptr, AMVS_EINVAL, std::string("write failed: ") + path);
}

int amvs_write_ply(const char *path, const double *points, const int64_t *colors, int64_t n)
{
    if (!path || n < 0 || (n > 0 && (!points || !colors))) return fail(nullptr, AMVS_EINVAL, "bad argument");
    return write_ply(path, points, nullptr, colors, n);
}

int amvs_write_ply_normals(const char *path, const double *points, const float *normals, const int64_t *colors, int64_t n)
{
    if (!path || !normals || n < 0 || (n > 0 && (!points || !colors))) return fail(nullptr, AMVS_EINVAL, "bad argument");
    return write_ply(path, points, normals, colors, n);
}

}  // extern "C"
#pragma GCC visibility pop
