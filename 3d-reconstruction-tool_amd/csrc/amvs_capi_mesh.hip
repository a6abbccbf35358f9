// amvs_capi_mesh.hip -- the TSDF and mesh entry points of the C ABI (include/amvs.h; amvs_mesh.hip,
// amvs_mesh_fill.hip, amvs_mesh_clean.hip, amvs_mesh_decimate.hip, amvs_mesh_render.hip, amvs_mesh_color.hip,
// amvs_mesh_texture.hip).
#include "amvs_ctx.h"

#include <cmath>
#include <vector>

using namespace amvs::host;

#pragma GCC visibility push(default)
extern "C" {

// the grid of a TSDF volume: finite origin, positive finite voxel, every dimension >= 2, the point budget
static int check_tsdf_grid(amvs_ctx *c, const std::string &who, const float origin[3], float voxel, const int32_t dims[3])
{
    if (!(voxel > 0.0f) || !std::isfinite(voxel)) return fail(c, AMVS_EINVAL, who + ": voxel must be positive and finite");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(origin[a])) return fail(c, AMVS_EINVAL, who + ": origin must be finite");
    if (dims[0] < 2 || dims[1] < 2 || dims[2] < 2) return fail(c, AMVS_EINVAL, who + ": every dimension must be >= 2");
    const long long points = (long long)dims[0] * dims[1] * dims[2];
    if (dims[0] > AMVS_TSDF_MAX_POINTS || dims[1] > AMVS_TSDF_MAX_POINTS || dims[2] > AMVS_TSDF_MAX_POINTS ||
        points > AMVS_TSDF_MAX_POINTS)
        return fail(c, AMVS_EINVAL, who + ": volume of " + std::to_string(dims[0]) + " x " + std::to_string(dims[1]) +
                                        " x " + std::to_string(dims[2]) + " grid points is over the budget of " +
                                        std::to_string((long long)AMVS_TSDF_MAX_POINTS) + " (AMVS_TSDF_MAX_POINTS)");
    return AMVS_OK;
}

// AMVS_OK, or the failure of entry point `name` with HIP's error string
static int hip_rc(amvs_ctx *c, const char *name, hipError_t e)
{
    return e == hipSuccess ? AMVS_OK : fail(c, AMVS_EHIP, std::string(name) + ": " + hipGetErrorString(e));
}

// HIPCHK with the entry point's name in the message instead of the call's text
#define MESH_HIPCHK(c, name, call)                                \
    do {                                                          \
        if (int rc_ = hip_rc((c), (name), (call))) return rc_;    \
    } while (0)

// AMVS_OK, or the failure of entry point `name` on a context without a current mesh
static int need_mesh(amvs_ctx *c, const char *name)
{
    if (amvs::tsdf_has_mesh(c->tsdf.get())) return AMVS_OK;
    return fail(c, AMVS_EINVAL, std::string(name) + ": no mesh (amvs_tsdf_extract or amvs_mesh_set)");
}

int amvs_tsdf_integrate(amvs_ctx *c, int n_maps, const void *depth, const void *conf, int maps_on_device,
                        const int *view_ids, const uint8_t *colors_bgr_host, const float K[9], const float *poses,
                        float min_views, const float origin[3], float voxel, const int32_t dims[3], float trunc)
{
    if (!c) return AMVS_EINVAL;
    if (n_maps < 1 || !depth || !conf || !K || !poses || !origin || !dims)
        return fail(c, AMVS_EINVAL, "tsdf_integrate: bad argument");
    if ((view_ids != nullptr) == (colors_bgr_host != nullptr))
        return fail(c, AMVS_EINVAL, "tsdf_integrate: give exactly one colour source (view_ids or colors_bgr_host)");
    if (!(trunc > 0.0f) || !std::isfinite(trunc)) return fail(c, AMVS_EINVAL, "tsdf_integrate: trunc must be positive and finite");
    int rc = check_tsdf_grid(c, "tsdf_integrate", origin, voxel, dims);
    if (rc) return rc;
    std::vector<int> slots(n_maps);
    if (view_ids && (rc = check_colour_views(c, n_maps, view_ids))) return rc;
    for (int j = 0; j < n_maps; ++j) slots[j] = view_ids ? view_ids[j] : j;
    if ((rc = bind_device(c))) return rc;
    if (!c->tsdf) c->tsdf.reset(amvs::tsdf_state_new());
    MESH_HIPCHK(c, "tsdf_integrate", amvs::tsdf_integrate(c->tsdf.get(), c->cache, (const float *)depth, (const float *)conf,
                maps_on_device != 0, n_maps, c->H, c->W, view_ids ? c->d_bgr.get() : colors_bgr_host, view_ids != nullptr,
                view_ids ? c->n_views : n_maps, slots.data(), K, poses, min_views, origin, voxel, dims, trunc, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_tsdf_set_volume(amvs_ctx *c, const float *tsdf, const float *weight, const float *color_sum, const float origin[3],
                         float voxel, const int32_t dims[3])
{
    if (!c) return AMVS_EINVAL;
    if (!tsdf || !weight || !color_sum || !origin || !dims) return fail(c, AMVS_EINVAL, "tsdf_set_volume: bad argument");
    int rc = check_tsdf_grid(c, "tsdf_set_volume", origin, voxel, dims);
    if (rc) return rc;
    if ((rc = bind_device(c))) return rc;
    if (!c->tsdf) c->tsdf.reset(amvs::tsdf_state_new());
    MESH_HIPCHK(c, "tsdf_set_volume", amvs::tsdf_set_volume(c->tsdf.get(), c->cache, tsdf, weight, color_sum, origin, voxel, dims,
                c->stream));
    return checked(c, AMVS_OK);
}

int amvs_tsdf_extract(amvs_ctx *c, int64_t *n_vertices, int64_t *n_faces)
{
    if (!c) return AMVS_EINVAL;
    if (!n_vertices || !n_faces) return fail(c, AMVS_EINVAL, "tsdf_extract: NULL output");
    if (!amvs::tsdf_has_volume(c->tsdf.get())) return fail(c, AMVS_EINVAL, "tsdf_extract: no volume (amvs_tsdf_integrate)");
    int rc = bind_device(c);
    if (rc) return rc;
    long long nv = 0, nf = 0;
    MESH_HIPCHK(c, "tsdf_extract", amvs::tsdf_extract(c->tsdf.get(), c->cache, &nv, &nf, c->stream));
    *n_vertices = nv; *n_faces = nf;
    return checked(c, AMVS_OK);
}

int amvs_fetch_mesh(amvs_ctx *c, float *vertices, int32_t *faces, uint8_t *colors_rgb)
{
    if (!c) return AMVS_EINVAL;
    if (!amvs::tsdf_has_mesh(c->tsdf.get())) return fail(c, AMVS_EINVAL, "fetch_mesh: no mesh (amvs_tsdf_extract)");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::tsdf_fetch_mesh(c->tsdf.get(), vertices, faces, colors_rgb, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_tsdf_fetch_volume(amvs_ctx *c, float *tsdf, float *weight, float *color_sum)
{
    if (!c) return AMVS_EINVAL;
    if (!amvs::tsdf_has_volume(c->tsdf.get())) return fail(c, AMVS_EINVAL, "tsdf_fetch_volume: no volume (amvs_tsdf_integrate)");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::tsdf_fetch_volume(c->tsdf.get(), tsdf, weight, color_sum, c->stream));
    return checked(c, AMVS_OK);
}

// ---- hole filling (amvs_mesh_fill.hip): in place on the context's current volume ----
int amvs_tsdf_fill(amvs_ctx *c, int steps, int min_neighbours, int64_t *filled_per_step, int64_t *n_filled)
{
    if (!c) return AMVS_EINVAL;
    if (steps < 1 || steps > AMVS_FILL_MAX_STEPS)
        return fail(c, AMVS_EINVAL, "tsdf_fill: steps must lie in 1 .. " + std::to_string(AMVS_FILL_MAX_STEPS));
    if (min_neighbours < 1 || min_neighbours > 6) return fail(c, AMVS_EINVAL, "tsdf_fill: min_neighbours must lie in 1 .. 6");
    if (!amvs::tsdf_has_volume(c->tsdf.get()))
        return fail(c, AMVS_EINVAL, "tsdf_fill: no volume (amvs_tsdf_integrate or amvs_tsdf_set_volume)");
    int rc = bind_device(c);
    if (rc) return rc;
    std::vector<long long> per_step((size_t)steps, 0);
    long long total = 0;
    MESH_HIPCHK(c, "tsdf_fill", amvs::tsdf_fill(c->tsdf.get(), c->cache, steps, min_neighbours, per_step.data(), &total,
                c->stream));
    if (filled_per_step)
        for (int s = 0; s < steps; ++s) filled_per_step[s] = per_step[(size_t)s];
    if (n_filled) *n_filled = total;
    return checked(c, AMVS_OK);
}

int amvs_tsdf_fetch_fill(amvs_ctx *c, uint8_t *gen)
{
    if (!c) return AMVS_EINVAL;
    if (!amvs::tsdf_has_fill(c->tsdf.get()))
        return fail(c, AMVS_EINVAL, "tsdf_fetch_fill: no fill of the current volume (amvs_tsdf_fill)");
    if (!gen) return fail(c, AMVS_EINVAL, "tsdf_fetch_fill: NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::tsdf_fetch_fill(c->tsdf.get(), gen, c->stream));
    return checked(c, AMVS_OK);
}

// ---- mesh clean-up (amvs_mesh_clean.hip): in place on the context's current mesh ----
int amvs_mesh_set(amvs_ctx *c, const float *vertices, int64_t n_vertices, const int32_t *faces, int64_t n_faces,
                  const uint8_t *colors_rgb)
{
    if (!c) return AMVS_EINVAL;
    if (n_vertices < 0 || n_faces < 0 || (n_vertices > 0 && !vertices) || (n_faces > 0 && !faces))
        return fail(c, AMVS_EINVAL, "mesh_set: bad argument");
    if (n_vertices > INT32_MAX || 3 * n_faces > INT32_MAX)
        return fail(c, AMVS_EINVAL, "mesh_set: mesh too large (int32 vertex ids, 3 * n_faces <= INT32_MAX)");
    for (int64_t i = 0; i < 3 * n_vertices; ++i)
        if (!std::isfinite(vertices[i])) return fail(c, AMVS_EINVAL, "mesh_set: vertex " + std::to_string(i / 3) + " is not finite");
    for (int64_t f = 0; f < n_faces; ++f) {
        const int32_t a = faces[3 * f], b = faces[3 * f + 1], d = faces[3 * f + 2];
        if (a < 0 || b < 0 || d < 0 || a >= n_vertices || b >= n_vertices || d >= n_vertices)
            return fail(c, AMVS_EINVAL, "mesh_set: face " + std::to_string(f) + " has a vertex id out of range");
        if (a == b || a == d || b == d)
            return fail(c, AMVS_EINVAL, "mesh_set: face " + std::to_string(f) + " has a repeated vertex id");
    }
    int rc = bind_device(c);
    if (rc) return rc;
    if (!c->tsdf) c->tsdf.reset(amvs::tsdf_state_new());
    MESH_HIPCHK(c, "mesh_set", amvs::mesh_set(c->tsdf.get(), c->cache, vertices, n_vertices, faces, n_faces, colors_rgb,
                c->stream));
    return checked(c, AMVS_OK);
}

int amvs_mesh_filter_components(amvs_ctx *c, int64_t min_faces, int keep_largest, int64_t *n_components, int64_t *n_vertices,
                                int64_t *n_faces)
{
    if (!c) return AMVS_EINVAL;
    if (!n_components || !n_vertices || !n_faces) return fail(c, AMVS_EINVAL, "mesh_filter_components: NULL output");
    if (int rc = need_mesh(c, "mesh_filter_components")) return rc;
    int rc = bind_device(c);
    if (rc) return rc;
    long long nc = 0, nv = 0, nf = 0;
    MESH_HIPCHK(c, "mesh_filter_components", amvs::mesh_filter_components(c->tsdf.get(), c->cache, min_faces, keep_largest != 0,
                &nc, &nv, &nf, c->stream));
    *n_components = nc; *n_vertices = nv; *n_faces = nf;
    return checked(c, AMVS_OK);
}

int amvs_mesh_smooth(amvs_ctx *c, int iterations, float lambda, float mu, int fix_boundary)
{
    if (!c) return AMVS_EINVAL;
    if (iterations < 0 || iterations > 1000) return fail(c, AMVS_EINVAL, "mesh_smooth: iterations must lie in 0 .. 1000");
    if (!(lambda > 0.0f && lambda <= 1.0f)) return fail(c, AMVS_EINVAL, "mesh_smooth: lambda must lie in (0, 1]");
    if (!std::isfinite(mu)) return fail(c, AMVS_EINVAL, "mesh_smooth: mu must be finite");
    if (int rc = need_mesh(c, "mesh_smooth")) return rc;
    int rc = bind_device(c);
    if (rc) return rc;
    MESH_HIPCHK(c, "mesh_smooth", amvs::mesh_smooth(c->tsdf.get(), c->cache, iterations, lambda, mu, fix_boundary != 0, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_mesh_normals(amvs_ctx *c)
{
    if (!c) return AMVS_EINVAL;
    if (int rc = need_mesh(c, "mesh_normals")) return rc;
    int rc = bind_device(c);
    if (rc) return rc;
    MESH_HIPCHK(c, "mesh_normals", amvs::mesh_normals(c->tsdf.get(), c->cache, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_mesh_decimate(amvs_ctx *c, const float origin[3], float cell, int64_t *n_vertices, int64_t *n_faces)
{
    if (!c) return AMVS_EINVAL;
    if (!n_vertices || !n_faces) return fail(c, AMVS_EINVAL, "mesh_decimate: NULL output");
    if (!origin) return fail(c, AMVS_EINVAL, "mesh_decimate: NULL origin");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(origin[a])) return fail(c, AMVS_EINVAL, "mesh_decimate: origin must be finite");
    if (!(cell > 0.0f) || !std::isfinite(cell)) return fail(c, AMVS_EINVAL, "mesh_decimate: cell must be positive and finite");
    if (int rc = need_mesh(c, "mesh_decimate")) return rc;
    int rc = bind_device(c);
    if (rc) return rc;
    long long bad = -1, nv = 0, nf = 0;
    MESH_HIPCHK(c, "mesh_decimate", amvs::mesh_decimate(c->tsdf.get(), c->cache, origin, cell, &bad, &nv, &nf, c->stream));
    if (bad >= 0) return fail(c, AMVS_EINVAL, "mesh_decimate: vertex " + std::to_string(bad) + " outside the cluster grid");
    *n_vertices = nv; *n_faces = nf;
    return checked(c, AMVS_OK);
}

int amvs_mesh_decimate_quadric(amvs_ctx *c, const float origin[3], float cell, float regularisation, int64_t *n_vertices,
                               int64_t *n_faces, int64_t *n_fallback)
{
    if (!c) return AMVS_EINVAL;
    if (!n_vertices || !n_faces || !n_fallback) return fail(c, AMVS_EINVAL, "mesh_decimate_quadric: NULL output");
    if (!origin) return fail(c, AMVS_EINVAL, "mesh_decimate_quadric: NULL origin");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(origin[a])) return fail(c, AMVS_EINVAL, "mesh_decimate_quadric: origin must be finite");
    if (!(cell > 0.0f) || !std::isfinite(cell)) return fail(c, AMVS_EINVAL, "mesh_decimate_quadric: cell must be positive and finite");
    if (!(regularisation > 0.0f && regularisation <= 1.0f))
        return fail(c, AMVS_EINVAL, "mesh_decimate_quadric: regularisation must be in (0, 1]");
    if (int rc = need_mesh(c, "mesh_decimate_quadric")) return rc;
    int rc = bind_device(c);
    if (rc) return rc;
    long long bad = -1, nv = 0, nf = 0, nk = 0;
    MESH_HIPCHK(c, "mesh_decimate_quadric", amvs::mesh_decimate_quadric(c->tsdf.get(), c->cache, origin, cell, regularisation, &bad,
                &nv, &nf, &nk, c->stream));
    if (bad >= 0) return fail(c, AMVS_EINVAL, "mesh_decimate_quadric: vertex " + std::to_string(bad) + " outside the cluster grid");
    *n_vertices = nv; *n_faces = nf; *n_fallback = nk;
    return checked(c, AMVS_OK);
}

int amvs_fetch_mesh_attributes(amvs_ctx *c, float *normals, int32_t *labels)
{
    if (!c) return AMVS_EINVAL;
    if (int rc = need_mesh(c, "fetch_mesh_attributes")) return rc;
    if (normals && !amvs::mesh_has_normals(c->tsdf.get()))
        return fail(c, AMVS_EINVAL, "fetch_mesh_attributes: no current normals (amvs_mesh_normals)");
    if (labels && !amvs::mesh_has_labels(c->tsdf.get()))
        return fail(c, AMVS_EINVAL, "fetch_mesh_attributes: no current labels (amvs_mesh_filter_components)");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::mesh_fetch_attributes(c->tsdf.get(), normals, labels, c->stream));
    return checked(c, AMVS_OK);
}

// ---- rendering and visibility (amvs_mesh_render.hip): the current mesh seen from given cameras ----
int amvs_set_render_tuning(amvs_ctx *c, int large_face_pixels)
{
    if (!c) return AMVS_EINVAL;
    if (large_face_pixels < 0) return fail(c, AMVS_EINVAL, "set_render_tuning: large_face_pixels must be >= 0 (0 = automatic)");
    if (!c->tsdf) c->tsdf.reset(amvs::tsdf_state_new());
    amvs::mesh_set_render_tuning(c->tsdf.get(), large_face_pixels);
    return AMVS_OK;
}

int amvs_mesh_render(amvs_ctx *c, int n_views, const float K[9], const float *poses, float near, int64_t *n_skipped)
{
    if (!c) return AMVS_EINVAL;
    if (int rc = need_mesh(c, "mesh_render")) return rc;
    if (n_views < 1) return fail(c, AMVS_EINVAL, "mesh_render: n_views must be >= 1");
    if (!K || !poses) return fail(c, AMVS_EINVAL, "mesh_render: NULL K or poses");
    if (!(near > 0.0f) || !std::isfinite(near)) return fail(c, AMVS_EINVAL, "mesh_render: near must be positive and finite");
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(K[i])) return fail(c, AMVS_EINVAL, "mesh_render: K must be finite");
    if ((long long)n_views * c->H * c->W > INT32_MAX)
        return fail(c, AMVS_EINVAL, "mesh_render: " + std::to_string(n_views) + " views of " + std::to_string(c->H) + " x " +
                                        std::to_string(c->W) + " pixels are over the limit (n_views * H * W <= INT32_MAX)");
    for (long long i = 0; i < 12ll * n_views; ++i)
        if (!std::isfinite(poses[i])) return fail(c, AMVS_EINVAL, "mesh_render: pose " + std::to_string(i / 12) + " is not finite");
    int rc = bind_device(c);
    if (rc) return rc;
    std::vector<long long> skipped(n_skipped ? (size_t)n_views : 0);
    MESH_HIPCHK(c, "mesh_render", amvs::mesh_render(c->tsdf.get(), c->cache, n_views, c->H, c->W, K, poses, near,
                n_skipped ? skipped.data() : nullptr, c->stream));
    for (size_t m = 0; m < skipped.size(); ++m) n_skipped[m] = skipped[m];
    return checked(c, AMVS_OK);
}

int amvs_fetch_render(amvs_ctx *c, int first, int count, float *depth_out, int32_t *face_out)
{
    if (!c) return AMVS_EINVAL;
    if (!amvs::mesh_has_render(c->tsdf.get())) return fail(c, AMVS_EINVAL, "fetch_render: no current render (amvs_mesh_render)");
    const int n = amvs::mesh_render_views(c->tsdf.get());
    if (first < 0 || count < 1 || first > n - count)
        return fail(c, AMVS_EINVAL, "fetch_render: views " + std::to_string(first) + " .. " + std::to_string((long long)first + count - 1) +
                                        " are not among the " + std::to_string(n) + " rendered");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::mesh_fetch_render(c->tsdf.get(), first, count, depth_out, face_out, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_mesh_visibility(amvs_ctx *c, float depth_tolerance, int64_t *n_seen)
{
    if (!c) return AMVS_EINVAL;
    if (!amvs::mesh_has_render(c->tsdf.get())) return fail(c, AMVS_EINVAL, "mesh_visibility: no current render (amvs_mesh_render)");
    if (!(depth_tolerance >= 0.0f) || !std::isfinite(depth_tolerance))
        return fail(c, AMVS_EINVAL, "mesh_visibility: depth_tolerance must be finite and not negative");
    int rc = bind_device(c);
    if (rc) return rc;
    long long seen = 0;
    MESH_HIPCHK(c, "mesh_visibility", amvs::mesh_visibility(c->tsdf.get(), c->cache, depth_tolerance, &seen, c->stream));
    if (n_seen) *n_seen = seen;
    return checked(c, AMVS_OK);
}

int amvs_fetch_mesh_visibility(amvs_ctx *c, int32_t *counts)
{
    if (!c) return AMVS_EINVAL;
    if (!amvs::mesh_has_visibility(c->tsdf.get()))
        return fail(c, AMVS_EINVAL, "fetch_mesh_visibility: no current counts (amvs_mesh_visibility)");
    if (!counts) return fail(c, AMVS_EINVAL, "fetch_mesh_visibility: NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::mesh_fetch_visibility(c->tsdf.get(), counts, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_mesh_filter_visible(amvs_ctx *c, int min_views, int64_t *n_vertices, int64_t *n_faces)
{
    if (!c) return AMVS_EINVAL;
    if (!n_vertices || !n_faces) return fail(c, AMVS_EINVAL, "mesh_filter_visible: NULL output");
    if (!amvs::mesh_has_visibility(c->tsdf.get()))
        return fail(c, AMVS_EINVAL, "mesh_filter_visible: no current counts (amvs_mesh_visibility)");
    if (min_views < 1) return fail(c, AMVS_EINVAL, "mesh_filter_visible: min_views must be >= 1");
    int rc = bind_device(c);
    if (rc) return rc;
    long long nv = 0, nf = 0;
    MESH_HIPCHK(c, "mesh_filter_visible", amvs::mesh_filter_visible(c->tsdf.get(), c->cache, min_views, &nv, &nf, c->stream));
    *n_vertices = nv; *n_faces = nf;
    return checked(c, AMVS_OK);
}

// ---- colours from the views (amvs_mesh_color.hip) ----
int amvs_mesh_color_views(amvs_ctx *c, const int *view_ids, const uint8_t *colors_bgr_host, float depth_tolerance, float min_cos,
                          int best_view, int64_t *n_colored)
{
    if (!c) return AMVS_EINVAL;
    if (!amvs::mesh_has_render(c->tsdf.get())) return fail(c, AMVS_EINVAL, "mesh_color_views: no current render (amvs_mesh_render)");
    if (!amvs::mesh_has_normals(c->tsdf.get())) return fail(c, AMVS_EINVAL, "mesh_color_views: no current normals (amvs_mesh_normals)");
    if ((view_ids != nullptr) == (colors_bgr_host != nullptr))
        return fail(c, AMVS_EINVAL, "mesh_color_views: give exactly one colour source (view_ids or colors_bgr_host)");
    if (!(depth_tolerance >= 0.0f) || !std::isfinite(depth_tolerance))
        return fail(c, AMVS_EINVAL, "mesh_color_views: depth_tolerance must be finite and not negative");
    if (!(min_cos >= 0.0f && min_cos < 1.0f)) return fail(c, AMVS_EINVAL, "mesh_color_views: min_cos must lie in [0, 1)");
    const int n = amvs::mesh_render_views(c->tsdf.get());
    int rc;
    if (view_ids && (rc = check_colour_views(c, n, view_ids))) {
        c->err = "mesh_color_views: " + c->err;
        return rc;
    }
    std::vector<int> slots(n);
    for (int j = 0; j < n; ++j) slots[j] = view_ids ? view_ids[j] : j;
    if ((rc = bind_device(c))) return rc;
    long long colored = 0;
    MESH_HIPCHK(c, "mesh_color_views", amvs::mesh_color_views(c->tsdf.get(), c->cache, view_ids ? c->d_bgr.get() : colors_bgr_host,
                view_ids != nullptr, view_ids ? c->n_views : n, slots.data(), depth_tolerance, min_cos, best_view != 0, &colored,
                c->stream));
    if (n_colored) *n_colored = colored;
    return checked(c, AMVS_OK);
}

int amvs_fetch_render_color(amvs_ctx *c, int first, int count, uint8_t *rgb_out)
{
    if (!c) return AMVS_EINVAL;
    if (!amvs::mesh_has_render(c->tsdf.get()))
        return fail(c, AMVS_EINVAL, "fetch_render_color: no current render (amvs_mesh_render)");
    const int n = amvs::mesh_render_views(c->tsdf.get());
    if (first < 0 || count < 1 || first > n - count)
        return fail(c, AMVS_EINVAL, "fetch_render_color: views " + std::to_string(first) + " .. " +
                                        std::to_string((long long)first + count - 1) + " are not among the " + std::to_string(n) +
                                        " rendered");
    if (!rgb_out) return fail(c, AMVS_EINVAL, "fetch_render_color: NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    MESH_HIPCHK(c, "fetch_render_color", amvs::mesh_fetch_render_color(c->tsdf.get(), c->cache, first, count, rgb_out, c->stream));
    return checked(c, AMVS_OK);
}

// ---- texture from the views (amvs_mesh_texture.hip) ----
int amvs_mesh_texture(amvs_ctx *c, const int *view_ids, const uint8_t *colors_bgr_host, float depth_tolerance, float min_cos,
                      int best_view, int texels, int cells_per_row, int *width, int *height, int64_t *n_texels,
                      int64_t *n_textured)
{
    if (!c) return AMVS_EINVAL;
    if (!amvs::mesh_has_render(c->tsdf.get())) return fail(c, AMVS_EINVAL, "mesh_texture: no current render (amvs_mesh_render)");
    if ((view_ids != nullptr) == (colors_bgr_host != nullptr))
        return fail(c, AMVS_EINVAL, "mesh_texture: give exactly one colour source (view_ids or colors_bgr_host)");
    if (!(depth_tolerance >= 0.0f) || !std::isfinite(depth_tolerance))
        return fail(c, AMVS_EINVAL, "mesh_texture: depth_tolerance must be finite and not negative");
    if (!(min_cos >= 0.0f && min_cos < 1.0f)) return fail(c, AMVS_EINVAL, "mesh_texture: min_cos must lie in [0, 1)");
    if (texels < 1 || texels > AMVS_TEXTURE_MAX_TEXELS)
        return fail(c, AMVS_EINVAL, "mesh_texture: texels must lie in 1 .. " + std::to_string(AMVS_TEXTURE_MAX_TEXELS));
    if (cells_per_row < 0) return fail(c, AMVS_EINVAL, "mesh_texture: cells_per_row must be >= 0 (0 = automatic)");
    const int n = amvs::mesh_render_views(c->tsdf.get());
    int rc;
    if (view_ids && (rc = check_colour_views(c, n, view_ids))) {
        c->err = "mesh_texture: " + c->err;
        return rc;
    }
    long long nf = 0, cols = 0, wt = 0, ht = 0;
    amvs::mesh_texture_layout(c->tsdf.get(), texels, cells_per_row, &nf, &cols, &wt, &ht);
    if (wt > AMVS_TEXTURE_MAX_SIDE || ht > AMVS_TEXTURE_MAX_SIDE)
        return fail(c, AMVS_EINVAL, "mesh_texture: an atlas of " + std::to_string(wt) + " x " + std::to_string(ht) + " texels for " +
                                        std::to_string(nf) + " faces is over the limit of " + std::to_string(AMVS_TEXTURE_MAX_SIDE) +
                                        " a side (AMVS_TEXTURE_MAX_SIDE)");
    std::vector<int> slots(n);
    for (int j = 0; j < n; ++j) slots[j] = view_ids ? view_ids[j] : j;
    if ((rc = bind_device(c))) return rc;
    long long textured = 0;
    MESH_HIPCHK(c, "mesh_texture", amvs::mesh_texture(c->tsdf.get(), c->cache, view_ids ? c->d_bgr.get() : colors_bgr_host,
                view_ids != nullptr, view_ids ? c->n_views : n, slots.data(), depth_tolerance, min_cos, best_view != 0, texels,
                (int)cols, (int)wt, (int)ht, &textured, c->stream));
    if (width) *width = (int)wt;
    if (height) *height = (int)ht;
    if (n_texels) *n_texels = nf * ((long long)(texels + 1) * (texels + 2) / 2 + texels);
    if (n_textured) *n_textured = textured;
    return checked(c, AMVS_OK);
}

int amvs_fetch_mesh_texture(amvs_ctx *c, uint8_t *atlas_rgb, float *uv)
{
    if (!c) return AMVS_EINVAL;
    if (!amvs::mesh_has_texture(c->tsdf.get())) return fail(c, AMVS_EINVAL, "fetch_mesh_texture: no current texture (amvs_mesh_texture)");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::mesh_fetch_texture(c->tsdf.get(), atlas_rgb, uv, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_fetch_render_texture(amvs_ctx *c, int first, int count, uint8_t *rgb_out)
{
    if (!c) return AMVS_EINVAL;
    if (!amvs::mesh_has_render(c->tsdf.get()))
        return fail(c, AMVS_EINVAL, "fetch_render_texture: no current render (amvs_mesh_render)");
    if (!amvs::mesh_has_texture(c->tsdf.get()))
        return fail(c, AMVS_EINVAL, "fetch_render_texture: no current texture (amvs_mesh_texture)");
    const int n = amvs::mesh_render_views(c->tsdf.get());
    if (first < 0 || count < 1 || first > n - count)
        return fail(c, AMVS_EINVAL, "fetch_render_texture: views " + std::to_string(first) + " .. " +
                                        std::to_string((long long)first + count - 1) + " are not among the " + std::to_string(n) +
                                        " rendered");
    if (!rgb_out) return fail(c, AMVS_EINVAL, "fetch_render_texture: NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    MESH_HIPCHK(c, "fetch_render_texture", amvs::mesh_fetch_render_texture(c->tsdf.get(), c->cache, first, count, rgb_out, c->stream));
    return checked(c, AMVS_OK);
}

}  // extern "C"
#pragma GCC visibility pop
