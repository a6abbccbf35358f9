// amvs_capi_match.hip -- the entry points of include/amvs_match.h: resident descriptors and their exact matching, the
// accumulating cloud of the pair triangulation, and the bounds and grid voxel steps on the resident cloud.
#include "amvs_ctx.h"
#include "../../include/amvs_match.h"

#include <cmath>
#include <utility>

using namespace amvs::host;

namespace {

const char *slot_error(const amvs_ctx *c, int slot)
{
    if (slot < 0 || slot >= AMVS_DESC_MAX_SLOTS) return "slot outside 0 .. AMVS_DESC_MAX_SLOTS - 1";
    const auto it = c->desc.find(slot);
    if (it == c->desc.end() || it->second.n < 0) return "descriptor slot was never set";
    return nullptr;
}

// the parameter errors amvs_desc_knn2 and amvs_desc_match share; NULL = fine
const char *search_error(const amvs_ctx *c, int slot_q, int slot_t, bool both_ways)
{
    if (const char *why = slot_error(c, slot_q)) return why;
    if (const char *why = slot_error(c, slot_t)) return why;
    if (c->desc.at(slot_t).n < 2) return "fewer than 2 train rows";
    if (both_ways && c->desc.at(slot_q).n < 2) return "cross_check with fewer than 2 query rows";
    return nullptr;
}

bool finite3(const double *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int amvs_desc_set(amvs_ctx *c, int slot, const uint8_t *desc_u8, int n, int d)
{
    if (!c) return AMVS_EINVAL;
    if (d != AMVS_DESC_DIM) return fail(c, AMVS_EINVAL, "descriptors must have 128 dimensions");
    if (n < 0 || n > AMVS_DESC_MAX_ROWS) return fail(c, AMVS_EINVAL, "n outside 0 .. AMVS_DESC_MAX_ROWS");
    if (slot < 0 || slot >= AMVS_DESC_MAX_SLOTS) return fail(c, AMVS_EINVAL, "slot outside 0 .. AMVS_DESC_MAX_SLOTS - 1");
    if (n > 0 && !desc_u8) return fail(c, AMVS_EINVAL, "NULL descriptors");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::desc_set(desc_u8, n, c->cache, c->desc[slot], c->stream));
    return checked(c, AMVS_OK);
}

int amvs_desc_knn2(amvs_ctx *c, int slot_q, int slot_t, int32_t *idx_out, int32_t *dist2_out)
{
    if (!c) return AMVS_EINVAL;
    if (const char *why = search_error(c, slot_q, slot_t, false)) return fail(c, AMVS_EINVAL, why);
    const amvs::DescSlot &q = c->desc.at(slot_q), &t = c->desc.at(slot_t);
    if (q.n > 0 && (!idx_out || !dist2_out)) return fail(c, AMVS_EINVAL, "NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    static_assert(sizeof(int) == sizeof(int32_t), "index width");
    HIPCHK(c, amvs::desc_knn2_host(q, t, c->cache, idx_out, dist2_out, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_desc_match(amvs_ctx *c, int slot_q, int slot_t, float ratio, int cross_check, int32_t *q_idx_out, int32_t *t_idx_out,
                    int32_t *dist2_out, int64_t *n_matches)
{
    if (!c) return AMVS_EINVAL;
    if (!n_matches) return fail(c, AMVS_EINVAL, "NULL n_matches");
    if (!(ratio > 0.0f) || !std::isfinite(ratio)) return fail(c, AMVS_EINVAL, "ratio must be positive and finite");
    if (const char *why = search_error(c, slot_q, slot_t, cross_check != 0)) return fail(c, AMVS_EINVAL, why);
    const amvs::DescSlot &q = c->desc.at(slot_q), &t = c->desc.at(slot_t);
    if (q.n > 0 && (!q_idx_out || !t_idx_out || !dist2_out)) return fail(c, AMVS_EINVAL, "NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    long long m = 0;
    HIPCHK(c, amvs::desc_match(q, t, ratio, cross_check != 0, c->cache, q_idx_out, t_idx_out, dist2_out, &m, c->stream));
    *n_matches = m;
    return checked(c, AMVS_OK);
}

int amvs_pair_cloud_begin(amvs_ctx *c)
{
    if (!c) return AMVS_EINVAL;
    c->pair_cloud.n = 0;
    c->pair_cloud.open = true;
    return checked(c, AMVS_OK);
}

int amvs_pair_triangulate(amvs_ctx *c, const double K[9], const double R1[9], const double t1[3], const double R2[9],
                          const double t2[3], const float *pts1, const float *pts2, const uint8_t *rgb, int m, double depth_min,
                          double depth_max, double cos_min_parallax, double max_reproj, int64_t *n_accepted)
{
    if (!c) return AMVS_EINVAL;
    if (!n_accepted || !K || !R1 || !t1 || !R2 || !t2) return fail(c, AMVS_EINVAL, "NULL argument");
    if (m < 0 || m > (1 << 24)) return fail(c, AMVS_EINVAL, "m outside 0 .. 2^24");
    if (m > 0 && (!pts1 || !pts2 || !rgb)) return fail(c, AMVS_EINVAL, "NULL candidates");
    if (std::isnan(depth_min) || std::isnan(depth_max) || std::isnan(cos_min_parallax) || std::isnan(max_reproj))
        return fail(c, AMVS_EINVAL, "a threshold is NaN");
    if (!c->pair_cloud.open) return fail(c, AMVS_EINVAL, "amvs_pair_triangulate without amvs_pair_cloud_begin");
    int rc = bind_device(c);
    if (rc) return rc;
    long long k = 0;
    const amvs::PairThresholds thr{depth_min, depth_max, cos_min_parallax, max_reproj};
    HIPCHK(c, amvs::pair_triangulate(K, R1, t1, R2, t2, pts1, pts2, rgb, m, thr, c->cache, c->pair_cloud, &k, c->stream));
    *n_accepted = k;
    return checked(c, AMVS_OK);
}

int amvs_pair_cloud_finish(amvs_ctx *c, int64_t *total)
{
    if (!c) return AMVS_EINVAL;
    if (!total) return fail(c, AMVS_EINVAL, "NULL output");
    if (!c->pair_cloud.open) return fail(c, AMVS_EINVAL, "amvs_pair_cloud_finish without amvs_pair_cloud_begin");
    Cloud next;
    next.pts = std::move(c->pair_cloud.pts);
    next.rgb = std::move(c->pair_cloud.rgb);
    next.n = c->pair_cloud.n;
    c->pair_cloud = amvs::PairCloud{};
    c->cloud = std::move(next);
    *total = c->cloud.n;
    return checked(c, AMVS_OK);
}

int amvs_cloud_bounds(amvs_ctx *c, const uint8_t *keep_mask, double min_out[3], double max_out[3])
{
    if (!c) return AMVS_EINVAL;
    if (!min_out || !max_out) return fail(c, AMVS_EINVAL, "NULL output");
    if (c->cloud.n < 1) return fail(c, AMVS_EINVAL, "no resident cloud");
    int rc = bind_device(c);
    if (rc) return rc;
    const hipError_t e = amvs::cloud_bounds(c->cloud.pts.get(), c->cloud.n, keep_mask, c->cache, min_out, max_out, c->stream);
    if (e == hipErrorInvalidValue) return fail(c, AMVS_EINVAL, "cloud_bounds: no kept point");
    if (e != hipSuccess) return fail(c, AMVS_EHIP, std::string("cloud_bounds: ") + hipGetErrorString(e));
    return checked(c, AMVS_OK);
}

int amvs_cloud_voxel_downsample_grid(amvs_ctx *c, const uint8_t *keep_mask, const double origin[3], double voxel_size,
                                     int64_t *count)
{
    if (!c) return AMVS_EINVAL;
    if (!count || !origin) return fail(c, AMVS_EINVAL, "NULL argument");
    if (!(voxel_size > 0.0) || !std::isfinite(voxel_size) || !finite3(origin))
        return fail(c, AMVS_EINVAL, "voxel_size must be positive and finite, origin finite");
    if (c->cloud.n < 1) return fail(c, AMVS_EINVAL, "no resident cloud");
    int rc = bind_device(c);
    if (rc) return rc;
    double mn[3], mx[3];
    long long not_finite = 0;
    hipError_t e = amvs::cloud_bounds(c->cloud.pts.get(), c->cloud.n, keep_mask, c->cache, mn, mx, c->stream, &not_finite);
    if (e == hipSuccess && not_finite > 0) return fail(c, AMVS_EINVAL, "voxel_downsample_grid: a kept point is not finite");
    Cloud next;                         // (the resident cloud is the input: replaced once the new one is made)
    if (e == hipSuccess) {
        // the voxel-index box of the kept points: floor((x - origin) / voxel) is monotone in x
        long long lo[3], ext[3];
        long double cells = 1.0L;
        for (int a = 0; a < 3; ++a) {
            const double flo = std::floor((mn[a] - origin[a]) / voxel_size), fhi = std::floor((mx[a] - origin[a]) / voxel_size);
            if (!std::isfinite(flo) || !std::isfinite(fhi) || std::fabs(flo) > 4.0e18 || std::fabs(fhi) > 4.0e18)
                return fail(c, AMVS_EINVAL, "voxel_downsample_grid: kept points not finite or outside the int64 voxel range");
            lo[a] = (long long)flo;
            cells *= (long double)(fhi - flo) + 1.0L;
        }
        if (cells > 4.0e18L) return fail(c, AMVS_EINVAL, "voxel_downsample_grid: the kept points span more than 2^62 voxels");
        for (int a = 0; a < 3; ++a) ext[a] = (long long)std::floor((mx[a] - origin[a]) / voxel_size) - lo[a] + 1;
        e = amvs::voxel_downsample_grid(c->cloud.pts.get(), c->cloud.rgb.get(), c->cloud.n, keep_mask, origin, voxel_size, lo, ext,
                                        c->cache, next.pts, next.rgb, &next.n, c->stream);
    } else if (e == hipErrorInvalidValue) {
        e = hipSuccess;                 // no kept point: an empty cloud
    }
    if (e != hipSuccess) return fail(c, AMVS_EHIP, std::string("voxel_downsample_grid: ") + hipGetErrorString(e));
    c->cloud = std::move(next);
    *count = c->cloud.n;
    return checked(c, AMVS_OK);
}

int amvs_match_selftest_sqrt(amvs_ctx *c, const double *in, int n, double *out)
{
    if (!c) return AMVS_EINVAL;
    if (n < 0 || n > (1 << 24) || (n > 0 && (!in || !out))) return fail(c, AMVS_EINVAL, "bad argument");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::selftest_sqrt(in, n, out, c->cache, c->stream));
    return checked(c, AMVS_OK);
}

}  // extern "C"
#pragma GCC visibility pop
