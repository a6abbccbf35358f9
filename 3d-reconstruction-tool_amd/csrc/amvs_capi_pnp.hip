// amvs_capi_pnp.hip -- the entry points of include/amvs_resection.h: hypotheses, scoring, inliers, the refit and the
// RANSAC that chains them (kernels and host steps in amvs_pnp.hip, the step's arithmetic in amvs_pnp_step.h).
#include "amvs_ctx.h"
#include "amvs_pnp_host.h"
#include "amvs_pnp_step.h"
#include "../../include/amvs_resection.h"

using namespace amvs::host;

namespace {

// the parameter errors the five entry points share; NULL = fine
const char *points_error(const float *pts3d, const float *pts2d, int m, const double *K)
{
    if (m < 6 || m > AMVS_PNP_MAX_POINTS) return "m outside 6 .. AMVS_PNP_MAX_POINTS";
    if (!pts3d || !pts2d) return "NULL points";
    return amvs::pnp_intrinsics_error(K);
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int amvs_pnp_hypotheses(amvs_ctx *c, const float *pts3d, const float *pts2d, int m, const double K[9], uint64_t seed, int first,
                        int count, int32_t *idx_out, double *R_out, double *t_out)
{
    if (!c) return AMVS_EINVAL;
    if (const char *why = points_error(pts3d, pts2d, m, K)) return fail(c, AMVS_EINVAL, why);
    if (first < 0) return fail(c, AMVS_EINVAL, "first < 0");
    if (count < 1 || count > AMVS_PNP_MAX_HYP) return fail(c, AMVS_EINVAL, "count outside 1 .. AMVS_PNP_MAX_HYP");
    if (!idx_out || !R_out || !t_out) return fail(c, AMVS_EINVAL, "NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    static_assert(sizeof(int) == sizeof(int32_t), "index width");
    HIPCHK(c, amvs::pnp_hypotheses(pts3d, pts2d, m, K, seed, first, count, idx_out, R_out, t_out, c->cache, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_pnp_score(amvs_ctx *c, const double *R, const double *t, int n, const float *pts3d, const float *pts2d, int m,
                   const double K[9], double threshold, int32_t *counts_out)
{
    if (!c) return AMVS_EINVAL;
    if (const char *why = points_error(pts3d, pts2d, m, K)) return fail(c, AMVS_EINVAL, why);
    if (n < 1 || n > AMVS_PNP_MAX_HYP) return fail(c, AMVS_EINVAL, "n outside 1 .. AMVS_PNP_MAX_HYP");
    if (bad_threshold(threshold)) return fail(c, AMVS_EINVAL, "threshold must be positive and finite");
    if (!R || !t || !counts_out) return fail(c, AMVS_EINVAL, "NULL argument");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::pnp_score(R, t, n, pts3d, pts2d, m, K, threshold, counts_out, c->cache, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_pnp_inliers(amvs_ctx *c, const double R[9], const double t[3], const float *pts3d, const float *pts2d, int m,
                     const double K[9], double threshold, uint8_t *mask_out, int64_t *count)
{
    if (!c) return AMVS_EINVAL;
    if (const char *why = points_error(pts3d, pts2d, m, K)) return fail(c, AMVS_EINVAL, why);
    if (bad_threshold(threshold)) return fail(c, AMVS_EINVAL, "threshold must be positive and finite");
    if (!R || !t || !mask_out || !count) return fail(c, AMVS_EINVAL, "NULL argument");
    int rc = bind_device(c);
    if (rc) return rc;
    long long k = 0;
    HIPCHK(c, amvs::pnp_inliers(R, t, pts3d, pts2d, m, K, threshold, mask_out, &k, c->cache, c->stream));
    *count = k;
    return checked(c, AMVS_OK);
}

int amvs_pnp_refine(amvs_ctx *c, const float *pts3d, const float *pts2d, int m, const double K[9], const double R_in[9],
                    const double t_in[3], const uint8_t *mask, double R_out[9], double t_out[3], int32_t *steps, double *cost,
                    int64_t *n_used)
{
    if (!c) return AMVS_EINVAL;
    if (const char *why = points_error(pts3d, pts2d, m, K)) return fail(c, AMVS_EINVAL, why);
    if (!R_in || !t_in) return fail(c, AMVS_EINVAL, "NULL pose");
    if (!R_out || !t_out || !steps || !cost || !n_used) return fail(c, AMVS_EINVAL, "NULL output");
    const long long n_set = mask ? count_set(mask, m) : m;
    if (n_set < 6) return fail(c, AMVS_EINVAL, "fewer than 6 correspondences in the set");
    int rc = bind_device(c);
    if (rc) return rc;
    int taken = 0;
    HIPCHK(c, amvs::pnp_refine(pts3d, pts2d, m, K, R_in, t_in, mask, R_out, t_out, &taken, cost, c->cache, c->stream));
    *steps = taken;
    *n_used = n_set;
    return checked(c, AMVS_OK);
}

int amvs_pnp_ransac(amvs_ctx *c, const float *pts3d, const float *pts2d, int m, const double K[9], double threshold,
                    double confidence, int max_hypotheses, uint64_t seed, double R_out[9], double t_out[3], uint8_t *mask_out,
                    int64_t *n_inliers, int32_t info_out[3])
{
    if (!c) return AMVS_EINVAL;
    if (const char *why = points_error(pts3d, pts2d, m, K)) return fail(c, AMVS_EINVAL, why);
    if (bad_threshold(threshold)) return fail(c, AMVS_EINVAL, "threshold must be positive and finite");
    if (!(confidence > 0.0 && confidence < 1.0)) return fail(c, AMVS_EINVAL, "confidence must be inside (0, 1)");
    if (max_hypotheses < 1 || max_hypotheses > AMVS_PNP_MAX_HYP)
        return fail(c, AMVS_EINVAL, "max_hypotheses outside 1 .. AMVS_PNP_MAX_HYP");
    if (!R_out || !t_out || !mask_out || !n_inliers || !info_out) return fail(c, AMVS_EINVAL, "NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    long long k = 0;
    int info[3] = {0, 0, 0};
    HIPCHK(c, amvs::pnp_ransac(pts3d, pts2d, m, K, threshold, confidence, max_hypotheses, seed, R_out, t_out, mask_out, &k, info,
                               c->cache, c->stream));
    *n_inliers = k;
    for (int i = 0; i < 3; ++i) info_out[i] = info[i];
    return checked(c, AMVS_OK);
}

}  // extern "C"
#pragma GCC visibility pop
