// amvs_capi_twoview.hip -- the entry points of include/amvs_twoview.h: the decomposition of F (host arithmetic,
// amvs_twoview_host.h), the cheirality counts and mask, the relative pose that chains them, and the triangulation that
// returns every candidate (kernels and host steps in amvs_twoview.hip).
#include "amvs_ctx.h"
#include "amvs_twoview_dev.h"
#include "amvs_twoview_host.h"
#include "../../include/amvs_twoview.h"

#include <cmath>

using namespace amvs::host;

namespace {

// the parameter errors the scoring entry points share; NULL = fine
const char *matches_error(const float *pts1, const float *pts2, int m, const double *K, double max_depth)
{
    if (m < 1 || m > AMVS_TWOVIEW_MAX_MATCHES) return "m outside 1 .. AMVS_TWOVIEW_MAX_MATCHES";
    if (!pts1 || !pts2) return "NULL points";
    if (!(max_depth > 0.0)) return "max_depth must be positive (+infinity is allowed)";
    return amvs::pnp_intrinsics_error(K);
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int amvs_twoview_decompose(amvs_ctx *c, const double F[9], const double K[9], double R_out[2][9], double t_out[3], double w_out[3],
                           int32_t *ok)
{
    if (!c) return AMVS_EINVAL;
    if (!F) return fail(c, AMVS_EINVAL, "NULL F");
    if (const char *why = amvs::pnp_intrinsics_error(K)) return fail(c, AMVS_EINVAL, why);
    if (!R_out || !t_out || !w_out || !ok) return fail(c, AMVS_EINVAL, "NULL output");
    *ok = amvs::twoview_decompose(F, K, &R_out[0][0], t_out, w_out) ? 1 : 0;
    return AMVS_OK;
}

int amvs_twoview_score(amvs_ctx *c, const double *R, const double *t, int n, const float *pts1, const float *pts2, int m,
                       const double K[9], double max_depth, int32_t *counts_out)
{
    if (!c) return AMVS_EINVAL;
    if (const char *why = matches_error(pts1, pts2, m, K, max_depth)) return fail(c, AMVS_EINVAL, why);
    if (n < 1 || n > AMVS_TWOVIEW_MAX_POSES) return fail(c, AMVS_EINVAL, "n outside 1 .. AMVS_TWOVIEW_MAX_POSES");
    if (!R || !t || !counts_out) return fail(c, AMVS_EINVAL, "NULL argument");
    int rc = bind_device(c);
    if (rc) return rc;
    static_assert(sizeof(int) == sizeof(int32_t), "count width");
    HIPCHK(c, amvs::twoview_score(R, t, n, pts1, pts2, m, K, max_depth, counts_out, c->cache, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_twoview_front(amvs_ctx *c, const double R[9], const double t[3], const float *pts1, const float *pts2, int m,
                       const double K[9], double max_depth, uint8_t *mask_out, int64_t *count)
{
    if (!c) return AMVS_EINVAL;
    if (const char *why = matches_error(pts1, pts2, m, K, max_depth)) return fail(c, AMVS_EINVAL, why);
    if (!R || !t || !mask_out || !count) return fail(c, AMVS_EINVAL, "NULL argument");
    int rc = bind_device(c);
    if (rc) return rc;
    long long k = 0;
    HIPCHK(c, amvs::twoview_front(R, t, pts1, pts2, m, K, max_depth, mask_out, &k, c->cache, c->stream));
    *count = k;
    return checked(c, AMVS_OK);
}

int amvs_twoview_pose(amvs_ctx *c, const double F[9], const double K[9], const float *pts1, const float *pts2, int m,
                      double max_depth, double R_out[9], double t_out[3], uint8_t *mask_out, int64_t *n_front, int32_t info_out[5])
{
    if (!c) return AMVS_EINVAL;
    if (const char *why = matches_error(pts1, pts2, m, K, max_depth)) return fail(c, AMVS_EINVAL, why);
    if (!F) return fail(c, AMVS_EINVAL, "NULL F");
    if (!R_out || !t_out || !mask_out || !n_front || !info_out) return fail(c, AMVS_EINVAL, "NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    long long k = 0;
    int info[5] = {0, 0, 0, 0, 0};
    bool model = false;
    HIPCHK(c, amvs::twoview_pose(F, K, pts1, pts2, m, max_depth, R_out, t_out, mask_out, &k, info, &model, c->cache, c->stream));
    *n_front = k;
    for (int i = 0; i < 5; ++i) info_out[i] = info[i];
    return checked(c, AMVS_OK);
}

int amvs_twoview_triangulate(amvs_ctx *c, const double K[9], const double R1[9], const double t1[3], const double R2[9],
                             const double t2[3], const float *pts1, const float *pts2, int m, double depth_min, double depth_max,
                             double cos_max_parallax, double max_reproj, double *X_out, uint8_t *valid_out, double *cos_out,
                             int64_t *n_valid)
{
    if (!c) return AMVS_EINVAL;
    if (m < 0 || m > AMVS_TWOVIEW_MAX_MATCHES) return fail(c, AMVS_EINVAL, "m outside 0 .. AMVS_TWOVIEW_MAX_MATCHES");
    if (const char *why = amvs::pnp_intrinsics_error(K)) return fail(c, AMVS_EINVAL, why);
    if (!R1 || !t1 || !R2 || !t2 || !n_valid) return fail(c, AMVS_EINVAL, "NULL argument");
    if (m > 0 && (!pts1 || !pts2 || !X_out || !valid_out || !cos_out)) return fail(c, AMVS_EINVAL, "NULL array with m > 0");
    if (std::isnan(depth_min) || std::isnan(depth_max) || std::isnan(cos_max_parallax) || std::isnan(max_reproj))
        return fail(c, AMVS_EINVAL, "a threshold is NaN");
    int rc = bind_device(c);
    if (rc) return rc;
    long long k = 0;
    const amvs::TwoviewThresholds thr{depth_min, depth_max, cos_max_parallax, max_reproj};
    HIPCHK(c, amvs::twoview_triangulate(K, R1, t1, R2, t2, pts1, pts2, m, thr, X_out, valid_out, cos_out, &k, c->cache, c->stream));
    *n_valid = k;
    return checked(c, AMVS_OK);
}

}  // extern "C"
#pragma GCC visibility pop
