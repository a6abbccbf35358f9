// amvs_capi_fmat.hip -- the entry points of include/amvs_epipolar.h: hypotheses, scoring, inliers, the refit and the
// RANSAC that chains them (kernels and host steps in amvs_fmat.hip).
#include "amvs_ctx.h"
#include "amvs_fmat_host.h"
#include "../../include/amvs_epipolar.h"

using namespace amvs::host;

namespace {

// the parameter errors the five entry points share; NULL = fine
const char *points_error(const float *pts1, const float *pts2, int m)
{
    if (m < 8 || m > AMVS_FMAT_MAX_MATCHES) return "m outside 8 .. AMVS_FMAT_MAX_MATCHES";
    if (!pts1 || !pts2) return "NULL points";
    return nullptr;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int amvs_fmat_hypotheses(amvs_ctx *c, const float *pts1, const float *pts2, int m, uint64_t seed, int first, int count,
                         int32_t *idx_out, double *F_out)
{
    if (!c) return AMVS_EINVAL;
    if (const char *why = points_error(pts1, pts2, m)) return fail(c, AMVS_EINVAL, why);
    if (first < 0) return fail(c, AMVS_EINVAL, "first < 0");
    if (count < 1 || count > AMVS_FMAT_MAX_HYP) return fail(c, AMVS_EINVAL, "count outside 1 .. AMVS_FMAT_MAX_HYP");
    if (!idx_out || !F_out) return fail(c, AMVS_EINVAL, "NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    static_assert(sizeof(int) == sizeof(int32_t), "index width");
    HIPCHK(c, amvs::fmat_hypotheses(pts1, pts2, m, seed, first, count, idx_out, F_out, c->cache, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_fmat_score(amvs_ctx *c, const double *F, int n, const float *pts1, const float *pts2, int m, double threshold,
                    int32_t *counts_out)
{
    if (!c) return AMVS_EINVAL;
    if (const char *why = points_error(pts1, pts2, m)) return fail(c, AMVS_EINVAL, why);
    if (n < 1 || n > AMVS_FMAT_MAX_HYP) return fail(c, AMVS_EINVAL, "n outside 1 .. AMVS_FMAT_MAX_HYP");
    if (bad_threshold(threshold)) return fail(c, AMVS_EINVAL, "threshold must be positive and finite");
    if (!F || !counts_out) return fail(c, AMVS_EINVAL, "NULL argument");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::fmat_score(F, n, pts1, pts2, m, threshold, counts_out, c->cache, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_fmat_inliers(amvs_ctx *c, const double F[9], const float *pts1, const float *pts2, int m, double threshold,
                      uint8_t *mask_out, int64_t *count)
{
    if (!c) return AMVS_EINVAL;
    if (const char *why = points_error(pts1, pts2, m)) return fail(c, AMVS_EINVAL, why);
    if (bad_threshold(threshold)) return fail(c, AMVS_EINVAL, "threshold must be positive and finite");
    if (!F || !mask_out || !count) return fail(c, AMVS_EINVAL, "NULL argument");
    int rc = bind_device(c);
    if (rc) return rc;
    long long k = 0;
    HIPCHK(c, amvs::fmat_inliers(F, pts1, pts2, m, threshold, mask_out, &k, c->cache, c->stream));
    *count = k;
    return checked(c, AMVS_OK);
}

int amvs_fmat_fit(amvs_ctx *c, const float *pts1, const float *pts2, const uint8_t *mask, int m, double F_out[9], int64_t *n_used)
{
    if (!c) return AMVS_EINVAL;
    if (const char *why = points_error(pts1, pts2, m)) return fail(c, AMVS_EINVAL, why);
    if (!F_out || !n_used) return fail(c, AMVS_EINVAL, "NULL output");
    const long long n_set = mask ? count_set(mask, m) : m;
    if (n_set < 8) return fail(c, AMVS_EINVAL, "fewer than 8 matches in the set");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::fmat_fit(pts1, pts2, mask, m, n_set, F_out, c->cache, c->stream));
    *n_used = n_set;
    return checked(c, AMVS_OK);
}

int amvs_fmat_ransac(amvs_ctx *c, const float *pts1, const float *pts2, int m, double threshold, double confidence,
                     int max_hypotheses, uint64_t seed, double F_out[9], uint8_t *mask_out, int64_t *n_inliers, int32_t info_out[3])
{
    if (!c) return AMVS_EINVAL;
    if (const char *why = points_error(pts1, pts2, m)) return fail(c, AMVS_EINVAL, why);
    if (bad_threshold(threshold)) return fail(c, AMVS_EINVAL, "threshold must be positive and finite");
    if (!(confidence > 0.0 && confidence < 1.0)) return fail(c, AMVS_EINVAL, "confidence must be inside (0, 1)");
    if (max_hypotheses < 1 || max_hypotheses > AMVS_FMAT_MAX_HYP)
        return fail(c, AMVS_EINVAL, "max_hypotheses outside 1 .. AMVS_FMAT_MAX_HYP");
    if (!F_out || !mask_out || !n_inliers || !info_out) return fail(c, AMVS_EINVAL, "NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    long long k = 0;
    int info[3] = {0, 0, 0};
    HIPCHK(c, amvs::fmat_ransac(pts1, pts2, m, threshold, confidence, max_hypotheses, seed, F_out, mask_out, &k, info, c->cache,
                                c->stream));
    *n_inliers = k;
    for (int i = 0; i < 3; ++i) info_out[i] = info[i];
    return checked(c, AMVS_OK);
}

}  // extern "C"
#pragma GCC visibility pop
