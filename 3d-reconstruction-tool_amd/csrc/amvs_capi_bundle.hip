// amvs_capi_bundle.hip -- the entry points of include/amvs_bundle.h: the cost, the normal sums, the reduced system, one
// step and the iteration (kernels and host steps in amvs_bundle.hip, the checks and index lists in amvs_bundle_host.h).
#include "amvs_ctx.h"
#include "amvs_bundle_dev.h"

using namespace amvs::host;

#pragma GCC visibility push(default)
extern "C" {

int amvs_ba_cost(amvs_ctx *c, const double *R, const double *t, int C, const double *X, int P, const int32_t *cam, const int32_t *pt,
                 const float *uv, int N, const double K[9], double *cost, int64_t *active, double *err2_out)
{
    if (!c) return AMVS_EINVAL;
    const amvs::BaProblem q{R, t, C, X, P, cam, pt, uv, N, K, nullptr};
    if (!cost || !active || !err2_out) return fail(c, AMVS_EINVAL, "NULL output");
    if (const char *why = amvs::ba_problem_error(q, false)) return fail(c, AMVS_EINVAL, why);
    int rc = bind_device(c);
    if (rc) return rc;
    long long a = 0;
    HIPCHK(c, amvs::ba_cost(q, cost, &a, err2_out, c->cache, c->stream));
    *active = a;
    return checked(c, AMVS_OK);
}

int amvs_ba_normal(amvs_ctx *c, const double *R, const double *t, int C, const double *X, int P, const int32_t *cam, const int32_t *pt,
                   const float *uv, int N, const double K[9], const uint8_t *fixed, double *U_out, double *gc_out, double *V_out,
                   double *gp_out, int32_t *counts_out)
{
    if (!c) return AMVS_EINVAL;
    const amvs::BaProblem q{R, t, C, X, P, cam, pt, uv, N, K, fixed};
    if (!U_out || !gc_out || !V_out || !gp_out || !counts_out) return fail(c, AMVS_EINVAL, "NULL output");
    if (const char *why = amvs::ba_problem_error(q, true)) return fail(c, AMVS_EINVAL, why);
    int rc = bind_device(c);
    if (rc) return rc;
    static_assert(sizeof(int) == sizeof(int32_t), "index width");
    HIPCHK(c, amvs::ba_normal(q, U_out, gc_out, V_out, gp_out, counts_out, c->cache, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_ba_schur(amvs_ctx *c, const double *R, const double *t, int C, const double *X, int P, const int32_t *cam, const int32_t *pt,
                  const float *uv, int N, const double K[9], const uint8_t *fixed, int refine_points, double lambda, double *S_out,
                  double *rhs_out, int32_t *slot_out, uint8_t *held_out)
{
    if (!c) return AMVS_EINVAL;
    const amvs::BaProblem q{R, t, C, X, P, cam, pt, uv, N, K, fixed};
    if (!S_out || !rhs_out || !slot_out || !held_out) return fail(c, AMVS_EINVAL, "NULL output");
    if (const char *why = amvs::ba_problem_error(q, true)) return fail(c, AMVS_EINVAL, why);
    if (amvs::ba_bad_damping(lambda)) return fail(c, AMVS_EINVAL, "lambda must be finite and not negative");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::ba_schur(q, refine_points, lambda, S_out, rhs_out, slot_out, held_out, c->cache, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_ba_step(amvs_ctx *c, const double *R, const double *t, int C, const double *X, int P, const int32_t *cam, const int32_t *pt,
                 const float *uv, int N, const double K[9], const uint8_t *fixed, int refine_points, double lambda, int32_t *ok,
                 double *dc_out, double *dp_out, double *R_out, double *t_out, double *X_out)
{
    if (!c) return AMVS_EINVAL;
    const amvs::BaProblem q{R, t, C, X, P, cam, pt, uv, N, K, fixed};
    if (!ok || !dc_out || !dp_out || !R_out || !t_out || !X_out) return fail(c, AMVS_EINVAL, "NULL output");
    if (const char *why = amvs::ba_problem_error(q, true)) return fail(c, AMVS_EINVAL, why);
    if (amvs::ba_bad_damping(lambda)) return fail(c, AMVS_EINVAL, "lambda must be finite and not negative");
    int rc = bind_device(c);
    if (rc) return rc;
    int have = 0;
    HIPCHK(c, amvs::ba_step(q, refine_points, lambda, &have, dc_out, dp_out, R_out, t_out, X_out, c->cache, c->stream));
    *ok = have;
    return checked(c, AMVS_OK);
}

int amvs_ba_solve(amvs_ctx *c, const double *R, const double *t, int C, const double *X, int P, const int32_t *cam, const int32_t *pt,
                  const float *uv, int N, const double K[9], const uint8_t *fixed, int refine_points, double lambda0, double ftol,
                  int max_trials, double *R_out, double *t_out, double *X_out, double info_out[6])
{
    if (!c) return AMVS_EINVAL;
    const amvs::BaProblem q{R, t, C, X, P, cam, pt, uv, N, K, fixed};
    if (!R_out || !t_out || !X_out || !info_out) return fail(c, AMVS_EINVAL, "NULL output");
    if (const char *why = amvs::ba_problem_error(q, true)) return fail(c, AMVS_EINVAL, why);
    if (amvs::ba_bad_damping(lambda0)) return fail(c, AMVS_EINVAL, "lambda0 must be finite and not negative");
    if (amvs::ba_bad_damping(ftol)) return fail(c, AMVS_EINVAL, "ftol must be finite and not negative");
    if (max_trials < 1) return fail(c, AMVS_EINVAL, "max_trials < 1");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::ba_solve(q, refine_points, lambda0, ftol, max_trials, R_out, t_out, X_out, info_out, c->cache, c->stream));
    return checked(c, AMVS_OK);
}

}  // extern "C"
#pragma GCC visibility pop
