// amvs_capi_sfm.hip -- the entry points of include/amvs_sfm.h: every parameter check, the host side of the track state (the
// layout, which views are registered, their poses) and the choice of the pairs a call walks; the kernels are in amvs_sfm.hip.
#include "amvs_ctx.h"
#include "amvs_sfm_state.h"
#include "amvs_pnp_step.h"
#include "../../include/amvs_sfm.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace amvs::host;
using amvs::SfmSeg;
using amvs::SfmState;
using amvs::SfmTriPair;

static_assert(AMVS_SFM_MAX_VIEWS <= (1 << 12), "amvs_sfm_drop packs a view into 12 bits of its keys");
static_assert(sizeof(int) == sizeof(int32_t), "index width");

namespace {

// the state of an open reconstruction, or NULL with the error set
SfmState *open_state(amvs_ctx *c)
{
    if (!c->sfm.open) {
        fail(c, AMVS_EINVAL, "no track state: call amvs_sfm_begin first");
        return nullptr;
    }
    return &c->sfm;
}

// the rows of the pairs with exactly one registered view (view < 0), or of the pairs of `view` with a registered view
int segments_of(const SfmState &s, int view, std::vector<SfmSeg> &segs)
{
    int total = 0;
    auto add = [&](int p) {
        const int i = s.pair_views[2 * p], j = s.pair_views[2 * p + 1], n = s.pair_start[p + 1] - s.pair_start[p];
        if (n <= 0 || s.registered[i] == s.registered[j]) return;
        segs.push_back(SfmSeg{s.pair_start[p], total, s.registered[j] ? 1 : 0});
        total += n;
    };
    if (view < 0)
        for (int p = 0; p < s.P; ++p) add(p);
    else
        for (int p : s.pairs_of[view]) add(p);
    return total;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int amvs_sfm_begin(amvs_ctx *c, int V, const int32_t *n_kp, const float *kp, int P, const int32_t *pair_views, const int32_t *pair_start,
                   const int32_t *rows)
{
    if (!c) return AMVS_EINVAL;
    if (V < 1 || V > AMVS_SFM_MAX_VIEWS) return fail(c, AMVS_EINVAL, "V outside 1 .. AMVS_SFM_MAX_VIEWS");
    if (!n_kp) return fail(c, AMVS_EINVAL, "NULL n_kp");
    if (P < 0 || (long long)P > (long long)V * (V - 1) / 2) return fail(c, AMVS_EINVAL, "P outside 0 .. V (V - 1) / 2");
    if (!pair_start || (P > 0 && !pair_views)) return fail(c, AMVS_EINVAL, "NULL pairs");
    std::vector<int> off((size_t)V + 1, 0);
    long long G = 0;
    int widest = 0;
    for (int v = 0; v < V; ++v) {
        if (n_kp[v] < 0) return fail(c, AMVS_EINVAL, "a negative keypoint count");
        G += n_kp[v];
        if (G > AMVS_SFM_MAX_KEYPOINTS) return fail(c, AMVS_EINVAL, "more than AMVS_SFM_MAX_KEYPOINTS keypoints");
        off[(size_t)v + 1] = (int)G;
        widest = std::max(widest, (int)n_kp[v]);
    }
    if (G > 0 && !kp) return fail(c, AMVS_EINVAL, "NULL kp");
    if (pair_start[0] != 0) return fail(c, AMVS_EINVAL, "pair_start[0] must be 0");
    for (int p = 0; p < P; ++p) {
        const int i = pair_views[2 * p], j = pair_views[2 * p + 1];
        if (i < 0 || j >= V || i >= j) return fail(c, AMVS_EINVAL, "a pair needs 0 <= i < j < V");
        if (p > 0 && !(pair_views[2 * p - 2] < i || (pair_views[2 * p - 2] == i && pair_views[2 * p - 1] < j)))
            return fail(c, AMVS_EINVAL, "pairs must be strictly ascending in (i, j)");
        if (pair_start[p + 1] < pair_start[p]) return fail(c, AMVS_EINVAL, "pair_start must not descend");
        if (pair_start[p + 1] > AMVS_SFM_MAX_ROWS) return fail(c, AMVS_EINVAL, "more than AMVS_SFM_MAX_ROWS rows");
    }
    const long long M = pair_start[P];
    if (M > 0 && !rows) return fail(c, AMVS_EINVAL, "NULL rows");
    {   // every index in range, no keypoint twice on one side of a pair: seen[side][k] = the last pair that named k, plus one
        std::vector<int> seen[2] = {std::vector<int>((size_t)widest, 0), std::vector<int>((size_t)widest, 0)};
        for (int p = 0; p < P; ++p) {
            const int n[2] = {n_kp[pair_views[2 * p]], n_kp[pair_views[2 * p + 1]]};
            for (int m = pair_start[p]; m < pair_start[p + 1]; ++m)
                for (int side = 0; side < 2; ++side) {
                    const int k = rows[2 * (size_t)m + side];
                    if (k < 0 || k >= n[side]) return fail(c, AMVS_EINVAL, "a row names a keypoint outside its view");
                    if (seen[side][(size_t)k] == p + 1) return fail(c, AMVS_EINVAL, "a keypoint appears twice on one side of a pair");
                    seen[side][(size_t)k] = p + 1;
                }
        }
    }
    int rc = bind_device(c);
    if (rc) return rc;
    SfmState &s = c->sfm;
    s.open = false;
    s.V = V;
    s.P = P;
    s.G = G;
    s.M = M;
    s.off = std::move(off);
    s.pair_views.assign(pair_views, pair_views + 2 * (size_t)P);
    s.pair_start.assign(pair_start, pair_start + (size_t)P + 1);
    s.pairs_of.assign((size_t)V, std::vector<int>());
    for (int p = 0; p < P; ++p) {           // pair order is (i, j) order: per view the other view ascends
        s.pairs_of[(size_t)pair_views[2 * p]].push_back(p);
        s.pairs_of[(size_t)pair_views[2 * p + 1]].push_back(p);
    }
    s.registered.assign((size_t)V, 0);
    s.pose.assign(12 * (size_t)V, 0.0);
    HIPCHK(c, amvs::sfm_upload(s, kp, rows, c->cache, c->stream));
    s.open = true;
    return checked(c, AMVS_OK);
}

int amvs_sfm_register(amvs_ctx *c, int view, const double R[9], const double t[3], const int32_t *kp, const int32_t *pid,
                      const uint8_t *mask, int m, int64_t *n_set)
{
    if (!c) return AMVS_EINVAL;
    SfmState *s = open_state(c);
    if (!s) return AMVS_EINVAL;
    if (view < 0 || view >= s->V) return fail(c, AMVS_EINVAL, "view out of range");
    if (s->registered[(size_t)view]) return fail(c, AMVS_EINVAL, "the view is registered already");
    if (!R || !t || !n_set) return fail(c, AMVS_EINVAL, "NULL argument");
    if (m < 0 || (m > 0 && (!kp || !pid))) return fail(c, AMVS_EINVAL, "m < 0 or a NULL array with m > 0");
    const int n_view = s->off[(size_t)view + 1] - s->off[(size_t)view];
    std::vector<int> kps, pids;
    for (int i = 0; i < m; ++i) {
        if (mask && !mask[i]) continue;
        if (kp[i] < 0 || kp[i] >= n_view) return fail(c, AMVS_EINVAL, "a kp outside the view's keypoints");
        if (pid[i] < 0 || pid[i] >= s->n_points) return fail(c, AMVS_EINVAL, "a pid outside the points");
        kps.push_back(kp[i]);
        pids.push_back(pid[i]);
    }
    for (const std::vector<int> *list : {&kps, &pids}) {
        std::vector<int> sorted(*list);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return fail(c, AMVS_EINVAL, list == &kps ? "a kp is repeated" : "a pid is repeated");
    }
    int rc = bind_device(c);
    if (rc) return rc;
    long long k = 0;
    HIPCHK(c, amvs::sfm_register(*s, view, kps.data(), pids.data(), (int)kps.size(), &k, c->cache, c->stream));
    s->registered[(size_t)view] = 1;
    std::memcpy(&s->pose[12 * (size_t)view], R, 9 * sizeof(double));
    std::memcpy(&s->pose[12 * (size_t)view + 9], t, 3 * sizeof(double));
    *n_set = k;
    return checked(c, AMVS_OK);
}

int amvs_sfm_scores(amvs_ctx *c, int32_t *scores_out)
{
    if (!c) return AMVS_EINVAL;
    SfmState *s = open_state(c);
    if (!s) return AMVS_EINVAL;
    if (!scores_out) return fail(c, AMVS_EINVAL, "NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    std::vector<SfmSeg> segs;
    const int total = segments_of(*s, -1, segs);
    HIPCHK(c, amvs::sfm_scores(*s, segs, total, scores_out, c->cache, c->stream));
    for (int v = 0; v < s->V; ++v)
        if (s->registered[(size_t)v]) scores_out[v] = -1;
    return checked(c, AMVS_OK);
}

int amvs_sfm_correspondences(amvs_ctx *c, int view, int32_t *kp_out, int32_t *pid_out, float *X_out, float *x_out, int64_t *m)
{
    if (!c) return AMVS_EINVAL;
    SfmState *s = open_state(c);
    if (!s) return AMVS_EINVAL;
    if (view < 0 || view >= s->V) return fail(c, AMVS_EINVAL, "view out of range");
    if (s->registered[(size_t)view]) return fail(c, AMVS_EINVAL, "the view is registered already");
    if (!m) return fail(c, AMVS_EINVAL, "NULL m");
    if (s->off[(size_t)view + 1] > s->off[(size_t)view] && (!kp_out || !pid_out || !X_out || !x_out))
        return fail(c, AMVS_EINVAL, "NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    std::vector<SfmSeg> segs;
    const int total = segments_of(*s, view, segs);
    long long k = 0;
    HIPCHK(c, amvs::sfm_correspondences(*s, view, segs, total, kp_out, pid_out, X_out, x_out, &k, c->cache, c->stream));
    *m = k;
    return checked(c, AMVS_OK);
}

int amvs_sfm_triangulate(amvs_ctx *c, int view, const double K[9], double depth_min, double depth_baselines, double cos_max_parallax,
                         double max_reproj, int64_t *n_new, int32_t *new_per_view)
{
    if (!c) return AMVS_EINVAL;
    SfmState *s = open_state(c);
    if (!s) return AMVS_EINVAL;
    if (view < 0 || view >= s->V) return fail(c, AMVS_EINVAL, "view out of range");
    if (!s->registered[(size_t)view]) return fail(c, AMVS_EINVAL, "the view is not registered");
    if (const char *why = amvs::pnp_intrinsics_error(K)) return fail(c, AMVS_EINVAL, why);
    if (std::isnan(depth_min) || std::isnan(depth_baselines) || std::isnan(cos_max_parallax) || std::isnan(max_reproj))
        return fail(c, AMVS_EINVAL, "a threshold is NaN");
    if (!n_new || !new_per_view) return fail(c, AMVS_EINVAL, "NULL output");
    const int n_view = s->off[(size_t)view + 1] - s->off[(size_t)view];
    if (s->n_points + n_view > AMVS_SFM_MAX_POINTS) return fail(c, AMVS_EINVAL, "n_points + n_view above AMVS_SFM_MAX_POINTS");
    int rc = bind_device(c);
    if (rc) return rc;
    std::vector<SfmTriPair> pairs;
    for (int p : s->pairs_of[(size_t)view]) {
        const int lo = s->pair_views[2 * p], hi = s->pair_views[2 * p + 1], r = lo == view ? hi : lo;
        if (!s->registered[(size_t)r]) continue;
        SfmTriPair q;
        q.r = r;
        q.row0 = s->pair_start[p];
        q.count = s->pair_start[p + 1] - s->pair_start[p];
        const double *p1 = &s->pose[12 * (size_t)lo], *p2 = &s->pose[12 * (size_t)hi];
        std::memcpy(q.R1, p1, sizeof(q.R1));
        std::memcpy(q.t1, p1 + 9, sizeof(q.t1));
        std::memcpy(q.R2, p2, sizeof(q.R2));
        std::memcpy(q.t2, p2 + 9, sizeof(q.t2));
        double C1[3], C2[3], d[3];
        for (int i = 0; i < 3; ++i) {
            C1[i] = -((q.R1[i] * q.t1[0] + q.R1[3 + i] * q.t1[1]) + q.R1[6 + i] * q.t1[2]);
            C2[i] = -((q.R2[i] * q.t2[0] + q.R2[3 + i] * q.t2[1]) + q.R2[6 + i] * q.t2[2]);
            d[i] = C2[i] - C1[i];
        }
        q.depth_max = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) * depth_baselines;
        pairs.push_back(q);
    }
    long long k = 0;
    HIPCHK(c, amvs::sfm_triangulate(*s, K, pairs, n_view, depth_min, cos_max_parallax, max_reproj, new_per_view, &k, c->cache, c->stream));
    *n_new = k;
    return checked(c, AMVS_OK);
}

int amvs_sfm_counts(amvs_ctx *c, int64_t *n_points, int64_t *n_alive, int64_t *n_obs)
{
    if (!c) return AMVS_EINVAL;
    SfmState *s = open_state(c);
    if (!s) return AMVS_EINVAL;
    if (!n_points || !n_alive || !n_obs) return fail(c, AMVS_EINVAL, "NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    long long a = 0, o = 0;
    HIPCHK(c, amvs::sfm_counts(*s, &a, &o, c->cache, c->stream));
    *n_points = s->n_points;
    *n_alive = a;
    *n_obs = o;
    return checked(c, AMVS_OK);
}

int amvs_sfm_observations(amvs_ctx *c, int32_t *cam, int32_t *pt, float *uv, int64_t capacity, int64_t *n)
{
    if (!c) return AMVS_EINVAL;
    SfmState *s = open_state(c);
    if (!s) return AMVS_EINVAL;
    if (!n) return fail(c, AMVS_EINVAL, "NULL n");
    int rc = bind_device(c);
    if (rc) return rc;
    long long a = 0, o = 0;
    HIPCHK(c, amvs::sfm_counts(*s, &a, &o, c->cache, c->stream));
    *n = o;
    if (capacity < o) return fail(c, AMVS_EINVAL, "capacity below the number of observations");
    if (o > 0 && (!cam || !pt || !uv)) return fail(c, AMVS_EINVAL, "NULL output");
    HIPCHK(c, amvs::sfm_observations(*s, cam, pt, uv, o, c->cache, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_sfm_points_get(amvs_ctx *c, double *X, uint8_t *alive, int64_t capacity)
{
    if (!c) return AMVS_EINVAL;
    SfmState *s = open_state(c);
    if (!s) return AMVS_EINVAL;
    if (capacity < s->n_points) return fail(c, AMVS_EINVAL, "capacity below n_points");
    if (s->n_points > 0 && (!X || !alive)) return fail(c, AMVS_EINVAL, "NULL output");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::sfm_points_get(*s, X, alive, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_sfm_points_set(amvs_ctx *c, const double *X, const uint8_t *alive, int64_t n)
{
    if (!c) return AMVS_EINVAL;
    SfmState *s = open_state(c);
    if (!s) return AMVS_EINVAL;
    if (n != s->n_points) return fail(c, AMVS_EINVAL, "n must be n_points");
    if (n > 0 && (!X || !alive)) return fail(c, AMVS_EINVAL, "NULL input");
    int rc = bind_device(c);
    if (rc) return rc;
    std::vector<unsigned char> alive_now((size_t)n), alive_new((size_t)n);
    HIPCHK(c, amvs::sfm_points_get(*s, nullptr, alive_now.data(), c->stream));
    for (int64_t i = 0; i < n; ++i) {
        alive_new[(size_t)i] = alive[i] ? 1 : 0;
        if (alive_new[(size_t)i] && !alive_now[(size_t)i]) return fail(c, AMVS_EINVAL, "a dead point cannot come back");
    }
    HIPCHK(c, amvs::sfm_points_set(*s, X, alive_new.data(), c->cache, c->stream));
    return checked(c, AMVS_OK);
}

int amvs_sfm_pose_set(amvs_ctx *c, int view, const double R[9], const double t[3])
{
    if (!c) return AMVS_EINVAL;
    SfmState *s = open_state(c);
    if (!s) return AMVS_EINVAL;
    if (view < 0 || view >= s->V) return fail(c, AMVS_EINVAL, "view out of range");
    if (!s->registered[(size_t)view]) return fail(c, AMVS_EINVAL, "the view is not registered");
    if (!R || !t) return fail(c, AMVS_EINVAL, "NULL pose");
    std::memcpy(&s->pose[12 * (size_t)view], R, 9 * sizeof(double));
    std::memcpy(&s->pose[12 * (size_t)view + 9], t, 3 * sizeof(double));
    return AMVS_OK;
}

int amvs_sfm_drop(amvs_ctx *c, const int32_t *cam, const int32_t *pt, int n, int min_obs, int64_t *obs_dropped, int64_t *points_dropped)
{
    if (!c) return AMVS_EINVAL;
    SfmState *s = open_state(c);
    if (!s) return AMVS_EINVAL;
    if (n < 0 || min_obs < 0) return fail(c, AMVS_EINVAL, "n or min_obs negative");
    if (n > 0 && (!cam || !pt)) return fail(c, AMVS_EINVAL, "NULL array with n > 0");
    if (!obs_dropped || !points_dropped) return fail(c, AMVS_EINVAL, "NULL output");
    std::vector<long long> keys((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (cam[i] < 0 || cam[i] >= s->V) return fail(c, AMVS_EINVAL, "a cam out of range");
        if (pt[i] < 0 || pt[i] >= s->n_points) return fail(c, AMVS_EINVAL, "a pt out of range");
        keys[(size_t)i] = ((long long)pt[i] << 12) | cam[i];
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    int rc = bind_device(c);
    if (rc) return rc;
    long long od = 0, pd = 0;
    HIPCHK(c, amvs::sfm_drop(*s, keys.data(), (int)keys.size(), min_obs, &od, &pd, c->cache, c->stream));
    *obs_dropped = od;
    *points_dropped = pd;
    return checked(c, AMVS_OK);
}

}  // extern "C"
#pragma GCC visibility pop
