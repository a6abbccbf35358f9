// amvs_bundle_host.h -- the host parts of the bundle adjustment (include/amvs_bundle.h): the parameter checks, the three
// integer lists a call uploads (point segments, per-camera observation lists, the pair list with its segments), and the
// dense solve of the header as a reference.  Plain C++ without the HIP runtime, so that it also compiles into a
// stand-alone host program (tools/bundle_host_check.cpp).  Built with -ffp-contract=off like everything else.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/amvs_bundle.h"
#include "amvs_pnp_step.h"

namespace amvs {

constexpr int BA_CAM_SUMS = 29;       // per camera: U (21), gc (6), cost, act -- the layout of PNP_SUMS
constexpr int BA_SEG_SUMS = 42;       // per segment of S: the 36 entries of a block, then the 6 of the right-hand side

// The problem of a call, as the entry points take it.
struct BaProblem {
    const double *R, *t;
    int C;
    const double *X;
    int P;
    const int32_t *cam, *pt;
    const float *uv;
    int N;
    const double *K;
    const uint8_t *fixed;
};

inline bool ba_is_fixed(const BaProblem &q, int c) { return q.fixed ? q.fixed[c] != 0 : c == 0; }

// the header's errors of the problem; NULL = fine.  need_free: every entry point but amvs_ba_cost.
inline const char *ba_problem_error(const BaProblem &q, bool need_free)
{
    if (!q.R || !q.t || !q.X || !q.cam || !q.pt || !q.uv) return "NULL argument";
    if (const char *why = pnp_intrinsics_error(q.K)) return why;
    if (q.C < 1 || q.C > AMVS_BA_MAX_CAMERAS) return "C outside 1 .. AMVS_BA_MAX_CAMERAS";
    if (q.P < 1 || q.P > AMVS_BA_MAX_POINTS) return "P outside 1 .. AMVS_BA_MAX_POINTS";
    if (q.N < 1 || q.N > AMVS_BA_MAX_OBS) return "N outside 1 .. AMVS_BA_MAX_OBS";
    for (int k = 0; k < q.N; ++k) {
        if (q.cam[k] < 0 || q.cam[k] >= q.C) return "camera index out of range";
        if (q.pt[k] < 0 || q.pt[k] >= q.P) return "point index out of range";
        if (k > 0 && !(q.pt[k - 1] < q.pt[k] || (q.pt[k - 1] == q.pt[k] && q.cam[k - 1] < q.cam[k])))
            return "observations not strictly ascending in (pt, cam)";
    }
    if (!need_free) return nullptr;
    int n_free = 0;
    for (int c = 0; c < q.C; ++c) n_free += ba_is_fixed(q, c) ? 0 : 1;
    if (n_free == 0) return "no free camera";
    long long pairs = 0;
    for (int k = 0; k < q.N;) {
        long long f = 0;
        int e = k;
        for (; e < q.N && q.pt[e] == q.pt[k]; ++e) f += ba_is_fixed(q, q.cam[e]) ? 0 : 1;
        pairs += f * (f + 1) / 2;
        if (pairs > AMVS_BA_MAX_PAIRS) return "more than AMVS_BA_MAX_PAIRS pairs";
        k = e;
    }
    return nullptr;
}

inline bool ba_bad_damping(double v) { return !std::isfinite(v) || v < 0.0; }

// The integer lists of a call.  A "block" is AMVS_BA_BLOCK consecutive positions of one list: [3b] = its camera or segment,
// [3b+1], [3b+2] = the range of positions in cam_list / pair_k.
struct BaLists {
    int F = 0, n = 0;
    std::vector<int> slot;                      // [C]: the slot of a free camera, -1 for a fixed one
    std::vector<int> pt_start;                  // [P+1]: the observations of point p are pt_start[p] .. pt_start[p+1]-1
    std::vector<int> cam_list;                  // [N]: the observations stable-sorted by camera
    std::vector<int> cam_blk0;                  // [C+1]: the blocks of camera c are cam_blk0[c] .. cam_blk0[c+1]-1
    std::vector<int> cam_blk;                   // [3 * blocks]
    std::vector<int> pair_k, pair_k2;           // the pairs k <= k' of free cameras, stable-sorted by (slot, slot)
    std::vector<int> seg_ab;                    // [2 * segments]: the slots (a, b) of a segment; every (a, a), and (a, b) with pairs
    std::vector<int> seg_blk0;                  // [segments + 1]
    std::vector<int> seg_blk;                   // [3 * blocks]
};

inline void ba_build_lists(const BaProblem &q, bool with_pairs, BaLists &L)
{
    const int C = q.C, P = q.P, N = q.N;
    L.slot.assign(C, -1);
    L.F = 0;
    for (int c = 0; c < C; ++c)
        if (!ba_is_fixed(q, c)) L.slot[c] = L.F++;
    L.n = 6 * L.F;
    L.pt_start.assign(P + 1, 0);
    for (int k = 0; k < N; ++k) L.pt_start[q.pt[k] + 1] += 1;
    for (int p = 0; p < P; ++p) L.pt_start[p + 1] += L.pt_start[p];
    // the camera lists: a stable counting sort
    std::vector<int> cam_start(C + 1, 0);
    for (int k = 0; k < N; ++k) cam_start[q.cam[k] + 1] += 1;
    for (int c = 0; c < C; ++c) cam_start[c + 1] += cam_start[c];
    L.cam_list.assign(N, 0);
    {
        std::vector<int> at(cam_start.begin(), cam_start.end() - 1);
        for (int k = 0; k < N; ++k) L.cam_list[at[q.cam[k]]++] = k;
    }
    L.cam_blk0.assign(C + 1, 0);
    L.cam_blk.clear();
    for (int c = 0; c < C; ++c) {
        for (int b = cam_start[c]; b < cam_start[c + 1]; b += AMVS_BA_BLOCK) {
            const int e = b + AMVS_BA_BLOCK < cam_start[c + 1] ? b + AMVS_BA_BLOCK : cam_start[c + 1];
            L.cam_blk.insert(L.cam_blk.end(), {c, b, e});
        }
        L.cam_blk0[c + 1] = (int)(L.cam_blk.size() / 3);
    }
    L.pair_k.clear(); L.pair_k2.clear(); L.seg_ab.clear(); L.seg_blk.clear();
    L.seg_blk0.assign(1, 0);
    if (!with_pairs) return;
    // the pair list: count per (slot, slot), then place in the order of generation (stable)
    const size_t F = (size_t)L.F;
    std::vector<long long> count(F * F + 1, 0);
    for (int p = 0; p < P; ++p)
        for (int k = L.pt_start[p]; k < L.pt_start[p + 1]; ++k) {
            const int a = L.slot[q.cam[k]];
            if (a < 0) continue;
            for (int k2 = k; k2 < L.pt_start[p + 1]; ++k2) {
                const int b = L.slot[q.cam[k2]];
                if (b >= 0) count[(size_t)a * F + (size_t)b + 1] += 1;
            }
        }
    for (size_t s = 0; s < F * F; ++s) count[s + 1] += count[s];
    const long long n_pairs = count[F * F];
    L.pair_k.assign((size_t)n_pairs, 0);
    L.pair_k2.assign((size_t)n_pairs, 0);
    {
        std::vector<long long> at(count.begin(), count.end() - 1);
        for (int p = 0; p < P; ++p)
            for (int k = L.pt_start[p]; k < L.pt_start[p + 1]; ++k) {
                const int a = L.slot[q.cam[k]];
                if (a < 0) continue;
                for (int k2 = k; k2 < L.pt_start[p + 1]; ++k2) {
                    const int b = L.slot[q.cam[k2]];
                    if (b < 0) continue;
                    const long long w = at[(size_t)a * F + (size_t)b]++;
                    L.pair_k[(size_t)w] = k;
                    L.pair_k2[(size_t)w] = k2;
                }
            }
    }
    for (int a = 0; a < L.F; ++a)
        for (int b = a; b < L.F; ++b) {
            const long long s0 = count[(size_t)a * F + (size_t)b], s1 = count[(size_t)a * F + (size_t)b + 1];
            if (a != b && s0 == s1) continue;
            const int seg = (int)(L.seg_ab.size() / 2);
            L.seg_ab.insert(L.seg_ab.end(), {a, b});
            for (long long i = s0; i < s1; i += AMVS_BA_BLOCK) {
                const long long e = i + AMVS_BA_BLOCK < s1 ? i + AMVS_BA_BLOCK : s1;
                L.seg_blk.insert(L.seg_blk.end(), {seg, (int)i, (int)e});
            }
            L.seg_blk0.push_back((int)(L.seg_blk.size() / 3));
        }
}

// The dense solve of the header, as written: S [n][n] row-major (its upper triangle is read), x = the solution.  false:
// NO STEP.  The device's panels must reproduce this bit for bit.
inline bool ba_dense_solve_ref(int n, const double *S, const double *rhs, double *x)
{
    std::vector<double> L((size_t)n * n, 0.0), y(n);
    for (int j = 0; j < n; ++j) {
        double s = S[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) s = s - L[(size_t)j * n + k] * L[(size_t)j * n + k];
        if (!(s > 0.0 && s < INFINITY)) return false;
        L[(size_t)j * n + j] = std::sqrt(s);
        for (int i = j + 1; i < n; ++i) {
            double v = S[(size_t)j * n + i];
            for (int k = 0; k < j; ++k) v = v - L[(size_t)i * n + k] * L[(size_t)j * n + k];
            L[(size_t)i * n + j] = v / L[(size_t)j * n + j];
        }
    }
    for (int i = 0; i < n; ++i) {
        double s = rhs[i];
        for (int k = 0; k < i; ++k) s = s - L[(size_t)i * n + k] * y[k];
        y[i] = s / L[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = y[i];
        for (int k = n - 1; k > i; --k) s = s - L[(size_t)k * n + i] * x[k];
        x[i] = s / L[(size_t)i * n + i];
    }
    return true;
}

}  // namespace amvs
