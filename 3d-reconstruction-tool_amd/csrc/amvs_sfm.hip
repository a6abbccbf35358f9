// amvs_sfm.hip -- the kernels of the resident track state (include/amvs_sfm.h; the definition is the header's, the judge
// tests/sfm_state_restatement.py: integers exactly, points bit for bit).
//
// The data is flat: rows[m] = the two global keypoint indices of match row m, owner[g] = the point of keypoint g.  The
// entry points decide on the host which pairs a call walks (the registered flags are there) and hand the kernels those pairs'
// row ranges as SEGMENTS laid end to end; a lane finds its segment by bisection of the segment starts (a few dozen
// entries, read through the cache by every lane), so a workgroup may hold rows of several pairs.
//
// sfm_score_rows_kernel:  one lane per row: an 8-byte row load, one 4-byte gather into owner, a flag byte stored for the
//     keypoint of the unregistered side.  sfm_score_count_kernel: one lane per keypoint, the flags of a wave counted by
//     ballot and added once per wave when the wave lies in one view (else per lane).
// sfm_corr_a/b/c_kernel:  stages A and B of the header by atomicMin on int32 ranks in global memory, then the keep flag;
//     the kept keypoints are compacted by hipCUB and sfm_corr_gather_kernel writes their rows.
// sfm_tri_kernel:  one lane per row of ONE pair: two gathers into owner, tri_candidate of amvs_twoview_tri.h for the rows
//     with both keypoints un-owned, a flag and the point into scratch; hipCUB scans the flags, sfm_tri_base_kernel (one
//     lane) advances the id base, sfm_tri_assign_kernel writes X, alive and the two owners.  The next pair's launches queue
//     behind these: the one sequential dependence of the header is stream order.
// sfm_obs_*:  the owned keypoints compacted, (id << 32 | g) keys sorted by hipCUB (g ascending is view ascending), decoded.
// sfm_drop_*:  a keypoint bisects the sorted (point, view) keys of the call; observation counts per point by atomicAdd.
//
// Every data-dependent global index goes through AMVS_IDX.  All results are integers or the bits of tri_candidate, so no
// launch shape enters any of them.
//
// -ffp-contract=off (Makefile): a * b + c below is two roundings, on the device and on the host.
#define AMVS_TU_ID 26
#include "amvs_check.h"
#include "amvs_dlt4.h"
#include "amvs_sfm_state.h"
#include "amvs_twoview_host.h"
#include "amvs_twoview_tri.h"
#include "../../include/amvs_sfm.h"

#include <hipcub/hipcub.hpp>

#include <climits>
#include <cstring>

namespace amvs {

namespace {

constexpr int B = AMVS_SFM_BLOCK;
using Lease = ScratchCache::Lease;

inline dim3 grid_for(long long n) { return dim3((unsigned)((n + B - 1) / B)); }

// the segment of position t: the last s with seg[s].first <= t
__device__ __forceinline__ SfmSeg seg_of(const SfmSeg *__restrict__ seg, int n_seg, int t)
{
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[AMVS_IDX(mid, n_seg)].first <= t) lo = mid; else hi = mid - 1;
    }
    return seg[AMVS_IDX(lo, n_seg)];
}

// the number of lanes of the wave with p set, in every lane
__device__ __forceinline__ int wave_count(bool p) { return __popcll(__ballot(p)); }

__global__ __launch_bounds__(B) void sfm_fill_kernel(int *__restrict__ a, long long n, int value)
{
    const long long i = (long long)blockIdx.x * B + threadIdx.x;
    if (i < n) a[i] = value;
}

// ---- scores ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(B) void sfm_score_rows_kernel(const SfmSeg *__restrict__ seg, int n_seg, int total, const int2 *__restrict__ rows,
                                                           long long M, const int *__restrict__ owner, long long G,
                                                           unsigned char *__restrict__ flag)
{
    const int t = (int)(blockIdx.x * B + threadIdx.x);
    if (t >= total) return;
    const SfmSeg s = seg_of(seg, n_seg, t);
    const int2 row = rows[AMVS_IDX((long long)s.row0 + (t - s.first), M)];
    const int g_reg = s.side ? row.y : row.x, g_new = s.side ? row.x : row.y;
    if (owner[AMVS_IDX(g_reg, G)] >= 0) flag[AMVS_IDX(g_new, G)] = 1;
}

__global__ __launch_bounds__(B) void sfm_score_count_kernel(const unsigned char *__restrict__ flag, const int *__restrict__ kview, long long G,
                                                            int V, int *__restrict__ counts)
{
    const long long g = (long long)blockIdx.x * B + threadIdx.x;
    const bool live = g < G;
    const bool set = live && flag[g] != 0;
    const int v = live ? kview[g] : -1;
    const int v0 = __shfl(v, 0);                       // lane 0 of a wave is live whenever any lane is
    if (__all(v == v0 || !live)) {
        const int c = wave_count(set);
        if (c != 0 && (threadIdx.x & 63) == 0) atomicAdd(&counts[AMVS_IDX(v0, V)], c);
    } else if (set) {
        atomicAdd(&counts[AMVS_IDX(v, V)], 1);
    }
}

// ---- correspondences ------------------------------------------------------------------------------------------------
// stage A: best[k] = the lowest rank among the candidates of keypoint k of the view (keypoints off .. off + n_view - 1)
__global__ __launch_bounds__(B) void sfm_corr_a_kernel(const SfmSeg *__restrict__ seg, int n_seg, int total, const int2 *__restrict__ rows,
                                                       long long M, const int *__restrict__ owner, long long G, int off, int n_view,
                                                       int *__restrict__ best)
{
    const int t = (int)(blockIdx.x * B + threadIdx.x);
    if (t >= total) return;
    const SfmSeg s = seg_of(seg, n_seg, t);
    const int m = s.row0 + (t - s.first);
    const int2 row = rows[AMVS_IDX(m, M)];
    const int g_reg = s.side ? row.y : row.x, g_new = s.side ? row.x : row.y;
    if (owner[AMVS_IDX(g_reg, G)] >= 0) atomicMin(&best[AMVS_IDX(g_new - off, n_view)], m);
}

// the point of the candidate row `m` of a keypoint of the view: the owner of the row's OTHER keypoint
__device__ __forceinline__ int corr_point(const int2 *__restrict__ rows, long long M, const int *__restrict__ owner, long long G, int off,
                                          int n_view, int m)
{
    const int2 row = rows[AMVS_IDX(m, M)];
    const bool mine_is_x = row.x >= off && row.x < off + n_view;      // the two keypoints of a row lie in different views
    return owner[AMVS_IDX(mine_is_x ? row.y : row.x, G)];
}

// stage B: pbest[p] = the lowest best[k] among the keypoints whose candidate point is p
__global__ __launch_bounds__(B) void sfm_corr_b_kernel(const int *__restrict__ best, int off, int n_view, const int2 *__restrict__ rows,
                                                       long long M, const int *__restrict__ owner, long long G, int *__restrict__ pbest,
                                                       long long n_points)
{
    const int k = (int)(blockIdx.x * B + threadIdx.x);
    if (k >= n_view) return;
    const int m = best[k];
    if (m == INT_MAX) return;
    const int p = corr_point(rows, M, owner, G, off, n_view, m);
    atomicMin(&pbest[AMVS_IDX(p, n_points)], m);
}

// keep[k] and point[k]
__global__ __launch_bounds__(B) void sfm_corr_c_kernel(const int *__restrict__ best, int off, int n_view, const int2 *__restrict__ rows,
                                                       long long M, const int *__restrict__ owner, long long G, const int *__restrict__ pbest,
                                                       long long n_points, unsigned char *__restrict__ keep, int *__restrict__ point)
{
    const int k = (int)(blockIdx.x * B + threadIdx.x);
    if (k >= n_view) return;
    const int m = best[k];
    int p = -1;
    bool kept = false;
    if (m != INT_MAX) {
        p = corr_point(rows, M, owner, G, off, n_view, m);
        kept = pbest[AMVS_IDX(p, n_points)] == m;
    }
    keep[k] = kept ? 1 : 0;
    point[k] = p;
}

__global__ __launch_bounds__(B) void sfm_corr_gather_kernel(const int *__restrict__ sel, const int *__restrict__ n_sel, int off, int n_view,
                                                            const int *__restrict__ point, const double *__restrict__ X, long long n_points,
                                                            const float2 *__restrict__ kp, int *__restrict__ pid_out,
                                                            float *__restrict__ X_out, float2 *__restrict__ x_out)
{
    const int i = (int)(blockIdx.x * B + threadIdx.x);
    if (i >= *n_sel) return;
    const int k = sel[i];
    const int p = point[AMVS_IDX(k, n_view)];
    const long long pp = AMVS_IDX((long long)p, n_points);
    pid_out[i] = p;
    X_out[3 * i] = (float)X[3 * pp];
    X_out[3 * i + 1] = (float)X[3 * pp + 1];
    X_out[3 * i + 2] = (float)X[3 * pp + 2];
    x_out[i] = kp[off + k];
}

// ---- triangulation --------------------------------------------------------------------------------------------------
// rows row0 .. row0 + count - 1 of one pair: flag[i] and cand[i] for the rows with both keypoints un-owned
__global__ __launch_bounds__(B) void sfm_tri_kernel(const TriArgs a, const int2 *__restrict__ rows, long long M, int row0, int count,
                                                    const int *__restrict__ owner, long long G, const float2 *__restrict__ kp,
                                                    int *__restrict__ flag, double *__restrict__ cand)
{
    const int i = (int)(blockIdx.x * B + threadIdx.x);
    if (i >= count) return;
    const int2 row = rows[AMVS_IDX((long long)row0 + i, M)];
    const long long g1 = AMVS_IDX((long long)row.x, G), g2 = AMVS_IDX((long long)row.y, G);
    bool ok = false;
    if (owner[g1] < 0 && owner[g2] < 0) {
        const float2 p1 = kp[g1], p2 = kp[g2];
        double X[3], cs;
        ok = tri_candidate(a, (double)p1.x, (double)p1.y, (double)p2.x, (double)p2.y, X, &cs);
        cand[3 * (size_t)i] = X[0];
        cand[3 * (size_t)i + 1] = X[1];
        cand[3 * (size_t)i + 2] = X[2];
    }
    flag[i] = ok ? 1 : 0;
}

// one lane: the number of new points of step `step` and the id base of the next step
__global__ void sfm_tri_base_kernel(const int *__restrict__ flag, const int *__restrict__ scan, int count, int step, int *__restrict__ made,
                                    long long *__restrict__ base)
{
    const int n = scan[count - 1] + flag[count - 1];
    made[step] = n;
    base[step + 1] = base[step] + n;
}

__global__ __launch_bounds__(B) void sfm_tri_assign_kernel(const int2 *__restrict__ rows, long long M, int row0, int count,
                                                           const int *__restrict__ flag, const int *__restrict__ scan,
                                                           const double *__restrict__ cand, const long long *__restrict__ base, int step,
                                                           int *__restrict__ owner, long long G, double *__restrict__ X,
                                                           unsigned char *__restrict__ alive, long long capacity)
{
    const int i = (int)(blockIdx.x * B + threadIdx.x);
    if (i >= count || !flag[i]) return;
    const long long id = AMVS_IDX(base[step] + scan[i], capacity);
    const int2 row = rows[AMVS_IDX((long long)row0 + i, M)];
    X[3 * id] = cand[3 * (size_t)i];
    X[3 * id + 1] = cand[3 * (size_t)i + 1];
    X[3 * id + 2] = cand[3 * (size_t)i + 2];
    alive[id] = 1;
    owner[AMVS_IDX(row.x, G)] = (int)id;
    owner[AMVS_IDX(row.y, G)] = (int)id;
}

// ---- counts, observations, drop -------------------------------------------------------------------------------------
__global__ __launch_bounds__(B) void sfm_count_owned_kernel(const int *__restrict__ owner, long long G, unsigned long long *__restrict__ out)
{
    const long long g = (long long)blockIdx.x * B + threadIdx.x;
    const int c = wave_count(g < G && owner[g] >= 0);
    if (c != 0 && (threadIdx.x & 63) == 0) atomicAdd(out, (unsigned long long)c);
}

__global__ __launch_bounds__(B) void sfm_count_alive_kernel(const unsigned char *__restrict__ alive, long long n, unsigned long long *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * B + threadIdx.x;
    const int c = wave_count(i < n && alive[i] != 0);
    if (c != 0 && (threadIdx.x & 63) == 0) atomicAdd(out, (unsigned long long)c);
}

__global__ __launch_bounds__(B) void sfm_owned_flag_kernel(const int *__restrict__ owner, long long G, unsigned char *__restrict__ flag)
{
    const long long g = (long long)blockIdx.x * B + threadIdx.x;
    if (g < G) flag[g] = owner[g] >= 0 ? 1 : 0;
}

__global__ __launch_bounds__(B) void sfm_obs_key_kernel(const int *__restrict__ sel, long long n, const int *__restrict__ owner, long long G,
                                                        unsigned long long *__restrict__ key)
{
    const long long i = (long long)blockIdx.x * B + threadIdx.x;
    if (i >= n) return;
    const int g = sel[i];
    key[i] = ((unsigned long long)(unsigned)owner[AMVS_IDX(g, G)] << 32) | (unsigned)g;
}

__global__ __launch_bounds__(B) void sfm_obs_decode_kernel(const unsigned long long *__restrict__ key, long long n, const int *__restrict__ kview,
                                                           const float2 *__restrict__ kp, long long G, int *__restrict__ cam,
                                                           int *__restrict__ pt, float2 *__restrict__ uv)
{
    const long long i = (long long)blockIdx.x * B + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = key[i];
    const long long g = AMVS_IDX((long long)(k & 0xFFFFFFFFull), G);
    cam[i] = kview[g];
    pt[i] = (int)(k >> 32);
    uv[i] = kp[g];
}

// step 1 of amvs_sfm_drop: a keypoint whose (owner, view) is among the sorted keys becomes un-owned
__global__ __launch_bounds__(B) void sfm_drop_obs_kernel(const long long *__restrict__ keys, int n, const int *__restrict__ kview,
                                                         int *__restrict__ owner, long long G, unsigned long long *__restrict__ dropped)
{
    const long long g = (long long)blockIdx.x * B + threadIdx.x;
    bool hit = false;
    if (g < G) {
        const int p = owner[g];
        if (p >= 0) {
            const long long want = ((long long)p << 12) | kview[g];
            int lo = 0, hi = n;                                          // first key >= want
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (keys[AMVS_IDX(mid, n)] < want) lo = mid + 1; else hi = mid;
            }
            hit = lo < n && keys[AMVS_IDX(lo, n)] == want;
            if (hit) owner[g] = -1;
        }
    }
    const int c = wave_count(hit);
    if (c != 0 && (threadIdx.x & 63) == 0) atomicAdd(dropped, (unsigned long long)c);
}

__global__ __launch_bounds__(B) void sfm_obs_per_point_kernel(const int *__restrict__ owner, long long G, int *__restrict__ n_obs,
                                                              long long n_points)
{
    const long long g = (long long)blockIdx.x * B + threadIdx.x;
    if (g >= G) return;
    const int p = owner[g];
    if (p >= 0) atomicAdd(&n_obs[AMVS_IDX(p, n_points)], 1);
}

// step 2: a live point with fewer than min_obs observations dies
__global__ __launch_bounds__(B) void sfm_drop_points_kernel(const int *__restrict__ n_obs, long long n_points, int min_obs,
                                                            unsigned char *__restrict__ alive, unsigned long long *__restrict__ died)
{
    const long long p = (long long)blockIdx.x * B + threadIdx.x;
    const bool dies = p < n_points && alive[p] != 0 && n_obs[p] < min_obs;
    if (dies) alive[p] = 0;
    const int c = wave_count(dies);
    if (c != 0 && (threadIdx.x & 63) == 0) atomicAdd(died, (unsigned long long)c);
}

// invariant (I2): a keypoint whose owner is dead becomes un-owned
__global__ __launch_bounds__(B) void sfm_unown_dead_kernel(int *__restrict__ owner, long long G, const unsigned char *__restrict__ alive,
                                                           long long n_points)
{
    const long long g = (long long)blockIdx.x * B + threadIdx.x;
    if (g >= G) return;
    const int p = owner[g];
    if (p >= 0 && alive[AMVS_IDX(p, n_points)] == 0) owner[g] = -1;
}

__global__ __launch_bounds__(B) void sfm_register_kernel(const int *__restrict__ kp_in, const int *__restrict__ pid_in, int n, int off, int n_view,
                                                         const unsigned char *__restrict__ alive, long long n_points, int *__restrict__ owner,
                                                         unsigned long long *__restrict__ n_set)
{
    const int i = (int)(blockIdx.x * B + threadIdx.x);
    bool set = false;
    if (i < n) {
        const int p = pid_in[i];
        set = alive[AMVS_IDX(p, n_points)] != 0;
        if (set) owner[off + AMVS_IDX(kp_in[i], n_view)] = p;
    }
    const int c = wave_count(set);
    if (c != 0 && (threadIdx.x & 63) == 0) atomicAdd(n_set, (unsigned long long)c);
}

// the indices 0 .. n - 1 with flag set, ascending, into sel; their number into d_count (an int on the device)
hipError_t select_flagged(const unsigned char *flag, long long n, int *sel, int *d_count, ScratchCache &cache, Lease &tmp, hipStream_t st)
{
    hipcub::CountingInputIterator<int> iota(0);
    size_t bytes = 0;
    STCHK(hipcub::DeviceSelect::Flagged(nullptr, bytes, iota, flag, sel, d_count, (int)n, st));
    STCHK(cache.lease(tmp, bytes));
    return hipcub::DeviceSelect::Flagged(tmp.get(), bytes, iota, flag, sel, d_count, (int)n, st);
}

hipError_t upload_segs(const std::vector<SfmSeg> &segs, Lease &l, ScratchCache &cache, hipStream_t st)
{
    STCHK(cache.lease(l, sizeof(SfmSeg) * segs.size()));
    return hipMemcpyAsync(l.get(), segs.data(), sizeof(SfmSeg) * segs.size(), hipMemcpyHostToDevice, st);
}

// X and alive with room for `need` points, the first n_points kept.  The old blocks are released only after the stream
// has drained: queued work may still read them.
hipError_t grow_points(SfmState &s, long long need, ScratchCache &cache, hipStream_t st)
{
    if ((long long)s.alive.capacity() >= need && (long long)s.X.capacity() >= 3 * need) return hipSuccess;
    long long cap = std::max<long long>(need, 2 * (long long)s.alive.capacity());
    cap = std::min<long long>(std::max<long long>(cap, 1024), std::max<long long>(need, AMVS_SFM_MAX_POINTS));
    DeviceBuffer<double> X;
    DeviceBuffer<unsigned char> alive;
    STCHK(X.reserve(3 * (size_t)cap, cache));
    STCHK(alive.reserve((size_t)cap, cache));
    if (s.n_points > 0) {
        STCHK(hipMemcpyAsync(X.get(), s.X.get(), sizeof(double) * 3 * (size_t)s.n_points, hipMemcpyDeviceToDevice, st));
        STCHK(hipMemcpyAsync(alive.get(), s.alive.get(), (size_t)s.n_points, hipMemcpyDeviceToDevice, st));
    }
    STCHK(hipStreamSynchronize(st));
    s.X = std::move(X);
    s.alive = std::move(alive);
    return hipSuccess;
}

}  // namespace

hipError_t sfm_upload(SfmState &s, const float *kp_h, const int *rows_h, ScratchCache &cache, hipStream_t st)
{
    // nothing of an earlier state is in use: every entry point synchronises before it returns
    std::vector<int> kview((size_t)s.G);
    for (int v = 0; v < s.V; ++v)
        for (int g = s.off[v]; g < s.off[v + 1]; ++g) kview[(size_t)g] = v;
    std::vector<int2> rows((size_t)s.M);
    for (int p = 0; p < s.P; ++p) {
        const int oi = s.off[s.pair_views[2 * p]], oj = s.off[s.pair_views[2 * p + 1]];
        for (int m = s.pair_start[p]; m < s.pair_start[p + 1]; ++m)
            rows[(size_t)m] = make_int2(oi + rows_h[2 * (size_t)m], oj + rows_h[2 * (size_t)m + 1]);
    }
    STCHK(s.kp.reserve(std::max<size_t>((size_t)s.G, 1), cache));
    STCHK(s.kview.reserve(std::max<size_t>((size_t)s.G, 1), cache));
    STCHK(s.owner.reserve(std::max<size_t>((size_t)s.G, 1), cache));
    STCHK(s.rows.reserve(std::max<size_t>((size_t)s.M, 1), cache));
    if (s.G > 0) {
        STCHK(hipMemcpyAsync(s.kp.get(), kp_h, sizeof(float2) * (size_t)s.G, hipMemcpyHostToDevice, st));
        STCHK(hipMemcpyAsync(s.kview.get(), kview.data(), sizeof(int) * (size_t)s.G, hipMemcpyHostToDevice, st));
        STCHK(hipMemsetAsync(s.owner.get(), 0xFF, sizeof(int) * (size_t)s.G, st));
    }
    if (s.M > 0) STCHK(hipMemcpyAsync(s.rows.get(), rows.data(), sizeof(int2) * (size_t)s.M, hipMemcpyHostToDevice, st));
    s.n_points = 0;
    return hipStreamSynchronize(st);
}

hipError_t sfm_register(SfmState &s, int view, const int *kp_h, const int *pid_h, int n, long long *n_set, ScratchCache &cache,
                        hipStream_t st)
{
    *n_set = 0;
    if (n <= 0) return hipSuccess;
    Lease in, cnt;
    STCHK(cache.lease(in, sizeof(int) * 2 * (size_t)n));
    STCHK(cache.lease(cnt, sizeof(unsigned long long)));
    int *d = in.get<int>();
    STCHK(hipMemcpyAsync(d, kp_h, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
    STCHK(hipMemcpyAsync(d + n, pid_h, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
    STCHK(hipMemsetAsync(cnt.get(), 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(sfm_register_kernel, grid_for(n), dim3(B), 0, st, (const int *)d, (const int *)(d + n), n, s.off[view],
                       s.off[view + 1] - s.off[view], (const unsigned char *)s.alive.get(), s.n_points, s.owner.get(),
                       cnt.get<unsigned long long>());
    STCHK(hipGetLastError());
    unsigned long long k = 0;
    STCHK(hipMemcpyAsync(&k, cnt.get(), sizeof(k), hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
    *n_set = (long long)k;
    return hipSuccess;
}

hipError_t sfm_scores(SfmState &s, const std::vector<SfmSeg> &segs, int total, int *counts_h, ScratchCache &cache, hipStream_t st)
{
    for (int v = 0; v < s.V; ++v) counts_h[v] = 0;
    if (total <= 0 || s.G <= 0) return hipSuccess;
    Lease seg, flag, counts;
    STCHK(upload_segs(segs, seg, cache, st));
    STCHK(cache.lease(flag, (size_t)s.G));
    STCHK(cache.lease(counts, sizeof(int) * (size_t)s.V));
    STCHK(hipMemsetAsync(flag.get(), 0, (size_t)s.G, st));
    STCHK(hipMemsetAsync(counts.get(), 0, sizeof(int) * (size_t)s.V, st));
    hipLaunchKernelGGL(sfm_score_rows_kernel, grid_for(total), dim3(B), 0, st, (const SfmSeg *)seg.get(), (int)segs.size(), total,
                       (const int2 *)s.rows.get(), s.M, (const int *)s.owner.get(), s.G, flag.get<unsigned char>());
    STCHK(hipGetLastError());
    hipLaunchKernelGGL(sfm_score_count_kernel, grid_for(s.G), dim3(B), 0, st, (const unsigned char *)flag.get(), (const int *)s.kview.get(),
                       s.G, s.V, counts.get<int>());
    STCHK(hipGetLastError());
    STCHK(hipMemcpyAsync(counts_h, counts.get(), sizeof(int) * (size_t)s.V, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t sfm_correspondences(SfmState &s, int view, const std::vector<SfmSeg> &segs, int total, int *kp_h, int *pid_h, float *X_h,
                               float *x_h, long long *m, ScratchCache &cache, hipStream_t st)
{
    *m = 0;
    const int off = s.off[view], n_view = s.off[view + 1] - off;
    if (total <= 0 || n_view <= 0 || s.n_points <= 0) return hipSuccess;
    Lease seg, best, pbest, keep, point, sel, cnt, tmp, out;
    STCHK(upload_segs(segs, seg, cache, st));
    STCHK(cache.lease(best, sizeof(int) * (size_t)n_view));
    STCHK(cache.lease(pbest, sizeof(int) * (size_t)s.n_points));
    STCHK(cache.lease(keep, (size_t)n_view));
    STCHK(cache.lease(point, sizeof(int) * (size_t)n_view));
    STCHK(cache.lease(sel, sizeof(int) * (size_t)n_view));
    STCHK(cache.lease(cnt, sizeof(int)));
    STCHK(cache.lease(out, (sizeof(int) + 5 * sizeof(float)) * (size_t)n_view));
    hipLaunchKernelGGL(sfm_fill_kernel, grid_for(n_view), dim3(B), 0, st, best.get<int>(), (long long)n_view, INT_MAX);
    hipLaunchKernelGGL(sfm_fill_kernel, grid_for(s.n_points), dim3(B), 0, st, pbest.get<int>(), s.n_points, INT_MAX);
    STCHK(hipGetLastError());
    const int2 *rows = s.rows.get();
    const int *owner = s.owner.get();
    hipLaunchKernelGGL(sfm_corr_a_kernel, grid_for(total), dim3(B), 0, st, (const SfmSeg *)seg.get(), (int)segs.size(), total, rows, s.M,
                       owner, s.G, off, n_view, best.get<int>());
    hipLaunchKernelGGL(sfm_corr_b_kernel, grid_for(n_view), dim3(B), 0, st, (const int *)best.get(), off, n_view, rows, s.M, owner, s.G,
                       pbest.get<int>(), s.n_points);
    hipLaunchKernelGGL(sfm_corr_c_kernel, grid_for(n_view), dim3(B), 0, st, (const int *)best.get(), off, n_view, rows, s.M, owner, s.G,
                       (const int *)pbest.get(), s.n_points, keep.get<unsigned char>(), point.get<int>());
    STCHK(hipGetLastError());
    STCHK(select_flagged(keep.get<unsigned char>(), n_view, sel.get<int>(), cnt.get<int>(), cache, tmp, st));
    int *d_pid = out.get<int>();
    float *d_X = reinterpret_cast<float *>(d_pid + n_view);
    float2 *d_x = reinterpret_cast<float2 *>(d_X + 3 * (size_t)n_view);
    hipLaunchKernelGGL(sfm_corr_gather_kernel, grid_for(n_view), dim3(B), 0, st, (const int *)sel.get(), (const int *)cnt.get(), off, n_view,
                       (const int *)point.get(), (const double *)s.X.get(), s.n_points, (const float2 *)s.kp.get(), d_pid, d_X, d_x);
    STCHK(hipGetLastError());
    int k = 0;
    STCHK(hipMemcpyAsync(&k, cnt.get(), sizeof(int), hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
    if (k > 0) {
        STCHK(hipMemcpyAsync(kp_h, sel.get(), sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, st));
        STCHK(hipMemcpyAsync(pid_h, d_pid, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, st));
        STCHK(hipMemcpyAsync(X_h, d_X, sizeof(float) * 3 * (size_t)k, hipMemcpyDeviceToHost, st));
        STCHK(hipMemcpyAsync(x_h, d_x, sizeof(float2) * (size_t)k, hipMemcpyDeviceToHost, st));
        STCHK(hipStreamSynchronize(st));
    }
    *m = k;
    return hipSuccess;
}

hipError_t sfm_triangulate(SfmState &s, const double *K, const std::vector<SfmTriPair> &pairs, long long max_new, double depth_min,
                           double cos_max_parallax, double max_reproj, int *new_h, long long *n_new, ScratchCache &cache, hipStream_t st)
{
    *n_new = 0;
    for (int v = 0; v < s.V; ++v) new_h[v] = 0;
    int steps = 0, longest = 0;
    long long room = 0;
    for (const SfmTriPair &p : pairs)
        if (p.count > 0) { ++steps; longest = std::max(longest, p.count); room += p.count; }
    if (steps == 0) return hipSuccess;
    STCHK(grow_points(s, s.n_points + std::min(room, max_new), cache, st));     // the caller has checked n_points + max_new against the limit
    const long long capacity = (long long)s.alive.capacity();
    Lease flag, scan, cand, made, base, tmp;
    STCHK(cache.lease(flag, sizeof(int) * (size_t)longest));
    STCHK(cache.lease(scan, sizeof(int) * (size_t)longest));
    STCHK(cache.lease(cand, sizeof(double) * 3 * (size_t)longest));
    STCHK(cache.lease(made, sizeof(int) * (size_t)steps));
    STCHK(cache.lease(base, sizeof(long long) * (size_t)(steps + 1)));
    size_t bytes = 0;
    STCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, flag.get<int>(), scan.get<int>(), longest, st));
    STCHK(cache.lease(tmp, bytes));
    STCHK(hipMemcpyAsync(base.get(), &s.n_points, sizeof(long long), hipMemcpyHostToDevice, st));
    int step = 0;
    for (const SfmTriPair &p : pairs) {
        if (p.count <= 0) continue;
        const TwoviewThresholds thr{depth_min, p.depth_max, cos_max_parallax, max_reproj};
        const TriArgs a = tri_args(K, p.R1, p.t1, p.R2, p.t2, thr);
        hipLaunchKernelGGL(sfm_tri_kernel, grid_for(p.count), dim3(B), 0, st, a, (const int2 *)s.rows.get(), s.M, p.row0, p.count,
                           (const int *)s.owner.get(), s.G, (const float2 *)s.kp.get(), flag.get<int>(), cand.get<double>());
        STCHK(hipGetLastError());
        STCHK(hipcub::DeviceScan::ExclusiveSum(tmp.get(), bytes, flag.get<int>(), scan.get<int>(), p.count, st));   // sized for the longest
        hipLaunchKernelGGL(sfm_tri_base_kernel, dim3(1), dim3(1), 0, st, (const int *)flag.get(), (const int *)scan.get(), p.count, step,
                           made.get<int>(), base.get<long long>());
        hipLaunchKernelGGL(sfm_tri_assign_kernel, grid_for(p.count), dim3(B), 0, st, (const int2 *)s.rows.get(), s.M, p.row0, p.count,
                           (const int *)flag.get(), (const int *)scan.get(), (const double *)cand.get(), (const long long *)base.get(), step,
                           s.owner.get(), s.G, s.X.get(), s.alive.get(), capacity);
        STCHK(hipGetLastError());
        ++step;
    }
    std::vector<int> made_h((size_t)steps);
    STCHK(hipMemcpyAsync(made_h.data(), made.get(), sizeof(int) * (size_t)steps, hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
    step = 0;
    for (const SfmTriPair &p : pairs) {
        if (p.count <= 0) continue;
        new_h[p.r] = made_h[(size_t)step++];
        *n_new += new_h[p.r];
    }
    s.n_points += *n_new;
    return hipSuccess;
}

hipError_t sfm_counts(SfmState &s, long long *n_alive, long long *n_obs, ScratchCache &cache, hipStream_t st)
{
    *n_alive = *n_obs = 0;
    Lease cnt;
    STCHK(cache.lease(cnt, 2 * sizeof(unsigned long long)));
    unsigned long long *d = cnt.get<unsigned long long>();
    STCHK(hipMemsetAsync(d, 0, 2 * sizeof(unsigned long long), st));
    if (s.n_points > 0) hipLaunchKernelGGL(sfm_count_alive_kernel, grid_for(s.n_points), dim3(B), 0, st, (const unsigned char *)s.alive.get(), s.n_points, d);
    if (s.G > 0) hipLaunchKernelGGL(sfm_count_owned_kernel, grid_for(s.G), dim3(B), 0, st, (const int *)s.owner.get(), s.G, d + 1);
    STCHK(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    STCHK(hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
    *n_alive = (long long)h[0];
    *n_obs = (long long)h[1];
    return hipSuccess;
}

hipError_t sfm_observations(SfmState &s, int *cam_h, int *pt_h, float *uv_h, long long n_obs, ScratchCache &cache, hipStream_t st)
{
    if (n_obs <= 0) return hipSuccess;
    Lease flag, sel, cnt, tmp, keyA, keyB, out;
    STCHK(cache.lease(flag, (size_t)s.G));
    STCHK(cache.lease(sel, sizeof(int) * (size_t)s.G));
    STCHK(cache.lease(cnt, sizeof(int)));
    STCHK(cache.lease(keyA, sizeof(unsigned long long) * (size_t)n_obs));
    STCHK(cache.lease(keyB, sizeof(unsigned long long) * (size_t)n_obs));
    STCHK(cache.lease(out, (2 * sizeof(int) + sizeof(float2)) * (size_t)n_obs));
    hipLaunchKernelGGL(sfm_owned_flag_kernel, grid_for(s.G), dim3(B), 0, st, (const int *)s.owner.get(), s.G, flag.get<unsigned char>());
    STCHK(hipGetLastError());
    STCHK(select_flagged(flag.get<unsigned char>(), s.G, sel.get<int>(), cnt.get<int>(), cache, tmp, st));   // n_obs of them: nothing changed the owners since the count
    hipLaunchKernelGGL(sfm_obs_key_kernel, grid_for(n_obs), dim3(B), 0, st, (const int *)sel.get(), n_obs, (const int *)s.owner.get(), s.G,
                       keyA.get<unsigned long long>());
    STCHK(hipGetLastError());
    {
        Lease tmp2;
        size_t bytes = 0;
        STCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, keyA.get<unsigned long long>(), keyB.get<unsigned long long>(), (int)n_obs, 0, 64, st));
        STCHK(cache.lease(tmp2, bytes));
        STCHK(hipcub::DeviceRadixSort::SortKeys(tmp2.get(), bytes, keyA.get<unsigned long long>(), keyB.get<unsigned long long>(), (int)n_obs, 0, 64, st));
        int *d_cam = out.get<int>(), *d_pt = d_cam + n_obs;
        float2 *d_uv = reinterpret_cast<float2 *>(d_pt + n_obs);
        hipLaunchKernelGGL(sfm_obs_decode_kernel, grid_for(n_obs), dim3(B), 0, st, (const unsigned long long *)keyB.get(), n_obs,
                           (const int *)s.kview.get(), (const float2 *)s.kp.get(), s.G, d_cam, d_pt, d_uv);
        STCHK(hipGetLastError());
        STCHK(hipMemcpyAsync(cam_h, d_cam, sizeof(int) * (size_t)n_obs, hipMemcpyDeviceToHost, st));
        STCHK(hipMemcpyAsync(pt_h, d_pt, sizeof(int) * (size_t)n_obs, hipMemcpyDeviceToHost, st));
        STCHK(hipMemcpyAsync(uv_h, d_uv, sizeof(float2) * (size_t)n_obs, hipMemcpyDeviceToHost, st));
        STCHK(hipStreamSynchronize(st));              // before tmp2 goes back to the cache
    }
    return hipSuccess;
}

hipError_t sfm_points_get(SfmState &s, double *X_h, unsigned char *alive_h, hipStream_t st)
{
    if (s.n_points <= 0) return hipSuccess;
    if (X_h) STCHK(hipMemcpyAsync(X_h, s.X.get(), sizeof(double) * 3 * (size_t)s.n_points, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(alive_h, s.alive.get(), (size_t)s.n_points, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t sfm_points_set(SfmState &s, const double *X_h, const unsigned char *alive_h, ScratchCache &cache, hipStream_t st)
{
    (void)cache;
    if (s.n_points <= 0) return hipSuccess;
    STCHK(hipMemcpyAsync(s.X.get(), X_h, sizeof(double) * 3 * (size_t)s.n_points, hipMemcpyHostToDevice, st));
    STCHK(hipMemcpyAsync(s.alive.get(), alive_h, (size_t)s.n_points, hipMemcpyHostToDevice, st));
    if (s.G > 0) {
        hipLaunchKernelGGL(sfm_unown_dead_kernel, grid_for(s.G), dim3(B), 0, st, s.owner.get(), s.G, (const unsigned char *)s.alive.get(),
                           s.n_points);
        STCHK(hipGetLastError());
    }
    return hipStreamSynchronize(st);
}

hipError_t sfm_drop(SfmState &s, const long long *keys_h, int n, int min_obs, long long *obs_dropped, long long *points_dropped,
                    ScratchCache &cache, hipStream_t st)
{
    *obs_dropped = *points_dropped = 0;
    if (s.G <= 0 || s.n_points <= 0) return hipSuccess;
    Lease keys, cnt, per;
    STCHK(cache.lease(keys, sizeof(long long) * (size_t)std::max(n, 1)));
    STCHK(cache.lease(cnt, 2 * sizeof(unsigned long long)));
    STCHK(cache.lease(per, sizeof(int) * (size_t)s.n_points));
    unsigned long long *d = cnt.get<unsigned long long>();
    STCHK(hipMemsetAsync(d, 0, 2 * sizeof(unsigned long long), st));
    STCHK(hipMemsetAsync(per.get(), 0, sizeof(int) * (size_t)s.n_points, st));
    if (n > 0) {
        STCHK(hipMemcpyAsync(keys.get(), keys_h, sizeof(long long) * (size_t)n, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(sfm_drop_obs_kernel, grid_for(s.G), dim3(B), 0, st, (const long long *)keys.get(), n, (const int *)s.kview.get(),
                           s.owner.get(), s.G, d);
    }
    hipLaunchKernelGGL(sfm_obs_per_point_kernel, grid_for(s.G), dim3(B), 0, st, (const int *)s.owner.get(), s.G, per.get<int>(), s.n_points);
    hipLaunchKernelGGL(sfm_drop_points_kernel, grid_for(s.n_points), dim3(B), 0, st, (const int *)per.get(), s.n_points, min_obs,
                       s.alive.get(), d + 1);
    hipLaunchKernelGGL(sfm_unown_dead_kernel, grid_for(s.G), dim3(B), 0, st, s.owner.get(), s.G, (const unsigned char *)s.alive.get(),
                       s.n_points);
    STCHK(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    STCHK(hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
    *obs_dropped = (long long)h[0];
    *points_dropped = (long long)h[1];
    return hipSuccess;
}

}  // namespace amvs

AMVS_CHECK_TU(sfm)
