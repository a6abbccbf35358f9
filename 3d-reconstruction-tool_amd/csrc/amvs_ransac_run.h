// amvs_ransac_run.h -- the RANSAC the pose estimators share (amvs_fmat.hip, amvs_pnp.hip): the kernel that adds block
// partials in ascending order and the one that finds the best count of a batch, the scratch of the refit and inlier
// passes with the second half of each, and ransac_run, the one statement of the policy of include/amvs_epipolar.h and
// include/amvs_resection.h.  Private to the library.  The kernels are static and the rest is in an unnamed namespace:
// a unit that includes this compiles its own two kernels, so only a unit that launches them does.
#pragma once
#include "amvs_buffer.h"
#include "amvs_ransac_common.h"

#include <cmath>
#include <cstring>

namespace amvs {

// out[0] = count, out[1] = hypothesis of the best of counts[0 .. n): count descending, index ascending.  One workgroup.
static __global__ __launch_bounds__(1024) void ransac_argmax_kernel(const int *__restrict__ counts, int n, int first, int *__restrict__ out)
{
    __shared__ unsigned long long sh[1024];
    unsigned long long best = 0ull;
    for (int j = (int)threadIdx.x; j < n; j += 1024) {
        const unsigned long long key = ((unsigned long long)(unsigned)counts[j] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)j);
        if (key > best) best = key;
    }
    sh[threadIdx.x] = best;
    __syncthreads();
    for (int step = 512; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step && sh[threadIdx.x + step] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (int)(sh[0] >> 32);
        out[1] = first + (int)(0xFFFFFFFFu - (unsigned)(sh[0] & 0xFFFFFFFFull));
    }
}

// total[e] = the partials of entry e added in ascending block order, from +0.0
static __global__ __launch_bounds__(64) void ransac_total_kernel(const double *__restrict__ part, int n_blocks, int entries, double *__restrict__ total)
{
    const int e = (int)threadIdx.x;
    if (e >= entries) return;
    double acc = 0.0;
    for (int b = 0; b < n_blocks; ++b) acc = acc + part[(size_t)b * entries + e];
    total[e] = acc;
}

namespace {

// scratch of the refit passes and inlier passes of one call: the block partials of `entries` sums, their totals, a counter
struct Work {
    ScratchCache::Lease part, total, count;
    hipError_t reserve(size_t entries, size_t n_blocks, ScratchCache &cache)
    {
        hipError_t e = cache.lease(part, sizeof(double) * entries * n_blocks);
        if (e == hipSuccess) e = cache.lease(total, sizeof(double) * 64);
        if (e == hipSuccess) e = cache.lease(count, sizeof(int) * 2);
        return e;
    }
};

// the second half of a pass, after the unit's partials kernel has filled w.part: out[entries] = the totals
inline hipError_t pass_totals(Work &w, int n_blocks, int entries, double *out, hipStream_t st)
{
    hipLaunchKernelGGL(ransac_total_kernel, dim3(1), dim3(64), 0, st, (const double *)w.part.get(), n_blocks, entries, w.total.get<double>());
    STCHK(hipGetLastError());
    STCHK(hipMemcpyAsync(out, w.total.get(), sizeof(double) * entries, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

// *count = what launch(counter), a unit's inlier kernel on `st`, adds to the zeroed counter
template <class Launch>
hipError_t count_inliers(Work &w, long long *count, hipStream_t st, Launch launch)
{
    STCHK(hipMemsetAsync(w.count.get(), 0, sizeof(int), st));
    launch(w.count.get<int>());
    STCHK(hipGetLastError());
    int c = 0;
    STCHK(hipMemcpyAsync(&c, w.count.get(), sizeof(int), hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
    *count = c;
    return hipSuccess;
}

// RANSAC over the m correspondences of a model M, which supplies what differs between the estimators:
//     M::SAMPLE, M::BATCH                 the correspondences of a sample, the hypotheses of a batch
//     M::Estimate                         one estimate, value-initialised to the all-zero "no model"
//     M.prepare(cache, st)                the points uploaded, the scratch and the buffers of a batch leased
//     M.hypotheses(first, count, st)      launch: hypotheses first .. first + count into the batch buffers
//     M.score(n, counts_d, st)            launch: counts_d[j] += the inliers of hypothesis j of the batch buffers
//     M.fetch(e, st)                      the async copies of hypothesis 0 of the batch buffers into e
//     M.inliers(e, mask_d, &n, st)        mask_d and the count of the inliers of e; synchronises
//     M.refit(e, mask_d, n, st)           e refitted to the n members of mask_d, in place; synchronises
//     M::all_inliers(w)                   the probability that a sample is all inliers at the inlier ratio w, in the
//                                         order of operations its header fixes
// Batches of hypotheses are scored until the header's adaptive bound or max_hypotheses is reached; the best count wins,
// the earliest hypothesis among equals; the answer is the better of two refits, the second on a tie.  info = [the
// hypotheses tried, the best one, its count].  *out, mask_h and *n_inliers are zero when there is no model.
template <class M>
hipError_t ransac_run(M &model, int m, double confidence, int max_hypotheses, typename M::Estimate *out, unsigned char *mask_h,
                      long long *n_inliers, int info[3], ScratchCache &cache, hipStream_t st)
{
    ScratchCache::Lease counts, best2, mask_a, mask_b;
    STCHK(model.prepare(cache, st));
    STCHK(cache.lease(counts, sizeof(int) * M::BATCH));
    STCHK(cache.lease(best2, sizeof(int) * 2));
    STCHK(cache.lease(mask_a, (size_t)m));
    STCHK(cache.lease(mask_b, (size_t)m));

    int done = 0, best = -1, best_h = 0;
    for (;;) {
        const int nb = max_hypotheses - done < M::BATCH ? max_hypotheses - done : M::BATCH;
        model.hypotheses(done, nb, st);
        STCHK(hipGetLastError());
        STCHK(hipMemsetAsync(counts.get(), 0, sizeof(int) * (size_t)nb, st));
        model.score(nb, counts.get<int>(), st);
        STCHK(hipGetLastError());
        hipLaunchKernelGGL(ransac_argmax_kernel, dim3(1), dim3(1024), 0, st, (const int *)counts.get(), nb, done, best2.get<int>());
        STCHK(hipGetLastError());
        int got[2] = {0, 0};
        STCHK(hipMemcpyAsync(got, best2.get(), sizeof(got), hipMemcpyDeviceToHost, st));
        STCHK(hipStreamSynchronize(st));
        if (got[0] > best) { best = got[0]; best_h = got[1]; }     // (a later batch wins only with a larger count)
        done += nb;
        const double p = M::all_inliers((double)best / (double)m);
        double N;
        if (p >= 1.0) N = 0.0;
        else if (1.0 - p == 1.0) N = (double)max_hypotheses;
        else N = std::ceil(std::log(1.0 - confidence) / std::log(1.0 - p));
        if ((double)done >= N || done == max_hypotheses) break;
    }
    info[0] = done; info[1] = best_h; info[2] = best;

    *out = typename M::Estimate{};
    std::memset(mask_h, 0, (size_t)m);
    *n_inliers = 0;
    if (best < M::SAMPLE) return hipSuccess;

    // the best hypothesis again (the sampler is a function of h), its inliers, and the two refits
    typename M::Estimate e1, e2;
    model.hypotheses(best_h, 1, st);
    STCHK(hipGetLastError());
    STCHK(model.fetch(e1, st));
    STCHK(hipStreamSynchronize(st));
    long long n0 = 0, n1 = 0, n2 = 0;
    unsigned char *ma = mask_a.get<unsigned char>(), *mb = mask_b.get<unsigned char>();
    STCHK(model.inliers(e1, ma, &n0, st));
    if (n0 < M::SAMPLE) return hipSuccess;              // (n0 == best >= SAMPLE: unreachable, kept as the refit's precondition)
    STCHK(model.refit(e1, ma, n0, st));
    STCHK(model.inliers(e1, mb, &n1, st));
    if (n1 < M::SAMPLE) return hipSuccess;
    e2 = e1;
    STCHK(model.refit(e2, mb, n1, st));
    STCHK(model.inliers(e2, ma, &n2, st));
    const bool second = n2 >= n1;
    *out = second ? e2 : e1;
    *n_inliers = second ? n2 : n1;
    STCHK(hipMemcpyAsync(mask_h, second ? ma : mb, (size_t)m, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

}  // namespace

}  // namespace amvs
