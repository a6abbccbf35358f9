// amvs_mesh_fill.hip -- hole filling in the TSDF volume before the extraction: the signed distance and the mean colour
// grow from the observed grid points into the unobserved ones next to them, one layer of 6-neighbours per step
// (include/amvs.h amvs_tsdf_fill, amvs_tsdf_fetch_fill; the definition is the header's).  No reference counterpart.
// Judged against tests/mesh_fill_restatement.py, a NumPy statement of the header's definition with the same float32
// operations in the same order (bit-identical volume, generations, counts and extracted mesh).
//
// The generations: gen[p] = 1 for a point observed before the call, s + 1 for a point step s filled, 0 for a point still
// unobserved.  A point is known at step s if 1 <= gen <= s.
//
// fill_step_kernel, one lane per grid point, x fastest, one launch per step.  Nearly every lane is done after its own
// byte (gen != 0: observed or filled earlier).  A lane with gen == 0 reads the bytes of its in-grid neighbours and, of
// the known ones only, tsdf, weight and the three colour sums.
//
// The step runs IN PLACE, without a second copy of the volume, and still equals the header's simultaneous definition
// ("all points of a step are decided from the state before the step"): a point written during step s gets gen = s + 1,
// and that is the only value a step writes into a byte that was 0.  A lane that reads this byte while step s runs sees
// either the old 0 or the new s + 1 -- a byte cannot tear, and a stale cache line holds the 0 -- and both fail
// 1 <= gen <= s.  So neither the byte nor the floats behind it (which may be half written) are used by any lane of the
// same step; what a lane does use, points with 1 <= gen <= s, no lane of step s writes.  The launch boundary orders step
// s before step s + 1.  gen is therefore read and written through one pointer that is not __restrict__, and so are the
// three arrays of the volume.
//
// No float atomics and no result that depends on arrival order: a point belongs to one lane, which sums its neighbours in
// the header's order in registers.  The only atomic is the integer count of the points a step filled, one 64-bit add per
// wave into the step's own counter.
#define AMVS_TU_ID 15
#include "amvs_check.h"
#include "amvs_kernels.h"
#include "amvs_mesh_state.h"

#include <vector>

namespace amvs {

namespace {

__global__ __launch_bounds__(256) void fill_init_kernel(const float *__restrict__ weight, int n, unsigned char *__restrict__ gen)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) gen[p] = weight[p] > 0.0f ? 1 : 0;
}

__global__ __launch_bounds__(256) void fill_step_kernel(float *tsdf, float *weight, float *color_sum, unsigned char *gen, Grid g,
                                                        int step, int min_neighbours, unsigned long long *filled)
{
    const int n = g.nx * g.ny * g.nz;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    bool fill = false;
    if (p < n && gen[p] == 0) {
        const int i = p % g.nx, j = (p / g.nx) % g.ny, k = p / (g.nx * g.ny);
        const int plane = g.nx * g.ny;
        // (i-1), (i+1), (j-1), (j+1), (k-1), (k+1)
        const int offset[6] = {-1, 1, -g.nx, g.nx, -plane, plane};
        const bool inside[6] = {i > 0, i + 1 < g.nx, j > 0, j + 1 < g.ny, k > 0, k + 1 < g.nz};
        int c = 0;
        float acc = 0.0f, cacc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            if (!inside[d]) continue;
            const int q = AMVS_IDX(p + offset[d], n);
            const int gq = gen[q];
            if (gq < 1 || gq > step) continue;        // not known at this step: nothing else of q is read
            ++c;
            acc = acc + tsdf[q];
            const float w = weight[q];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) cacc[ch] = cacc[ch] + color_sum[3 * q + ch] / w;
        }
        if (c >= min_neighbours) {
            const float fc = (float)c;
            tsdf[p] = acc / fc;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) color_sum[3 * p + ch] = cacc[ch] / fc;
            weight[p] = 1.0f;
            gen[p] = (unsigned char)(step + 1);
            fill = true;
        }
    }
    const unsigned long long done = __ballot(fill);
    if (done && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)done) - 1))
        atomicAdd(filled, (unsigned long long)__popcll(done));
}

}  // namespace

bool tsdf_has_fill(const TsdfState *s) { return s && s->have_volume && s->have_fill; }

hipError_t tsdf_fill(TsdfState *s, ScratchCache &cache, int steps, int min_neighbours, long long *filled_per_step,
                     long long *n_filled, hipStream_t st)
{
    s->drop_mesh();
    s->have_fill = false;
    const long long n = s->n;
    ScratchCache::Lease counts;
    MCHK(cache.lease(counts, 8 * (size_t)steps));
    MCHK(hipMemsetAsync(counts.get(), 0, 8 * (size_t)steps, st));
    MCHK(s->fill_gen.reserve((size_t)n, cache));
    MCHK(launch(fill_init_kernel, n, st, s->weight.get(), (int)n, s->fill_gen.get()));
    for (int step = 1; step <= steps; ++step)
        MCHK(launch(fill_step_kernel, n, st, s->tsdf.get(), s->weight.get(), s->color.get(), s->fill_gen.get(), s->g, step,
                    min_neighbours, counts.get<unsigned long long>() + (step - 1)));
    std::vector<unsigned long long> h((size_t)steps, 0ull);
    MCHK(hipMemcpyAsync(h.data(), counts.get(), 8 * (size_t)steps, hipMemcpyDeviceToHost, st));
    MCHK(hipStreamSynchronize(st));
    long long total = 0;
    for (int q = 0; q < steps; ++q) {
        if (filled_per_step) filled_per_step[q] = (long long)h[q];
        total += (long long)h[q];
    }
    if (n_filled) *n_filled = total;
    s->have_fill = true;
    return hipSuccess;
}

hipError_t tsdf_fetch_fill(TsdfState *s, unsigned char *gen, hipStream_t st)
{
    if (gen) MCHK(hipMemcpyAsync(gen, s->fill_gen.get(), (size_t)s->n, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

}  // namespace amvs

AMVS_CHECK_TU(mesh_fill)
