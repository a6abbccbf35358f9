// amvs_kernel_common.h -- device helpers shared by the five sweep translation units: the sweep step in its exact
// (amvs_kernels.hip), fast (amvs_kernels_fast.hip) and run-time-patch (amvs_generic.hip) form and the plane sweeps
// (amvs_sweep_exact.hip, amvs_sweep_fast.hip, amvs_generic.hip).  What is stated here is stated once; DESIGN.md
// section 4 lists the row stages that are still written out per kernel, and why.
#pragma once
#include "amvs_kernels.h"
#include "amvs_device.h"
#include "amvs_dispatch.h"
#include "amvs_strip_order.h"

#include <type_traits>

namespace amvs {

// The job table is never written while a sweep kernel runs: reading it through the
// constant address space lets the compiler use scalar loads (s_load) for the poses.
typedef const __attribute__((address_space(4))) Job *JobCP;

// Opaque copy of a uniform pointer.  Loads through the result cannot be hoisted above this
// point, so the row loops re-issue their scalar loads (s_load from the scalar cache) every
// iteration instead of keeping ~90 pose / intrinsics values live and spilling SGPRs into VGPR
// lanes (v_writelane / v_readlane), which cost 14 % of the VALU stream before.
AMVS_DEV JobCP reload(JobCP p)
{
    asm volatile("" : "+s"(p));
    return p;
}

// (Non-temporal hints on the streaming state were measured without effect on MI355X -- 31.8 vs 31.7
// G px-hyp/s -- and are not used.)

// per-row validity bits of the last K/2+1 rows packed into one (or two) registers
template <int K, int S> struct Hist {
    // (more than 64 bits from 21 x 21 with 6 sources on: a 128-bit integer, two more shifts per row)
    typedef typename std::conditional<(S * (K / 2 + 1) <= 32), uint32_t,
                                      typename std::conditional<(S * (K / 2 + 1) <= 64), unsigned long long, unsigned __int128>::type>::type T;
};

// Depth state maps carry, in the sign bit, the normal buffer that holds the pixel's current normal
// (StepArgs::nbuf); depths themselves are positive.
AMVS_DEV float depth_untag(float d, unsigned mask) { return __uint_as_float(__float_as_uint(d) & mask); }
AMVS_DEV unsigned depth_buffer(float d) { return __float_as_uint(d) >> 31; }
AMVS_DEV float depth_tag(float d, unsigned buffer) { return __uint_as_float(__float_as_uint(d) | (buffer << 31)); }

// Reference gray of the packed path: the low byte of the view's padded row-pair map, which is addressed from its
// pixel (0,0) (row pitch W + 2 AMVS_PAIR_BORDER): valid texel indices are [-origin, elems - origin).  The row loads
// use clamped indices -- `live ? pix + PADW * yr : 0`: dead lanes read element 0 -- so there is no branch in the load
// path.  (Macros, so that the index-checked build records the line of the kernel that expands them.)
#define AMVS_REF_PAIR_IDX(i, H, W) AMVS_IDX_LOHI((i), -((long long)AMVS_PAIR_BORDER * ((W) + 2 * AMVS_PAIR_BORDER) + AMVS_PAIR_BORDER), (long long)((H) + 2 * AMVS_PAIR_BORDER) * ((W) + 2 * AMVS_PAIR_BORDER) - ((long long)AMVS_PAIR_BORDER * ((W) + 2 * AMVS_PAIR_BORDER) + AMVS_PAIR_BORDER))
// texel i of such a map (AMVS_CODE_BYTES, amvs_device.h: one byte per texel instead of a row pair)
#if AMVS_CODE_BYTES
#define AMVS_REF_CODE(ref_pairs, i) (((const __attribute__((address_space(1))) uint8_t *)(ref_pairs))[i])
#else
#define AMVS_REF_CODE(ref_pairs, i) ((ref_pairs)[i])
#endif

// Depth hypothesis a pixel is sampled at in this step: the (offset) pixel's current depth for
// propagation / evaluation / confidence -- depth_min outside the image (the F.pad value) --, a clamped random
// perturbation of it, depth + (rand*2-1)*range, for refinement (mvs_patchmatch.py:430-436, :468-473).
// `d_raw` is d_in at the pixel (+ offset) when `inb`.
AMVS_DEV float candidate_depth(const StepArgs &a, int mode, bool inb, float d_raw, uint32_t h0)
{
    const float dc = inb ? depth_untag(d_raw, a.depth_mask) : a.depth_min;
    const float delta = (rng_uniform(h0) * 2.0f - 1.0f) * a.depth_range;
    float d = dc + delta;
    d = d < a.depth_min ? a.depth_min : d;
    d = d > a.depth_max ? a.depth_max : d;
    return mode == MODE_REFINE ? d : dc;
}

// Cost of a pixel from the sum over its valid sources: their average, +inf when fewer than two
// (mvs_patchmatch.py:387-388).  QDIV: the exact arithmetic's correctly rounded quotient; otherwise
// total * RN(1 / cden) (fast arithmetic).
template <bool QDIV>
AMVS_DEV float average_cost(float total, float cnt)
{
    const float cden = cnt + 1e-8f;              // 1e-8 ... S: always inside the lean reciprocal's range
    bool cden_ok = true;
    const float rc = rcp_t<true>(cden, cden_ok);
    const float avg = QDIV ? qdiv(total, cden, rc) : total * rc;
    return cnt >= 2.0f ? avg : __builtin_inff();
}

// Queued winners: one 32-bit entry each (the queue of a wave is 2 x 64 entries = 512 bytes of LDS; round 4 --
// 8-byte entries before -- so that the paired-band exchange of the 11 x 11 patch fits beside the rings at four
// workgroups per CU).  Pixel indices are below 2^29 (amvs_create).
//
// Normal update of `n` queued refinement winners (entries head .. head+n-1 of the ring `nq`), one
// per lane: normal <- normalize(normal + randn * range)   (mvs_patchmatch.py:475-476).  Entry: pixel
// index with the winner's normal buffer in bit 31; the pixel's hash (a pure function of the pixel and the
// launch's stream key) is formed again here.
AMVS_DEV uint32_t refine_entry(int pc, unsigned buf_c) { return (unsigned)pc | (buf_c << 31); }

AMVS_DEV void refine_normals(const uint32_t *nq, int head, int n, int lane, float *nbuf0, float *nbuf1, float normal_range,
                             StreamKey key, int hw)
{
    (void)hw;                                                  // (pixels per map: the index-checked build's extent)
    if (lane < n) {
        const uint32_t e = nq[(head + lane) & (2 * AMVS_WAVE - 1)];
        const uint32_t pc = e & 0x7FFFFFFFu;
        float *np = ((e >> 31) ? nbuf1 : nbuf0) + 3ll * AMVS_IDX((int)pc, hw);
        float g0, g1, g2;
        rng_normals3(pixel_hash(pc, key), g0, g1, g2);
        float cn0 = np[0] + g0 * normal_range;
        float cn1 = np[1] + g1 * normal_range;
        float cn2 = np[2] + g2 * normal_range;
        normalize3(cn0, cn1, cn2);
        np[0] = cn0; np[1] = cn1; np[2] = cn2;
    }
}

// Propagation winners (mvs_patchmatch.py:452-455), queued like the refinement winners and moved 64 at
// a time: pixel pc takes the pre-step normal of its neighbour pn = pc + noff (zero outside the image, F.pad
// :431-442) into the buffer it does not currently use.  Entry: pc | neighbour inside the image << 29 |
// neighbour's buffer << 30 | pc's current buffer << 31.
// Nothing writes a neighbour's CURRENT normal during a propagation launch and nothing reads the
// buffer a winner writes (StepArgs::nbuf), so the move may happen any time before the launch ends.
AMVS_DEV uint32_t propagate_entry(int pc, unsigned buf_c, bool inb_c, unsigned buf_n)
{
    return (unsigned)pc | ((inb_c ? 1u : 0u) << 29) | (buf_n << 30) | (buf_c << 31);
}

AMVS_DEV void propagate_normals(const uint32_t *nq, int head, int n, int lane, float *nbuf0, float *nbuf1, int noff, int hw)
{
    (void)hw;
    if (lane < n) {
        const uint32_t e = nq[(head + lane) & (2 * AMVS_WAVE - 1)];
        const int pc = AMVS_IDX((int)(e & 0x1FFFFFFFu), hw);
        const bool inb_c = (e >> 29) & 1u;
        const int pn = AMVS_IDX(inb_c ? pc + noff : 0, hw);
        // (three consecutive dwords each way: hipcc merges them into one dwordx3 access)
        const float *src = (((e >> 30) & 1u) ? nbuf1 : nbuf0) + 3ll * pn;
        const float t0 = src[0], t1 = src[1], t2 = src[2];
        float *dst = ((e >> 31) ? nbuf0 : nbuf1) + 3ll * pc;
        dst[0] = inb_c ? t0 : 0.0f;
        dst[1] = inb_c ? t1 : 0.0f;
        dst[2] = inb_c ? t2 : 0.0f;
    }
}

// AMVS_WG_WAVES horizontally adjacent strips share one workgroup (one CU, started together) and
// re-align with a barrier every AMVS_WG_SYNC_ROWS rows: x-neighbours sample overlapping epipolar
// bands of the sources, and they only share those lines in L1 / L2 while they work on the same rows.
// Four waves (one per SIMD, so the workgroup granularity costs no occupancy) re-aligned every 8 rows
// measured +1.8 % over single-wave workgroups (39.5 vs 38.85 G px-hyp/s; 16 rows the same, no
// barrier +0.5 %).  With 10 waves the HBM-side traffic halves -- and the launch
// gets slower, because a 5- or 10-wave workgroup fits only twice / once per CU.
#ifndef AMVS_WG_WAVES
#define AMVS_WG_WAVES 4
#endif
#ifndef AMVS_WG_SYNC_ROWS
#define AMVS_WG_SYNC_ROWS 8
#endif
// Paired-band schedule (StepArgs::paired): a workgroup is AMVS_PAIR_COLS strip columns x 2 vertically
// adjacent bands (2 -> 4 waves, 4 -> 8 waves); compiled where the exchange rows fit beside the rings at four
// workgroups per CU
#ifndef AMVS_PAIR_COLS
#define AMVS_PAIR_COLS 2
#endif
constexpr int PAIR_WAVES = 2 * AMVS_PAIR_COLS;

// strip of wave `wv` of this block (amvs_strip_order.h; wave-uniform); false: the wave has none
AMVS_DEV bool sweep_strip(const StepArgs &a, bool pair, int wg_waves, int wv, StripPos &p)
{
    return strip_decode(a.n_jobs, a.tiles_x, a.tiles_y, a.band_major, pair, AMVS_PAIR_COLS, wg_waves, a.edge_first,
                        (int)blockIdx.x, (int)gridDim.x, wv, p);
}
constexpr bool step_pair_supported_ks(int K, int S) { return K >= 5 && K <= 11 && S <= 4; }

// Workgroup timeline (-DAMVS_STEP_TRACE, tools/step_timeline.py; the shipped build compiles it away): wave 0 of
// every sweep workgroup records, with ordinary stores, [0] the constant-rate wall clock (100 MHz) at entry, [1] before
// exit, [2] the XCC it runs on, [3] job << 40 | strip row << 20 | strip column into StepArgs::trace[4 * block].
#ifdef AMVS_STEP_TRACE
AMVS_DEV void step_trace_entry(const StepArgs &a, int wv, int lane, int job_id, int ty, int tx)
{
    if (a.trace && wv == 0 && lane == 0) {
        unsigned long long *r = a.trace + 4ull * blockIdx.x;
        r[0] = wall_clock64();
        r[2] = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xFu;              // hwreg(HW_REG_XCC_ID, 0, 4)
        r[3] = ((unsigned long long)job_id << 40) | ((unsigned long long)ty << 20) | (unsigned long long)tx;
    }
}
AMVS_DEV void step_trace_exit(const StepArgs &a, int wv, int lane)
{
    if (a.trace && wv == 0 && lane == 0) a.trace[4ull * blockIdx.x + 1] = wall_clock64();
}
#define AMVS_TRACE_ENTRY(...) step_trace_entry(__VA_ARGS__)
#define AMVS_TRACE_EXIT(...) step_trace_exit(__VA_ARGS__)
#else
#define AMVS_TRACE_ENTRY(...) ((void)0)
#define AMVS_TRACE_EXIT(...) ((void)0)
#endif

// Plane sweep: the running best of a strip's output pixels lives in LDS ([row][lane]) as 16-bit keys
// (votes << 12 | 4095 - plane of the chunk), or -- SweepArgs::key8, chunks of at most 32 planes -- as 8-bit keys
// (votes << 5 | 31 - plane) in the same array, for strips twice as high; KeyT selects the width.  Plane d of the chunk
// that starts at d_begin enters row yc of the strip that starts at y0.  The chunk's first plane always enters
// (torch.max over a volume that starts at 0 votes): its key (0 << 12) | 4095 -- (0 << 5) | 31 -- beats the initial 0.
template <class KeyT>
AMVS_DEV void sweep_best_update(KeyT *best, int yc, int y0, int lane, uint32_t votes, int d, int d_begin)
{
    constexpr int PLANE_BITS = sizeof(KeyT) == 1 ? 5 : 12;
    static_assert((1 << PLANE_BITS) == (sizeof(KeyT) == 1 ? AMVS_SWEEP_MAX_CHUNK8 : AMVS_SWEEP_MAX_CHUNK), "planes of a chunk");
    const uint32_t keyv = (votes << PLANE_BITS) | (uint32_t)((1 << PLANE_BITS) - 1 - (d - d_begin));
    const uint32_t cur = best[(yc - y0) * AMVS_WAVE + lane];
    if (keyv > cur) best[(yc - y0) * AMVS_WAVE + lane] = (KeyT)keyv;
}

static_assert(list_max(SourceCounts{}) == AMVS_KMAX_SRC, "SourceCounts ends at AMVS_KMAX_SRC (Job::src, Job::fsrc)");
static_assert(list_max(CompiledPatches{}) <= AMVS_MAX_PATCH, "a compiled patch size beyond AMVS_MAX_PATCH");

// The step kernels are specialised for these two modes; every other mode runs their <-1> instantiation, which
// reads the mode from StepArgs.  The paired-band schedule exists for the listed modes only.
using StepModes = IntList<MODE_REFINE, MODE_PROP>;
template <class F>
void dispatch_step_mode(int mode, F &&f)
{
    if (!dispatch(StepModes{}, mode, false, [&](auto m) { return f(m), true; })) f(std::integral_constant<int, -1>{});
}

#if defined(AMVS_HSUM_LDS) && AMVS_WG_WAVES > 1
#error "the LDS horizontal-sum variant keeps one exchange buffer per workgroup: build it with -DAMVS_WG_WAVES=1"
#endif

}  // namespace amvs
