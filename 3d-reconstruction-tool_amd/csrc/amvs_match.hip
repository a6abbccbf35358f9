// amvs_match.hip -- exact 2-nearest-neighbour search over 128-dimensional 8-bit descriptors on the matrix cores, the
// ratio test and the compaction of the matches (include/amvs_match.h; the definition is the header's, the judge is
// tests/match_restatement.py, bit for bit).
//
// Storage.  A slot keeps its rows as signed bytes (value - 128, which leaves every distance unchanged) in the order
// the matrix instruction reads them: for every block of 32 rows and every step s = 0..3 of 32 dimensions, the 64
// 16-byte fragments of a wave's lanes are contiguous -- lane l holds row (l & 31), dimensions 32 s + 16 (l >> 5) ..
// + 15.  A wave's operand load is therefore one fully coalesced 1 KiB read, for queries and train rows alike, and the
// kernel needs no LDS staging (and so has no bank conflicts to pad away).  v_mfma_i32_32x32x32_i8 maps its A and B
// operands to the reduction index by the same rule, so only "same dimensions in the same lane half" matters.  Rows up
// to the next multiple of 32 are stored as zeros; `norm` is the sum of squares of a row's signed bytes, `normk` is
// 2^31 - (norm << 8) + 255 - (row & 255) for a real row and 0 for a padded one.
//
// desc_knn2_kernel.  A wave owns NQ = 4 tiles of 32 queries as B operands (64 VGPRs, loaded once): the accumulator's
// column is then the query, so the 16 accumulator values of a lane all belong to ONE query and 16 different train rows,
// and the top-2 update needs no cross-lane traffic.  A train tile's fragments are loaded once for the NQ query tiles:
// with one query tile per wave the kernel was bound by the vector memory path (8 KiB of operand loads per 128 matrix
// cycles of a wave; 3.09 ms at 100 k x 100 k against 1.81 ms now).  Per train tile a wave issues
// 8 loads (4 operand fragments, 4 of normk) and, per query tile, 4 matrix instructions and per output
//     key = (dot << 9) + normk  =  2^31 + 256 (2 q.t - |t|^2) + 255 - (row & 255)        (one v_lshl_add_u32)
// -- LARGER is nearer and, among equals, the lower row; the query's own |q|^2 orders nothing within a lane; a real key
// is above 0 and a padded row's key, whose dot product is 0, is 0: padding can never win -- then
//     second = med3(best, second, key), best = max(best, key):
// three vector instructions per output.  After a chunk of 256 train rows the pair is widened to 64-bit (s << 32) | j and
// merged into the running pair; at the end the two lane halves of a query are merged through one shuffle and the pair
// of this workgroup's share of the train set is stored.  desc_knn2_merge_kernel merges the shares by the same order.
// No atomics, no floating point: the result cannot depend on the launch shape.
#define AMVS_TU_ID 19
#include "amvs_check.h"
#include "amvs_kernels.h"
#include "amvs_match_state.h"
#include "../../include/amvs_match.h"

#include <hipcub/hipcub.hpp>

namespace amvs {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr unsigned long long NONE64 = ~0ull;
// keys of a chunk: KEY_BIAS + 256 (2 q.t - |t|^2) + 255 - (row & 255); 2 q.t - |t|^2 = |q|^2 - s lies in (-2^23, 2^21], so a
// real key lies in (0, 2^31 + 2^29]; a padded row's key is PAD_KEY, below every real one
constexpr unsigned KEY_BIAS = 0x80000000u, PAD_KEY = 0u;
constexpr int TILE = AMVS_DESC_TILE, CHUNK = AMVS_DESC_CHUNK, QBLOCK = AMVS_DESC_QUERY_BLOCK;
constexpr int NQ = QBLOCK / (4 * TILE);          // query tiles of a wave: a train fragment is loaded once for all of them
static_assert(TILE == 32 && CHUNK == 256 && QBLOCK == 4 * TILE * NQ && AMVS_DESC_DIM == 128, "the kernel's shape");

inline dim3 grid_for(long long n) { long long b = (n + 255) / 256; return dim3((unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b))); }

// one lane per stored row (n_pad of them): re-orders the row into fragments, norms beside it
__global__ __launch_bounds__(256) void desc_pack_kernel(const uint4 *__restrict__ src, int n, int n_pad, uint4 *__restrict__ frag,
                                                        int *__restrict__ norm, unsigned *__restrict__ normk)
{
    for (int row = (int)(blockIdx.x * blockDim.x + threadIdx.x); row < n_pad; row += (int)(gridDim.x * blockDim.x)) {
        const int tile = row >> 5, r = row & 31;
        int sq = 0;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (row < n) {
                v = src[(size_t)row * 8 + p];
                v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
                const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int x = (int)(signed char)((w[k] >> (8 * b)) & 0xFFu);
                        sq += x * x;
                    }
            }
            frag[((size_t)(tile * 4 + (p >> 1)) * 64) + (size_t)((p & 1) * 32 + r)] = v;
        }
        norm[row] = sq;
        normk[row] = row < n ? KEY_BIAS - ((unsigned)sq << 8) + (255u - (unsigned)(row & (CHUNK - 1))) : PAD_KEY;
    }
}

// (b, s) <- the two smallest of {b, s, kb, ks}; b <= s and kb <= ks, equal only when NONE64
__device__ __forceinline__ void merge2(unsigned long long &b, unsigned long long &s, unsigned long long kb, unsigned long long ks)
{
    const unsigned long long lo = b < kb ? b : kb, hi = b < kb ? kb : b, s2 = s < ks ? s : ks;
    b = lo;
    s = hi < s2 ? hi : s2;
}

// the median of three: with best >= second it is the new second best
__device__ __forceinline__ unsigned med3(unsigned a, unsigned b, unsigned c)
{
    unsigned r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

__device__ __forceinline__ void load_tile(const v4i *__restrict__ tfrag, const uint4 *__restrict__ tnormk, int tile, int l,
                                          v4i (&a)[4], uint4 (&nk)[4])
{
#pragma unroll
    for (int s = 0; s < 4; ++s) a[s] = tfrag[(size_t)(tile * 4 + s) * 64 + l];
#pragma unroll
    for (int g = 0; g < 4; ++g) nk[g] = tnormk[(size_t)tile * 8 + (l >> 5) + 2 * g];
}

// one 32-row train tile against the wave's NQ query tiles: per query tile four matrix instructions, then the top-2
// update of the lane's 16 outputs.  Accumulator register r of lane l is train row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the
// tile and query l & 31 of the query tile.
__device__ __forceinline__ void tile_update(const v4i (&a)[4], const v4i (&bq)[NQ][4], const uint4 (&nk)[4], unsigned (&best)[NQ],
                                            unsigned (&second)[NQ])
{
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
        v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], bq[u][s], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint4 k4 = nk[r >> 2];
            const unsigned base = (r & 3) == 0 ? k4.x : (r & 3) == 1 ? k4.y : (r & 3) == 2 ? k4.z : k4.w;
            // key = 2^31 + 256 (2 q.t - |t|^2) + 255 - (row & 255): LARGER is nearer, and among equals the lower row; the
            // query's own |q|^2 orders nothing and enters when the pair is widened.  (Plain C on purpose: the compiler
            // places the wait states between the matrix instruction and the first read of its result; inside inline
            // assembly it would not.)
            const unsigned key = ((unsigned)acc[r] << 9) + base;
            second[u] = med3(best[u], second[u], key);
            best[u] = max(best[u], key);
        }
    }
}

__global__ __launch_bounds__(256) void desc_knn2_kernel(const v4i *__restrict__ qfrag, const int *__restrict__ qnorm, int n_q,
                                                        const v4i *__restrict__ tfrag, const uint4 *__restrict__ tnormk,
                                                        int n_t_tiles, int n_chunks, int chunks_per_split,
                                                        unsigned long long *__restrict__ partial)
{
    const int l = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const int n_q_tiles = (n_q + TILE - 1) / TILE;
    const int qtile0 = ((int)blockIdx.x * 4 + w) * NQ;
    if (qtile0 >= n_q_tiles) return;                         // (a whole wave; the kernel has no barrier)
    // a query tile past the last one is the last one once more; its results are not stored
    v4i bq[NQ][4];
    unsigned nqk[NQ];
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
        const int qt = min(qtile0 + u, n_q_tiles - 1);
#pragma unroll
        for (int s = 0; s < 4; ++s) bq[u][s] = qfrag[(size_t)(qt * 4 + s) * 64 + l];
        nqk[u] = (unsigned)qnorm[qt * TILE + (l & 31)] << 8;  // (below the slot's padded row count)
    }
    const int split = (int)blockIdx.y;
    const int c0 = split * chunks_per_split, c1 = min(c0 + chunks_per_split, n_chunks);
    unsigned long long B[NQ], S[NQ];
#pragma unroll
    for (int u = 0; u < NQ; ++u) B[u] = S[u] = NONE64;
    // two operand sets in turn: the next tile's operands and keys are in flight while the current tile is worked on
    v4i a0[4], a1[4];
    uint4 nk0[4], nk1[4];
    const int tile_begin = c0 * (CHUNK / TILE), tile_end = min(c1 * (CHUNK / TILE), n_t_tiles);
    if (tile_begin < tile_end) load_tile(tfrag, tnormk, tile_begin, l, a0, nk0);
    for (int chunk = c0; chunk < c1; ++chunk) {
        unsigned best[NQ], second[NQ];
#pragma unroll
        for (int u = 0; u < NQ; ++u) best[u] = second[u] = PAD_KEY;
        const int t0 = chunk * (CHUNK / TILE), t1 = min(t0 + CHUNK / TILE, n_t_tiles);
        for (int tile = t0; tile < t1; tile += 2) {
            // (a tile past the end of this share is the last one loaded once more, and not used)
            load_tile(tfrag, tnormk, min(tile + 1, tile_end - 1), l, a1, nk1);
            tile_update(a0, bq, nk0, best, second);
            load_tile(tfrag, tnormk, min(tile + 2, tile_end - 1), l, a0, nk0);
            if (tile + 1 < t1) tile_update(a1, bq, nk1, best, second);
        }
        const unsigned long long row0 = (unsigned long long)chunk * CHUNK;
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            // 256 |q|^2 - (key - 2^31) + 255 = 256 s + (row & 255)
            const unsigned wb = nqk[u] + 255u + KEY_BIAS - best[u], ws = nqk[u] + 255u + KEY_BIAS - second[u];
            const unsigned long long kb = best[u] != PAD_KEY ? ((unsigned long long)(wb >> 8) << 32) | (row0 + (wb & 255u)) : NONE64;
            const unsigned long long ks = second[u] != PAD_KEY ? ((unsigned long long)(ws >> 8) << 32) | (row0 + (ws & 255u)) : NONE64;
            merge2(B[u], S[u], kb, ks);
        }
    }
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
        const unsigned long long oB = __shfl_xor(B[u], 32), oS = __shfl_xor(S[u], 32);
        merge2(B[u], S[u], oB, oS);
        const int q = (qtile0 + u) * TILE + (l & 31);
        if (l < 32 && q < n_q) {
            unsigned long long *o = partial + ((size_t)split * n_q + q) * 2;
            o[0] = B[u];
            o[1] = S[u];
        }
    }
}

__global__ __launch_bounds__(256) void desc_knn2_merge_kernel(const unsigned long long *__restrict__ partial, int splits, int n_q,
                                                              int *__restrict__ idx, int *__restrict__ dist2)
{
    for (int q = (int)(blockIdx.x * blockDim.x + threadIdx.x); q < n_q; q += (int)(gridDim.x * blockDim.x)) {
        unsigned long long B = NONE64, S = NONE64;
        for (int s = 0; s < splits; ++s) {
            const unsigned long long *p = partial + ((size_t)s * n_q + q) * 2;
            merge2(B, S, p[0], p[1]);
        }
        idx[2 * q] = (int)(B & 0xFFFFFFFFull);      dist2[2 * q] = (int)(B >> 32);
        idx[2 * q + 1] = (int)(S & 0xFFFFFFFFull);  dist2[2 * q + 1] = (int)(S >> 32);
    }
}

// the ratio test of the header; with rev_*: and the reverse search keeps row j1 with best index i
__global__ __launch_bounds__(256) void desc_ratio_kernel(const int *__restrict__ idx, const int *__restrict__ dist2, int n_q,
                                                         double ratio2, const int *__restrict__ rev_idx,
                                                         const int *__restrict__ rev_dist2, int n_t, unsigned char *__restrict__ flag)
{
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n_q; i += (int)(gridDim.x * blockDim.x)) {
        bool keep = (double)dist2[2 * i] < ratio2 * (double)dist2[2 * i + 1];
        if (keep && rev_idx) {
            const int j = AMVS_IDX(idx[2 * i], n_t);
            keep = rev_idx[2 * j] == i && (double)rev_dist2[2 * j] < ratio2 * (double)rev_dist2[2 * j + 1];
        }
        flag[i] = keep ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void desc_gather_kernel(const int *__restrict__ sel, int m, int n_q, const int *__restrict__ idx,
                                                          const int *__restrict__ dist2, int *__restrict__ out)
{
    for (int k = (int)(blockIdx.x * blockDim.x + threadIdx.x); k < m; k += (int)(gridDim.x * blockDim.x)) {
        const int i = AMVS_IDX(sel[k], n_q);
        out[k] = i;
        out[(size_t)n_q + k] = idx[2 * i];
        out[2 * (size_t)n_q + k] = dist2[2 * i];
    }
}

int padded(int n) { return (n + TILE - 1) / TILE * TILE; }

}  // namespace

int desc_knn2_splits(int n_q, int n_t, int *chunks_per_split)
{
    const int q_blocks = (n_q + QBLOCK - 1) / QBLOCK, chunks = (n_t + CHUNK - 1) / CHUNK;
    const int want = std::max(1, std::min(chunks, 2048 / std::max(q_blocks, 1)));
    const int cps = (chunks + want - 1) / want;
    if (chunks_per_split) *chunks_per_split = cps;
    return (chunks + cps - 1) / cps;
}

hipError_t desc_set_device(const unsigned char *desc_d, int n, ScratchCache &cache, DescSlot &slot, hipStream_t st)
{
    slot.n = -1;
    const int n_pad = padded(n);
    if (n_pad > 0) {
        STCHK(slot.frag.reserve((size_t)n_pad * 8, cache));
        STCHK(slot.norm.reserve((size_t)n_pad, cache));
        STCHK(slot.normk.reserve((size_t)n_pad, cache));
        hipLaunchKernelGGL(desc_pack_kernel, grid_for(n_pad), dim3(256), 0, st, (const uint4 *)desc_d, n, n_pad, slot.frag.get(),
                           slot.norm.get(), slot.normk.get());
        STCHK(hipGetLastError());
        STCHK(hipStreamSynchronize(st));
    }
    slot.n = n;
    return hipSuccess;
}

hipError_t desc_set(const unsigned char *desc_h, int n, ScratchCache &cache, DescSlot &slot, hipStream_t st)
{
    slot.n = -1;
    ScratchCache::Lease src;
    if (n > 0) {
        STCHK(cache.lease(src, (size_t)n * AMVS_DESC_DIM));
        STCHK(hipMemcpyAsync(src.get(), desc_h, (size_t)n * AMVS_DESC_DIM, hipMemcpyHostToDevice, st));
    }
    return desc_set_device(src.get<unsigned char>(), n, cache, slot, st);   // (synchronises: the staging lease goes back idle)
}

// idx, dist2: [n_q][2] int32 on the device.  Does not synchronise unless it fails.
hipError_t desc_knn2(const DescSlot &q, const DescSlot &t, ScratchCache &cache, ScratchCache::Lease &partial, int *idx, int *dist2,
                     hipStream_t st)
{
    if (q.n <= 0) return hipSuccess;
    int cps = 1;
    const int splits = desc_knn2_splits(q.n, t.n, &cps);
    const int n_t_tiles = padded(t.n) / TILE, n_chunks = (t.n + CHUNK - 1) / CHUNK;
    STCHK(cache.lease(partial, sizeof(unsigned long long) * 2 * (size_t)splits * q.n));
    hipLaunchKernelGGL(desc_knn2_kernel, dim3((unsigned)((q.n + QBLOCK - 1) / QBLOCK), (unsigned)splits), dim3(256), 0, st,
                       (const v4i *)q.frag.get(), (const int *)q.norm.get(), q.n, (const v4i *)t.frag.get(),
                       (const uint4 *)t.normk.get(), n_t_tiles, n_chunks, cps, partial.get<unsigned long long>());
    STCHK(hipGetLastError());
    hipLaunchKernelGGL(desc_knn2_merge_kernel, grid_for(q.n), dim3(256), 0, st, (const unsigned long long *)partial.get(), splits, q.n,
                       idx, dist2);
    STCHK(hipGetLastError());
    return hipSuccess;
}

// the host copies are made here; synchronises `st`
hipError_t desc_knn2_host(const DescSlot &q, const DescSlot &t, ScratchCache &cache, int *idx_h, int *dist2_h, hipStream_t st)
{
    if (q.n <= 0) return hipSuccess;
    ScratchCache::Lease partial, out;
    const size_t n2 = 2 * (size_t)q.n;
    STCHK(cache.lease(out, sizeof(int) * 2 * n2));
    int *idx = out.get<int>(), *dist2 = idx + n2;
    STCHK(desc_knn2(q, t, cache, partial, idx, dist2, st));
    STCHK(hipMemcpyAsync(idx_h, idx, sizeof(int) * n2, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(dist2_h, dist2, sizeof(int) * n2, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t desc_match(const DescSlot &q, const DescSlot &t, float ratio, bool cross_check, ScratchCache &cache, int *q_idx_h,
                      int *t_idx_h, int *dist2_h, long long *n_matches, hipStream_t st)
{
    *n_matches = 0;
    if (q.n <= 0) return hipSuccess;
    const double ratio2 = (double)ratio * (double)ratio;
    ScratchCache::Lease partial, partial_rev, fwd, rev, flag, sel, cnt, tmp, out;
    const size_t n2 = 2 * (size_t)q.n, r2 = 2 * (size_t)t.n;
    STCHK(cache.lease(fwd, sizeof(int) * 2 * n2));
    int *idx = fwd.get<int>(), *dist2 = idx + n2, *ridx = nullptr, *rdist2 = nullptr;
    STCHK(desc_knn2(q, t, cache, partial, idx, dist2, st));
    if (cross_check) {
        STCHK(cache.lease(rev, sizeof(int) * 2 * r2));
        ridx = rev.get<int>();
        rdist2 = ridx + r2;
        STCHK(desc_knn2(t, q, cache, partial_rev, ridx, rdist2, st));
    }
    STCHK(cache.lease(flag, (size_t)q.n));
    STCHK(cache.lease(sel, sizeof(int) * (size_t)q.n));
    STCHK(cache.lease(cnt, sizeof(int)));
    STCHK(cache.lease(out, sizeof(int) * 3 * (size_t)q.n));
    hipLaunchKernelGGL(desc_ratio_kernel, grid_for(q.n), dim3(256), 0, st, (const int *)idx, (const int *)dist2, q.n, ratio2,
                       (const int *)ridx, (const int *)rdist2, t.n, flag.get<unsigned char>());
    STCHK(hipGetLastError());
    hipcub::CountingInputIterator<int> iota(0);
    size_t bytes = 0;
    STCHK(hipcub::DeviceSelect::Flagged(nullptr, bytes, iota, flag.get<unsigned char>(), sel.get<int>(), cnt.get<int>(), q.n, st));
    STCHK(cache.lease(tmp, bytes));
    STCHK(hipcub::DeviceSelect::Flagged(tmp.get(), bytes, iota, flag.get<unsigned char>(), sel.get<int>(), cnt.get<int>(), q.n, st));
    int m = 0;
    STCHK(hipMemcpyAsync(&m, cnt.get(), sizeof(int), hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
    if (m > 0) {
        hipLaunchKernelGGL(desc_gather_kernel, grid_for(m), dim3(256), 0, st, (const int *)sel.get(), m, q.n, (const int *)idx,
                           (const int *)dist2, out.get<int>());
        STCHK(hipGetLastError());
        STCHK(hipMemcpyAsync(q_idx_h, out.get<int>(), sizeof(int) * m, hipMemcpyDeviceToHost, st));
        STCHK(hipMemcpyAsync(t_idx_h, out.get<int>() + q.n, sizeof(int) * m, hipMemcpyDeviceToHost, st));
        STCHK(hipMemcpyAsync(dist2_h, out.get<int>() + 2 * (size_t)q.n, sizeof(int) * m, hipMemcpyDeviceToHost, st));
        STCHK(hipStreamSynchronize(st));
    }
    *n_matches = m;
    return hipSuccess;
}

}  // namespace amvs

AMVS_CHECK_TU(match)
