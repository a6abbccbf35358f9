// amvs_sift_keypoints.hip -- the keypoint stages of SIFT on a resident scale space (include/amvs_features.h; the
// definition is the header's, judged against tests/features_restatement.py bit for bit): extrema, refinement,
// orientations, canonical order, selection, descriptors.
//
// extrema_kernel: one lane per interior pixel of the three inner difference layers of an octave; a hit is appended
// through an atomic counter, in an order the later sort makes irrelevant.  When more hits are counted than the array
// holds, the host enlarges it to the count and runs the search again: nothing is truncated.
// refine_kernel: one lane per candidate, the header's 3 x 3 solve and tests.
// orient_kernel / describe_kernel: one wave per keypoint, four per workgroup.  The 36 and the 128 bins are 64-bit
// integers in LDS; a contribution is rounded once to a multiple of 2^-20 and added with an integer atomic, so the sums
// do not depend on the lanes' order.  A keypoint's float32 arithmetic is that of amvs_sift_math.h.
// The canonical order and the n_features strongest come from rocprim's radix sort on 64-bit keys.
#include "amvs_features_state.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace amvs {

namespace {

constexpr int BORDER = 5, MAX_STEPS = 5, ORI_BINS = 36, WAVES = 4;
constexpr float FIX = 1048576.0f, FLT_EPS = 1.1920929e-07f;
constexpr long long MAX_BLOCKS = 8192;

struct Cand { int o, i, r, c; };
// a refined candidate: (i, r, c) where the refinement ended, key the canonical key of the extremum it began at
struct Kp {
    unsigned long long key;
    int valid, o, i, r, c;
    float x, y, size, scl, response;
};
struct Ori {
    Kp k;
    float angle;
    int pad;
};

#define KCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

__global__ __launch_bounds__(256) void extrema_kernel(const SiftPyramid p, int o, float pre, Cand *__restrict__ cand, int cap,
                                                      int *__restrict__ count)
{
    const int h = p.h[o], w = p.w[o], ih = h - 2 * BORDER, iw = w - 2 * BORDER;      // both > 0: the host checks
    const long long per = (long long)ih * iw, n = 3 * per;
    const ptrdiff_t px = (ptrdiff_t)h * w;
    const float *d0 = p.dog + p.d_off[o];
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long long)gridDim.x * 256) {
        const int l = (int)(idx / per);
        const long long rem = idx - l * per;
        const int i = 1 + l, r = BORDER + (int)(rem / iw), c = BORDER + (int)(rem % iw);
        const float *q = d0 + i * px + (ptrdiff_t)r * w + c;
        const float v = *q;
        if (!(v > pre || v < -pre)) continue;
        bool ge = true, le = true;
        for (int dl = -1; dl <= 1; ++dl)
            for (int dr = -1; dr <= 1; ++dr)
                for (int dc = -1; dc <= 1; ++dc) {
                    const float nb = q[dl * px + (ptrdiff_t)dr * w + dc];
                    ge = ge && v >= nb;
                    le = le && v <= nb;
                }
        if ((v > pre && ge) || (v < -pre && le)) {
            const int slot = atomicAdd(count, 1);
            if (slot < cap) cand[slot] = Cand{o, i, r, c};
        }
    }
}

__global__ __launch_bounds__(256) void refine_kernel(const SiftPyramid p, const SiftParams prm, const Cand *__restrict__ cand, int n,
                                                     Kp *__restrict__ out)
{
    const int j = (int)(blockIdx.x * 256 + threadIdx.x);
    if (j >= n) return;
    const Cand cd = cand[j];
    const int o = cd.o, h = p.h[o], w = p.w[o];
    const ptrdiff_t px = (ptrdiff_t)h * w;
    const float *d0 = p.dog + p.d_off[o];
    int i = cd.i, r = cd.r, c = cd.c;
    Kp k{};
    k.key = ((unsigned long long)o << 36) | ((unsigned long long)cd.i << 34) | ((unsigned long long)cd.r << 20) |
            ((unsigned long long)cd.c << 6);
    k.o = o;
    const float img_scale = 1.0f / 255.0f, deriv = img_scale * 0.5f, second = img_scale, cross = img_scale * 0.25f;
    float gx = 0, gy = 0, gs = 0, dxx = 0, dyy = 0, dxy = 0, xc = 0, xr = 0, xi = 0, val = 0;
    bool converged = false, alive = true;
    for (int step = 0; step < MAX_STEPS && alive; ++step) {
        const float *q = d0 + i * px + (ptrdiff_t)r * w + c, *pv = q - px, *nx = q + px;
        val = q[0];
        gx = (q[1] - q[-1]) * deriv;
        gy = (q[w] - q[-w]) * deriv;
        gs = (nx[0] - pv[0]) * deriv;
        const float v2 = val * 2.0f;
        dxx = (q[1] + q[-1] - v2) * second;
        dyy = (q[w] + q[-w] - v2) * second;
        const float dss = (nx[0] + pv[0] - v2) * second;
        dxy = (q[w + 1] - q[w - 1] - q[-w + 1] + q[-w - 1]) * cross;
        const float dxs = (nx[1] - nx[-1] - pv[1] + pv[-1]) * cross;
        const float dys = (nx[w] - nx[-w] - pv[w] + pv[-w]) * cross;
        const float c00 = dyy * dss - dys * dys;
        const float c01 = dxs * dys - dxy * dss;
        const float c02 = dxy * dys - dxs * dyy;
        const float det = dxx * c00 + dxy * c01 + dxs * c02;
        if (det == 0.0f) { alive = false; break; }
        const float c11 = dxx * dss - dxs * dxs;
        const float c12 = dxy * dxs - dxx * dys;
        const float c22 = dxx * dyy - dxy * dxy;
        xc = -((c00 * gx + c01 * gy + c02 * gs) / det);
        xr = -((c01 * gx + c11 * gy + c12 * gs) / det);
        xi = -((c02 * gx + c12 * gy + c22 * gs) / det);
        if (!(fabsf(xc) <= 1e6f && fabsf(xr) <= 1e6f && fabsf(xi) <= 1e6f)) { alive = false; break; }
        if (fabsf(xc) < 0.5f && fabsf(xr) < 0.5f && fabsf(xi) < 0.5f) { converged = true; break; }
        c += (int)rintf(xc);
        r += (int)rintf(xr);
        i += (int)rintf(xi);
        if (i < 1 || i > SIFT_LAYERS || c < BORDER || c >= w - BORDER || r < BORDER || r >= h - BORDER) alive = false;
    }
    if (alive && converged) {
        const float t = gx * xc + gy * xr + gs * xi;
        const float contr = val * img_scale + t * 0.5f;
        const float tr = dxx + dyy, det2 = dxx * dyy - dxy * dxy, edge = prm.edge_threshold;
        const bool weak = fabsf(contr) * (float)SIFT_LAYERS < prm.contrast_threshold;
        const bool edgy = det2 <= 0.0f || tr * tr * edge >= (edge + 1.0f) * (edge + 1.0f) * det2;
        if (!weak && !edgy) {
            const float e = ((float)i + xi) * (1.0f / 3.0f);
            const float scl = prm.sigma * sift_expf(e * 0.6931472f);
            const float full = (float)(1 << o), po = full * 0.5f;
            k.valid = 1;
            k.i = i; k.r = r; k.c = c;
            k.x = ((float)c + xc) * po;
            k.y = ((float)r + xr) * po;
            k.size = scl * full;
            k.scl = scl;
            k.response = fabsf(contr);
        }
    }
    out[j] = k;
}

__device__ __forceinline__ const float *gauss_image(const SiftPyramid &p, int o, int i)
{
    return p.gauss + p.g_off[o] + (size_t)i * ((size_t)p.h[o] * p.w[o]);
}

__global__ __launch_bounds__(256) void orient_kernel(const SiftPyramid p, const Kp *__restrict__ kps, int n, Ori *__restrict__ out, int cap,
                                                     int *__restrict__ count)
{
    __shared__ unsigned long long hist[WAVES][ORI_BINS];
    __shared__ float hq[WAVES][ORI_BINS], sm[WAVES][ORI_BINS];
    const int wv = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const int j = (int)blockIdx.x * WAVES + wv;
    const bool live = j < n && kps[j].valid != 0;
    if (lane < ORI_BINS) hist[wv][lane] = 0ull;
    __syncthreads();
    Kp k{};
    if (live) {
        k = kps[j];
        const int h = p.h[k.o], w = p.w[k.o];
        const float *img = gauss_image(p, k.o, k.i);
        const int radius = (int)rintf(4.5f * k.scl), side = 2 * radius + 1, total = side * side;
        const float sp = 1.5f * k.scl, es = -1.0f / ((2.0f * sp) * sp);
        for (int s = lane; s < total; s += 64) {
            const int di = s / side - radius, dj = s % side - radius, y = k.r + di, x = k.c + dj;
            if (y <= 0 || y >= h - 1 || x <= 0 || x >= w - 1) continue;
            const float *q = img + (size_t)y * w + x;
            const float dx = q[1] - q[-1], dy = q[-w] - q[w];
            const float ori = sift_atan2deg(dy, dx), mag = sqrtf(dx * dx + dy * dy);
            const float wgt = sift_expf((float)(di * di + dj * dj) * es);
            int b = (int)rintf(ori * 0.1f);
            if (b >= ORI_BINS) b -= ORI_BINS;
            if (b < 0) b += ORI_BINS;
            atomicAdd(&hist[wv][b], (unsigned long long)(long long)rintf((wgt * mag) * FIX));
        }
    }
    __syncthreads();
    if (lane < ORI_BINS) hq[wv][lane] = (float)(long long)hist[wv][lane] * (1.0f / FIX);
    __syncthreads();
    if (lane < ORI_BINS) {
        const float *g = hq[wv];
        const int b = lane;
        sm[wv][b] = (g[(b + 34) % ORI_BINS] + g[(b + 2) % ORI_BINS]) * 0.0625f + (g[(b + 35) % ORI_BINS] + g[(b + 1) % ORI_BINS]) * 0.25f +
                    g[b] * 0.375f;
    }
    __syncthreads();
    if (live && lane < ORI_BINS) {
        float mx = sm[wv][0];
        for (int b = 1; b < ORI_BINS; ++b) mx = fmaxf(mx, sm[wv][b]);
        const float lf = sm[wv][(lane + 35) % ORI_BINS], ct = sm[wv][lane], rt = sm[wv][(lane + 1) % ORI_BINS];
        if (ct > lf && ct > rt && ct >= 0.8f * mx) {
            float bf = (float)lane + (0.5f * (lf - rt)) / ((lf - 2.0f * ct) + rt);
            if (bf < 0.0f) bf = bf + (float)ORI_BINS;
            if (bf >= (float)ORI_BINS) bf = bf - (float)ORI_BINS;
            float ang = 360.0f - 10.0f * bf;
            if (fabsf(ang - 360.0f) < FLT_EPS) ang = 0.0f;
            const int slot = atomicAdd(count, 1);
            if (slot < cap) {
                Ori r{};
                r.k = k;
                r.k.key = k.key | (unsigned long long)lane;
                r.angle = ang;
                out[slot] = r;
            }
        }
    }
}

// kp [n][6] and desc [n][128] of the keypoints ori[perm[j]], j < n
__global__ __launch_bounds__(256) void describe_kernel(const SiftPyramid p, const Ori *__restrict__ ori, const unsigned *__restrict__ perm,
                                                       int n, float *__restrict__ kp_out, unsigned char *__restrict__ desc_out)
{
    __shared__ unsigned long long hist[WAVES][128];
    const int wv = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const int j = (int)blockIdx.x * WAVES + wv;
    const bool live = j < n;
    hist[wv][lane] = 0ull;
    hist[wv][lane + 64] = 0ull;
    __syncthreads();
    if (live) {
        const Ori kr = ori[perm[j]];
        const Kp &k = kr.k;
        const int h = p.h[k.o], w = p.w[k.o];
        const float *img = gauss_image(p, k.o, k.i);
        float a = 360.0f - kr.angle;
        if (fabsf(a - 360.0f) < FLT_EPS) a = 0.0f;
        float sn, cs;
        sift_sincosdeg(a, &sn, &cs);
        const float hw = 3.0f * k.scl;
        int radius = (int)rintf(hw * 1.4142135f * 2.5f);
        radius = radius < h + w ? radius : h + w;
        cs = cs / hw;
        sn = sn / hw;
        const int side = 2 * radius + 1, total = side * side;
        for (int s = lane; s < total; s += 64) {
            const int di = s / side - radius, dj = s % side - radius, y = k.r + di, x = k.c + dj;
            const float fi = (float)di, fj = (float)dj;
            const float c_rot = fj * cs - fi * sn, r_rot = fj * sn + fi * cs;
            const float rbin = r_rot + 1.5f, cbin = c_rot + 1.5f;
            if (!(rbin > -1.0f && rbin < 4.0f && cbin > -1.0f && cbin < 4.0f) || y <= 0 || y >= h - 1 || x <= 0 || x >= w - 1) continue;
            const float *q = img + (size_t)y * w + x;
            const float dx = q[1] - q[-1], dy = q[-w] - q[w];
            const float og = sift_atan2deg(dy, dx), mag = sqrtf(dx * dx + dy * dy);
            const float wgt = sift_expf((c_rot * c_rot + r_rot * r_rot) * -0.125f);
            const float obin = (og - a) * 0.022222223f;
            const float m = mag * wgt;
            const float r0f = floorf(rbin), c0f = floorf(cbin), o0f = floorf(obin);
            const float fr = rbin - r0f, fc = cbin - c0f, fo = obin - o0f;
            const int r0 = (int)r0f, c0 = (int)c0f, o0 = ((int)o0f) & 7;          // mod 8 into 0 .. 7
            const float v1 = m * fr, v0 = m - v1;
            const float v11 = v1 * fc, v10 = v1 - v11, v01 = v0 * fc, v00 = v0 - v01;
            const float vrc[4] = {v00, v01, v10, v11};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int rr = r0 + (t >> 1), cc = c0 + (t & 1);
                if (rr < 0 || rr > 3 || cc < 0 || cc > 3) continue;
                const float hi = vrc[t] * fo, lo = vrc[t] - hi;
                unsigned long long *cell = &hist[wv][(rr * 4 + cc) * 8];
                atomicAdd(cell + o0, (unsigned long long)(long long)rintf(lo * FIX));
                atomicAdd(cell + ((o0 + 1) & 7), (unsigned long long)(long long)rintf(hi * FIX));
            }
        }
        if (lane == 0) {
            float *row = kp_out + (size_t)j * 6;
            row[0] = k.x; row[1] = k.y; row[2] = k.size; row[3] = kr.angle; row[4] = k.response;
            row[5] = (float)(k.o + 256 * k.i);
        }
    }
    __syncthreads();
    if (live) {
        // every lane sums the 128 squares serially, in bin order (LDS broadcasts): one sum, in the header's order
        const unsigned long long *hh = hist[wv];
        float v = (float)(long long)hh[0] * (1.0f / FIX);
        float acc = v * v;
        for (int b = 1; b < 128; ++b) {
            v = (float)(long long)hh[b] * (1.0f / FIX);
            acc = acc + v * v;
        }
        const float thr = sqrtf(acc) * 0.2f;
        v = fminf((float)(long long)hh[0] * (1.0f / FIX), thr);
        acc = v * v;
        for (int b = 1; b < 128; ++b) {
            v = fminf((float)(long long)hh[b] * (1.0f / FIX), thr);
            acc = acc + v * v;
        }
        const float scale = 512.0f / fmaxf(sqrtf(acc), FLT_EPS);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int b = lane + 64 * t;
            const int u = (int)rintf(fminf((float)(long long)hh[b] * (1.0f / FIX), thr) * scale);
            desc_out[(size_t)j * 128 + b] = (unsigned char)(u < 255 ? u : 255);
        }
    }
}

__global__ __launch_bounds__(256) void canonical_keys_kernel(const Ori *__restrict__ ori, int n, unsigned long long *__restrict__ keys,
                                                             unsigned *__restrict__ idx)
{
    const int j = (int)(blockIdx.x * 256 + threadIdx.x);
    if (j >= n) return;
    keys[j] = ori[j].k.key;
    idx[j] = (unsigned)j;
}

// (response descending, canonical index ascending) as one ascending 64-bit key: a response is not negative, so its bits
// order as it does
__global__ __launch_bounds__(256) void response_keys_kernel(const Ori *__restrict__ ori, const unsigned *__restrict__ perm, int n,
                                                            unsigned long long *__restrict__ keys)
{
    const int j = (int)(blockIdx.x * 256 + threadIdx.x);
    if (j >= n) return;
    const unsigned bits = (unsigned)__float_as_int(ori[perm[j]].k.response);
    keys[j] = ((unsigned long long)(~bits) << 32) | (unsigned)j;
}

__global__ __launch_bounds__(256) void low_words_kernel(const unsigned long long *__restrict__ keys, int n, unsigned *__restrict__ out)
{
    const int j = (int)(blockIdx.x * 256 + threadIdx.x);
    if (j < n) out[j] = (unsigned)(keys[j] & 0xffffffffull);
}

__global__ __launch_bounds__(256) void gather_kernel(const unsigned *__restrict__ perm, const unsigned *__restrict__ sel, int n,
                                                     unsigned *__restrict__ out)
{
    const int j = (int)(blockIdx.x * 256 + threadIdx.x);
    if (j < n) out[j] = perm[sel[j]];
}

unsigned blocks_for(long long n, int per = 256)
{
    const long long b = (n + per - 1) / per;
    return (unsigned)(b < 1 ? 1 : b);
}

template <class K, class V>
hipError_t sort_pairs(const K *kin, K *kout, const V *vin, V *vout, int n, ScratchCache &cache, ScratchCache::Lease &tmp, hipStream_t st)
{
    size_t bytes = 0;
    KCHK(rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, (size_t)n, 0, 8 * sizeof(K), st));
    KCHK(cache.lease(tmp, bytes));
    return rocprim::radix_sort_pairs(tmp.get(), bytes, kin, kout, vin, vout, (size_t)n, 0, 8 * sizeof(K), st);
}

template <class K>
hipError_t sort_keys(const K *kin, K *kout, int n, ScratchCache &cache, ScratchCache::Lease &tmp, hipStream_t st)
{
    size_t bytes = 0;
    KCHK(rocprim::radix_sort_keys(nullptr, bytes, kin, kout, (size_t)n, 0, 8 * sizeof(K), st));
    KCHK(cache.lease(tmp, bytes));
    return rocprim::radix_sort_keys(tmp.get(), bytes, kin, kout, (size_t)n, 0, 8 * sizeof(K), st);
}

}  // namespace

hipError_t sift_keypoints(SiftState &s, const SiftParams &prm, int n_features, int max_features, ScratchCache &cache, bool *too_many,
                          hipStream_t st)
{
    *too_many = false;
    s.n_kp = -1;
    SiftPyramid p{};
    p.gauss = s.gauss.get();
    p.dog = s.dog.get();
    p.n_octaves = s.n_octaves;
    for (int o = 0; o < s.n_octaves; ++o) {
        p.h[o] = s.h[o]; p.w[o] = s.w[o];
        p.g_off[o] = s.g_off[o]; p.d_off[o] = s.d_off[o];
    }
    ScratchCache::Lease counter, cand, kps, ori, keys_a, keys_b, idx_a, idx_b, idx_c, tmp;
    KCHK(cache.lease(counter, sizeof(int)));
    int *count = counter.get<int>();

    // candidates: search, and search again with room for all of them if the first array was too small
    int n_cand = 0;
    for (long long cap = 1 << 14;;) {
        KCHK(cache.lease(cand, (size_t)cap * sizeof(Cand)));
        KCHK(hipMemsetAsync(count, 0, sizeof(int), st));
        for (int o = 0; o < s.n_octaves; ++o) {
            if (s.h[o] <= 2 * BORDER || s.w[o] <= 2 * BORDER) continue;
            const long long n = 3ll * (s.h[o] - 2 * BORDER) * (s.w[o] - 2 * BORDER);
            const long long b = (n + 255) / 256;
            hipLaunchKernelGGL(extrema_kernel, dim3((unsigned)(b < MAX_BLOCKS ? b : MAX_BLOCKS)), dim3(256), 0, st, p, o, prm.pre_threshold,
                               cand.get<Cand>(), (int)cap, count);
            KCHK(hipGetLastError());
        }
        KCHK(hipMemcpyAsync(&n_cand, count, sizeof(int), hipMemcpyDeviceToHost, st));
        KCHK(hipStreamSynchronize(st));
        if (n_cand <= cap) break;
        cap = n_cand;
    }

    int n_ori = 0;
    if (n_cand > 0) {
        KCHK(cache.lease(kps, (size_t)n_cand * sizeof(Kp)));
        hipLaunchKernelGGL(refine_kernel, dim3(blocks_for(n_cand)), dim3(256), 0, st, p, prm, cand.get<Cand>(), n_cand, kps.get<Kp>());
        KCHK(hipGetLastError());
        for (long long cap = 2ll * n_cand + 64;;) {
            KCHK(cache.lease(ori, (size_t)cap * sizeof(Ori)));
            KCHK(hipMemsetAsync(count, 0, sizeof(int), st));
            hipLaunchKernelGGL(orient_kernel, dim3(blocks_for(n_cand, WAVES)), dim3(256), 0, st, p, kps.get<Kp>(), n_cand, ori.get<Ori>(),
                               (int)cap, count);
            KCHK(hipGetLastError());
            KCHK(hipMemcpyAsync(&n_ori, count, sizeof(int), hipMemcpyDeviceToHost, st));
            KCHK(hipStreamSynchronize(st));
            if (n_ori <= cap) break;
            cap = n_ori;
        }
    }
    if (n_ori > max_features) {
        *too_many = true;
        return hipSuccess;
    }
    int n_out = n_ori;
    if (n_ori > 0) {
        const size_t n = (size_t)n_ori;
        KCHK(cache.lease(keys_a, n * 8));
        KCHK(cache.lease(keys_b, n * 8));
        KCHK(cache.lease(idx_a, n * 4));
        KCHK(cache.lease(idx_b, n * 4));
        unsigned long long *ka = keys_a.get<unsigned long long>(), *kb = keys_b.get<unsigned long long>();
        unsigned *ia = idx_a.get<unsigned>(), *perm = idx_b.get<unsigned>();
        hipLaunchKernelGGL(canonical_keys_kernel, dim3(blocks_for(n_ori)), dim3(256), 0, st, ori.get<Ori>(), n_ori, ka, ia);
        KCHK(hipGetLastError());
        KCHK(sort_pairs(ka, kb, ia, perm, n_ori, cache, tmp, st));                   // perm: canonical index -> record
        if (n_features > 0 && n_ori > n_features) {
            n_out = n_features;
            KCHK(cache.lease(idx_c, n * 4));
            hipLaunchKernelGGL(response_keys_kernel, dim3(blocks_for(n_ori)), dim3(256), 0, st, ori.get<Ori>(), perm, n_ori, ka);
            KCHK(hipGetLastError());
            KCHK(sort_keys(ka, kb, n_ori, cache, tmp, st));
            hipLaunchKernelGGL(low_words_kernel, dim3(blocks_for(n_out)), dim3(256), 0, st, kb, n_out, ia);
            KCHK(hipGetLastError());
            unsigned *sel = idx_c.get<unsigned>();
            KCHK(sort_keys(ia, sel, n_out, cache, tmp, st));                         // the kept canonical indices, ascending
            hipLaunchKernelGGL(gather_kernel, dim3(blocks_for(n_out)), dim3(256), 0, st, perm, sel, n_out, ia);
            KCHK(hipGetLastError());
            perm = ia;
        }
        KCHK(s.kp.reserve((size_t)n_out * 6, cache));
        KCHK(s.desc.reserve((size_t)n_out * 8, cache));
        hipLaunchKernelGGL(describe_kernel, dim3(blocks_for(n_out, WAVES)), dim3(256), 0, st, p, ori.get<Ori>(), perm, n_out, s.kp.get(),
                           (unsigned char *)s.desc.get());
        KCHK(hipGetLastError());
        KCHK(hipStreamSynchronize(st));
    }
    s.n_kp = n_out;
    return hipSuccess;
}

}  // namespace amvs
