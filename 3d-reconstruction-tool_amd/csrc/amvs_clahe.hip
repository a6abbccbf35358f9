// amvs_clahe.hip -- CLAHE on a gray 8-bit image (include/amvs_features.h; the definition is the header's, judged against
// tests/features_restatement.py byte for byte; parity with cv2 is UNPINNED).
//
// clahe_lut_kernel: one workgroup of 256 lanes per tile.  The lanes walk the tile's pixels of the padded image (the
// padding is never stored: a padded pixel is read through the folded reflection) and count them into a 256-bin
// histogram in LDS with integer atomics, whose result does not depend on arrival order.  Then the first wave alone
// clips, redistributes and integrates: lane l owns bins 4 l .. 4 l + 3, the excess is summed across the wave by
// shuffles, the residual's bins k * step have a closed form, and the cumulative sum is a wave scan of the lanes' four-bin
// totals.  All of it is integer arithmetic but the final float32 product and rint.
//
// clahe_apply_kernel: one lane per pixel; the four LUT bytes are gathers from a table of grid_x * grid_y * 256 bytes
// that stays in cache.
//
// -ffp-contract=off (Makefile): a * b + c below is two roundings, as the header says.
#include "amvs_features_state.h"

namespace amvs {

namespace {

__global__ __launch_bounds__(256) void clahe_lut_kernel(const unsigned char *__restrict__ gray, int h, int w, int tw, int th,
                                                        int grid_x, int limit, unsigned char *__restrict__ lut)
{
    __shared__ int hist[256];
    const int tile = (int)blockIdx.x, ty = tile / grid_x, tx = tile - ty * grid_x;
    const int lane = (int)threadIdx.x;
    hist[lane] = 0;
    __syncthreads();
    const int area = tw * th;
    for (int p = lane; p < area; p += 256) {
        const int py = p / tw, px = p - py * tw;
        const int y = fold101(ty * th + py, h), x = fold101(tx * tw + px, w);       // inside [0, h) x [0, w) by construction
        atomicAdd(&hist[gray[(size_t)y * w + x]], 1);
    }
    __syncthreads();
    if (lane >= 64) return;
    int b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = hist[4 * lane + k];
    if (limit > 0) {
        int excess = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            excess += b[k] > limit ? b[k] - limit : 0;
            b[k] = b[k] < limit ? b[k] : limit;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) excess += __shfl_xor(excess, d);
        const int batch = excess / 256, residual = excess - 256 * batch;
        const int step = residual > 0 ? 256 / residual : 256;       // residual < 256: step >= 1
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int v = 4 * lane + k;
            b[k] += batch + ((residual > 0 && v % step == 0 && v / step < residual) ? 1 : 0);
        }
    }
    // inclusive scan of the lanes' totals, then the four running sums of the lane
    const int own = b[0] + b[1] + b[2] + b[3];
    int run = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(run, d);
        if (lane >= d) run += up;
    }
    int c = run - own;
    const float scale = 255.0f / (float)area;
    unsigned char *q = lut + (size_t)tile * 256 + 4 * lane;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c += b[k];
        const int v = (int)rintf((float)c * scale);
        q[k] = (unsigned char)(v < 255 ? v : 255);
    }
}

__global__ __launch_bounds__(256) void clahe_apply_kernel(const unsigned char *__restrict__ gray, int h, int w, int tw, int th,
                                                          int grid_x, int grid_y, const unsigned char *__restrict__ lut,
                                                          unsigned char *__restrict__ out)
{
    const float inv_tw = 1.0f / (float)tw, inv_th = 1.0f / (float)th;
    const long long n = (long long)h * w;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int y = (int)(i / w), x = (int)(i - (long long)y * w);
        const float fy = (float)y * inv_th - 0.5f, fx = (float)x * inv_tw - 0.5f;
        const float y1f = floorf(fy), x1f = floorf(fx);
        const float ya = fy - y1f, xa = fx - x1f, ya1 = 1.0f - ya, xa1 = 1.0f - xa;
        int y1 = (int)y1f, x1 = (int)x1f;                          // -1 .. grid - 1
        const int y2 = y1 + 1 < grid_y - 1 ? y1 + 1 : grid_y - 1, x2 = x1 + 1 < grid_x - 1 ? x1 + 1 : grid_x - 1;
        y1 = y1 > 0 ? y1 : 0;
        x1 = x1 > 0 ? x1 : 0;
        y1 = y1 < grid_y - 1 ? y1 : grid_y - 1;                     // (cannot bite: y < h <= grid_y * th; keeps the gather inside
        x1 = x1 < grid_x - 1 ? x1 : grid_x - 1;                     //  the table whatever the rounding of y * inv_th)
        const int v = gray[i];
        const float l11 = (float)lut[((size_t)y1 * grid_x + x1) * 256 + v], l12 = (float)lut[((size_t)y1 * grid_x + x2) * 256 + v];
        const float l21 = (float)lut[((size_t)y2 * grid_x + x1) * 256 + v], l22 = (float)lut[((size_t)y2 * grid_x + x2) * 256 + v];
        const float r = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya;
        const int o = (int)rintf(r);
        out[i] = (unsigned char)(o < 0 ? 0 : (o > 255 ? 255 : o));
    }
}

constexpr long long MAX_BLOCKS = 8192;

}  // namespace

hipError_t launch_clahe_luts(const unsigned char *gray, int h, int w, int grid_x, int grid_y, int limit, unsigned char *lut,
                             hipStream_t st)
{
    const int tw = (w + grid_x - 1) / grid_x, th = (h + grid_y - 1) / grid_y;
    hipLaunchKernelGGL(clahe_lut_kernel, dim3((unsigned)(grid_x * grid_y)), dim3(256), 0, st, gray, h, w, tw, th, grid_x, limit, lut);
    return hipGetLastError();
}

hipError_t launch_clahe_apply(const unsigned char *gray, int h, int w, int grid_x, int grid_y, const unsigned char *lut,
                              unsigned char *out, hipStream_t st)
{
    const int tw = (w + grid_x - 1) / grid_x, th = (h + grid_y - 1) / grid_y;
    const long long blocks = ((long long)h * w + 255) / 256;
    hipLaunchKernelGGL(clahe_apply_kernel, dim3((unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS)), dim3(256), 0, st, gray, h, w,
                       tw, th, grid_x, grid_y, lut, out);
    return hipGetLastError();
}

}  // namespace amvs
