// amvs_sift.hip -- the Gaussian / difference-of-Gaussian scale space of SIFT (include/amvs_features.h; the definition is
// the header's, judged against tests/features_restatement.py bit for bit; parity with cv2 is UNPINNED, DESIGN.md
// section 19).  The stage is bandwidth-bound: a blur reads and writes every pixel of a level twice.
//
// blur_rows_kernel: a workgroup of 256 lanes takes a tile of 256 columns x 4 rows.  The rows are staged in LDS with a
// halo of r pixels on each side, read through the folded reflection, so one code path serves every radius, also a
// radius beyond the image side; lane l then sums the 2 r + 1 taps of column l from LDS, serially in tap order.
// blur_cols_kernel: a tile of 64 columns x 64 rows; its 64 + 2 r source rows (folded) are staged in LDS, a wave reads
// one LDS row at consecutive columns (no bank conflict), and every lane sums 16 output pixels of its column.  It writes
// the Gaussian image and, from the same registers, its difference with the previous image of the octave: no level is
// read back just to be subtracted.  The taps arrive in the argument block and are read with scalar loads.
//
// -ffp-contract=off (Makefile): tap * value + acc below is two roundings, as the header says.
#include "amvs_features_state.h"

namespace amvs {

namespace {

constexpr int ROW_TILE_W = 256, ROW_TILE_H = 4, COL_TILE_W = 64, COL_TILE_H = 64, COL_ROWS_PER_LANE = 16;
constexpr long long MAX_BLOCKS = 1024;              // of the grid-stride kernels: four workgroups a compute unit

__global__ __launch_bounds__(256) void upsample_kernel(const unsigned char *__restrict__ gray, int h, int w, float *__restrict__ up)
{
    const int W2 = 2 * w;
    const long long n = 4ll * h * w;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int y = (int)(i / W2), x = (int)(i - (long long)y * W2);
        const int ky = y >> 1, kx = x >> 1;
        const int fy = (y & 1) ? (ky + 1 < h - 1 ? ky + 1 : h - 1) : (ky - 1 > 0 ? ky - 1 : 0);
        const int fx = (x & 1) ? (kx + 1 < w - 1 ? kx + 1 : w - 1) : (kx - 1 > 0 ? kx - 1 : 0);
        const unsigned char *pn = gray + (size_t)ky * w, *pf = gray + (size_t)fy * w;
        const float rn = 0.75f * (float)pn[kx] + 0.25f * (float)pn[fx];
        const float rf = 0.75f * (float)pf[kx] + 0.25f * (float)pf[fx];
        up[i] = 0.75f * rn + 0.25f * rf;
    }
}

__global__ __launch_bounds__(256) void blur_rows_kernel(const float *__restrict__ in, int h, int w, const GaussTaps taps,
                                                        float *__restrict__ out)
{
    __shared__ float tile[ROW_TILE_H][ROW_TILE_W + 2 * SIFT_MAX_RADIUS];
    const int r = taps.r, lane = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * ROW_TILE_W, y0 = (int)blockIdx.y * ROW_TILE_H;
    const int span = ROW_TILE_W + 2 * r;                  // <= the tile's width: r <= SIFT_MAX_RADIUS
#pragma unroll
    for (int k = 0; k < ROW_TILE_H; ++k) {
        const int y = y0 + k;
        if (y < h)
            for (int s = lane; s < span; s += 256) tile[k][s] = in[(size_t)y * w + fold101(x0 - r + s, w)];
    }
    __syncthreads();
    const int x = x0 + lane;
    if (x >= w) return;
#pragma unroll
    for (int k = 0; k < ROW_TILE_H; ++k) {
        const int y = y0 + k;
        if (y >= h) break;
        float acc = taps.w[0] * tile[k][lane];
        for (int j = 1; j <= 2 * r; ++j) acc = acc + taps.w[j] * tile[k][lane + j];
        out[(size_t)y * w + x] = acc;
    }
}

__global__ __launch_bounds__(256) void blur_cols_kernel(const float *__restrict__ in, int h, int w, const GaussTaps taps,
                                                        float *__restrict__ out, const float *__restrict__ prev,
                                                        float *__restrict__ dog)
{
    __shared__ float tile[COL_TILE_H + 2 * SIFT_MAX_RADIUS][COL_TILE_W];
    const int r = taps.r, lx = (int)(threadIdx.x & 63u), grp = (int)(threadIdx.x >> 6);
    const int x = (int)blockIdx.x * COL_TILE_W + lx, y0 = (int)blockIdx.y * COL_TILE_H;
    const int span = COL_TILE_H + 2 * r;                  // <= the tile's height
    if (x < w)
        for (int s = grp; s < span; s += 4) tile[s][lx] = in[(size_t)fold101(y0 - r + s, h) * w + x];
    __syncthreads();
    if (x >= w) return;
    for (int k = 0; k < COL_ROWS_PER_LANE; ++k) {
        const int oy = grp * COL_ROWS_PER_LANE + k, y = y0 + oy;
        if (y >= h) break;
        float acc = taps.w[0] * tile[oy][lx];
        for (int j = 1; j <= 2 * r; ++j) acc = acc + taps.w[j] * tile[oy + j][lx];
        const size_t i = (size_t)y * w + x;
        out[i] = acc;
        if (dog) dog[i] = acc - prev[i];
    }
}

__global__ __launch_bounds__(256) void halve_kernel(const float *__restrict__ in, int w, int h2, int w2, float *__restrict__ out)
{
    const long long n = (long long)h2 * w2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int y = (int)(i / w2), x = (int)(i - (long long)y * w2);
        out[i] = in[(size_t)(2 * y) * w + 2 * x];           // 2 y <= h - 1 and 2 x <= w - 1: h2 = h / 2, w2 = w / 2
    }
}

unsigned stride_blocks(long long n)
{
    const long long blocks = (n + 255) / 256;
    return (unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
}

}  // namespace

hipError_t launch_sift_upsample(const unsigned char *gray, int h, int w, float *up, hipStream_t st)
{
    hipLaunchKernelGGL(upsample_kernel, dim3(stride_blocks(4ll * h * w)), dim3(256), 0, st, gray, h, w, up);
    return hipGetLastError();
}

hipError_t launch_sift_blur(const float *in, int h, int w, const GaussTaps &taps, float *tmp, float *out, const float *prev,
                            float *dog, hipStream_t st)
{
    if (taps.r < 0 || taps.r > SIFT_MAX_RADIUS) return hipErrorInvalidValue;      // the LDS tiles hold SIFT_MAX_RADIUS of halo
    hipLaunchKernelGGL(blur_rows_kernel, dim3((unsigned)((w + ROW_TILE_W - 1) / ROW_TILE_W), (unsigned)((h + ROW_TILE_H - 1) / ROW_TILE_H)),
                       dim3(256), 0, st, in, h, w, taps, tmp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(blur_cols_kernel, dim3((unsigned)((w + COL_TILE_W - 1) / COL_TILE_W), (unsigned)((h + COL_TILE_H - 1) / COL_TILE_H)),
                       dim3(256), 0, st, tmp, h, w, taps, out, prev, dog);
    return hipGetLastError();
}

hipError_t launch_sift_halve(const float *in, int h, int w, float *out, hipStream_t st)
{
    hipLaunchKernelGGL(halve_kernel, dim3(stride_blocks((long long)(h / 2) * (w / 2))), dim3(256), 0, st, in, w, h / 2, w / 2, out);
    return hipGetLastError();
}

}  // namespace amvs
