// amvs_mesh_texture.hip -- a texture atlas of the current mesh taken from the images of the views that see it, its UVs,
// and the current render shaded with the atlas (include/amvs.h amvs_mesh_texture, amvs_fetch_mesh_texture,
// amvs_fetch_render_texture).  No reference counterpart.  Judged against tests/mesh_texture_restatement.py, a NumPy
// statement of the definitions in the header with the same float32 operations in the same order (bit-identical atlas,
// UVs, counts and pictures).
//
// The parameterisation is a fixed right triangle of N texel intervals per leg for every face, two faces to a square cell
// of C = N + 3 texels, the odd face mirrored through the cell's centre: no chart growing, no packing, and a texel's
// owner follows from its position alone.
//
// No float atomics, and no result that depends on arrival order: a texel slot belongs to one lane, which walks the views
// in ascending order in registers, and a pixel of the textured render to one lane.  The only atomic is the integer count
// of the texels a view reached, one add per wave.
//
// texture_kernel, one lane per texel slot in CELL order (slot t -> cell t / C^2, then row and column within the cell), not
// in the atlas's row order: a wave then holds neighbouring points of one or two faces, so the face's ids and corners are
// a few cache lines for all its lanes, and the depth and image gathers of the walk fall on neighbouring pixels, as
// color_views_kernel relies on for neighbouring vertices.  A lane whose slot is in no face's set stores zeros.  The
// cameras are uniform loads, the views run in a register loop, and image bytes are loaded only for the views that passed
// every test.
//
// The walk over the views (steps a to f of amvs_mesh_color_views) is stated here a second time, word for word as in
// color_views_kernel: moved into a header that both units include it compiled, in amvs_mesh_color.hip, to the same
// instructions with two scalar registers exchanged and one loop latch reordered, which is not identical, so that unit
// stayed as it was (DESIGN.md section 8 "Texture").
//
// uv_kernel, one lane per face.  render_texture_kernel, one lane per pixel of the asked views, beside
// render_color_kernel in structure: the face the rasteriser left there is set up again by face_setup, the edge functions
// give the perspective-correct position in the face's triangle of texels, and the atlas is sampled bilinearly there.
#define AMVS_TU_ID 14
#include "amvs_check.h"
#include "amvs_kernels.h"
#include "amvs_mesh_state.h"
#include "amvs_mesh_project.h"

namespace amvs {

namespace {

// round half up, clamped to a byte
__device__ __forceinline__ unsigned char color_u8(float q)
{
    return (unsigned char)fminf(255.0f, fmaxf(0.0f, floorf(q + 0.5f)));
}

// Steps a to f of amvs_mesh_color_views for the point (X, Y, Z) with the normal (nx, ny, nz).  Returns whether a view was
// reached; then acc holds S_ch of the blend or the val of the best view (B, G, R) and wsum the sum of the weights or the
// largest.  bgr: [bgr_pixels][3], image slot[m] belongs to rendered view m.
template <bool BEST>
__device__ __forceinline__ bool walk_views(float X, float Y, float Z, float nx, float ny, float nz, const float *__restrict__ cams,
                                           const Kmat &K, int n_views, int H, int W, float near, float tolerance, float min_cos,
                                           const float *__restrict__ depth, long long map_elems,
                                           const unsigned char *__restrict__ bgr, long long bgr_pixels,
                                           const int *__restrict__ slot, float acc[3], float &wsum)
{
    bool reached = false;
    const long long hw = (long long)H * W;
    const float last_x = (float)(W - 1), last_y = (float)(H - 1);
    acc[0] = acc[1] = acc[2] = 0.0f;
    wsum = 0.0f;
    for (int m = 0; m < n_views; ++m) {
        const float *P = cams + 12 * m;
        const Projected p = project(P, K, X, Y, Z);
        if (!(p.zc > near)) continue;
        const float x0 = floorf(p.u), y0 = floorf(p.v);
        if (!(x0 >= 0.0f && x0 < last_x && y0 >= 0.0f && y0 < last_y)) continue;      // false for NaN
        const float ax = p.u - x0, ay = p.v - y0;
        const long long pix = (long long)(int)y0 * W + (int)x0;
        const long long tap[4] = {pix, pix + 1, pix + W, pix + W + 1};
        bool clear = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = depth[AMVS_IDX(m * hw + tap[k], map_elems)];
            clear = clear && d > 0.0f && p.zc <= d + tolerance && d <= p.zc + tolerance;
        }
        if (!clear) continue;
        const float ncx = (P[0] * nx + P[1] * ny) + P[2] * nz;
        const float ncy = (P[3] * nx + P[4] * ny) + P[5] * nz;
        const float ncz = (P[6] * nx + P[7] * ny) + P[8] * nz;
        const float dot = (ncx * p.xc + ncy * p.yc) + ncz * p.zc;
        const float len = sqrtf((p.xc * p.xc + p.yc * p.yc) + p.zc * p.zc);
        const float w = (-dot) / len;
        if (!(w > min_cos)) continue;                                                  // false for NaN
        if (BEST && reached && !(w > wsum)) continue;                                   // a tie stays with the lower view
        const long long image = (long long)slot[m] * hw;
        long long q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = 3 * AMVS_IDX(image + tap[k], bgr_pixels);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float f00 = (float)bgr[q[0] + ch], f10 = (float)bgr[q[1] + ch];
            const float f01 = (float)bgr[q[2] + ch], f11 = (float)bgr[q[3] + ch];
            const float top = f00 + ax * (f10 - f00);
            const float bot = f01 + ax * (f11 - f01);
            const float val = top + ay * (bot - top);
            acc[ch] = BEST ? val : acc[ch] + w * val;
        }
        wsum = BEST ? w : wsum + w;
        reached = true;
    }
    return reached;
}

// atlas: [Ht][Wt][3] RGB with Wt = cols * C, Ht = rows * C, C = N + 3; slots = rows * cols * C * C, every one written once
template <bool BEST>
__global__ __launch_bounds__(256) void texture_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                      const unsigned char *__restrict__ rgb, long long n_vertices, long long n_faces,
                                                      const float *__restrict__ cams, Kmat K, int n_views, int H, int W, float near,
                                                      float tolerance, float min_cos, const float *__restrict__ depth,
                                                      long long map_elems, const unsigned char *__restrict__ bgr,
                                                      long long bgr_pixels, const int *__restrict__ slot, int N, int cols,
                                                      long long slots, unsigned char *__restrict__ atlas,
                                                      unsigned long long *__restrict__ n_textured)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool reached = false;
    if (t < slots) {
        const int C = N + 3, cc = C * C;
        const long long cell = t / cc;
        const int r = (int)(t - cell * cc);
        const int ly = r / C, lx = r - ly * C;
        const bool odd = lx + ly > N + 2;                             // the diagonal lx + ly = N + 2 belongs to nobody
        const int i = odd ? C - 1 - lx : lx, j = odd ? C - 1 - ly : ly;
        const long long f = 2 * cell + (odd ? 1 : 0);
        const long long wt = (long long)cols * C;
        const long long at = 3 * AMVS_IDX(((cell / cols) * C + ly) * wt + (cell % cols) * C + lx, slots);
        unsigned char out[3] = {0, 0, 0};                             // R, G, B
        if (i <= N && j <= N && i + j <= N + 1 && f < n_faces) {
            const long long i0 = AMVS_IDX((long long)faces[3 * f], n_vertices);
            const long long i1 = AMVS_IDX((long long)faces[3 * f + 1], n_vertices);
            const long long i2 = AMVS_IDX((long long)faces[3 * f + 2], n_vertices);
            const float x0 = verts[3 * i0], y0 = verts[3 * i0 + 1], z0 = verts[3 * i0 + 2];
            const float x1 = verts[3 * i1], y1 = verts[3 * i1 + 1], z1 = verts[3 * i1 + 2];
            const float x2 = verts[3 * i2], y2 = verts[3 * i2 + 1], z2 = verts[3 * i2 + 2];
            const float fn = (float)N;
            const float b1 = (float)i / fn, b2 = (float)j / fn, b0 = (1.0f - b1) - b2;
            const float X = (b0 * x0 + b1 * x1) + b2 * x2;
            const float Y = (b0 * y0 + b1 * y1) + b2 * y2;
            const float Z = (b0 * z0 + b1 * z1) + b2 * z2;
            // the face's normal, formed as amvs_mesh_normals forms it
            const float ax = x1 - x0, ay = y1 - y0, az = z1 - z0;
            const float bx = x2 - x0, by = y2 - y0, bz = z2 - z0;
            float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
            const float l = sqrtf((nx * nx + ny * ny) + nz * nz);
            if (l > 0.0f) { nx = nx / l; ny = ny / l; nz = nz / l; }
            else { nx = 0.0f; ny = 0.0f; nz = 0.0f; }
            float acc[3], wsum;
            reached = walk_views<BEST>(X, Y, Z, nx, ny, nz, cams, K, n_views, H, W, near, tolerance, min_cos, depth, map_elems, bgr,
                                       bgr_pixels, slot, acc, wsum);
            if (reached) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) out[2 - ch] = color_u8(BEST ? acc[ch] : acc[ch] / wsum);
            } else {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    out[ch] = color_u8((b0 * (float)rgb[3 * i0 + ch] + b1 * (float)rgb[3 * i1 + ch]) + b2 * (float)rgb[3 * i2 + ch]);
            }
        }
        atlas[at] = out[0];
        atlas[at + 1] = out[1];
        atlas[at + 2] = out[2];
    }
    const unsigned long long done = __ballot(reached);
    if (done && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)done) - 1)) atomicAdd(n_textured, (unsigned long long)__popcll(done));
}

// uv: [F][3][2], corner k at the atlas texel of its face's texel (0,0), (N,0), (0,N)
__global__ __launch_bounds__(256) void uv_kernel(long long n_faces, int N, int cols, int Wt, int Ht, float *__restrict__ uv)
{
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_faces) return;
    const int C = N + 3;
    const long long cell = f >> 1;
    const int cx = (int)(cell % cols) * C, cy = (int)(cell / cols) * C;
    const bool odd = (f & 1) != 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = k == 1 ? N : 0, j = k == 2 ? N : 0;
        const int X = odd ? cx + C - 1 - i : cx + i, Y = odd ? cy + C - 1 - j : cy + j;
        uv[6 * f + 2 * k] = ((float)X + 0.5f) / (float)Wt;
        uv[6 * f + 2 * k + 1] = 1.0f - ((float)Y + 0.5f) / (float)Ht;
    }
}

// out: [count][H][W][3] RGB of the views first .. first + count - 1
__global__ __launch_bounds__(256) void render_texture_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                             const unsigned char *__restrict__ atlas, long long n_vertices,
                                                             long long n_faces, const float *__restrict__ cams, Kmat K, int first,
                                                             long long pixels, int H, int W, float near,
                                                             const float *__restrict__ depth, const int *__restrict__ face, int N,
                                                             int cols, long long texels, unsigned char *__restrict__ out)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pixels) return;
    const long long hw = (long long)H * W;
    const int view = first + (int)(p / hw);
    const int pix = (int)(p % hw);
    const long long at = (long long)view * hw + pix;
    float q[3] = {0.0f, 0.0f, 0.0f};
    const int id = face[at];
    FaceSetup s;
    if (id >= 0) {
        const long long f = AMVS_IDX((long long)id, n_faces);
        if (face_setup(verts, faces, f, n_vertices, cams + 12 * (long long)view, K, near, H, W, s) == FACE_DRAWS) {
            const int fx = (pix % W) << SUB_SHIFT, fy = (pix / W) << SUB_SHIFT;
            long long w0, w1, w2;
            edge_inside(s.x1, s.y1, s.x2, s.y2, fx, fy, w0);
            edge_inside(s.x2, s.y2, s.x0, s.y0, fx, fy, w1);
            edge_inside(s.x0, s.y0, s.x1, s.y1, fx, fy, w2);
            const float a = (float)s.area;
            const float b1 = (float)w1 / a, b2 = (float)w2 / a;
            const float z = depth[at];
            const float e1 = z * (b1 * s.iz1), e2 = z * (b2 * s.iz2);
            const float g1 = s.flip ? e2 : e1, g2 = s.flip ? e1 : e2;
            const float fn = (float)N;
            const float x = fminf(fmaxf(g1 * fn, 0.0f), fn), y = fminf(fmaxf(g2 * fn, 0.0f), fn);
            const int i = min((int)floorf(x), N - 1);
            int j = min((int)floorf(y), N - 1);
            const float ax = x - (float)i;
            float ay = y - (float)j;
            if (i + j >= N) { j = N - 1 - i; ay = 1.0f; }            // on the hypotenuse within rounding
            const int C = N + 3;
            const long long cell = f >> 1, wt = (long long)cols * C;
            const bool odd = (f & 1) != 0;
            const long long cx = (cell % cols) * C, cy = (cell / cols) * C;
            // the face's texel (i, j); one step in i or j is one texel right or down for an even face, left or up for an odd
            const long long base = odd ? (cy + C - 1 - j) * wt + cx + C - 1 - i : (cy + j) * wt + cx + i;
            const long long sx = odd ? -1 : 1, sy = odd ? -wt : wt;
            const long long t00 = 3 * AMVS_IDX(base, texels), t10 = 3 * AMVS_IDX(base + sx, texels);
            const long long t01 = 3 * AMVS_IDX(base + sy, texels), t11 = 3 * AMVS_IDX(base + sy + sx, texels);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float f00 = (float)atlas[t00 + ch], f10 = (float)atlas[t10 + ch];
                const float f01 = (float)atlas[t01 + ch], f11 = (float)atlas[t11 + ch];
                const float top = f00 + ax * (f10 - f00);
                const float bot = f01 + ax * (f11 - f01);
                q[ch] = top + ay * (bot - top);
            }
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[3 * p + ch] = color_u8(q[ch]);
}

}  // namespace

bool mesh_has_texture(const TsdfState *s) { return s && s->have_mesh && s->have_texture; }

void mesh_texture_layout(const TsdfState *s, int texels, int cells_per_row, long long *n_faces, long long *cols, long long *width,
                         long long *height)
{
    *n_faces = s->n_faces;
    const long long C = texels + 3, n_cells = (s->n_faces + 1) / 2;
    long long c = cells_per_row;
    if (n_cells == 0) {
        *cols = *width = *height = 0;
        return;
    }
    if (c == 0)
        while (c * c < n_cells) ++c;
    const long long rows = (n_cells + c - 1) / c;
    *cols = c; *width = c * C; *height = rows * C;
}

void mesh_texture_size(const TsdfState *s, int *texels, int *width, int *height)
{
    *texels = s->tex_N; *width = s->tex_W; *height = s->tex_H;
}

hipError_t mesh_texture(TsdfState *s, ScratchCache &cache, const unsigned char *bgr, bool bgr_on_device, long long bgr_images,
                        const int *slots_h, float tolerance, float min_cos, bool best_view, int texels, int cols, int width,
                        int height, long long *n_textured, hipStream_t st)
{
    const long long nf = s->n_faces, hw = (long long)s->render_H * s->render_W, slots = (long long)width * height;
    const int n_views = s->render_views;
    s->have_texture = false;
    ScratchCache::Lease count;
    MCHK(cache.lease(count, 8));
    MCHK(hipMemsetAsync(count.get(), 0, 8, st));
    MCHK(s->slots.reserve((size_t)n_views, cache));
    MCHK(hipMemcpyAsync(s->slots.get(), slots_h, sizeof(int) * (size_t)n_views, hipMemcpyHostToDevice, st));
    if (!bgr_on_device) {
        MCHK(s->stage_bgr.reserve(3 * (size_t)hw * (size_t)bgr_images, cache));
        MCHK(hipMemcpyAsync(s->stage_bgr.get(), bgr, 3 * (size_t)hw * (size_t)bgr_images, hipMemcpyHostToDevice, st));
        bgr = s->stage_bgr.get();
    }
    MCHK(s->tex_atlas.reserve(3 * at_least_one(slots), cache));
    MCHK(s->tex_uv.reserve(6 * at_least_one(nf), cache));
    if (nf > 0) {
        auto kernel = best_view ? texture_kernel<true> : texture_kernel<false>;
        MCHK(launch(kernel, slots, st, s->verts.get(), s->faces.get(), s->rgb.get(), s->n_vertices, nf, s->render_cams.get(),
                    kmat_of(s->render_K), n_views, s->render_H, s->render_W, s->render_near, tolerance, min_cos,
                    s->render_depth.get(), (long long)n_views * hw, bgr, hw * bgr_images, s->slots.get(), texels, cols, slots,
                    s->tex_atlas.get(), count.get<unsigned long long>()));
        MCHK(launch(uv_kernel, nf, st, nf, texels, cols, width, height, s->tex_uv.get()));
    }
    unsigned long long textured = 0;
    MCHK(hipMemcpyAsync(&textured, count.get(), 8, hipMemcpyDeviceToHost, st));
    MCHK(hipStreamSynchronize(st));
    if (n_textured) *n_textured = (long long)textured;
    s->tex_N = texels; s->tex_cols = cols; s->tex_W = width; s->tex_H = height;
    s->have_texture = true;
    return hipSuccess;
}

hipError_t mesh_fetch_texture(TsdfState *s, unsigned char *atlas_rgb, float *uv, hipStream_t st)
{
    const size_t texels = (size_t)s->tex_W * (size_t)s->tex_H;
    if (atlas_rgb && texels > 0) MCHK(hipMemcpyAsync(atlas_rgb, s->tex_atlas.get(), 3 * texels, hipMemcpyDeviceToHost, st));
    if (uv && s->n_faces > 0) MCHK(hipMemcpyAsync(uv, s->tex_uv.get(), sizeof(float) * 6 * (size_t)s->n_faces, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t mesh_fetch_render_texture(TsdfState *s, ScratchCache &cache, int first, int count, unsigned char *rgb_out, hipStream_t st)
{
    const long long hw = (long long)s->render_H * s->render_W, pixels = (long long)count * hw;
    ScratchCache::Lease picture;
    MCHK(cache.lease(picture, 3 * (size_t)pixels));
    MCHK(launch(render_texture_kernel, pixels, st, s->verts.get(), s->faces.get(), s->tex_atlas.get(), s->n_vertices, s->n_faces,
                s->render_cams.get(), kmat_of(s->render_K), first, pixels, s->render_H, s->render_W, s->render_near,
                s->render_depth.get(), s->render_face.get(), s->tex_N, s->tex_cols, (long long)s->tex_W * s->tex_H,
                picture.get<unsigned char>()));
    MCHK(hipMemcpyAsync(rgb_out, picture.get(), 3 * (size_t)pixels, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

}  // namespace amvs

AMVS_CHECK_TU(mesh_texture)
