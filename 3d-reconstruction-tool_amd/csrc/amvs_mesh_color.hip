// amvs_mesh_color.hip -- the colours of the current mesh taken from the images of the views that see it, through the
// current render, and the current render shaded with the vertex colours (include/amvs.h amvs_mesh_color_views,
// amvs_fetch_render_color).  No reference counterpart.  Judged against tests/mesh_color_restatement.py, a NumPy
// statement of the definitions in the header with the same float32 operations in the same order (bit-identical
// colours, count and pictures).
//
// No float atomics, and no result that depends on arrival order: a vertex belongs to one lane, which walks the views in
// ascending order in registers, and a pixel of the colour render to one lane.  The only atomic is the integer count of
// the recoloured vertices, one add per wave.
//
// color_views_kernel, one lane per vertex, views in a register loop as in visibility_kernel: projection (a) of the
// render (amvs_mesh_project.h), the 2 x 2 footprint at floorf(u), floorf(v), the four rendered depths (occlusion and
// outline test), the cosine between the normal and the direction to the camera, the bilinear sample of the three bytes.
// The four texels are fetched as twelve single-byte loads: a texel is 3 bytes at a 3-byte stride, so no wider load is
// aligned, and a wider unaligned one would read past the last image's end at the last footprint.  Neighbouring vertices
// of a mesh land on neighbouring pixels, so the bytes of a wave come from a few cache lines; the loads are issued
// only for the views that pass every test (DESIGN.md section 8 "Colours from the views" has the object code's figures).
//
// render_color_kernel, one lane per pixel of the asked views: the face the rasteriser left there is set up again by
// face_setup (the same instructions, so the same corners, order and area), the three edge functions give the
// barycentric weights, and the corners' colours are interpolated perspective-correctly with the pixel's rendered depth.
#define AMVS_TU_ID 13
#include "amvs_check.h"
#include "amvs_kernels.h"
#include "amvs_mesh_state.h"
#include "amvs_mesh_project.h"

namespace amvs {

namespace {

// (g) of the definition: round half up, clamped to a byte
__device__ __forceinline__ unsigned char color_u8(float q)
{
    return (unsigned char)fminf(255.0f, fmaxf(0.0f, floorf(q + 0.5f)));
}

// bgr: [bgr_pixels][3], image slot[m] belongs to rendered view m; rgb: the mesh's colours, RGB
template <bool BEST>
__global__ __launch_bounds__(256) void color_views_kernel(const float *__restrict__ verts, const float *__restrict__ normals,
                                                          long long n_vertices, const float *__restrict__ cams, Kmat K, int n_views,
                                                          int H, int W, float near, float tolerance, float min_cos,
                                                          const float *__restrict__ depth, long long map_elems,
                                                          const unsigned char *__restrict__ bgr, long long bgr_pixels,
                                                          const int *__restrict__ slot, unsigned char *__restrict__ rgb,
                                                          unsigned long long *__restrict__ n_colored)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool reached = false;
    if (v < n_vertices) {
        const float X = verts[3 * v], Y = verts[3 * v + 1], Z = verts[3 * v + 2];
        const float nx = normals[3 * v], ny = normals[3 * v + 1], nz = normals[3 * v + 2];
        const long long hw = (long long)H * W;
        const float last_x = (float)(W - 1), last_y = (float)(H - 1);
        float acc[3] = {0.0f, 0.0f, 0.0f};         // S_ch of the blend, val of the best view; B, G, R
        float wsum = 0.0f;                         // Wsum of the blend, the largest w so far
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
        if (reached) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) rgb[3 * v + 2 - ch] = color_u8(BEST ? acc[ch] : acc[ch] / wsum);
        }
    }
    const unsigned long long done = __ballot(reached);
    if (done && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)done) - 1)) atomicAdd(n_colored, (unsigned long long)__popcll(done));
}

// out: [count][H][W][3] RGB of the views first .. first + count - 1
__global__ __launch_bounds__(256) void render_color_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                           const unsigned char *__restrict__ rgb, long long n_vertices, long long n_faces,
                                                           const float *__restrict__ cams, Kmat K, int first, long long pixels, int H,
                                                           int W, float near, const float *__restrict__ depth,
                                                           const int *__restrict__ face, unsigned char *__restrict__ out)
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
            const float b0 = (float)w0 / a, b1 = (float)w1 / a, b2 = (float)w2 / a;
            const float z = depth[at];
            const long long i0 = AMVS_IDX((long long)faces[3 * f], n_vertices);
            const long long i1 = AMVS_IDX((long long)faces[3 * f + (s.flip ? 2 : 1)], n_vertices);
            const long long i2 = AMVS_IDX((long long)faces[3 * f + (s.flip ? 1 : 2)], n_vertices);
            const float t0 = b0 * s.iz0, t1 = b1 * s.iz1, t2 = b2 * s.iz2;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                q[ch] = z * ((t0 * (float)rgb[3 * i0 + ch] + t1 * (float)rgb[3 * i1 + ch]) + t2 * (float)rgb[3 * i2 + ch]);
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[3 * p + ch] = color_u8(q[ch]);
}

}  // namespace

hipError_t mesh_color_views(TsdfState *s, ScratchCache &cache, const unsigned char *bgr, bool bgr_on_device, long long bgr_images,
                            const int *slots_h, float tolerance, float min_cos, bool best_view, long long *n_colored, hipStream_t st)
{
    const long long nv = s->n_vertices, hw = (long long)s->render_H * s->render_W;
    const int n_views = s->render_views;
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
    if (nv > 0) {
        auto kernel = best_view ? color_views_kernel<true> : color_views_kernel<false>;
        MCHK(launch(kernel, nv, st, s->verts.get(), s->normals.get(), nv, s->render_cams.get(), kmat_of(s->render_K), n_views,
                    s->render_H, s->render_W, s->render_near, tolerance, min_cos, s->render_depth.get(), (long long)n_views * hw, bgr,
                    hw * bgr_images, s->slots.get(), s->rgb.get(), count.get<unsigned long long>()));
    }
    unsigned long long colored = 0;
    MCHK(hipMemcpyAsync(&colored, count.get(), 8, hipMemcpyDeviceToHost, st));
    MCHK(hipStreamSynchronize(st));
    if (n_colored) *n_colored = (long long)colored;
    s->have_texture = false;          // the atlas falls back to the vertex colours where no view reaches
    return hipSuccess;
}

hipError_t mesh_fetch_render_color(TsdfState *s, ScratchCache &cache, int first, int count, unsigned char *rgb_out, hipStream_t st)
{
    const long long hw = (long long)s->render_H * s->render_W, pixels = (long long)count * hw;
    ScratchCache::Lease picture;
    MCHK(cache.lease(picture, 3 * (size_t)pixels));
    MCHK(launch(render_color_kernel, pixels, st, s->verts.get(), s->faces.get(), s->rgb.get(), s->n_vertices, s->n_faces,
                s->render_cams.get(), kmat_of(s->render_K), first, pixels, s->render_H, s->render_W, s->render_near,
                s->render_depth.get(), s->render_face.get(), picture.get<unsigned char>()));
    MCHK(hipMemcpyAsync(rgb_out, picture.get(), 3 * (size_t)pixels, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

}  // namespace amvs

AMVS_CHECK_TU(mesh_color)
