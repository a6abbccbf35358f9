// amvs_mesh_render.hip -- the current mesh seen from given cameras: a z-buffer rasteriser (depth and face-id maps),
// per-vertex visibility counts against those maps, and the filter that drops what too few views see.
// No reference counterpart.  Judged against tests/mesh_render_restatement.py, a NumPy statement of the definition in
// include/amvs.h (amvs_mesh_render) with the same float32 operations in the same order, exact integer coverage and
// the same 64-bit keys (bit-identical maps, counts and filtered mesh).
//
// No float atomics, and no result that depends on arrival order: coverage is decided in int64 on 1/256-pixel
// coordinates, a fragment is the key (bits(z) << 32 | face) and a pixel keeps the smallest key with a 64-bit integer
// atomicMin (z > 0 and finite, so the bit pattern orders like the float; equal depth goes to the smaller face id).
//
// (a) Keys [n_views][H][W] are set to all ones.
// (b) raster_small_kernel, one lane per (view, face): projects the three vertices as tsdf_integrate_kernel does,
//     orients the face, clamps its bounding box to the image.  A face with a vertex that is not usable is counted
//     (one add per wave and view) and left out.  A box of at most `large` pixels is walked by the lane itself; a
//     larger one is appended to the view's list through a counter that the wave's lanes share one add on.
// (c) raster_large_kernel, workgroups striding over every view's list: a workgroup sets the face up again (uniform)
//     and its 256 lanes stride over the box.  It runs after (b) in stream order and reads the counts (b) left on the
//     device: no read-back, no host synchronisation between the two.  Which of the two kernels draws a face cannot
//     show in the maps: both issue the same keys.
// (d) The atomic is issued for every fragment.  Loading the pixel's key first and leaving when it is not larger (keys
//     only decrease, so that would be safe) was built and measured: it did not help.
// (e) split_kernel: depth = upper word (0.0f where the key is still all ones), face = lower word (-1 there).
//
// Visibility: one lane per vertex walks the views in order and counts those where the vertex is in front of `near`,
// lands on a pixel of the image and is not behind that pixel's rendered depth by more than the tolerance.  The filter
// keeps the faces whose three vertices reach min_views, compacts them in order and drops the unused vertices as
// extraction pass (d) does.  The projection, the face set-up and the edge function are amvs_mesh_project.h's, shared
// with amvs_mesh_color.hip.
#define AMVS_TU_ID 12
#include "amvs_check.h"
#include "amvs_kernels.h"
#include "amvs_mesh_state.h"
#include "amvs_mesh_project.h"

#include <algorithm>
#include <vector>

namespace amvs {

namespace {

constexpr unsigned long long NO_KEY = ~0ull;
constexpr int AUTO_LARGE_PIXELS = 256;        // box size from which a face goes to the workgroup path
constexpr int LARGE_GRID = 1024;              // workgroups per view of the large-face kernel
constexpr int MAX_GRID_Y = 65535;

// (c), (d), (e) of the definition for one pixel of the face's clamped box (so 256 px, 256 py lie inside the face's own
// box and every difference is at most 2^29); keys = the view's key map of `hw` pixels
__device__ __forceinline__ void draw_pixel(const FaceSetup &s, int px, int py, unsigned face, int W, long long hw,
                                           unsigned long long *__restrict__ keys)
{
    const int fx = px << SUB_SHIFT, fy = py << SUB_SHIFT;
    long long w0, w1, w2;
    const bool in0 = edge_inside(s.x1, s.y1, s.x2, s.y2, fx, fy, w0);
    const bool in1 = edge_inside(s.x2, s.y2, s.x0, s.y0, fx, fy, w1);
    const bool in2 = edge_inside(s.x0, s.y0, s.x1, s.y1, fx, fy, w2);
    if (!(in0 && in1 && in2)) return;
    const float a = (float)s.area;
    const float b0 = (float)w0 / a, b1 = (float)w1 / a, b2 = (float)w2 / a;
    const float z = 1.0f / ((b0 * s.iz0 + b1 * s.iz1) + b2 * s.iz2);
    if (!(z > 0.0f && z < __builtin_inff())) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)face;
    // no load of the current key first to skip the atomic: measured, it saved nothing and cost up to a fifth of the
    // call: the lane has to wait for the load, the atomic returns nothing and is not waited for
    atomicMin(keys + AMVS_IDX((long long)py * W + px, hw), key);
}

// (b) blockIdx.y = view - view0.  list: [n_views][n_faces] face ids, count / skipped: [n_views]
__global__ __launch_bounds__(256) void raster_small_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                           long long n_vertices, long long n_faces, const float *__restrict__ cams,
                                                           Kmat K, int view0, int n_views, int H, int W, float near, int large,
                                                           unsigned long long *__restrict__ keys, unsigned *__restrict__ list,
                                                           unsigned *__restrict__ count, unsigned long long *__restrict__ skipped)
{
    const int view = view0 + (int)blockIdx.y;
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long hw = (long long)H * W;
    const int lane = threadIdx.x & 63;
    FaceSetup s;
    const int state = f < n_faces ? face_setup(verts, faces, f, n_vertices, cams + 12 * (long long)view, K, near, H, W, s) : FACE_EMPTY;
    const unsigned long long skip = __ballot(state == FACE_SKIPPED);
    if (skip && lane == __ffsll((long long)skip) - 1) atomicAdd(&skipped[AMVS_IDX(view, n_views)], (unsigned long long)__popcll(skip));
    const bool is_large = state == FACE_DRAWS && s.bw * s.bh > large;
    const unsigned long long big = __ballot(is_large);
    if (big) {                                                // uniform over the wave
        const int leader = __ffsll((long long)big) - 1;
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(&count[AMVS_IDX(view, n_views)], (unsigned)__popcll(big));
        base = __shfl(base, leader);
        if (is_large) {
            const long long at = (long long)base + __popcll(big & ((1ull << lane) - 1ull));
            list[(long long)view * n_faces + AMVS_IDX(at, n_faces)] = (unsigned)f;
        }
    }
    if (state != FACE_DRAWS || is_large) return;
    unsigned long long *const kv = keys + (long long)view * hw;
    for (int py = s.lo_y; py < s.lo_y + s.bh; ++py)
        for (int px = s.lo_x; px < s.lo_x + s.bw; ++px) draw_pixel(s, px, py, (unsigned)f, W, hw, kv);
}

// (c) blockIdx.y = view - view0; the workgroups of a view stride over its list
__global__ __launch_bounds__(256) void raster_large_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                           long long n_vertices, long long n_faces, const float *__restrict__ cams,
                                                           Kmat K, int view0, int n_views, int H, int W, float near,
                                                           unsigned long long *__restrict__ keys, const unsigned *__restrict__ list,
                                                           const unsigned *__restrict__ count)
{
    const int view = view0 + (int)blockIdx.y;
    const long long hw = (long long)H * W;
    const long long n = min((long long)count[AMVS_IDX(view, n_views)], n_faces);
    unsigned long long *const kv = keys + (long long)view * hw;
    for (long long i = blockIdx.x; i < n; i += gridDim.x) {
        const long long f = AMVS_IDX((long long)list[(long long)view * n_faces + i], n_faces);
        FaceSetup s;
        if (face_setup(verts, faces, f, n_vertices, cams + 12 * (long long)view, K, near, H, W, s) != FACE_DRAWS) continue;
        const int pixels = s.bw * s.bh;                       // <= H * W <= INT32_MAX
        for (int q = threadIdx.x; q < pixels; q += 256) {
            const int row = q / s.bw;
            draw_pixel(s, s.lo_x + (q - row * s.bw), s.lo_y + row, (unsigned)f, W, hw, kv);
        }
    }
}

__global__ __launch_bounds__(256) void split_kernel(const unsigned long long *__restrict__ keys, long long n, float *__restrict__ depth,
                                                    int *__restrict__ face)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const unsigned long long key = keys[p];
    const bool drawn = key != NO_KEY;
    depth[p] = drawn ? __uint_as_float((unsigned)(key >> 32)) : 0.0f;
    face[p] = drawn ? (int)(unsigned)(key & 0xFFFFFFFFull) : -1;
}

__global__ __launch_bounds__(256) void visibility_kernel(const float *__restrict__ verts, long long n_vertices,
                                                         const float *__restrict__ cams, Kmat K, int n_views, int H, int W, float near,
                                                         float tolerance, const float *__restrict__ depth, long long map_elems,
                                                         int *__restrict__ counts, unsigned long long *__restrict__ n_seen)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int c = 0;
    if (v < n_vertices) {
        const float X = verts[3 * v], Y = verts[3 * v + 1], Z = verts[3 * v + 2];
        const long long hw = (long long)H * W;
        const float fW = (float)W, fH = (float)H;
        for (int m = 0; m < n_views; ++m) {
            const Projected p = project(cams + 12 * m, K, X, Y, Z);
            if (!(p.zc > near)) continue;
            const float fx = floorf(p.u + 0.5f), fy = floorf(p.v + 0.5f);
            if (!(fx >= 0.0f && fx < fW && fy >= 0.0f && fy < fH)) continue;
            const float d = depth[AMVS_IDX(m * hw + ((long long)(int)fy * W + (int)fx), map_elems)];
            if (d == 0.0f || p.zc <= d + tolerance) ++c;
        }
        counts[v] = c;
    }
    const unsigned long long seen = __ballot(c > 0);
    if (seen && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)seen) - 1)) atomicAdd(n_seen, (unsigned long long)__popcll(seen));
}

__global__ __launch_bounds__(256) void visible_keep_kernel(const int *__restrict__ faces, const int *__restrict__ counts, long long n_faces,
                                                           long long n_vertices, int min_views, unsigned *__restrict__ keep)
{
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_faces) return;
    bool k = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) k = k && counts[AMVS_IDX((long long)faces[3 * f + c], n_vertices)] >= min_views;
    keep[f] = k ? 1u : 0u;
}

}  // namespace

void mesh_set_render_tuning(TsdfState *s, int large_face_pixels) { s->render_large = large_face_pixels; }

hipError_t mesh_render(TsdfState *s, ScratchCache &cache, int n_views, int H, int W, const float K[9], const float *poses_h,
                       float near, long long *n_skipped_h, hipStream_t st)
{
    s->drop_views();
    const long long nv = s->n_vertices, nf = s->n_faces, hw = (long long)H * W, n = (long long)n_views * hw;
    MCHK(s->render_keys.reserve((size_t)n, cache));
    MCHK(s->render_depth.reserve((size_t)n, cache)); MCHK(s->render_face.reserve((size_t)n, cache));
    MCHK(s->render_cams.reserve(12 * (size_t)n_views, cache));
    MCHK(s->render_count.reserve((size_t)n_views, cache)); MCHK(s->render_skipped.reserve((size_t)n_views, cache));
    MCHK(s->render_list.reserve(at_least_one((long long)n_views * nf), cache));
    MCHK(hipMemcpyAsync(s->render_cams.get(), poses_h, 48 * (size_t)n_views, hipMemcpyHostToDevice, st));
    MCHK(hipMemsetAsync(s->render_keys.get(), 0xFF, 8 * (size_t)n, st));
    MCHK(hipMemsetAsync(s->render_count.get(), 0, 4 * (size_t)n_views, st));
    MCHK(hipMemsetAsync(s->render_skipped.get(), 0, 8 * (size_t)n_views, st));
    const Kmat k = kmat_of(K);
    const int large = s->render_large > 0 ? s->render_large : AUTO_LARGE_PIXELS;
    if (nf > 0) {
        const unsigned large_grid = (unsigned)std::min<long long>(nf, LARGE_GRID);
        for (int view0 = 0; view0 < n_views; view0 += MAX_GRID_Y) {
            const unsigned views = (unsigned)std::min(n_views - view0, MAX_GRID_Y);
            hipLaunchKernelGGL(raster_small_kernel, dim3(grid_of(nf).x, views), dim3(256), 0, st, (const float *)s->verts.get(),
                               (const int *)s->faces.get(), nv, nf, (const float *)s->render_cams.get(), k, view0, n_views, H, W, near,
                               large, s->render_keys.get(), s->render_list.get(), s->render_count.get(), s->render_skipped.get());
            MCHK(hipGetLastError());
            hipLaunchKernelGGL(raster_large_kernel, dim3(large_grid, views), dim3(256), 0, st, (const float *)s->verts.get(),
                               (const int *)s->faces.get(), nv, nf, (const float *)s->render_cams.get(), k, view0, n_views, H, W, near,
                               s->render_keys.get(), (const unsigned *)s->render_list.get(), (const unsigned *)s->render_count.get());
            MCHK(hipGetLastError());
        }
    }
    MCHK(launch(split_kernel, n, st, s->render_keys.get(), n, s->render_depth.get(), s->render_face.get()));
    std::vector<unsigned long long> skipped(n_skipped_h ? (size_t)n_views : 0);
    if (n_skipped_h) MCHK(hipMemcpyAsync(skipped.data(), s->render_skipped.get(), 8 * (size_t)n_views, hipMemcpyDeviceToHost, st));
    MCHK(hipStreamSynchronize(st));
    for (size_t m = 0; m < skipped.size(); ++m) n_skipped_h[m] = (long long)skipped[m];
    for (int i = 0; i < 9; ++i) s->render_K[i] = K[i];
    s->render_views = n_views; s->render_H = H; s->render_W = W; s->render_near = near;
    s->have_render = true;
    return hipSuccess;
}

bool mesh_has_render(const TsdfState *s) { return s && s->have_mesh && s->have_render; }
bool mesh_has_visibility(const TsdfState *s) { return s && s->have_mesh && s->have_render && s->have_visibility; }
int mesh_render_views(const TsdfState *s) { return mesh_has_render(s) ? s->render_views : 0; }

hipError_t mesh_fetch_render(TsdfState *s, int first, int count, float *depth, int *face, hipStream_t st)
{
    const size_t hw = (size_t)s->render_H * s->render_W;
    if (depth) MCHK(hipMemcpyAsync(depth, s->render_depth.get() + first * hw, 4 * count * hw, hipMemcpyDeviceToHost, st));
    if (face) MCHK(hipMemcpyAsync(face, s->render_face.get() + first * hw, 4 * count * hw, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t mesh_visibility(TsdfState *s, ScratchCache &cache, float tolerance, long long *n_seen, hipStream_t st)
{
    s->have_visibility = false;
    const long long nv = s->n_vertices;
    MCHK(s->vis_count.reserve(at_least_one(nv), cache));
    MCHK(s->vis_seen.reserve(1, cache));
    MCHK(hipMemsetAsync(s->vis_seen.get(), 0, 8, st));
    if (nv > 0) {
        MCHK(launch(visibility_kernel, nv, st, s->verts.get(), nv, s->render_cams.get(), kmat_of(s->render_K), s->render_views,
                    s->render_H, s->render_W, s->render_near, tolerance, s->render_depth.get(),
                    (long long)s->render_views * s->render_H * s->render_W, s->vis_count.get(), s->vis_seen.get()));
    }
    unsigned long long seen = 0;
    MCHK(hipMemcpyAsync(&seen, s->vis_seen.get(), 8, hipMemcpyDeviceToHost, st));
    MCHK(hipStreamSynchronize(st));
    *n_seen = (long long)seen;
    s->have_visibility = true;
    return hipSuccess;
}

hipError_t mesh_fetch_visibility(TsdfState *s, int *counts, hipStream_t st)
{
    if (s->n_vertices > 0) MCHK(hipMemcpyAsync(counts, s->vis_count.get(), 4 * (size_t)s->n_vertices, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t mesh_filter_visible(TsdfState *s, ScratchCache &cache, int min_views, long long *n_vertices, long long *n_faces,
                               hipStream_t st)
{
    const long long nv = s->n_vertices, nf = s->n_faces;
    if (nf > 0) {
        MCHK(s->fkeep.reserve((size_t)nf, cache));
        MCHK(launch(visible_keep_kernel, nf, st, s->faces.get(), s->vis_count.get(), nf, nv, min_views, s->fkeep.get()));
    }
    // the call counts as a change of the mesh also when every face stays: nothing derived from it is current
    s->topology_changed();
    Compaction k;
    MCHK(compact_mesh(s, cache, &k, st));
    MCHK(hipStreamSynchronize(st));
    *n_vertices = k.kept_v; *n_faces = k.kept_f;
    return hipSuccess;
}

}  // namespace amvs

AMVS_CHECK_TU(mesh_render)
