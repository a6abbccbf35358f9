// amvs_mesh.hip -- surface mesh from the per-view depth maps: TSDF fusion into a dense voxel grid, then
// marching tetrahedra on the Kuhn subdivision of every cube (no reference counterpart: the reference stops at
// the point cloud).  Judged against synthetic ground truth and tests/mesh_restatement.py, a NumPy statement of
// the same float32 operations in the same order (bit-identical volume and mesh).
//
// Grid point (i, j, k) is origin + (i, j, k) * voxel and lives at index (k * ny + j) * nx + i.
//
// Integration: one thread per grid point, the maps in a fixed order, the sums in registers, every output
// written once (no float atomics: their sums would depend on arrival order).  Per view, in float32 under
// -ffp-contract=off:
//   Xc = ((R0 X + R1 Y) + R2 Z) + t                 (row by row)
//   p  = (K0 Xc + K1 Yc) + K2 Zc ...,  u = p0 / p2, v = p1 / p2
//   skip unless Zc > 0; px = floorf(u + 0.5f), py = floorf(v + 0.5f) inside the image;
//   skip unless depth > 0 and conf >= min_views;  sdf = depth - Zc, skip if sdf < -trunc;
//   sum += fminf(1, sdf / trunc), weight += 1, colour sum += the pixel's RGB.
// tsdf = sum / weight (1 where weight == 0: unobserved, never meshed).
//
// Extraction (three passes, hipCUB scans between them):
//   (a) every grid point owns 7 lattice edges, to p + d for the direction masks d = 1 .. 7 (bit 0 = +x,
//       bit 1 = +y, bit 2 = +z: the axes, the face diagonals and the main diagonal).  An edge crosses when both
//       ends are observed and (f0 < 0) != (f1 < 0).  Vertex ids: exclusive scan of the per-point counts, then
//       direction order within a point.  Position P0 + t (P1 - P0), colour c0 + t (c1 - c0) of the two corners'
//       mean colours rounded with floorf(c + 0.5f), t = f0 / (f0 - f1).
//   (b) triangles per cube (the cube whose lowest corner is the point), scanned;
//   (c) faces in cube order, then tetrahedron order, then table order, wound so that the normal points toward
//       increasing TSDF (free space, the cameras' side);
//   (d) the vertices no face uses are dropped (keeping the order of the others) and the faces renumbered.
// The cube splits into the 6 tetrahedra 0 -> a -> a+b -> (1,1,1) along the main diagonal, one per axis order
// (x,y,z) (x,z,y) (y,x,z) (y,z,x) (z,x,y) (z,y,x).  Every tetrahedron edge then joins a corner to a corner that
// has all of its bits (it is one of the 7 lattice edges of its lower end), and every cube face is cut along the
// diagonal from its lowest corner, so neighbouring cubes agree and the mesh is watertight.  A tetrahedron is
// meshed only if all 4 corners are observed, so a crossing edge that only tetrahedra with an unobserved corner
// share has a vertex in (a) that (d) removes.
#define AMVS_TU_ID 9
#include "amvs_check.h"
#include "amvs_kernels.h"
#include "amvs_mesh_state.h"

#include <hipcub/hipcub.hpp>

namespace amvs {

namespace {

// tetrahedron edges (local vertex pairs) 0:(0,1) 1:(0,2) 2:(0,3) 3:(1,2) 4:(1,3) 5:(2,3)
__constant__ unsigned char k_edge_a[6] = {0, 0, 0, 1, 1, 2};
__constant__ unsigned char k_edge_b[6] = {1, 2, 3, 2, 3, 3};
// Triangles of the 16 sign cases (bit v set = local vertex v has f < 0), as tetrahedron edges, wound for a
// positively oriented tetrahedron (det(v1-v0, v2-v0, v3-v0) > 0) so the normal points toward the f >= 0
// vertices.  One vertex apart from the other three: one triangle on its 3 edges.  Two and two (inside p < q,
// outside r < s): the quad (p,r) (p,s) (q,s) (q,r) as the triangles [(p,r) (p,s) (q,s)] and [(p,r) (q,s) (q,r)].
// Cases 0 and 15 have none; a case's triangle count is 1 for an odd bit count, 2 for two bits.
__constant__ unsigned char k_tri[16][2][3] = {
    {{0, 0, 0}, {0, 0, 0}}, {{0, 1, 2}, {0, 0, 0}}, {{0, 4, 3}, {0, 0, 0}}, {{1, 2, 4}, {1, 4, 3}},
    {{1, 3, 5}, {0, 0, 0}}, {{0, 5, 2}, {0, 3, 5}}, {{0, 4, 5}, {0, 5, 1}}, {{2, 4, 5}, {0, 0, 0}},
    {{2, 5, 4}, {0, 0, 0}}, {{0, 1, 5}, {0, 5, 4}}, {{0, 5, 3}, {0, 2, 5}}, {{1, 5, 3}, {0, 0, 0}},
    {{1, 3, 4}, {1, 4, 2}}, {{0, 3, 4}, {0, 0, 0}}, {{0, 2, 1}, {0, 0, 0}}, {{0, 0, 0}, {0, 0, 0}}};
// Kuhn tetrahedra: cube corners (bit 0 = +x, 1 = +y, 2 = +z) of local vertices 1 and 2 (vertex 0 is corner 0,
// vertex 3 corner 7).  Odd axis orders (1, 2, 5) are negatively oriented: their triangles are wound backwards.
__constant__ unsigned char k_tet_c1[6] = {1, 1, 2, 2, 4, 4};
__constant__ unsigned char k_tet_c2[6] = {3, 5, 3, 6, 5, 6};

__device__ __forceinline__ int tri_count(unsigned c) { const int b = __popc(c); return b == 2 ? 2 : (b & 1); }

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(const float *__restrict__ depth, const float *__restrict__ conf,
                                                             long long map_elems, const unsigned char *__restrict__ bgr,
                                                             long long bgr_pixels, const int *__restrict__ color_slot,
                                                             const float *__restrict__ cams, Kmat K, int n_maps, int H, int W,
                                                             float min_views, float trunc, Grid g, float *__restrict__ tsdf,
                                                             float *__restrict__ weight, float *__restrict__ color_sum)
{
    const int n = g.nx * g.ny * g.nz;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int i = p % g.nx, j = (p / g.nx) % g.ny, k = p / (g.nx * g.ny);
    const float X = g.ox + (float)i * g.voxel, Y = g.oy + (float)j * g.voxel, Z = g.oz + (float)k * g.voxel;
    const long long HW = (long long)H * W;
    const float fW = (float)W, fH = (float)H;
    float s = 0.0f, w = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
    for (int m = 0; m < n_maps; ++m) {
        const float *P = cams + 12 * m;          // R row-major, t
        const float zc = ((P[6] * X + P[7] * Y) + P[8] * Z) + P[11];
        if (!(zc > 0.0f)) continue;
        const float xc = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[9];
        const float yc = ((P[3] * X + P[4] * Y) + P[5] * Z) + P[10];
        const float pu = (K.k[0] * xc + K.k[1] * yc) + K.k[2] * zc;
        const float pv = (K.k[3] * xc + K.k[4] * yc) + K.k[5] * zc;
        const float pw = (K.k[6] * xc + K.k[7] * yc) + K.k[8] * zc;
        const float fx = floorf(pu / pw + 0.5f), fy = floorf(pv / pw + 0.5f);
        if (!(fx >= 0.0f && fx < fW && fy >= 0.0f && fy < fH)) continue;
        const long long pix = (long long)(int)fy * W + (int)fx;
        const long long g_idx = AMVS_IDX(m * HW + pix, map_elems);
        const float d = depth[g_idx], cf = conf[g_idx];
        if (!(d > 0.0f) || !(cf >= min_views)) continue;
        const float sdf = d - zc;
        if (sdf < -trunc) continue;
        s += fminf(1.0f, sdf / trunc);
        w += 1.0f;
        const long long q = 3 * AMVS_IDX((long long)color_slot[m] * HW + pix, bgr_pixels);
        cb += (float)bgr[q]; cg += (float)bgr[q + 1]; cr += (float)bgr[q + 2];
    }
    tsdf[p] = w > 0.0f ? s / w : 1.0f;
    weight[p] = w;
    color_sum[3 * p] = cr; color_sum[3 * p + 1] = cg; color_sum[3 * p + 2] = cb;
}

// (a) crossing edges of every point: 7-bit mask (bit d-1 = direction d) and its population count
__global__ __launch_bounds__(256) void edge_mask_kernel(const float *__restrict__ tsdf, const float *__restrict__ weight, Grid g,
                                                        unsigned char *__restrict__ mask, unsigned *__restrict__ count)
{
    const int n = g.nx * g.ny * g.nz;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int i = p % g.nx, j = (p / g.nx) % g.ny, k = p / (g.nx * g.ny);
    unsigned bits = 0;
    if (weight[p] > 0.0f) {
        const bool in0 = tsdf[p] < 0.0f;
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            const int di = d & 1, dj = (d >> 1) & 1, dk = d >> 2;
            if (i + di >= g.nx || j + dj >= g.ny || k + dk >= g.nz) continue;
            const int q = p + di + g.nx * (dj + g.ny * dk);
            if (weight[q] > 0.0f && (tsdf[q] < 0.0f) != in0) bits |= 1u << (d - 1);
        }
    }
    mask[p] = (unsigned char)bits;
    count[p] = __popc(bits);
}

__device__ __forceinline__ unsigned char round_u8(float c)
{
    return (unsigned char)fminf(255.0f, fmaxf(0.0f, floorf(c + 0.5f)));
}

// (a) the vertices of every point's crossing edges, at vbase[p] + rank of the direction among its set bits
__global__ __launch_bounds__(256) void vertex_kernel(const float *__restrict__ tsdf, const float *__restrict__ weight,
                                                     const float *__restrict__ color_sum, Grid g,
                                                     const unsigned char *__restrict__ mask, const unsigned *__restrict__ vbase,
                                                     long long n_vertices, float *__restrict__ verts, unsigned char *__restrict__ rgb)
{
    const int n = g.nx * g.ny * g.nz;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const unsigned bits = mask[p];
    if (!bits) return;
    const int i = p % g.nx, j = (p / g.nx) % g.ny, k = p / (g.nx * g.ny);
    const float f0 = tsdf[p], w0 = weight[p];
    const float x0 = g.ox + (float)i * g.voxel, y0 = g.oy + (float)j * g.voxel, z0 = g.oz + (float)k * g.voxel;
    const float c0[3] = {color_sum[3 * p] / w0, color_sum[3 * p + 1] / w0, color_sum[3 * p + 2] / w0};
    unsigned id = vbase[p];
    for (int d = 1; d < 8; ++d) {
        if (!((bits >> (d - 1)) & 1u)) continue;
        const int di = d & 1, dj = (d >> 1) & 1, dk = d >> 2;
        const int q = AMVS_IDX(p + di + g.nx * (dj + g.ny * dk), n);
        const float f1 = tsdf[q], w1 = weight[q];
        const float t = f0 / (f0 - f1);
        const float x1 = g.ox + (float)(i + di) * g.voxel, y1 = g.oy + (float)(j + dj) * g.voxel,
                    z1 = g.oz + (float)(k + dk) * g.voxel;
        const long long v = AMVS_IDX((long long)id, n_vertices);
        verts[3 * v] = x0 + t * (x1 - x0);
        verts[3 * v + 1] = y0 + t * (y1 - y0);
        verts[3 * v + 2] = z0 + t * (z1 - z0);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float c1 = color_sum[3 * q + ch] / w1;
            rgb[3 * v + ch] = round_u8(c0[ch] + t * (c1 - c0[ch]));
        }
        ++id;
    }
}

// corner c of the cube at p: the point index and the "inside" / "observed" bits of all 8 corners
__device__ __forceinline__ void cube_corners(const float *__restrict__ tsdf, const float *__restrict__ weight, const Grid &g,
                                             int p, unsigned &inside, unsigned &observed)
{
    inside = 0; observed = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int q = p + (c & 1) + g.nx * (((c >> 1) & 1) + g.ny * (c >> 2));
        if (weight[q] > 0.0f) observed |= 1u << c;
        if (tsdf[q] < 0.0f) inside |= 1u << c;
    }
}

__device__ __forceinline__ bool interior_cube(const Grid &g, int p)
{
    const int i = p % g.nx, j = (p / g.nx) % g.ny, k = p / (g.nx * g.ny);
    return i + 1 < g.nx && j + 1 < g.ny && k + 1 < g.nz;
}

// sign case of Kuhn tetrahedron t from the cube's corner bits, or -1 if a corner is unobserved
__device__ __forceinline__ int tet_case(int t, unsigned inside, unsigned observed)
{
    const unsigned c1 = k_tet_c1[t], c2 = k_tet_c2[t];
    const unsigned need = 1u | (1u << c1) | (1u << c2) | 0x80u;
    if ((observed & need) != need) return -1;
    return (int)((inside & 1u) | (((inside >> c1) & 1u) << 1) | (((inside >> c2) & 1u) << 2) | (((inside >> 7) & 1u) << 3));
}

// cube corner of local tetrahedron vertex v (0 -> corner 0, 1 -> c1, 2 -> c2, 3 -> corner 7)
__device__ __forceinline__ unsigned tet_corner(unsigned v, unsigned c1, unsigned c2)
{
    return v == 0 ? 0u : v == 1 ? c1 : v == 2 ? c2 : 7u;
}

// (b) triangles of every cube
__global__ __launch_bounds__(256) void tri_count_kernel(const float *__restrict__ tsdf, const float *__restrict__ weight, Grid g,
                                                        unsigned *__restrict__ count)
{
    const int n = g.nx * g.ny * g.nz;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    unsigned total = 0;
    if (interior_cube(g, p)) {
        unsigned inside, observed;
        cube_corners(tsdf, weight, g, p, inside, observed);
        if (observed) {
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const int cs = tet_case(t, inside, observed);
                if (cs >= 0) total += tri_count((unsigned)cs);
            }
        }
    }
    count[p] = total;
}

// (c) faces: vertex ids of the crossing edges, in cube / tetrahedron / table order
__global__ __launch_bounds__(256) void face_kernel(const float *__restrict__ tsdf, const float *__restrict__ weight, Grid g,
                                                   const unsigned char *__restrict__ mask, const unsigned *__restrict__ vbase,
                                                   long long n_vertices, const unsigned *__restrict__ tcount,
                                                   const unsigned *__restrict__ tbase, long long n_faces, int *__restrict__ faces)
{
    const int n = g.nx * g.ny * g.nz;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || tcount[p] == 0) return;
    unsigned inside, observed;
    cube_corners(tsdf, weight, g, p, inside, observed);
    long long f = tbase[p];
    for (int t = 0; t < 6; ++t) {
        const int cs = tet_case(t, inside, observed);
        if (cs < 0) continue;
        const int nt = tri_count((unsigned)cs);
        const unsigned c1 = k_tet_c1[t], c2 = k_tet_c2[t];
        const bool flip = t == 1 || t == 2 || t == 5;
        for (int r = 0; r < nt; ++r) {
            int ids[3];
            for (int e = 0; e < 3; ++e) {
                const int te = k_tri[cs][r][e];
                const unsigned ca = tet_corner(k_edge_a[te], c1, c2), cb = tet_corner(k_edge_b[te], c1, c2);
                const unsigned dir = ca ^ cb;                 // ca's bits are a subset of cb's
                const int q = AMVS_IDX(p + (int)(ca & 1u) + g.nx * (int)(((ca >> 1) & 1u) + g.ny * (ca >> 2)), n);
                ids[e] = (int)AMVS_IDX((long long)vbase[q] + __popc(mask[q] & ((1u << (dir - 1)) - 1u)), n_vertices);
            }
            const long long o = 3 * AMVS_IDX(f, n_faces);
            faces[o] = ids[0];
            faces[o + 1] = flip ? ids[2] : ids[1];
            faces[o + 2] = flip ? ids[1] : ids[2];
            ++f;
        }
    }
}

// (d) drop the vertices no face uses (their edges are shared only by tetrahedra with an unobserved corner):
// flag the used ones (every writer stores the same 1), scan, move the kept vertices down, renumber the faces
__global__ __launch_bounds__(256) void vertex_used_kernel(const int *__restrict__ faces, long long n_ids, long long n_vertices,
                                                          unsigned *__restrict__ used)
{
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < n_ids) used[AMVS_IDX((long long)faces[f], n_vertices)] = 1u;
}

__global__ __launch_bounds__(256) void vertex_compact_kernel(const float *__restrict__ verts, const unsigned char *__restrict__ rgb,
                                                             const unsigned *__restrict__ used, const unsigned *__restrict__ new_id,
                                                             long long n_vertices, long long n_kept, float *__restrict__ verts_out,
                                                             unsigned char *__restrict__ rgb_out)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vertices || !used[v]) return;
    const long long o = AMVS_IDX((long long)new_id[v], n_kept);
#pragma unroll
    for (int c = 0; c < 3; ++c) { verts_out[3 * o + c] = verts[3 * v + c]; rgb_out[3 * o + c] = rgb[3 * v + c]; }
}

__global__ __launch_bounds__(256) void face_renumber_kernel(int *__restrict__ faces, long long n_ids, long long n_vertices,
                                                            const unsigned *__restrict__ new_id)
{
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < n_ids) faces[f] = (int)new_id[AMVS_IDX((long long)faces[f], n_vertices)];
}

// the kept faces in their order, each in its own corner order; MAPPED: the ids through vertex_map (n_vertices entries)
template <bool MAPPED>
__global__ __launch_bounds__(256) void face_compact_kernel(const int *__restrict__ faces, const unsigned *__restrict__ vertex_map,
                                                           const unsigned *__restrict__ keep, const unsigned *__restrict__ new_id,
                                                           long long n_faces, long long n_vertices, long long n_kept,
                                                           int *__restrict__ out)
{
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_faces || !keep[f]) return;
    const long long o = AMVS_IDX((long long)new_id[f], n_kept);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (MAPPED) out[3 * o + k] = (int)vertex_map[AMVS_IDX((long long)faces[3 * f + k], n_vertices)];
        else out[3 * o + k] = faces[3 * f + k];
    }
}

}  // namespace

// ---- what the mesh units share (amvs_mesh_state.h) -----------------------------------------------------------

hipError_t exclusive_scan(TsdfState *s, ScratchCache &cache, const unsigned *in, unsigned *out, long long n, hipStream_t st)
{
    size_t bytes = 0;
    MCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)n, st));
    MCHK(s->scan_tmp.reserve(bytes > 0 ? bytes : 1, cache));
    return hipcub::DeviceScan::ExclusiveSum(s->scan_tmp.get(), bytes, in, out, (int)n, st);
}

hipError_t scan_total(const unsigned *count, const unsigned *base, long long n, long long *total, hipStream_t st)
{
    unsigned h[2] = {0, 0};
    MCHK(hipMemcpyAsync(&h[0], count + n - 1, 4, hipMemcpyDeviceToHost, st));
    MCHK(hipMemcpyAsync(&h[1], base + n - 1, 4, hipMemcpyDeviceToHost, st));
    MCHK(hipStreamSynchronize(st));
    *total = (long long)h[0] + (long long)h[1];
    return hipSuccess;
}

int bits_for(long long n)
{
    int bits = 1;
    while (bits < 32 && (1ll << bits) < n) ++bits;
    return bits;
}

template <class K>
hipError_t sort_pairs(TsdfState *s, ScratchCache &cache, const K *key_in, K *key_out, const unsigned *val_in, unsigned *val_out,
                      long long n, int bits, hipStream_t st)
{
    size_t bytes = 0;
    MCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, key_in, key_out, val_in, val_out, (int)n, 0, bits, st));
    MCHK(s->scan_tmp.reserve(bytes > 0 ? bytes : 1, cache));
    return hipcub::DeviceRadixSort::SortPairs(s->scan_tmp.get(), bytes, key_in, key_out, val_in, val_out, (int)n, 0, bits, st);
}
template hipError_t sort_pairs(TsdfState *, ScratchCache &, const unsigned *, unsigned *, const unsigned *, unsigned *, long long, int,
                               hipStream_t);
template hipError_t sort_pairs(TsdfState *, ScratchCache &, const unsigned long long *, unsigned long long *, const unsigned *,
                               unsigned *, long long, int, hipStream_t);

hipError_t compact_faces(TsdfState *s, ScratchCache &cache, long long nv, long long nf, const unsigned *vertex_map,
                         long long *kept_f, hipStream_t st)
{
    *kept_f = 0;
    if (nf == 0) return hipSuccess;
    MCHK(s->fnew.reserve((size_t)nf, cache)); MCHK(s->faces2.reserve(3 * (size_t)nf, cache));
    MCHK(exclusive_scan(s, cache, s->fkeep.get(), s->fnew.get(), nf, st));
    MCHK(scan_total(s->fkeep.get(), s->fnew.get(), nf, kept_f, st));
    if (*kept_f == nf && !vertex_map) return hipSuccess;      // every face stays as it is
    s->topology_changed();
    if (*kept_f == 0) return hipSuccess;
    const auto kernel = vertex_map ? face_compact_kernel<true> : face_compact_kernel<false>;
    MCHK(launch(kernel, nf, st, s->faces.get(), vertex_map, s->fkeep.get(), s->fnew.get(), nf, nv, *kept_f, s->faces2.get()));
    std::swap(s->faces, s->faces2);
    return hipSuccess;
}

hipError_t drop_unused_vertices(TsdfState *s, ScratchCache &cache, long long nv, long long nf, long long *kept_v, hipStream_t st)
{
    *kept_v = 0;
    if (nv > 0 && nf > 0) {
        MCHK(hipMemsetAsync(s->vused.get(), 0, 4 * (size_t)nv, st));
        MCHK(launch(vertex_used_kernel, 3 * nf, st, s->faces.get(), 3 * nf, nv, s->vused.get()));
        MCHK(exclusive_scan(s, cache, s->vused.get(), s->vnew.get(), nv, st));
        MCHK(scan_total(s->vused.get(), s->vnew.get(), nv, kept_v, st));
    }
    if (*kept_v == nv) return hipSuccess;                     // every vertex is used: the new ids are the old ones
    s->topology_changed();
    if (*kept_v == 0) return hipSuccess;
    MCHK(launch(vertex_compact_kernel, nv, st, s->verts.get(), s->rgb.get(), s->vused.get(), s->vnew.get(), nv, *kept_v,
                s->verts2.get(), s->rgb2.get()));
    MCHK(launch(face_renumber_kernel, 3 * nf, st, s->faces.get(), 3 * nf, nv, s->vnew.get()));
    std::swap(s->verts, s->verts2);
    std::swap(s->rgb, s->rgb2);
    return hipSuccess;
}

hipError_t compact_mesh(TsdfState *s, ScratchCache &cache, Compaction *out, hipStream_t st)
{
    const long long nv = s->n_vertices, nf = s->n_faces;
    MCHK(compact_faces(s, cache, nv, nf, nullptr, &out->kept_f, st));
    MCHK(drop_unused_vertices(s, cache, nv, out->kept_f, &out->kept_v, st));
    out->removed = out->kept_f < nf || out->kept_v < nv;
    s->n_vertices = out->kept_v; s->n_faces = out->kept_f;
    return hipSuccess;
}

TsdfState *tsdf_state_new() { return new TsdfState(); }

void tsdf_state_free(TsdfState *s) { delete s; }

namespace {

// the volume of n grid points and the per-point buffers of the extraction's passes (a) and (b)
hipError_t reserve_volume(TsdfState *s, ScratchCache &cache, long long n)
{
    MCHK(s->tsdf.reserve(n, cache)); MCHK(s->weight.reserve(n, cache)); MCHK(s->color.reserve(3 * n, cache));
    MCHK(s->mask.reserve(n, cache));
    MCHK(s->vcount.reserve(n, cache)); MCHK(s->vbase.reserve(n, cache));
    MCHK(s->tcount.reserve(n, cache)); MCHK(s->tbase.reserve(n, cache));
    return hipSuccess;
}

}  // namespace

hipError_t tsdf_integrate(TsdfState *s, ScratchCache &cache, const float *depth, const float *conf, bool maps_on_device,
                          int n_maps, int H, int W, const unsigned char *bgr, bool bgr_on_device, long long bgr_images,
                          const int *slots_h, const float K[9], const float *poses_h, float min_views, const float origin[3],
                          float voxel, const int dims[3], float trunc, hipStream_t st)
{
    s->have_volume = s->have_fill = false;
    s->drop_mesh();
    const long long n = (long long)dims[0] * dims[1] * dims[2];
    const size_t hw = (size_t)H * W, nmap = hw * (size_t)n_maps;
    MCHK(reserve_volume(s, cache, n));
    MCHK(s->cams.reserve(12 * (size_t)n_maps, cache));
    MCHK(s->slots.reserve(n_maps, cache));
    MCHK(hipMemcpyAsync(s->cams.get(), poses_h, sizeof(float) * 12 * n_maps, hipMemcpyHostToDevice, st));
    MCHK(hipMemcpyAsync(s->slots.get(), slots_h, sizeof(int) * n_maps, hipMemcpyHostToDevice, st));
    if (!maps_on_device) {
        MCHK(s->stage_depth.reserve(nmap, cache));
        MCHK(s->stage_conf.reserve(nmap, cache));
        MCHK(hipMemcpyAsync(s->stage_depth.get(), depth, 4 * nmap, hipMemcpyHostToDevice, st));
        MCHK(hipMemcpyAsync(s->stage_conf.get(), conf, 4 * nmap, hipMemcpyHostToDevice, st));
        depth = s->stage_depth.get(); conf = s->stage_conf.get();
    }
    if (!bgr_on_device) {
        MCHK(s->stage_bgr.reserve(3 * hw * (size_t)bgr_images, cache));
        MCHK(hipMemcpyAsync(s->stage_bgr.get(), bgr, 3 * hw * (size_t)bgr_images, hipMemcpyHostToDevice, st));
        bgr = s->stage_bgr.get();
    }
    s->g = Grid{origin[0], origin[1], origin[2], voxel, dims[0], dims[1], dims[2]};
    s->n = n;
    Kmat km;
    for (int q = 0; q < 9; ++q) km.k[q] = K[q];
    MCHK(launch(tsdf_integrate_kernel, n, st, depth, conf, (long long)nmap, bgr, (long long)(hw * (size_t)bgr_images), s->slots.get(),
                s->cams.get(), km, n_maps, H, W, min_views, trunc, s->g, s->tsdf.get(), s->weight.get(), s->color.get()));
    MCHK(hipStreamSynchronize(st));
    s->have_volume = true;
    return hipSuccess;
}

hipError_t tsdf_set_volume(TsdfState *s, ScratchCache &cache, const float *tsdf, const float *weight, const float *color_sum,
                           const float origin[3], float voxel, const int dims[3], hipStream_t st)
{
    s->have_volume = s->have_fill = false;
    s->drop_mesh();
    const long long n = (long long)dims[0] * dims[1] * dims[2];
    MCHK(reserve_volume(s, cache, n));
    MCHK(hipMemcpyAsync(s->tsdf.get(), tsdf, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    MCHK(hipMemcpyAsync(s->weight.get(), weight, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    MCHK(hipMemcpyAsync(s->color.get(), color_sum, 12 * (size_t)n, hipMemcpyHostToDevice, st));
    MCHK(hipStreamSynchronize(st));
    s->g = Grid{origin[0], origin[1], origin[2], voxel, dims[0], dims[1], dims[2]};
    s->n = n;
    s->have_volume = true;
    return hipSuccess;
}

hipError_t tsdf_extract(TsdfState *s, ScratchCache &cache, long long *n_vertices, long long *n_faces, hipStream_t st)
{
    s->drop_mesh();
    const long long n = s->n;
    // (a) vertices
    MCHK(launch(edge_mask_kernel, n, st, s->tsdf.get(), s->weight.get(), s->g, s->mask.get(), s->vcount.get()));
    MCHK(exclusive_scan(s, cache, s->vcount.get(), s->vbase.get(), n, st));
    long long nv = 0;
    MCHK(scan_total(s->vcount.get(), s->vbase.get(), n, &nv, st));
    const size_t m = (size_t)(nv > 0 ? nv : 1);
    MCHK(s->verts.reserve(3 * m, cache)); MCHK(s->rgb.reserve(3 * m, cache));
    MCHK(s->verts2.reserve(3 * m, cache)); MCHK(s->rgb2.reserve(3 * m, cache));
    MCHK(s->vused.reserve(m, cache)); MCHK(s->vnew.reserve(m, cache));
    MCHK(launch(vertex_kernel, n, st, s->tsdf.get(), s->weight.get(), s->color.get(), s->g, s->mask.get(), s->vbase.get(), nv,
                s->verts.get(), s->rgb.get()));
    // (b) triangle counts
    MCHK(launch(tri_count_kernel, n, st, s->tsdf.get(), s->weight.get(), s->g, s->tcount.get()));
    MCHK(exclusive_scan(s, cache, s->tcount.get(), s->tbase.get(), n, st));
    long long nf = 0;
    MCHK(scan_total(s->tcount.get(), s->tbase.get(), n, &nf, st));
    MCHK(s->faces.reserve(3 * (size_t)(nf > 0 ? nf : 1), cache));
    // (c) faces
    MCHK(launch(face_kernel, n, st, s->tsdf.get(), s->weight.get(), s->g, s->mask.get(), s->vbase.get(), nv, s->tcount.get(),
                s->tbase.get(), nf, s->faces.get()));
    // (d) keep the vertices the faces use, in their order
    long long kept = 0;
    MCHK(drop_unused_vertices(s, cache, nv, nf, &kept, st));
    nv = kept;
    MCHK(hipStreamSynchronize(st));
    s->n_vertices = nv; s->n_faces = nf; s->have_mesh = true;
    *n_vertices = nv; *n_faces = nf;
    return hipSuccess;
}

bool tsdf_has_volume(const TsdfState *s) { return s && s->have_volume; }
bool tsdf_has_mesh(const TsdfState *s) { return s && s->have_mesh; }

hipError_t tsdf_fetch_mesh(TsdfState *s, float *verts, int *faces, unsigned char *rgb, hipStream_t st)
{
    if (s->n_vertices > 0) {
        if (verts) MCHK(hipMemcpyAsync(verts, s->verts.get(), 12 * (size_t)s->n_vertices, hipMemcpyDeviceToHost, st));
        if (rgb) MCHK(hipMemcpyAsync(rgb, s->rgb.get(), 3 * (size_t)s->n_vertices, hipMemcpyDeviceToHost, st));
    }
    if (s->n_faces > 0 && faces) MCHK(hipMemcpyAsync(faces, s->faces.get(), 12 * (size_t)s->n_faces, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t tsdf_fetch_volume(TsdfState *s, float *tsdf, float *weight, float *color_sum, hipStream_t st)
{
    if (tsdf) MCHK(hipMemcpyAsync(tsdf, s->tsdf.get(), 4 * (size_t)s->n, hipMemcpyDeviceToHost, st));
    if (weight) MCHK(hipMemcpyAsync(weight, s->weight.get(), 4 * (size_t)s->n, hipMemcpyDeviceToHost, st));
    if (color_sum) MCHK(hipMemcpyAsync(color_sum, s->color.get(), 12 * (size_t)s->n, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

}  // namespace amvs

AMVS_CHECK_TU(mesh)
