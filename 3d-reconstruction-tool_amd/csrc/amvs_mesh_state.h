// amvs_mesh_state.h -- what the surface-mesh translation units share: the context's volume-and-mesh state
// (amvs_mesh.hip builds the mesh, amvs_mesh_clean.hip and amvs_mesh_decimate.hip work on it in place,
// amvs_mesh_render.hip draws it into views and filters it by what they see), the hipCUB scan
// with its read-back, and the kernels of extraction pass (d) that drop unused vertices, which the component filter and
// the decimation run again.
// Include after defining AMVS_TU_ID (amvs_check.h): the kernels here are compiled into each including unit.
#pragma once
#include "amvs_check.h"
#include "amvs_buffer.h"

#include <hipcub/hipcub.hpp>

#include <cstdint>
#include <utility>

namespace amvs {

#define MCHK(call)                                 \
    do {                                           \
        hipError_t e_ = (call);                    \
        if (e_ != hipSuccess) return e_;           \
    } while (0)

struct Grid {
    float ox, oy, oz, voxel;
    int nx, ny, nz;
};

// every buffer grows only: a volume, a scan or a mesh no larger than the largest before allocates nothing
struct TsdfState {
    Grid g{};
    long long n = 0;                              // grid points
    bool have_volume = false, have_mesh = false;
    DeviceBuffer<float> tsdf, weight, color;      // [n], [n], [n][3]
    DeviceBuffer<unsigned char> mask;
    DeviceBuffer<unsigned> vcount, vbase, tcount, tbase;
    DeviceBuffer<unsigned char> scan_tmp;
    DeviceBuffer<float> cams;                     // [n_maps][12] R, t
    DeviceBuffer<int> slots;                      // colour image of every map
    DeviceBuffer<float> stage_depth, stage_conf;  // host maps
    DeviceBuffer<unsigned char> stage_bgr;        // host colour images
    DeviceBuffer<float> verts, verts2;
    DeviceBuffer<int> faces;
    DeviceBuffer<unsigned char> rgb, rgb2;
    DeviceBuffer<unsigned> vused, vnew;           // (d): used flags and new ids of the vertices
    long long n_vertices = 0, n_faces = 0;

    // ---- clean-up (amvs_mesh_clean.hip): attributes of the current mesh, each valid while its flag is set ----
    bool have_csr = false, have_pinned = false, have_labels = false, have_normals = false;
    DeviceBuffer<unsigned> row_count, row_start;  // [V + 1]: incident corners of every vertex and their exclusive scan
    DeviceBuffer<unsigned> corner_key, corner_key2, corner_id, corners;   // [3 F]: the sort's buffers; corners = the rows
    DeviceBuffer<unsigned char> pinned;           // [V]: on an edge that exactly one face has
    DeviceBuffer<int> parent, labels;             // [V]: union-find forest; smallest vertex id of the component
    DeviceBuffer<unsigned> comp_faces;            // [V]: faces of the component, at its label
    DeviceBuffer<unsigned long long> comp_stat;   // [2]: number of components; (faces << 32 | ~label) of the largest
    DeviceBuffer<unsigned> fkeep, fnew;           // [F]: kept flags and new ids of the faces
    DeviceBuffer<int> faces2;                     // [3 F]
    DeviceBuffer<float> face_normal, normals;     // [F][3], [V][3]

    // ---- decimation (amvs_mesh_decimate.hip): scratch of one call, nothing here outlives it ----
    DeviceBuffer<unsigned long long> dec_key, dec_key2;   // [V]: cell keys, as computed and sorted
    DeviceBuffer<unsigned> dec_id, dec_id2;       // [V]: vertex ids, ascending and in sorted-key order (the clusters' runs)
    DeviceBuffer<unsigned> dec_head, dec_before;  // [V]: run heads of the sorted keys and their exclusive scan
    DeviceBuffer<unsigned> dec_cluster, dec_start;        // [V]: cluster of every vertex; [C + 1]: start of every run
    DeviceBuffer<unsigned> dec_flag;              // [2]: smallest vertex id outside the cluster grid, or all ones; quadric fallbacks
    DeviceBuffer<unsigned> dec_ta, dec_tlo, dec_thi;      // [F]: smallest, middle and largest cluster id of the face
    DeviceBuffer<unsigned char> dec_even;         // [F]: winding of the face, rotated to start at its smallest id
    DeviceBuffer<unsigned> dec_fkey, dec_fkey2, dec_perm, dec_perm2;      // [F]: the group sorts' keys and permutation
    DeviceBuffer<float> dec_quadric;              // [V][9]: quadric placement, a00 a01 a02 a11 a12 a22 b0 b1 b2 of every vertex

    // ---- rendering (amvs_mesh_render.hip): the maps and the counts are attributes of the current mesh ----
    bool have_render = false, have_visibility = false;
    int render_large = 0;                         // amvs_set_render_tuning: box pixels of a large face, 0 = automatic
    int render_views = 0, render_H = 0, render_W = 0;     // what the maps were rendered with; the counts use the same
    float render_near = 0.0f, render_K[9] = {};
    DeviceBuffer<float> render_cams;              // [n_views][12] R, t
    DeviceBuffer<unsigned long long> render_keys; // [n_views][H][W]: bits(depth) << 32 | face, all ones = nothing drawn
    DeviceBuffer<float> render_depth;             // [n_views][H][W]
    DeviceBuffer<int> render_face;                // [n_views][H][W]
    DeviceBuffer<unsigned> render_list, render_count;     // [n_views][F]: the large faces of every view; [n_views]: how many
    DeviceBuffer<unsigned long long> render_skipped;      // [n_views]: faces with a vertex that is not usable
    DeviceBuffer<int> vis_count;                  // [V]: views that see the vertex
    DeviceBuffer<unsigned long long> vis_seen;    // [1]: vertices with a count > 0

    // the mesh moves or changes: what was rendered from it is no longer its picture
    void drop_views() { have_render = have_visibility = false; }

    // the mesh is about to be replaced: nothing derived from it stays
    void drop_mesh()
    {
        have_mesh = have_csr = have_pinned = have_labels = have_normals = false;
        drop_views();
    }
};

namespace {

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

inline dim3 grid_of(long long n) { return dim3((unsigned)((n + 255) / 256)); }

inline hipError_t exclusive_scan(TsdfState *s, ScratchCache &cache, const unsigned *in, unsigned *out, long long n, hipStream_t st)
{
    size_t bytes = 0;
    MCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)n, st));
    MCHK(s->scan_tmp.reserve(bytes > 0 ? bytes : 1, cache));
    return hipcub::DeviceScan::ExclusiveSum(s->scan_tmp.get(), bytes, in, out, (int)n, st);
}

// total of an exclusive scan: base[n-1] + count[n-1]
inline hipError_t scan_total(const unsigned *count, const unsigned *base, long long n, long long *total, hipStream_t st)
{
    unsigned h[2] = {0, 0};
    MCHK(hipMemcpyAsync(&h[0], count + n - 1, 4, hipMemcpyDeviceToHost, st));
    MCHK(hipMemcpyAsync(&h[1], base + n - 1, 4, hipMemcpyDeviceToHost, st));
    MCHK(hipStreamSynchronize(st));
    *total = (long long)h[0] + (long long)h[1];
    return hipSuccess;
}

// the vertices no face uses leave the mesh: the kept ones keep their order, the faces are renumbered.  nv, nf > 0.
inline hipError_t drop_unused_vertices(TsdfState *s, ScratchCache &cache, long long nv, long long nf, long long *kept,
                                       hipStream_t st)
{
    MCHK(hipMemsetAsync(s->vused.get(), 0, 4 * (size_t)nv, st));
    hipLaunchKernelGGL(vertex_used_kernel, grid_of(3 * nf), dim3(256), 0, st, (const int *)s->faces.get(), 3 * nf, nv,
                       s->vused.get());
    MCHK(hipGetLastError());
    MCHK(exclusive_scan(s, cache, s->vused.get(), s->vnew.get(), nv, st));
    MCHK(scan_total(s->vused.get(), s->vnew.get(), nv, kept, st));
    hipLaunchKernelGGL(vertex_compact_kernel, grid_of(nv), dim3(256), 0, st, (const float *)s->verts.get(),
                       (const unsigned char *)s->rgb.get(), (const unsigned *)s->vused.get(), (const unsigned *)s->vnew.get(), nv,
                       *kept, s->verts2.get(), s->rgb2.get());
    MCHK(hipGetLastError());
    hipLaunchKernelGGL(face_renumber_kernel, grid_of(3 * nf), dim3(256), 0, st, s->faces.get(), 3 * nf, nv,
                       (const unsigned *)s->vnew.get());
    MCHK(hipGetLastError());
    std::swap(s->verts, s->verts2);
    std::swap(s->rgb, s->rgb2);
    return hipSuccess;
}

}  // namespace

}  // namespace amvs
