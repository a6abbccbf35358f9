// amvs_mesh_clean.hip -- what follows the extraction: connected components and their filter, Taubin smoothing and
// vertex normals, in place on the context's current mesh (the one amvs_tsdf_extract made or amvs_mesh_set uploaded).
// No reference counterpart.  Judged against tests/mesh_clean_restatement.py, a NumPy statement of the same
// definitions with the same float32 operations in the same order (bit-identical positions, normals, labels).
//
// No float atomics: every float sum runs over a row of the vertex -> corner index in the row's order.  The integer
// atomics (counts, union-find hooks, maxima) give results that do not depend on arrival order.
//
// (a) Index.  Corner c = 3 * face + k holds vertex faces[c].  Row v lists the corners that hold v in ascending c:
//     counts with integer adds, the exclusive scan, and a stable radix sort of (vertex id, corner) whose values are
//     the rows laid end to end.  Built once per topology, kept until the faces change.
// (b) Components.  Union-find over the vertices: every face hooks the roots of its vertices, the larger root under
//     the smaller with a compare-and-swap, so parent[x] <= x always and the root of a finished tree is the smallest
//     id of its component: that id is the label.  Finds halve the path they walk.  A second kernel flattens.  Faces
//     per component are counted at the label, aggregated per wave before the add.  The filter keeps the components
//     with faces >= min_faces (and, with keep_largest, only the one with the most faces, a tie going to the smallest
//     label), compacts the faces in order, drops the vertices no face uses as extraction pass (d) does, and renames
//     the labels to the new ids.  min_faces <= 0 without keep_largest only labels.
// (c) Taubin smoothing on ping-pong position buffers: `iterations` times an umbrella step with factor lambda, then
//     one with factor mu unless mu == 0.  One step, per vertex with deg incident corners that is not pinned, per
//     component x, y, z, every operation rounded to float32:
//         s = 0;  for the row's corners in order: s += p[next corner of the face]; s += p[the one after]
//         m = s / (2.0f * (float)deg);  d = m - p;  p' = p + factor * d
//     deg == 0 and pinned vertices copy through.  With fix_boundary a vertex is pinned iff it has an edge that
//     exactly one face has (an edge on three or more faces does not pin).
// (d) Normals.  Per face n = cross(a, b), a = p1 - p0, b = p2 - p0:
//         (ay * bz - az * by,  az * bx - ax * bz,  ax * by - ay * bx)       not normalised: area weights
//     per vertex S = sum of n over the row's faces in row order, l = sqrtf((Sx * Sx + Sy * Sy) + Sz * Sz), normal
//     S / l, or (0, 0, 0) unless l > 0.
#define AMVS_TU_ID 10
#include "amvs_check.h"
#include "amvs_kernels.h"
#include "amvs_mesh_state.h"

namespace amvs {

namespace {

// ---- (a) index ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void corner_count_kernel(const int *__restrict__ faces, long long n_ids, long long n_vertices,
                                                           unsigned *__restrict__ count, unsigned *__restrict__ key,
                                                           unsigned *__restrict__ id)
{
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_ids) return;
    const int v = faces[c];
    atomicAdd(&count[AMVS_IDX((long long)v, n_vertices)], 1u);
    key[c] = (unsigned)v;
    id[c] = (unsigned)c;
}

// ---- (b) components ----------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void iota_kernel(int *__restrict__ a, long long n)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) a[v] = (int)v;
}

__device__ __forceinline__ int uf_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x's tree; every node on the way is pointed at its grandparent (an ancestor, so the forest stays a forest
// with parent <= self whatever other waves do meanwhile)
__device__ __forceinline__ int uf_find(int *__restrict__ parent, int x, long long n)
{
    int p = uf_load(parent + AMVS_IDX((long long)x, n));
    while (p != x) {
        const int g = uf_load(parent + AMVS_IDX((long long)p, n));
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void uf_union(int *__restrict__ parent, int a, int b, long long n)
{
    int ra = uf_find(parent, a, n), rb = uf_find(parent, b, n);
    while (ra != rb) {
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const int old = atomicCAS(parent + hi, hi, lo);      // hooks only a node that is still a root
        if (old == hi) return;
        ra = uf_find(parent, old, n);                        // hi was hooked meanwhile: go on from where it points
        rb = lo;
    }
}

__global__ __launch_bounds__(256) void uf_hook_kernel(const int *__restrict__ faces, long long n_faces, long long n_vertices,
                                                      int *__restrict__ parent)
{
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_faces) return;
    const int v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
    uf_union(parent, v0, v1, n_vertices);
    uf_union(parent, v0, v2, n_vertices);
}

// labels from the finished forest (read only); the roots are counted, one add per wave
__global__ __launch_bounds__(256) void uf_flatten_kernel(const int *__restrict__ parent, long long n_vertices, int *__restrict__ labels,
                                                         unsigned long long *__restrict__ stat)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool root = false;
    if (v < n_vertices) {
        int x = (int)v, p = parent[v];
        while (p != x) { x = p; p = parent[AMVS_IDX((long long)x, n_vertices)]; }
        labels[v] = x;
        root = x == (int)v;
    }
    const unsigned long long roots = __ballot(root);
    if (roots && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)roots) - 1)) atomicAdd(&stat[0], (unsigned long long)__popcll(roots));
}

// faces per component at its label: the lanes of a wave that share a label add once
__global__ __launch_bounds__(256) void comp_faces_kernel(const int *__restrict__ faces, const int *__restrict__ labels, long long n_faces,
                                                         long long n_vertices, unsigned *__restrict__ comp_faces)
{
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = f < n_faces;
    const int lab = valid ? labels[AMVS_IDX((long long)faces[3 * f], n_vertices)] : -1;
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(valid);
    while (todo) {                                            // uniform over the wave
        const int leader = __ffsll((long long)todo) - 1;
        const int l = __shfl(lab, leader);
        const unsigned long long same = __ballot(valid && lab == l);
        if (lane == leader) atomicAdd(&comp_faces[AMVS_IDX((long long)l, n_vertices)], (unsigned)__popcll(same));
        todo &= ~same;
    }
}

// the component with the most faces, the smallest label among equals: maximum of (faces << 32 | ~label) over the roots
__global__ __launch_bounds__(256) void comp_largest_kernel(const int *__restrict__ labels, const unsigned *__restrict__ comp_faces,
                                                           long long n_vertices, unsigned long long *__restrict__ stat)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vertices || labels[v] != (int)v) return;
    atomicMax(&stat[1], ((unsigned long long)comp_faces[v] << 32) | (0xFFFFFFFFull - (unsigned long long)v));
}

__global__ __launch_bounds__(256) void face_keep_kernel(const int *__restrict__ faces, const int *__restrict__ labels,
                                                        const unsigned *__restrict__ comp_faces, long long n_faces, long long n_vertices,
                                                        long long min_faces, int only_label, unsigned *__restrict__ keep)
{
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_faces) return;
    const int l = labels[AMVS_IDX((long long)faces[3 * f], n_vertices)];
    const bool k = (long long)comp_faces[AMVS_IDX((long long)l, n_vertices)] >= min_faces && (only_label < 0 || l == only_label);
    keep[f] = k ? 1u : 0u;
}

// after the vertices moved (order kept): the label of a kept vertex is the new id of its old label vertex
__global__ __launch_bounds__(256) void relabel_kernel(const int *__restrict__ labels, const unsigned *__restrict__ used,
                                                      const unsigned *__restrict__ new_id, long long n_vertices, long long n_kept,
                                                      int *__restrict__ out)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vertices || !used[v]) return;
    out[AMVS_IDX((long long)new_id[v], n_kept)] = (int)new_id[AMVS_IDX((long long)labels[v], n_vertices)];
}

// ---- (c) smoothing -----------------------------------------------------------------------------------------

__device__ __forceinline__ bool face_has(const int *__restrict__ faces, long long f, int u)
{
    return faces[3 * f] == u || faces[3 * f + 1] == u || faces[3 * f + 2] == u;
}

// One thread per corner: the edge from its vertex v to the face's next vertex a.  The faces that hold both are
// counted along the shorter of the two rows; exactly one (this face) pins both ends.  Every writer stores the same 1.
__global__ __launch_bounds__(256) void pinned_kernel(const int *__restrict__ faces, const unsigned *__restrict__ row_start,
                                                     const unsigned *__restrict__ corners, long long n_ids, long long n_vertices,
                                                     unsigned char *__restrict__ pinned)
{
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_ids) return;
    const long long f = c / 3;
    const int k = (int)(c - 3 * f);
    const int v = (int)AMVS_IDX((long long)faces[c], n_vertices), a = (int)AMVS_IDX((long long)faces[3 * f + (k + 1) % 3], n_vertices);
    const unsigned dv = row_start[v + 1] - row_start[v], da = row_start[a + 1] - row_start[a];
    const int walk = dv <= da ? v : a, other = dv <= da ? a : v;
    int shared = 0;
    for (unsigned r = row_start[walk]; r < row_start[walk + 1]; ++r)
        shared += face_has(faces, (long long)(AMVS_IDX((long long)corners[AMVS_IDX((long long)r, n_ids)], n_ids) / 3), other) ? 1 : 0;
    if (shared == 1) { pinned[v] = 1; pinned[a] = 1; }
}

__global__ __launch_bounds__(256) void umbrella_kernel(const float *__restrict__ p, const int *__restrict__ faces,
                                                       const unsigned *__restrict__ row_start, const unsigned *__restrict__ corners,
                                                       const unsigned char *__restrict__ pinned, long long n_ids, long long n_vertices,
                                                       float factor, float *__restrict__ out)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vertices) return;
    const float px = p[3 * v], py = p[3 * v + 1], pz = p[3 * v + 2];
    const unsigned r0 = row_start[v], r1 = row_start[v + 1];
    float ox = px, oy = py, oz = pz;
    if (r1 > r0 && !(pinned && pinned[v])) {
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;
        for (unsigned r = r0; r < r1; ++r) {
            const long long c = AMVS_IDX((long long)corners[AMVS_IDX((long long)r, n_ids)], n_ids);
            const long long f = c / 3;
            const int k = (int)(c - 3 * f);
            const long long n1 = AMVS_IDX((long long)faces[3 * f + (k + 1) % 3], n_vertices);
            const long long n2 = AMVS_IDX((long long)faces[3 * f + (k + 2) % 3], n_vertices);
            sx += p[3 * n1]; sy += p[3 * n1 + 1]; sz += p[3 * n1 + 2];
            sx += p[3 * n2]; sy += p[3 * n2 + 1]; sz += p[3 * n2 + 2];
        }
        const float den = 2.0f * (float)(r1 - r0);
        const float dx = sx / den - px, dy = sy / den - py, dz = sz / den - pz;
        ox = px + factor * dx; oy = py + factor * dy; oz = pz + factor * dz;
    }
    out[3 * v] = ox; out[3 * v + 1] = oy; out[3 * v + 2] = oz;
}

// ---- (d) normals -------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void face_normal_kernel(const float *__restrict__ p, const int *__restrict__ faces, long long n_faces,
                                                          long long n_vertices, float *__restrict__ fn)
{
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_faces) return;
    const long long v0 = AMVS_IDX((long long)faces[3 * f], n_vertices), v1 = AMVS_IDX((long long)faces[3 * f + 1], n_vertices),
                    v2 = AMVS_IDX((long long)faces[3 * f + 2], n_vertices);
    const float ax = p[3 * v1] - p[3 * v0], ay = p[3 * v1 + 1] - p[3 * v0 + 1], az = p[3 * v1 + 2] - p[3 * v0 + 2];
    const float bx = p[3 * v2] - p[3 * v0], by = p[3 * v2 + 1] - p[3 * v0 + 1], bz = p[3 * v2 + 2] - p[3 * v0 + 2];
    fn[3 * f] = ay * bz - az * by;
    fn[3 * f + 1] = az * bx - ax * bz;
    fn[3 * f + 2] = ax * by - ay * bx;
}

__global__ __launch_bounds__(256) void vertex_normal_kernel(const float *__restrict__ fn, const unsigned *__restrict__ row_start,
                                                            const unsigned *__restrict__ corners, long long n_ids, long long n_vertices,
                                                            float *__restrict__ normals)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vertices) return;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (unsigned r = row_start[v]; r < row_start[v + 1]; ++r) {
        const long long f = AMVS_IDX((long long)corners[AMVS_IDX((long long)r, n_ids)], n_ids) / 3;
        sx += fn[3 * f]; sy += fn[3 * f + 1]; sz += fn[3 * f + 2];
    }
    const float l = sqrtf((sx * sx + sy * sy) + sz * sz);
    const bool ok = l > 0.0f;
    normals[3 * v] = ok ? sx / l : 0.0f;
    normals[3 * v + 1] = ok ? sy / l : 0.0f;
    normals[3 * v + 2] = ok ? sz / l : 0.0f;
}

}  // namespace

// ---- host --------------------------------------------------------------------------------------------------

// (a): row_start[0 .. V] and corners[0 .. 3 F) of the current faces
hipError_t ensure_index(TsdfState *s, ScratchCache &cache, hipStream_t st)
{
    if (s->have_csr) return hipSuccess;
    const long long nv = s->n_vertices, nc = 3 * s->n_faces;
    MCHK(s->row_count.reserve((size_t)nv + 1, cache)); MCHK(s->row_start.reserve((size_t)nv + 1, cache));
    MCHK(s->corner_key.reserve(at_least_one(nc), cache)); MCHK(s->corner_key2.reserve(at_least_one(nc), cache));
    MCHK(s->corner_id.reserve(at_least_one(nc), cache)); MCHK(s->corners.reserve(at_least_one(nc), cache));
    MCHK(hipMemsetAsync(s->row_count.get(), 0, 4 * ((size_t)nv + 1), st));
    if (nc > 0) {
        MCHK(launch(corner_count_kernel, nc, st, s->faces.get(), nc, nv, s->row_count.get(), s->corner_key.get(), s->corner_id.get()));
    }
    MCHK(exclusive_scan(s, cache, s->row_count.get(), s->row_start.get(), nv + 1, st));
    if (nc > 0) {
        MCHK(sort_pairs(s, cache, (const unsigned *)s->corner_key.get(), s->corner_key2.get(), (const unsigned *)s->corner_id.get(),
                        s->corners.get(), nc, bits_for(nv), st));
    }
    s->have_csr = true;
    return hipSuccess;
}

// (d): face_normal[0 .. F) of the current faces and positions
hipError_t mesh_face_normals(TsdfState *s, ScratchCache &cache, hipStream_t st)
{
    const long long nv = s->n_vertices, nf = s->n_faces;
    MCHK(s->face_normal.reserve(3 * at_least_one(nf), cache));
    if (nf > 0) {
        MCHK(launch(face_normal_kernel, nf, st, s->verts.get(), s->faces.get(), nf, nv, s->face_normal.get()));
    }
    return hipSuccess;
}

namespace {

hipError_t ensure_pinned(TsdfState *s, ScratchCache &cache, hipStream_t st)
{
    if (s->have_pinned) return hipSuccess;
    MCHK(ensure_index(s, cache, st));
    const long long nv = s->n_vertices, nc = 3 * s->n_faces;
    MCHK(s->pinned.reserve(at_least_one(nv), cache));
    if (nv > 0) MCHK(hipMemsetAsync(s->pinned.get(), 0, (size_t)nv, st));
    if (nc > 0) {
        MCHK(launch(pinned_kernel, nc, st, s->faces.get(), s->row_start.get(), s->corners.get(), nc, nv, s->pinned.get()));
    }
    s->have_pinned = true;
    return hipSuccess;
}

// (b) labels[v], comp_faces[label] and the number of components of the current mesh
hipError_t label_components(TsdfState *s, ScratchCache &cache, long long *n_components, hipStream_t st)
{
    const long long nv = s->n_vertices, nf = s->n_faces;
    MCHK(s->parent.reserve(at_least_one(nv), cache)); MCHK(s->labels.reserve(at_least_one(nv), cache));
    MCHK(s->comp_faces.reserve(at_least_one(nv), cache)); MCHK(s->comp_stat.reserve(2, cache));
    MCHK(hipMemsetAsync(s->comp_stat.get(), 0, 16, st));
    *n_components = 0;
    if (nv == 0) return hipSuccess;
    MCHK(hipMemsetAsync(s->comp_faces.get(), 0, 4 * (size_t)nv, st));
    MCHK(launch(iota_kernel, nv, st, s->parent.get(), nv));
    if (nf > 0) {
        MCHK(launch(uf_hook_kernel, nf, st, s->faces.get(), nf, nv, s->parent.get()));
    }
    MCHK(launch(uf_flatten_kernel, nv, st, s->parent.get(), nv, s->labels.get(), s->comp_stat.get()));
    if (nf > 0) {
        MCHK(launch(comp_faces_kernel, nf, st, s->faces.get(), s->labels.get(), nf, nv, s->comp_faces.get()));
    }
    unsigned long long h = 0;
    MCHK(hipMemcpyAsync(&h, s->comp_stat.get(), 8, hipMemcpyDeviceToHost, st));
    MCHK(hipStreamSynchronize(st));
    *n_components = (long long)h;
    return hipSuccess;
}

}  // namespace

hipError_t mesh_set(TsdfState *s, ScratchCache &cache, const float *verts, long long nv, const int *faces, long long nf,
                    const unsigned char *rgb, hipStream_t st)
{
    s->drop_mesh();
    const size_t m = at_least_one(nv);
    MCHK(s->verts.reserve(3 * m, cache)); MCHK(s->rgb.reserve(3 * m, cache));
    MCHK(s->verts2.reserve(3 * m, cache)); MCHK(s->rgb2.reserve(3 * m, cache));
    MCHK(s->vused.reserve(m, cache)); MCHK(s->vnew.reserve(m, cache));
    MCHK(s->faces.reserve(3 * at_least_one(nf), cache));
    if (nv > 0) {
        MCHK(hipMemcpyAsync(s->verts.get(), verts, 12 * (size_t)nv, hipMemcpyHostToDevice, st));
        if (rgb) MCHK(hipMemcpyAsync(s->rgb.get(), rgb, 3 * (size_t)nv, hipMemcpyHostToDevice, st));
        else MCHK(hipMemsetAsync(s->rgb.get(), 0, 3 * (size_t)nv, st));
    }
    if (nf > 0) MCHK(hipMemcpyAsync(s->faces.get(), faces, 12 * (size_t)nf, hipMemcpyHostToDevice, st));
    MCHK(hipStreamSynchronize(st));
    s->n_vertices = nv; s->n_faces = nf; s->have_mesh = true;
    return hipSuccess;
}

hipError_t mesh_filter_components(TsdfState *s, ScratchCache &cache, long long min_faces, bool keep_largest, long long *n_components,
                                  long long *n_vertices, long long *n_faces, hipStream_t st)
{
    s->have_labels = false;
    s->positions_changed();           // nothing moves, but normals and render do not outlive a labelling
    const long long nv = s->n_vertices, nf = s->n_faces;
    MCHK(label_components(s, cache, n_components, st));
    *n_vertices = nv; *n_faces = nf;
    s->have_labels = true;
    if ((min_faces <= 0 && !keep_largest) || nv == 0) return hipSuccess;
    int only_label = -1;
    if (keep_largest) {
        MCHK(launch(comp_largest_kernel, nv, st, s->labels.get(), s->comp_faces.get(), nv, s->comp_stat.get()));
        unsigned long long h = 0;
        MCHK(hipMemcpyAsync(&h, s->comp_stat.get() + 1, 8, hipMemcpyDeviceToHost, st));
        MCHK(hipStreamSynchronize(st));
        only_label = (int)(0xFFFFFFFFull - (h & 0xFFFFFFFFull));
    }
    s->have_labels = false;           // until they are in the numbering of what stays
    if (nf > 0) {
        MCHK(s->fkeep.reserve((size_t)nf, cache));
        MCHK(launch(face_keep_kernel, nf, st, s->faces.get(), s->labels.get(), s->comp_faces.get(), nf, nv, min_faces, only_label,
                    s->fkeep.get()));
    }
    Compaction k;
    MCHK(compact_mesh(s, cache, &k, st));
    if (!k.removed) { s->have_labels = true; return hipSuccess; }        // the mesh is as it was: the index stays too
    if (k.kept_f > 0) {
        // labels into the new numbering (parent serves as the second buffer)
        MCHK(launch(relabel_kernel, nv, st, s->labels.get(), s->vused.get(), s->vnew.get(), nv, k.kept_v, s->parent.get()));
        std::swap(s->labels, s->parent);
    }
    MCHK(hipStreamSynchronize(st));
    s->have_labels = true;
    *n_vertices = k.kept_v; *n_faces = k.kept_f;
    return hipSuccess;
}

hipError_t mesh_smooth(TsdfState *s, ScratchCache &cache, int iterations, float lambda, float mu, bool fix_boundary, hipStream_t st)
{
    s->positions_changed();
    const long long nv = s->n_vertices, nc = 3 * s->n_faces;
    if (iterations > 0 && nv > 0) {
        MCHK(ensure_index(s, cache, st));
        if (fix_boundary) MCHK(ensure_pinned(s, cache, st));
        MCHK(s->verts2.reserve(3 * (size_t)nv, cache));
        const unsigned char *pin = fix_boundary ? s->pinned.get() : nullptr;
        for (int it = 0; it < iterations; ++it)
            for (int half = 0; half < 2; ++half) {
                if (half == 1 && mu == 0.0f) continue;
                MCHK(launch(umbrella_kernel, nv, st, s->verts.get(), s->faces.get(), s->row_start.get(), s->corners.get(), pin, nc, nv,
                            half == 0 ? lambda : mu, s->verts2.get()));
                std::swap(s->verts, s->verts2);
            }
    }
    return hipStreamSynchronize(st);
}

hipError_t mesh_normals(TsdfState *s, ScratchCache &cache, hipStream_t st)
{
    s->have_normals = false;
    const long long nv = s->n_vertices, nf = s->n_faces;
    MCHK(ensure_index(s, cache, st));
    MCHK(s->normals.reserve(3 * at_least_one(nv), cache));
    MCHK(mesh_face_normals(s, cache, st));
    if (nv > 0) {
        MCHK(launch(vertex_normal_kernel, nv, st, s->face_normal.get(), s->row_start.get(), s->corners.get(), 3 * nf, nv,
                    s->normals.get()));
    }
    MCHK(hipStreamSynchronize(st));
    s->have_normals = true;
    return hipSuccess;
}

bool mesh_has_normals(const TsdfState *s) { return s && s->have_mesh && s->have_normals; }
bool mesh_has_labels(const TsdfState *s) { return s && s->have_mesh && s->have_labels; }

hipError_t mesh_fetch_attributes(TsdfState *s, float *normals, int *labels, hipStream_t st)
{
    if (s->n_vertices > 0) {
        if (normals) MCHK(hipMemcpyAsync(normals, s->normals.get(), 12 * (size_t)s->n_vertices, hipMemcpyDeviceToHost, st));
        if (labels) MCHK(hipMemcpyAsync(labels, s->labels.get(), 4 * (size_t)s->n_vertices, hipMemcpyDeviceToHost, st));
    }
    return hipStreamSynchronize(st);
}

}  // namespace amvs

AMVS_CHECK_TU(mesh_clean)
