// amvs_mesh_decimate.hip -- decimation of the context's current mesh in place by vertex clustering on a grid of cubic
// cells.  No reference counterpart.  Judged against tests/mesh_decimate_restatement.py, a NumPy statement of the same
// definition with the same float32 operations in the same order (bit-identical positions, faces and colours).
//
// No float atomics: a cluster's position is a sequential sum over its members in ascending vertex id.  The integer
// atomics (the minimum of the out-of-range vertex ids; the count of the clusters that kept the mean, quadric placement)
// give results that do not depend on arrival order.
//
// (1) Cell.  Per vertex and axis q = (p - origin) / cell (two float32 operations, the division IEEE), i = floorf(q);
//     -2^20 <= i < 2^20 or the call is refused before anything of the mesh is overwritten.
//     key = (iz + 2^20) << 42 | (iy + 2^20) << 21 | (ix + 2^20).
// (2) Clusters.  A stable radix sort of (key, vertex id) over the 63 key bits; the heads of the runs of equal keys,
//     scanned, number the clusters in ascending key order (x fastest, the extraction's own point order) and every
//     run lists its members in ascending vertex id.
// (3) Representative.  One thread per cluster: s = 0; s += p[v] along the run; s / (float)count.  Colour: per channel
//     the integer sum, (2 sum + count) / (2 count) in integer division (round half up).
// (4) Faces.  The three ids go through the clustering; a face with a repeated id is dropped.  Of the others the triple
//     rotated to start at its smallest id is (a, b, c): the face's group is (a, min(b, c), max(b, c)) and its winding
//     b < c or not.  Three stable sorts of a permutation (by the largest id, then the middle, then the smallest one)
//     lay the groups end to end, every group in ascending face index.  One thread per group head walks its group:
//     net = faces of the one winding minus faces of the other; net == 0 drops the group (a flattened pocket, two
//     sheets back to back), otherwise the first face of the majority winding stays.  The kept faces are compacted in
//     their order, each in its own corner order.
// (5) The clusters no kept face uses leave the mesh as in extraction pass (d).
//
// Quadric placement (mesh_decimate_quadric; tests/mesh_quadric_restatement.py): steps (1), (2), (4), (5) and the colour
// of (3) as above; the position of a cluster is the minimiser of its members' area-weighted plane quadrics, tied to
// the mean m of (3) by a regulariser, or m itself where the solve is not trusted.  On the OLD faces and positions:
//     face normal   n = cross(p1 - p0, p2 - p0) as in amvs_mesh_clean.hip (d), not normalised
//     vertex v      Qv = 0; for the corners of v in ascending corner index, f the corner's face: e = p[faces[3 f]] - m,
//                   d = (nx ex + ny ey) + nz ez, Qv += (nx nx, nx ny, nx nz, ny ny, ny nz, nz nz, d nx, d ny, d nz)
//     cluster       S = 0; S += Qv along the run = (a00 a01 a02 a11 a12 a22 b0 b1 b2); the regularised LDL^T solve of
//                   cluster_solve_kernel in its stated order gives y; cand = m + y is taken iff t > 0, d1 > 0, d2 > 0,
//                   cand is finite and |y| <= 0.5f * cell on every axis (NaN compares false)
// The clusters that kept m are counted with one integer add per wave.
#define AMVS_TU_ID 11
#include "amvs_check.h"
#include "amvs_kernels.h"
#include "amvs_mesh_state.h"

namespace amvs {

namespace {

constexpr int DEC_HALF = 1 << 20;
constexpr unsigned DEC_NONE = 0xFFFFFFFFu;

struct Cells { float ox, oy, oz, cell; };

// (1) keys and vertex ids for the sort; the smallest vertex id with a cell index outside the grid, if any
__global__ __launch_bounds__(256) void cell_key_kernel(const float *__restrict__ verts, long long n_vertices, Cells g,
                                                       unsigned long long *__restrict__ key, unsigned *__restrict__ id,
                                                       unsigned *__restrict__ first_bad)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vertices) return;
    const float ix = floorf((verts[3 * v] - g.ox) / g.cell);
    const float iy = floorf((verts[3 * v + 1] - g.oy) / g.cell);
    const float iz = floorf((verts[3 * v + 2] - g.oz) / g.cell);
    const float lo = -(float)DEC_HALF, hi = (float)DEC_HALF;
    const bool ok = ix >= lo && ix < hi && iy >= lo && iy < hi && iz >= lo && iz < hi;       // false for inf and NaN
    unsigned long long k = 0;
    if (ok)
        k = ((unsigned long long)((int)iz + DEC_HALF) << 42) | ((unsigned long long)((int)iy + DEC_HALF) << 21) |
            (unsigned long long)((int)ix + DEC_HALF);
    else
        atomicMin(first_bad, (unsigned)v);
    key[v] = k;
    id[v] = (unsigned)v;
}

// (2) j heads a run of equal keys
__global__ __launch_bounds__(256) void key_head_kernel(const unsigned long long *__restrict__ key, long long n, unsigned *__restrict__ head)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) head[j] = (j == 0 || key[j] != key[j - 1]) ? 1u : 0u;
}

// (2) cluster of every vertex and the start of every run; start[n_clusters] = n
__global__ __launch_bounds__(256) void cluster_map_kernel(const unsigned *__restrict__ id, const unsigned *__restrict__ head,
                                                          const unsigned *__restrict__ before, long long n, long long n_clusters,
                                                          unsigned *__restrict__ cluster_of, unsigned *__restrict__ start)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long long c = AMVS_IDX((long long)before[j] + head[j] - 1, n_clusters);
    cluster_of[AMVS_IDX((long long)id[j], n)] = (unsigned)c;
    if (head[j]) start[c] = (unsigned)j;
    if (j == 0) start[n_clusters] = (unsigned)n;
}

// (3) one thread per cluster: the ordered sum over its run
__global__ __launch_bounds__(256) void representative_kernel(const float *__restrict__ verts, const unsigned char *__restrict__ rgb,
                                                             const unsigned *__restrict__ id, const unsigned *__restrict__ start,
                                                             long long n_vertices, long long n_clusters, float *__restrict__ verts_out,
                                                             unsigned char *__restrict__ rgb_out)
{
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_clusters) return;
    const unsigned r0 = start[c], r1 = start[c + 1];
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    unsigned long long cr = 0, cg = 0, cb = 0;
    for (unsigned r = r0; r < r1; ++r) {
        const long long v = AMVS_IDX((long long)id[AMVS_IDX((long long)r, n_vertices)], n_vertices);
        sx += verts[3 * v]; sy += verts[3 * v + 1]; sz += verts[3 * v + 2];
        cr += rgb[3 * v]; cg += rgb[3 * v + 1]; cb += rgb[3 * v + 2];
    }
    const unsigned long long count = r1 - r0;
    const float den = (float)(r1 - r0);
    verts_out[3 * c] = sx / den; verts_out[3 * c + 1] = sy / den; verts_out[3 * c + 2] = sz / den;
    rgb_out[3 * c] = (unsigned char)((2 * cr + count) / (2 * count));
    rgb_out[3 * c + 1] = (unsigned char)((2 * cg + count) / (2 * count));
    rgb_out[3 * c + 2] = (unsigned char)((2 * cb + count) / (2 * count));
}

// (4) the face in cluster ids, rotated to start at its smallest: group (a, lo, hi) and winding; live = no repeated id
__global__ __launch_bounds__(256) void face_triple_kernel(const int *__restrict__ faces, const unsigned *__restrict__ cluster_of,
                                                          long long n_faces, long long n_vertices, unsigned *__restrict__ ta,
                                                          unsigned *__restrict__ tlo, unsigned *__restrict__ thi,
                                                          unsigned char *__restrict__ even, unsigned *__restrict__ live)
{
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_faces) return;
    const unsigned g0 = cluster_of[AMVS_IDX((long long)faces[3 * f], n_vertices)];
    const unsigned g1 = cluster_of[AMVS_IDX((long long)faces[3 * f + 1], n_vertices)];
    const unsigned g2 = cluster_of[AMVS_IDX((long long)faces[3 * f + 2], n_vertices)];
    unsigned a = g0, b = g1, c = g2;
    if (g1 < g0 && g1 <= g2) { a = g1; b = g2; c = g0; }
    else if (g2 < g0 && g2 < g1) { a = g2; b = g0; c = g1; }
    ta[f] = a;
    tlo[f] = b < c ? b : c;
    thi[f] = b < c ? c : b;
    even[f] = b < c ? 1 : 0;
    live[f] = (g0 != g1 && g0 != g2 && g1 != g2) ? 1u : 0u;
}

// (4) the live faces in ascending index, with the first sort's keys
__global__ __launch_bounds__(256) void live_list_kernel(const unsigned *__restrict__ live, const unsigned *__restrict__ slot,
                                                        const unsigned *__restrict__ field, long long n_faces, long long n_live,
                                                        unsigned *__restrict__ perm, unsigned *__restrict__ key)
{
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_faces || !live[f]) return;
    const long long o = AMVS_IDX((long long)slot[f], n_live);
    perm[o] = (unsigned)f;
    key[o] = field[f];
}

// (4) the next sort's keys: a field of the faces in the permutation's order
__global__ __launch_bounds__(256) void gather_key_kernel(const unsigned *__restrict__ perm, const unsigned *__restrict__ field,
                                                         long long n_live, long long n_faces, unsigned *__restrict__ key)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_live) key[j] = field[AMVS_IDX((long long)perm[j], n_faces)];
}

__device__ __forceinline__ bool same_group(const unsigned *__restrict__ ta, const unsigned *__restrict__ tlo,
                                           const unsigned *__restrict__ thi, long long f, long long g)
{
    return ta[f] == ta[g] && tlo[f] == tlo[g] && thi[f] == thi[g];
}

// (4) one thread per position of the sorted permutation; the heads of the groups walk their group and keep at most
// one face.  keep[] is zero before.
__global__ __launch_bounds__(256) void group_decide_kernel(const unsigned *__restrict__ perm, const unsigned *__restrict__ ta,
                                                           const unsigned *__restrict__ tlo, const unsigned *__restrict__ thi,
                                                           const unsigned char *__restrict__ even, long long n_live, long long n_faces,
                                                           unsigned *__restrict__ keep)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_live) return;
    const long long f0 = AMVS_IDX((long long)perm[j], n_faces);
    if (j > 0 && same_group(ta, tlo, thi, f0, AMVS_IDX((long long)perm[j - 1], n_faces))) return;
    long long net = 0, first_even = -1, first_odd = -1;
    for (long long k = j; k < n_live; ++k) {
        const long long f = AMVS_IDX((long long)perm[k], n_faces);
        if (k > j && !same_group(ta, tlo, thi, f0, f)) break;
        if (even[f]) { ++net; if (first_even < 0) first_even = f; }
        else { --net; if (first_odd < 0) first_odd = f; }
    }
    if (net > 0) keep[first_even] = 1u;
    else if (net < 0) keep[first_odd] = 1u;
}

// quadric placement: one thread per old vertex walks its row of the vertex -> corner index; mean = the representatives
__global__ __launch_bounds__(256) void vertex_quadric_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                             const float *__restrict__ fn, const unsigned *__restrict__ row_start,
                                                             const unsigned *__restrict__ corners, const unsigned *__restrict__ cluster_of,
                                                             const float *__restrict__ mean, long long n_ids, long long n_vertices,
                                                             long long n_clusters, float *__restrict__ quadric)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vertices) return;
    const long long c = AMVS_IDX((long long)cluster_of[v], n_clusters);
    const float mx = mean[3 * c], my = mean[3 * c + 1], mz = mean[3 * c + 2];
    float q[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (unsigned r = row_start[v]; r < row_start[v + 1]; ++r) {
        const long long f = AMVS_IDX((long long)corners[AMVS_IDX((long long)r, n_ids)], n_ids) / 3;
        const long long v0 = AMVS_IDX((long long)faces[3 * f], n_vertices);
        const float ex = verts[3 * v0] - mx, ey = verts[3 * v0 + 1] - my, ez = verts[3 * v0 + 2] - mz;
        const float nx = fn[3 * f], ny = fn[3 * f + 1], nz = fn[3 * f + 2];
        const float d = (nx * ex + ny * ey) + nz * ez;
        q[0] += nx * nx; q[1] += nx * ny; q[2] += nx * nz; q[3] += ny * ny; q[4] += ny * nz; q[5] += nz * nz;
        q[6] += d * nx; q[7] += d * ny; q[8] += d * nz;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) quadric[9 * v + i] = q[i];
}

// quadric placement: one thread per cluster sums its members' quadrics along the run, solves and, where the candidate
// is accepted, overwrites the mean in pos; the others are counted, one add per wave
__global__ __launch_bounds__(256) void cluster_solve_kernel(const float *__restrict__ quadric, const unsigned *__restrict__ id,
                                                            const unsigned *__restrict__ start, long long n_vertices, long long n_clusters,
                                                            float regularisation, float cell, float *__restrict__ pos,
                                                            unsigned *__restrict__ n_fallback)
{
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool fallback = false;
    if (c < n_clusters) {
        float s[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (unsigned r = start[c]; r < start[c + 1]; ++r) {
            const long long v = AMVS_IDX((long long)id[AMVS_IDX((long long)r, n_vertices)], n_vertices);
#pragma unroll
            for (int i = 0; i < 9; ++i) s[i] += quadric[9 * v + i];
        }
        const float a00 = s[0], a01 = s[1], a02 = s[2], a11 = s[3], a12 = s[4], a22 = s[5], b0 = s[6], b1 = s[7], b2 = s[8];
        const float t = (a00 + a11) + a22;
        const float lam = regularisation * t;
        const float m00 = a00 + lam, m11 = a11 + lam, m22 = a22 + lam;
        const float l10 = a01 / m00, l20 = a02 / m00;
        const float d1 = m11 - l10 * a01;
        const float u12 = a12 - l20 * a01;
        const float l21 = u12 / d1;
        const float d2 = (m22 - l20 * a02) - l21 * u12;
        const float z1 = b1 - l10 * b0;
        const float z2 = (b2 - l20 * b0) - l21 * z1;
        const float y2 = z2 / d2;
        const float y1 = z1 / d1 - l21 * y2;
        const float y0 = (b0 / m00 - l10 * y1) - l20 * y2;
        const float cx = pos[3 * c] + y0, cy = pos[3 * c + 1] + y1, cz = pos[3 * c + 2] + y2;
        const float half = 0.5f * cell;
        const bool accept = t > 0.0f && d1 > 0.0f && d2 > 0.0f && isfinite(cx) && isfinite(cy) && isfinite(cz) &&
                            fabsf(y0) <= half && fabsf(y1) <= half && fabsf(y2) <= half;          // NaN is false
        if (accept) { pos[3 * c] = cx; pos[3 * c + 1] = cy; pos[3 * c + 2] = cz; }
        fallback = !accept;
    }
    const unsigned long long kept = __ballot(fallback);
    if (kept && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)kept) - 1)) atomicAdd(n_fallback, (unsigned)__popcll(kept));
}

// both placements: quadric == false is mesh_decimate, launch for launch
hipError_t decimate(TsdfState *s, ScratchCache &cache, const float origin[3], float cell, bool quadric, float regularisation,
                    long long *bad_vertex, long long *n_vertices, long long *n_faces, long long *n_fallback, hipStream_t st)
{
    const long long nv = s->n_vertices, nf = s->n_faces;
    const bool place = quadric && nv > 0 && nf > 0;      // without faces every cluster has t = 0 and keeps the mean
    *bad_vertex = -1;
    *n_vertices = nv; *n_faces = nf; *n_fallback = 0;
    long long nc = 0;
    if (nv > 0) {
        // (1), (2): nothing of the mesh or of its attributes is written before the range flag is back
        MCHK(s->dec_key.reserve((size_t)nv, cache)); MCHK(s->dec_key2.reserve((size_t)nv, cache));
        MCHK(s->dec_id.reserve((size_t)nv, cache)); MCHK(s->dec_id2.reserve((size_t)nv, cache));
        MCHK(s->dec_head.reserve((size_t)nv, cache)); MCHK(s->dec_before.reserve((size_t)nv, cache));
        MCHK(s->dec_cluster.reserve((size_t)nv, cache)); MCHK(s->dec_start.reserve((size_t)nv + 1, cache));
        MCHK(s->dec_flag.reserve(2, cache));
        MCHK(hipMemsetAsync(s->dec_flag.get(), 0xFF, 4, st));
        MCHK(launch(cell_key_kernel, nv, st, s->verts.get(), nv, Cells{origin[0], origin[1], origin[2], cell}, s->dec_key.get(),
                    s->dec_id.get(), s->dec_flag.get()));
        unsigned bad = DEC_NONE;
        MCHK(hipMemcpyAsync(&bad, s->dec_flag.get(), 4, hipMemcpyDeviceToHost, st));
        MCHK(hipStreamSynchronize(st));
        if (bad != DEC_NONE) { *bad_vertex = (long long)bad; return hipSuccess; }
        MCHK(sort_pairs(s, cache, (const unsigned long long *)s->dec_key.get(), s->dec_key2.get(), (const unsigned *)s->dec_id.get(),
                        s->dec_id2.get(), nv, 63, st));
        MCHK(launch(key_head_kernel, nv, st, s->dec_key2.get(), nv, s->dec_head.get()));
        MCHK(exclusive_scan(s, cache, s->dec_head.get(), s->dec_before.get(), nv, st));
        MCHK(scan_total(s->dec_head.get(), s->dec_before.get(), nv, &nc, st));
        MCHK(launch(cluster_map_kernel, nv, st, s->dec_id2.get(), s->dec_head.get(), s->dec_before.get(), nv, nc, s->dec_cluster.get(),
                    s->dec_start.get()));
        if (place) {
            // the index and the face normals of the mesh as it still is
            MCHK(ensure_index(s, cache, st));
            MCHK(mesh_face_normals(s, cache, st));
            MCHK(s->dec_quadric.reserve(9 * (size_t)nv, cache));
        }
    }
    const int *const old_faces = s->faces.get();
    s->topology_changed();
    long long kept_f = 0, kept_v = 0;
    if (nf > 0 && nv > 0) {
        // (4) before (3): the faces still hold the old ids
        MCHK(s->dec_ta.reserve((size_t)nf, cache)); MCHK(s->dec_tlo.reserve((size_t)nf, cache)); MCHK(s->dec_thi.reserve((size_t)nf, cache));
        MCHK(s->dec_even.reserve((size_t)nf, cache));
        MCHK(s->dec_fkey.reserve((size_t)nf, cache)); MCHK(s->dec_fkey2.reserve((size_t)nf, cache));
        MCHK(s->dec_perm.reserve((size_t)nf, cache)); MCHK(s->dec_perm2.reserve((size_t)nf, cache));
        MCHK(s->fkeep.reserve((size_t)nf, cache)); MCHK(s->fnew.reserve((size_t)nf, cache));
        MCHK(launch(face_triple_kernel, nf, st, s->faces.get(), s->dec_cluster.get(), nf, nv, s->dec_ta.get(), s->dec_tlo.get(),
                    s->dec_thi.get(), s->dec_even.get(), s->fkeep.get()));
        long long n_live = 0;
        MCHK(exclusive_scan(s, cache, s->fkeep.get(), s->fnew.get(), nf, st));
        MCHK(scan_total(s->fkeep.get(), s->fnew.get(), nf, &n_live, st));
        if (n_live > 0) {
            const int bits = bits_for(nc);
            MCHK(launch(live_list_kernel, nf, st, s->fkeep.get(), s->fnew.get(), s->dec_thi.get(), nf, n_live, s->dec_perm.get(),
                        s->dec_fkey.get()));
            MCHK(sort_pairs(s, cache, (const unsigned *)s->dec_fkey.get(), s->dec_fkey2.get(), (const unsigned *)s->dec_perm.get(),
                            s->dec_perm2.get(), n_live, bits, st));
            const unsigned *const fields[2] = {s->dec_tlo.get(), s->dec_ta.get()};
            for (const unsigned *field : fields) {
                std::swap(s->dec_perm, s->dec_perm2);
                MCHK(launch(gather_key_kernel, n_live, st, s->dec_perm.get(), field, n_live, nf, s->dec_fkey.get()));
                MCHK(sort_pairs(s, cache, (const unsigned *)s->dec_fkey.get(), s->dec_fkey2.get(), (const unsigned *)s->dec_perm.get(),
                                s->dec_perm2.get(), n_live, bits, st));
            }
            MCHK(hipMemsetAsync(s->fkeep.get(), 0, 4 * (size_t)nf, st));
            MCHK(launch(group_decide_kernel, n_live, st, s->dec_perm2.get(), s->dec_ta.get(), s->dec_tlo.get(), s->dec_thi.get(),
                        s->dec_even.get(), n_live, nf, s->fkeep.get()));
            // the kept faces in their order, in cluster ids and their own corner order
            MCHK(compact_faces(s, cache, nv, nf, s->dec_cluster.get(), &kept_f, st));
        }
    }
    unsigned fallback = 0;
    if (kept_f > 0 || place) {
        // (3) into the second buffers
        MCHK(launch(representative_kernel, nc, st, s->verts.get(), s->rgb.get(), s->dec_id2.get(), s->dec_start.get(), nv, nc,
                    s->verts2.get(), s->rgb2.get()));
    }
    if (place) {
        // the quadrics read the old faces (step (4) may have swapped them away) and the old positions; the count comes
        // back with the next read-back
        MCHK(hipMemsetAsync(s->dec_flag.get() + 1, 0, 4, st));
        MCHK(launch(vertex_quadric_kernel, nv, st, s->verts.get(), old_faces, s->face_normal.get(), s->row_start.get(),
                    s->corners.get(), s->dec_cluster.get(), s->verts2.get(), 3 * nf, nv, nc, s->dec_quadric.get()));
        MCHK(launch(cluster_solve_kernel, nc, st, s->dec_quadric.get(), s->dec_id2.get(), s->dec_start.get(), nv, nc, regularisation,
                    cell, s->verts2.get(), s->dec_flag.get() + 1));
        MCHK(hipMemcpyAsync(&fallback, s->dec_flag.get() + 1, 4, hipMemcpyDeviceToHost, st));
    }
    if (kept_f > 0) {
        // (5) back into the first buffers
        std::swap(s->verts, s->verts2);
        std::swap(s->rgb, s->rgb2);
    }
    MCHK(drop_unused_vertices(s, cache, nc, kept_f, &kept_v, st));
    MCHK(hipStreamSynchronize(st));
    s->n_vertices = kept_v; s->n_faces = kept_f;
    *n_vertices = kept_v; *n_faces = kept_f;
    *n_fallback = place ? (long long)fallback : nc;
    return hipSuccess;
}

}  // namespace

hipError_t mesh_decimate(TsdfState *s, ScratchCache &cache, const float origin[3], float cell, long long *bad_vertex,
                         long long *n_vertices, long long *n_faces, hipStream_t st)
{
    long long n_fallback = 0;
    return decimate(s, cache, origin, cell, false, 0.0f, bad_vertex, n_vertices, n_faces, &n_fallback, st);
}

hipError_t mesh_decimate_quadric(TsdfState *s, ScratchCache &cache, const float origin[3], float cell, float regularisation,
                                 long long *bad_vertex, long long *n_vertices, long long *n_faces, long long *n_fallback,
                                 hipStream_t st)
{
    return decimate(s, cache, origin, cell, true, regularisation, bad_vertex, n_vertices, n_faces, n_fallback, st);
}

}  // namespace amvs

AMVS_CHECK_TU(mesh_decimate)
