// amvs_mesh_state.h -- what the surface-mesh translation units share: the context's volume-and-mesh state
// (amvs_mesh.hip builds the mesh, amvs_mesh_fill.hip grows the volume into unobserved space, amvs_mesh_clean.hip and
// amvs_mesh_decimate.hip work on the mesh in place,
// amvs_mesh_render.hip draws it into views and filters it by what they see, amvs_mesh_color.hip colours it from the
// views' images and shades the render, amvs_mesh_texture.hip textures it from them), the rule of what goes stale when the
// mesh changes, and the declarations of the device code they share: the scans and the sort with their scratch, and
// the compaction of the kept faces and the used vertices (extraction pass (d)).  That code is compiled once, in
// amvs_mesh.hip: an index violation in it is reported with that unit's id and a line of that file.
#pragma once
#include "amvs_check.h"
#include "amvs_buffer.h"

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
    bool have_fill = false;                       // fill_gen holds the generations of a fill of the current volume
    DeviceBuffer<unsigned char> fill_gen;         // [n] (amvs_mesh_fill.hip)
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

    // ---- texture (amvs_mesh_texture.hip): the atlas and the UVs are attributes of the current mesh and its colours ----
    bool have_texture = false;
    int tex_N = 0, tex_cols = 0, tex_W = 0, tex_H = 0;    // texel intervals per leg, cells per row, atlas width and height
    DeviceBuffer<unsigned char> tex_atlas;        // [tex_H][tex_W][3] RGB
    DeviceBuffer<float> tex_uv;                   // [F][3][2]

    // What is still current after every operation (anything else of the mesh's attributes is stale):
    //
    //   operation                                          still current afterwards        set by it
    //   tsdf_integrate, tsdf_set_volume, tsdf_extract,     nothing                         the mesh (extract, set)
    //     mesh_set
    //   tsdf_fill (changes the volume, not its grid)       nothing                         nothing
    //   mesh_filter_components, label only or nothing      index, pinned                   labels; normals and render are
    //     removed                                                                          dropped although the mesh is unchanged
    //   mesh_filter_components, something removed          nothing                         labels, in the new numbering
    //   mesh_smooth, any iteration count, 0 included       index, pinned, labels           nothing; normals and render dropped
    //   mesh_normals                                       everything                      normals
    //   mesh_decimate, mesh_decimate_quadric               nothing                         nothing
    //   the same, refused for a vertex outside the grid    everything, mesh untouched      nothing
    //   mesh_render                                        index, pinned, labels, normals  render; visibility dropped
    //   mesh_visibility                                    all of these and the render     visibility
    //   mesh_filter_visible, also when nothing is removed  nothing                         nothing
    //   mesh_color_views (needs render and normals)        everything: positions, faces,   the colours of the vertices a
    //                                                      index, pinned, labels, normals, view reached
    //                                                      render, visibility
    //                                                                                      the texture is dropped: its
    //                                                                                      fall-back colours changed
    //   fetch_render_color                                 everything                      nothing
    //   mesh_texture (needs render)                        everything                      texture
    //   fetch_mesh_texture, fetch_render_texture           everything                      nothing
    //
    // The texture outlives what does not touch positions, faces or colours: mesh_normals, mesh_render (the mesh may be
    // drawn again from other cameras and shaded with the atlas), mesh_visibility and every fetch keep it.  Every other
    // row of the table drops it, through positions_changed().
    //
    // Every function that changes the mesh calls the one of these that applies, and so does the shared compaction
    // (amvs_mesh.hip) before it moves a face or a vertex.

    // the mesh is drawn again or differs from its picture: the maps and the counts are stale
    void drop_views() { have_render = have_visibility = false; }

    // vertices moved, faces and ids as they were: what was computed from the positions is stale
    void positions_changed()
    {
        have_normals = have_texture = false;
        drop_views();
    }

    // faces or vertex ids changed: so is everything that is indexed by them
    void topology_changed()
    {
        have_csr = have_pinned = have_labels = false;
        positions_changed();
    }

    // the mesh is about to be replaced: nothing derived from it stays
    void drop_mesh()
    {
        have_mesh = false;
        topology_changed();
    }
};

inline dim3 grid_of(long long n) { return dim3((unsigned)((n + 255) / 256)); }

// one thread per element, 256 to a workgroup, on `st`; n > 0 is the caller's business, as with the launch itself
template <class... P, class... A>
inline hipError_t launch(void (*kernel)(P...), long long n, hipStream_t st, A... args)
{
    hipLaunchKernelGGL(kernel, grid_of(n), dim3(256), 0, st, static_cast<P>(args)...);
    return hipGetLastError();
}
inline size_t at_least_one(long long n) { return (size_t)(n > 0 ? n : 1); }

namespace {
// intrinsics as a kernel argument.  Per unit on purpose: the symbol names of the kernels that take one carry it.
struct Kmat { float k[9]; };
}  // namespace

// ---- amvs_mesh.hip: device code every mesh unit uses, compiled there once -----------------------------------

// exclusive sum of in[0 .. n) into out; the scratch is the state's
hipError_t exclusive_scan(TsdfState *s, ScratchCache &cache, const unsigned *in, unsigned *out, long long n, hipStream_t st);
// total of an exclusive scan, read back: base[n-1] + count[n-1].  n > 0.  Synchronises.
hipError_t scan_total(const unsigned *count, const unsigned *base, long long n, long long *total, hipStream_t st);
// key bits that tell n values apart, 1 .. 32
int bits_for(long long n);
// stable sort of (key, value) pairs on the low `bits` bits of the key; K = unsigned or unsigned long long
template <class K>
hipError_t sort_pairs(TsdfState *s, ScratchCache &cache, const K *key_in, K *key_out, const unsigned *val_in, unsigned *val_out,
                      long long n, int bits, hipStream_t st);

// The faces f with fkeep[f] != 0 stay, in their order; with `vertex_map` their ids go through it (its extent: nv).
// Scans fkeep into fnew, reads the total back (one synchronisation) and, unless every face stays as it is, writes the
// kept ones into faces2 and swaps.  nf == 0 and *kept_f == 0 launch nothing.
hipError_t compact_faces(TsdfState *s, ScratchCache &cache, long long nv, long long nf, const unsigned *vertex_map,
                         long long *kept_f, hipStream_t st);
// Extraction pass (d): of nv vertices those that none of the first nf faces uses leave, the others keep their order and
// the faces are renumbered.  Leaves the used flags in vused and the new ids in vnew; one synchronisation.  Nothing
// moves when every vertex is used; nv == 0 or nf == 0 launch nothing and keep nothing.
hipError_t drop_unused_vertices(TsdfState *s, ScratchCache &cache, long long nv, long long nf, long long *kept_v, hipStream_t st);

struct Compaction {
    long long kept_f = 0, kept_v = 0;
    bool removed = false;             // a face or a vertex left
};
// compact_faces without a map, then drop_unused_vertices, then the counts of the state; the caller synchronises
hipError_t compact_mesh(TsdfState *s, ScratchCache &cache, Compaction *out, hipStream_t st);

}  // namespace amvs
