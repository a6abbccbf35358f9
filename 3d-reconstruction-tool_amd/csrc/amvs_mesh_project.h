// amvs_mesh_project.h -- the device functions amvs_mesh_render.hip and amvs_mesh_color.hip share: projection (a) of
// include/amvs.h amvs_mesh_render, the face set-up (b) and the integer edge function of the coverage (c).  Both units
// must form these bit for bit alike (the colour render sets a face up again for the pixel the rasteriser gave it), so
// they are stated once.  Everything is __forceinline__ and sits in the unit's anonymous namespace: no symbol, and the
// kernels of amvs_mesh_render.hip compile to the instructions they had when the functions stood in that file
// (DESIGN.md section 8 "Colours from the views").  Include after amvs_check.h (AMVS_TU_ID) and amvs_mesh_state.h
// (Kmat).  A violation of the AMVS_IDX in face_setup is reported with the including unit's id and a line of THIS file.
#pragma once
#include "amvs_check.h"
#include "amvs_mesh_state.h"

namespace amvs {

namespace {

constexpr int SUB_SHIFT = 8;                  // 256 fixed-point steps per pixel
constexpr float SUB = 256.0f;
constexpr float UV_LIMIT = 1048576.0f;        // 2^20 pixels: coordinates fit 2^28, products of differences 2^58

// (a) of the definition: camera coordinates and image position of a world point, every operation rounded on its own
struct Projected { float xc, yc, zc, u, v; };

__device__ __forceinline__ Projected project(const float *__restrict__ P, const Kmat &K, float X, float Y, float Z)
{
    Projected r;
    r.zc = ((P[6] * X + P[7] * Y) + P[8] * Z) + P[11];
    r.xc = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[9];
    r.yc = ((P[3] * X + P[4] * Y) + P[5] * Z) + P[10];
    const float pu = (K.k[0] * r.xc + K.k[1] * r.yc) + K.k[2] * r.zc;
    const float pv = (K.k[3] * r.xc + K.k[4] * r.yc) + K.k[5] * r.zc;
    const float pw = (K.k[6] * r.xc + K.k[7] * r.yc) + K.k[8] * r.zc;
    r.u = pu / pw;
    r.v = pv / pw;
    return r;
}

// a face ready to draw: corners in the order the coverage uses (area > 0), box clamped to the image; flip says that the
// second and third corner were exchanged
struct FaceSetup {
    int x0, y0, x1, y1, x2, y2;
    float iz0, iz1, iz2;
    long long area;
    int lo_x, lo_y, bw, bh;
    bool flip;
};

enum { FACE_DRAWS = 0, FACE_SKIPPED = 1, FACE_EMPTY = 2 };

__device__ __forceinline__ int face_setup(const float *__restrict__ verts, const int *__restrict__ faces, long long f,
                                          long long n_vertices, const float *__restrict__ P, const Kmat &K, float near, int H, int W,
                                          FaceSetup &s)
{
    int x[3], y[3];
    float iz[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long v = AMVS_IDX((long long)faces[3 * f + k], n_vertices);
        const Projected p = project(P, K, verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]);
        const bool usable = p.zc > near && fabsf(p.u) <= UV_LIMIT && fabsf(p.v) <= UV_LIMIT;      // false for NaN
        ok = ok && usable;
        x[k] = usable ? (int)rintf(p.u * SUB) : 0;
        y[k] = usable ? (int)rintf(p.v * SUB) : 0;
        iz[k] = 1.0f / p.zc;
    }
    if (!ok) return FACE_SKIPPED;
    long long area = (long long)(x[1] - x[0]) * (long long)(y[2] - y[0]) - (long long)(y[1] - y[0]) * (long long)(x[2] - x[0]);
    if (area == 0) return FACE_EMPTY;
    const bool flip = area < 0;
    s.flip = flip;
    s.x0 = x[0]; s.y0 = y[0]; s.iz0 = iz[0];
    s.x1 = flip ? x[2] : x[1]; s.y1 = flip ? y[2] : y[1]; s.iz1 = flip ? iz[2] : iz[1];
    s.x2 = flip ? x[1] : x[2]; s.y2 = flip ? y[1] : y[2]; s.iz2 = flip ? iz[1] : iz[2];
    s.area = flip ? -area : area;
    // pixels with 256 px inside [min, max]: ceil(min / 256) .. floor(max / 256) (arithmetic shifts), clamped
    const int min_x = min(x[0], min(x[1], x[2])), max_x = max(x[0], max(x[1], x[2]));
    const int min_y = min(y[0], min(y[1], y[2])), max_y = max(y[0], max(y[1], y[2]));
    s.lo_x = max((min_x + 255) >> SUB_SHIFT, 0);
    s.lo_y = max((min_y + 255) >> SUB_SHIFT, 0);
    s.bw = min(max_x >> SUB_SHIFT, W - 1) - s.lo_x + 1;
    s.bh = min(max_y >> SUB_SHIFT, H - 1) - s.lo_y + 1;
    return s.bw > 0 && s.bh > 0 ? FACE_DRAWS : FACE_EMPTY;
}

// edge a -> b against the point (px, py): the edge function, and whether the point is on the edge's inner side
__device__ __forceinline__ bool edge_inside(int ax, int ay, int bx, int by, int px, int py, long long &w)
{
    const int dx = bx - ax, dy = by - ay;
    w = (long long)dx * (long long)(py - ay) - (long long)dy * (long long)(px - ax);
    return w > 0 || (w == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

inline Kmat kmat_of(const float K[9])
{
    Kmat k;
    for (int i = 0; i < 9; ++i) k.k[i] = K[i];
    return k;
}

}  // namespace

}  // namespace amvs
