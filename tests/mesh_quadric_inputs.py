"""Hand-built inputs for the quadric-placement tests (a helper module, not a conftest; seeded, no GPU): what the meshes
of mesh_volumes.small_volumes(), mesh_clean_inputs.hand_built() and mesh_decimate_inputs lack.  Each is a
mesh_decimate_inputs.Case (name, vertices, faces, colours, cluster origin, cell) with two more attributes: `unit` (the
grids of the GPU comparison are cells of 2 and 3 units) and `regularisation` (None: any; a number: the value at which the
case shows what it was built for).  `target` is a point inside the cluster the case is about.

    flat            one cell holds a vertex of a sheet of large faces and seven vertices of a parallel sheet of small
                    ones, 0.25 apart along the common normal (1, 2, 2) / 3: all normals parallel, the mean lies near the
                    small sheet, the quadric minimum near the large one; accepted, and y is along the normal
    isolated        three vertices that no face uses in a cell of their own: t = 0
    zero_area       a face whose three vertices lie on one line, and a face with two vertices at the same position:
                    normals of zeros, clusters with t = 0 although they have faces
    wedge           two sheets z = 0.5 +- 0.5 x; the cluster holds their vertices at x = 0.7 and 0.95, the ridge x = 0
                    lies outside the half-cell bound
    singular        regularisation 1e-12 and coordinates that make every product exact: a triangle in the plane
                    x + y = 1 (a00 = a01 = a11: d1 = a11 - 1 * a01 = 0) and one in y + z = 1 (a00 = 0, a11 = a12 = a22:
                    d2 = a22 - 1 * a12 = 0), lam = 1e-12 t below half an ulp of either
    overflow_b      one cell of side 4e10 holds two parallel sheets 1e10 apart with normals of 9e14: a is finite
                    (8.1e29 per corner), d = 4.5e24 and b = d n overflows: t, d1, d2 pass, the candidate is not finite
    overflow_a      an octahedron with positions at 5e18: the normals are 2.5e37 (their sums stay finite, so that the
                    vertex normals computed afterwards hold no NaN), a is infinite, d1 is NaN
    pile            mesh_decimate_inputs.pile: a cluster of 300 members
    rotated_box     a Volume: 49^3 points on [-1, 1]^3, the box of half-extents (0.55, 0.4, 0.3) rotated by 0.3 rad
                    about x, then 0.4 rad about z, trunc 0.1: faces, edges and corners at no special angle
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_decimate_inputs as di  # noqa: E402
import mesh_volumes as mv  # noqa: E402

F32 = np.float32
NORMAL = np.array([1.0, 2.0, 2.0]) / 3.0
_U = np.array([2.0, -2.0, 1.0]) / 3.0
_W = np.array([2.0, 1.0, -2.0]) / 3.0


def _case(name, verts, faces, origin, cell, seed, unit=None, regularisation=None, target=None):
    c = di.Case(name, verts, faces, origin, cell, seed=seed)
    c.unit = F32(cell) / F32(2) if unit is None else F32(unit)
    c.regularisation = regularisation
    c.target = None if target is None else np.asarray(target, np.float64)
    return c


def _fan(centre, radius, n, base):
    ang = 2 * np.pi * (np.arange(n) + 0.25) / n
    rim = centre + radius * (np.cos(ang)[:, None] * _U + np.sin(ang)[:, None] * _W)
    i = np.arange(n)
    faces = np.stack([np.full(n, base), base + 1 + i, base + 1 + (i + 1) % n], -1)
    return np.concatenate([[centre], rim]), faces


def flat():
    c = np.array([0.5, 0.5, 0.5])
    va, fa = _fan(c - 0.15 * NORMAL, 2.0, 6, 0)
    vb, fb = _fan(c + 0.10 * NORMAL, 0.2, 6, len(va))
    return _case("flat cluster", np.concatenate([va, vb]), np.concatenate([fa, fb]), (0.0, 0.0, 0.0), 1.0, 41, target=c)


def isolated():
    v = [(0.2, 0.2, 0.2), (1.3, 0.2, 0.2), (0.2, 1.3, 0.2), (5.2, 5.3, 5.4), (5.6, 5.5, 5.1), (5.4, 5.8, 5.7)]
    return _case("isolated vertices in one cell", v, [(0, 1, 2)], (0.0, 0.0, 0.0), 1.0, 42, target=(5.5, 5.5, 5.5))


def zero_area():
    v = [(0.25, 0.5, 0.5), (1.25, 0.5, 0.5), (2.5, 0.5, 0.5),          # on one line
         (0.5, 2.5, 0.5), (0.5, 2.5, 0.5), (1.5, 2.5, 0.5)]           # two at the same position
    return _case("zero-area faces", v, [(0, 1, 2), (3, 4, 5)], (0.0, 0.0, 0.0), 1.0, 43, target=(0.5, 0.5, 0.5))


def wedge():
    xs, ys = (0.7, 0.95, 1.5, 2.5), (0.2, 0.8, 1.4)
    verts, faces = [], []
    for sign in (1.0, -1.0):
        base = len(verts)
        verts += [(x, y, 0.5 + sign * 0.5 * x) for y in ys for x in xs]
        for j in range(len(ys) - 1):
            for i in range(len(xs) - 1):
                a, b, c, d = (base + j * len(xs) + i, base + j * len(xs) + i + 1, base + (j + 1) * len(xs) + i,
                              base + (j + 1) * len(xs) + i + 1)
                faces += [(a, b, d), (a, d, c)] if sign > 0 else [(a, d, b), (a, c, d)]
    return _case("sharp wedge", verts, faces, (0.0, 0.0, -2.0), 1.0, 44, target=(0.8, 0.5, 0.5))


SINGULAR_REGULARISATION = 1e-12


def singular():
    v = [(0.25, 0.75, 0.25), (0.75, 0.25, 0.25), (0.5, 0.5, 0.75),        # x + y = 1: normal (-1/4, -1/4, 0)
         (2.25, 0.25, 0.75), (2.25, 0.75, 0.25), (2.75, 0.5, 0.5),        # y + z = 1: normal (0, -1/4, -1/4)
         (4.5, 0.5, 0.5), (5.5, 0.5, 0.5), (4.5, 1.5, 0.5)]               # a face that stays
    return _case("singular solves", v, [(0, 1, 2), (3, 4, 5), (6, 7, 8)], (0.0, 0.0, 0.0), 1.0, 45,
                 regularisation=SINGULAR_REGULARISATION)


def overflow_b():
    s, e = 1e10, 3e7
    v = [(s, s, s), (s + e, s, s), (s, s + e, s), (s, s, 2 * s), (s + e, s, 2 * s), (s, s + e, 2 * s)]
    return _case("overflow of b", v, [(0, 1, 2), (3, 4, 5)], (0.0, 0.0, 0.0), 4e10, 46, target=(s, s, s))


def overflow_a():
    ov, of = __import__("mesh_clean_inputs").octahedron()
    return _case("positions near 1e19", ov * 5e18, of, (0.0, 0.0, 0.0), 2e18, 47)


def pile():
    c = di.pile()
    c.unit, c.regularisation, c.target = F32(c.cell) / F32(2), None, np.array([0.5, 0.5, 0.5])
    return c


def hand_built():
    return [pile(), flat(), isolated(), zero_area(), wedge(), singular(), overflow_b(), overflow_a()]


BOX_HALF = np.array([0.55, 0.4, 0.3])
BOX_ROTATION = mv._rot(0.3, 0.0, 0.4)                           # Rz(0.4) Rx(0.3)


def box_distance(points):
    """Unsigned distance of every point (float64) to the surface of the rotated box."""
    local = np.asarray(points, np.float64) @ BOX_ROTATION          # R^T p, as rows
    q = np.abs(local) - BOX_HALF
    sdf = np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)
    return np.abs(sdf)


def rotated_box(n=49, trunc=0.1):
    origin = np.array([-1.0, -1.0, -1.0], F32)
    voxel = F32(2.0 / (n - 1))
    ax = [(origin[a] + np.arange(n, dtype=np.int64).astype(F32) * voxel).astype(np.float64) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    local = np.stack([x, y, z], -1) @ BOX_ROTATION
    q = np.abs(local) - BOX_HALF
    sdf = np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)
    tsdf = np.clip(sdf / trunc, -1.0, 1.0).astype(F32)
    weight = np.full(tsdf.shape, 2.0, F32)
    return mv.Volume(f"rotated box {n}^3", tsdf, weight, mv._position_colours(tsdf.shape, weight), origin, voxel)
