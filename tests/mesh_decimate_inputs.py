"""Hand-built inputs for the decimation tests (a helper module, not a conftest; seeded, no GPU): what the meshes of
mesh_volumes.small_volumes() and mesh_clean_inputs.hand_built() lack.  Each is a Case(name, vertices (V,3) float32,
faces (F,3) int32, colours (V,3) uint8, cluster origin, cell, accepted):

    windings        per (forward, backward) pair of WINDINGS three cells with four vertices each and forward + backward
                    faces with one corner in each cell, wound one way or the other: groups with net = +-2 and +-3, with
                    and without faces of the other winding, net = 0 with two faces on either side, and plain net = +-1;
                    the faces are shuffled, so the face that stays is seldom the first of its group
    pile            PILE vertices in one cell and a face from each to the same two others, all wound alike: a cluster
                    whose ordered sum is PILE terms long, and one group of PILE same-wound faces
    around_origin   a sphere around (0, 0, 0) with the cluster origin inside it: cell indices of either sign, and
                    vertices exactly at q = -1.0 and q = -0.0 (p = -0.0 on a grid whose origin is +0.0)
    range_edges     origin 0, cell 1, a triangle with one coordinate at an edge of the index range: 1 048 575.5 and
                    -1 048 576.0 are the last cells inside, 1 048 576.0 and -1 048 576.5 the first ones outside
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_volumes as mv  # noqa: E402

F32 = np.float32
# (faces wound (A, B, C), faces wound (A, C, B)) on one triple of cells
WINDINGS = ((2, 0), (0, 2), (3, 0), (0, 3), (3, 1), (1, 3), (4, 1), (1, 4), (4, 2), (2, 4), (2, 2), (1, 1), (1, 0), (0, 1))
PILE = 300


class Case:
    def __init__(self, name, verts, faces, origin, cell, accepted=True, seed=0):
        self.name = name
        self.verts = np.ascontiguousarray(verts, F32).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        self.colors = np.random.default_rng(2000 + seed).integers(0, 256, self.verts.shape, dtype=np.uint8)
        self.origin = np.asarray(origin, F32).reshape(3)
        self.cell = F32(cell)
        self.accepted = accepted

    def arrays(self):
        return self.verts, self.faces, self.colors


def windings(seed=21):
    """Cells of side 1 on the origin 0; triple n occupies the cells (4 n, 0, 0), (4 n + 1, 0, 0) and (4 n, 1, 0)."""
    rng = np.random.default_rng(seed)
    verts, faces = [], []
    for n, (fwd, bwd) in enumerate(WINDINGS):
        base = len(verts)
        for corner in ((4 * n, 0, 0), (4 * n + 1, 0, 0), (4 * n, 1, 0)):
            verts += [np.array(corner) + rng.uniform(0.1, 0.9, 3) for _ in range(4)]
        for _ in range(fwd + bwd):
            a, b, c = (base + 4 * k + int(rng.integers(4)) for k in range(3))
            faces.append((a, b, c) if len(faces) % 2 else (b, c, a))      # any rotation is the same winding
        for k in range(bwd):
            a, b, c = faces[-1 - k]
            faces[-1 - k] = (a, c, b)
    faces = np.array(faces)[rng.permutation(len(faces))]
    return Case("windings", np.array(verts), faces, (0.0, 0.0, 0.0), 1.0, seed=seed)


def pile(n=PILE, seed=22):
    rng = np.random.default_rng(seed)
    verts = np.concatenate([rng.uniform(0.05, 0.95, (n, 3)), [(1.5, 0.5, 0.5), (0.5, 1.5, 0.5)]])
    faces = np.stack([np.arange(n), np.full(n, n), np.full(n, n + 1)], -1)
    return Case(f"pile of {n}", verts, faces, (0.0, 0.0, 0.0), 1.0, seed=seed)


def around_origin(seed=23):
    """sphere_volume(17)'s mesh (radius 0.8 around 0) on a grid with origin (0, 0.01, -0.02) and cell 0.1875, and one
    more face with a vertex at x = -cell (q = -1.0 exactly) and one at x = -0.0 (q = -0.0: cell 0, not cell -1)."""
    v, f, _ = mv.sphere_volume(17, trunc=0.3).extract()
    cell = F32(0.1875)
    extra = np.array([(-cell, 0.3, 0.3), (-0.0, 0.3, 0.3), (0.25, 0.45, 0.3)], F32)
    n = len(v)
    return Case("sphere around the cluster origin", np.concatenate([v, extra]), np.concatenate([f, [(n, n + 1, n + 2)]]),
                (0.0, 0.01, -0.02), cell, seed=seed)


RANGE_EDGES = ((1048575.5, True), (-1048576.0, True), (1048576.0, False), (-1048576.5, False))


def range_edges():
    """One case per (axis, coordinate): a triangle near 0 with a further vertex at the edge coordinate on that axis."""
    out = []
    for axis in range(3):
        for n, (x, ok) in enumerate(RANGE_EDGES):
            v = np.array([(0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (0.5, 1.5, 0.5), (0.5, 0.5, 1.5)], F32)
            v[3, axis] = x
            out.append(Case(f"range edge {x} on axis {axis}", v, [(0, 1, 2), (0, 2, 3), (2, 1, 3)], (0.0, 0.0, 0.0), 1.0,
                            accepted=ok, seed=30 + 4 * axis + n))
    return out


def accepted_cases():
    return [pile(), windings(), around_origin()] + [c for c in range_edges() if c.accepted]


def refused_cases():
    return [c for c in range_edges() if not c.accepted]
