"""Hand-built meshes for the clean-up tests (a helper module, not a conftest; seeded, no GPU), next to the meshes
that mesh_volumes.small_volumes() extracts.  Each is a Mesh(name, vertices (V,3) float32, faces (F,3) int32, colours
(V,3) uint8):

    open_book          three faces on one edge, their other edges on one face each (everything pinned)
    closed_book        three faces on the edge a-b with every other edge on two or three faces: a and b lie on a
                       three-face edge and are not pinned
    fan                FAN_FACES faces round one vertex, closed: the centre has a row of FAN_FACES corners and is free,
                       the rim is pinned
    strip              STRIP_FACES faces in a line, vertex ids shuffled by a seeded permutation
    tie                two tetrahedra, 4 faces each; the faces of the one with the larger ids come first
    coincident         two faces on the same three vertices, wound oppositely: normal sums exactly zero, area not
    isolated           a quad with vertices that no face uses among its ids
    threshold          an octahedron (MIN_FACES faces) and an open fan of MIN_FACES - 1 faces
    empty, vertices_only, single_face
"""
import numpy as np

F32 = np.float32
FAN_FACES = 1200
STRIP_FACES = 100_000
MIN_FACES = 8


class Mesh:
    def __init__(self, name, verts, faces, seed=0):
        self.name = name
        self.verts = np.ascontiguousarray(verts, F32).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        self.colors = np.random.default_rng(1000 + seed).integers(0, 256, self.verts.shape, dtype=np.uint8)

    def arrays(self):
        return self.verts, self.faces, self.colors


def _jitter(seed, pts, scale=0.05):
    pts = np.asarray(pts, np.float64)
    return pts + scale * np.random.default_rng(seed).standard_normal(pts.shape)


def open_book():
    v = _jitter(1, [(0, 0, 1), (0, 0, -1), (1, 0, 0), (-0.5, 0.9, 0), (-0.5, -0.9, 0)])
    return Mesh("open book", v, [(0, 1, 2), (1, 0, 3), (0, 1, 4)], 1)


def closed_book():
    """a = 0, b = 1, apexes 2, 3, 4.  Pages (a, b, c_i); roofs (a, c_i, c_j) and floors (b, c_j, c_i).  Edge a-b and the
    edges a-c_i, b-c_i are on three faces, c_i-c_j on two."""
    v = _jitter(2, [(0, 0, 1), (0, 0, -1), (1, 0, 0), (-0.5, 0.9, 0), (-0.5, -0.9, 0)])
    f = [(0, 1, 2), (0, 1, 3), (0, 1, 4)]
    for i, j in ((2, 3), (3, 4), (4, 2)):
        f += [(0, i, j), (1, j, i)]
    return Mesh("closed book", v, f, 2)


def fan(n=FAN_FACES, closed=True, seed=3):
    """n faces (0, i, i + 1) round vertex 0: closed on n rim vertices, open on n + 1."""
    m = n if closed else n + 1
    ang = 2 * np.pi * np.arange(m) / (n + 1 - closed)
    rim = np.stack([np.cos(ang), np.sin(ang), 0.1 * np.sin(5 * ang)], -1)
    v = _jitter(seed, np.concatenate([[(0.1, -0.2, 0.5)], rim]), 0.01)
    i = np.arange(1, n + 1)
    f = np.stack([np.zeros(n, np.int64), i, i % m + 1 if closed else i + 1], -1)
    return Mesh(f"{'closed' if closed else 'open'} fan of {n} faces", v, f, seed)


def strip(n_faces=STRIP_FACES, seed=4):
    q = n_faces // 2
    x = np.arange(q + 1, dtype=np.float64) * 0.01
    v = np.concatenate([np.stack([x, np.zeros_like(x), np.sin(x)], -1), np.stack([x, np.full_like(x, 0.01), np.cos(x)], -1)])
    lo, hi = np.arange(q), np.arange(q) + q + 1
    f = np.concatenate([np.stack([lo, lo + 1, hi], -1), np.stack([lo + 1, hi + 1, hi], -1)])
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(v))                               # old id -> new id
    out = np.empty_like(v)
    out[perm] = v
    return Mesh(f"shuffled strip of {len(f)} faces", _jitter(seed, out, 0.001), perm[f], seed)


def _tetrahedron(base):
    return [(base, base + 2, base + 1), (base, base + 1, base + 3), (base + 1, base + 2, base + 3), (base + 2, base, base + 3)]


def tie():
    corners = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], np.float64)
    v = _jitter(5, np.concatenate([corners, corners + (3, 0, 0)]))
    return Mesh("two tetrahedra", v, _tetrahedron(4) + _tetrahedron(0), 5)


def coincident():
    v = _jitter(6, [(0, 0, 0), (1, 0, 0), (0, 1, 0)])
    return Mesh("coincident faces", v, [(0, 1, 2), (0, 2, 1)], 6)


def isolated():
    v = _jitter(7, [(9, 9, 9), (0, 0, 0), (1, 0, 0), (8, 8, 8), (1, 1, 0), (0, 1, 0), (7, 7, 7)])
    return Mesh("isolated vertices", v, [(1, 2, 4), (1, 4, 5)], 7)


def octahedron(base=0):
    top, bottom = base + 4, base + 5
    ring = [base, base + 1, base + 2, base + 3]
    f = []
    for i in range(4):
        a, b = ring[i], ring[(i + 1) % 4]
        f += [(a, b, top), (b, a, bottom)]
    v = [(1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    return np.array(v, np.float64), f


def threshold():
    ov, of = octahedron()
    small = fan(MIN_FACES - 1, closed=False, seed=8)
    v = np.concatenate([_jitter(8, ov), small.verts.astype(np.float64) + (4, 0, 0)])
    f = np.concatenate([small.faces.astype(np.int64) + len(ov), np.array(of)])
    m = Mesh(f"components of {MIN_FACES} and {MIN_FACES - 1} faces", v, f, 8)
    assert len(of) == MIN_FACES and len(small.faces) == MIN_FACES - 1
    return m


def empty():
    return Mesh("empty", np.zeros((0, 3)), np.zeros((0, 3)), 9)


def vertices_only():
    return Mesh("vertices only", _jitter(10, np.zeros((5, 3)), 1.0), np.zeros((0, 3)), 10)


def single_face():
    return Mesh("single face", _jitter(11, [(0, 0, 0), (1, 0, 0), (0, 1, 0)]), [(0, 1, 2)], 11)


def hand_built():
    """Large first, then small ones, the empty mesh in the middle: grow-only buffers see every order."""
    return [strip(), fan(), open_book(), empty(), closed_book(), tie(), coincident(), vertices_only(), isolated(),
            threshold(), single_face()]
