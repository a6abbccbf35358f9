"""NumPy restatement of the mesh clean-up (csrc/amvs_mesh_clean.hip, include/amvs.h amvs_mesh_*), written from the
definitions and not from the kernels (a helper module, not a conftest; no GPU).  The device results are compared
with it bit for bit, so every float32 operation is rounded on its own (`.astype(F32)` after each) and every sum runs
in the stated order.

Corner c = 3 * face + k holds vertex faces[face, k].  Row v of the index lists the corners that hold v in ascending
c.  An ordered sum over a row is a loop over the rank r within the row: every vertex with more than r corners adds
its r-th contribution.

    corner_index   (row starts, corners)
    labels         smallest vertex id of the vertex's component (vertices joined through faces)
    filter         keep the components with faces >= min_faces (keep_largest: only the one with the most faces, a tie
                   to the smallest label); faces, then vertices and colours compacted in order; fresh labels
    pinned         on an edge that exactly one face has
    smooth         Taubin: `iterations` times a step with factor lam, then one with factor mu unless mu == 0
                       s = 0; per corner in row order: s += p[next vertex of the face]; s += p[the one after]
                       m = s / (2 * deg); d = m - p; p' = p + factor * d          (deg == 0 or pinned: p' = p)
    normals        per face cross(p1 - p0, p2 - p0) = (ay bz - az by, az bx - ax bz, ax by - ay bx); per vertex the sum
                   S over the row, l = sqrt((Sx Sx + Sy Sy) + Sz Sz), S / l or 0 unless l > 0
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

F32 = np.float32


def _faces(faces):
    return np.asarray(faces, np.int64).reshape(-1, 3)


def corner_index(faces, n_vertices):
    """(start (V + 1,), corners (3 F,)): row v is corners[start[v]:start[v + 1]], ascending."""
    ids = _faces(faces).reshape(-1)
    corners = np.argsort(ids, kind="stable")
    start = np.zeros(n_vertices + 1, np.int64)
    np.cumsum(np.bincount(ids, minlength=n_vertices), out=start[1:])
    return start, corners


def labels(faces, n_vertices):
    f = _faces(faces)
    if n_vertices == 0:
        return np.zeros(0, np.int32)
    a = np.concatenate([f[:, 0], f[:, 0]])
    b = np.concatenate([f[:, 1], f[:, 2]])
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n_vertices, n_vertices))
    n, comp = connected_components(g, directed=False)
    smallest = np.full(n, n_vertices, np.int64)
    np.minimum.at(smallest, comp, np.arange(n_vertices))
    return smallest[comp].astype(np.int32)


def component_faces(faces, lab):
    """faces of every component, at its label (0 elsewhere)."""
    f = _faces(faces)
    return np.bincount(lab[f[:, 0]], minlength=len(lab)).astype(np.int64) if len(f) else np.zeros(len(lab), np.int64)


def filter(verts, faces, colors, min_faces=0, keep_largest=False):
    """(components before the filter, vertices, faces, colours, labels) after it."""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    f = _faces(faces)
    colors = np.asarray(colors, np.uint8).reshape(-1, 3)
    nv = len(verts)
    lab = labels(f, nv)
    n_comp = int((lab == np.arange(nv)).sum())
    if (min_faces <= 0 and not keep_largest) or nv == 0:
        return n_comp, verts.copy(), f.astype(np.int32), colors.copy(), lab
    count = component_faces(f, lab)
    keep = count >= min_faces                                     # by label
    if keep_largest:
        roots = np.flatnonzero(lab == np.arange(nv))
        best = roots[np.argmax(count[roots])]                     # argmax takes the first: the smallest label
        only = np.zeros(nv, bool)
        only[best] = True
        keep &= only
    f = f[keep[lab[f[:, 0]]]] if len(f) else f
    used = np.zeros(nv, bool)
    used[f.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    out_lab = new_id[lab[used]].astype(np.int32)
    return n_comp, verts[used], new_id[f].astype(np.int32).reshape(-1, 3), colors[used], out_lab


def pinned(faces, n_vertices):
    f = _faces(faces)
    pin = np.zeros(n_vertices, bool)
    if len(f) == 0:
        return pin
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    edges, count = np.unique(lo * n_vertices + hi, return_counts=True)
    once = edges[count == 1]
    pin[once // n_vertices] = True
    pin[once % n_vertices] = True
    return pin


def edge_face_counts(faces, n_vertices):
    """(lo, hi, faces on the edge) of every undirected edge."""
    f = _faces(faces)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    edges, count = np.unique(lo * max(n_vertices, 1) + hi, return_counts=True)
    return edges // max(n_vertices, 1), edges % max(n_vertices, 1), count


def _row_terms(f, start, corners, r, rows):
    """face, next vertex and the one after, of the r-th corner of the rows `rows`."""
    c = corners[start[rows] + r]
    face, k = c // 3, c % 3
    return face, f[face, (k + 1) % 3], f[face, (k + 2) % 3]


def umbrella_step(p, f, start, corners, factor, pin=None):
    deg = np.diff(start)
    s = np.zeros_like(p)
    for r in range(int(deg.max()) if len(deg) else 0):
        rows = np.flatnonzero(deg > r)
        _, n1, n2 = _row_terms(f, start, corners, r, rows)
        s[rows] = (s[rows] + p[n1]).astype(F32)
        s[rows] = (s[rows] + p[n2]).astype(F32)
    move = deg > 0
    if pin is not None:
        move &= ~pin
    den = (F32(2.0) * deg[move].astype(F32)).astype(F32)[:, None]
    m = (s[move] / den).astype(F32)
    d = (m - p[move]).astype(F32)
    out = p.copy()
    out[move] = (p[move] + (F32(factor) * d).astype(F32)).astype(F32)
    return out


def smooth(verts, faces, iterations, lam=0.5, mu=-0.53, fix_boundary=True):
    p = np.array(verts, F32).reshape(-1, 3)
    f = _faces(faces)
    if iterations <= 0 or len(p) == 0:
        return p
    start, corners = corner_index(f, len(p))
    pin = pinned(f, len(p)) if fix_boundary else None
    for _ in range(iterations):
        p = umbrella_step(p, f, start, corners, F32(lam), pin)
        if F32(mu) != 0:
            p = umbrella_step(p, f, start, corners, F32(mu), pin)
    return p


def face_normals(verts, faces):
    p = np.asarray(verts, F32).reshape(-1, 3)
    f = _faces(faces)
    a = (p[f[:, 1]] - p[f[:, 0]]).astype(F32)
    b = (p[f[:, 2]] - p[f[:, 0]]).astype(F32)

    def det(u, v, w, x):                                          # u v - w x, every operation rounded
        return ((u * v).astype(F32) - (w * x).astype(F32)).astype(F32)

    return np.stack([det(a[:, 1], b[:, 2], a[:, 2], b[:, 1]), det(a[:, 2], b[:, 0], a[:, 0], b[:, 2]),
                     det(a[:, 0], b[:, 1], a[:, 1], b[:, 0])], -1).astype(F32).reshape(-1, 3)


def normal_sums(verts, faces):
    """(S, l): the ordered sums of the face normals and their float32 lengths."""
    p = np.asarray(verts, F32).reshape(-1, 3)
    f = _faces(faces)
    start, corners = corner_index(f, len(p))
    fn = face_normals(p, f)
    deg = np.diff(start)
    s = np.zeros_like(p)
    for r in range(int(deg.max()) if len(deg) else 0):
        rows = np.flatnonzero(deg > r)
        s[rows] = (s[rows] + fn[corners[start[rows] + r] // 3]).astype(F32)
    with np.errstate(all="ignore"):
        sq = (s * s).astype(F32)
        l = np.sqrt(((sq[:, 0] + sq[:, 1]).astype(F32) + sq[:, 2]).astype(F32)).astype(F32)
    return s, l


def normals(verts, faces):
    s, l = normal_sums(verts, faces)
    ok = l > 0
    out = np.zeros_like(s)
    with np.errstate(all="ignore"):
        out[ok] = (s[ok] / l[ok, None]).astype(F32)
    return out


def pipeline(verts, faces, colors, min_faces=0, keep_largest=False, iterations=0, lam=0.5, mu=-0.53, fix_boundary=True):
    """reconstruct_mesh's order: filter -> smooth -> normals.  (components before, vertices, faces, colours, labels,
    normals)."""
    n_comp, v, f, c, lab = filter(verts, faces, colors, min_faces, keep_largest)
    v = smooth(v, f, iterations, lam, mu, fix_boundary)
    return n_comp, v, f, c, lab, normals(v, f)
