"""NumPy restatement of the mesh decimation (csrc/amvs_mesh_decimate.hip, include/amvs.h amvs_mesh_decimate), written
from the definition and not from the kernels (a helper module, not a conftest; no GPU).  The device results are
compared with it bit for bit, so every float32 operation is rounded on its own (`.astype(F32)` after each) and every
sum runs in the stated order.

Vertex clustering on a grid of cubic cells of side `cell` whose corner (0, 0, 0) sits at `origin`:

    cell of a vertex   per axis q = (p - origin) / cell, i = floor(q), -2^20 <= i < 2^20 or the call is refused
                       (OutOfGrid); key = (iz + 2^20) << 42 | (iy + 2^20) << 21 | (ix + 2^20)
    clusters           the distinct keys in ascending order are the provisional new vertex ids
    representative     s = 0; s += p[v] over the members in ascending old id; s / (float)count.  Colour: per channel
                       the integer sum, (2 sum + count) // (2 count)
    faces              ids mapped; a face with a repeated id goes; the others are grouped by their unordered triple;
                       a face's winding is its triple rotated to start at the smallest id; net = faces of the one
                       winding minus faces of the other; net == 0: the group goes, else the face with the smallest
                       index among those of the majority winding stays, in its own corner order; survivors keep
                       their relative order
    unused clusters    leave as in extraction pass (d): the others keep their order, the faces are renumbered

An ordered sum over a cluster is a loop over the rank r within the cluster: every cluster with more than r members
adds its r-th one.
"""
import numpy as np

F32 = np.float32
HALF = 1 << 20


class OutOfGrid(ValueError):
    """A vertex whose cell index leaves [-2^20, 2^20) on some axis; `vertex` is the smallest such id."""

    def __init__(self, vertex):
        super().__init__(f"mesh_decimate: vertex {vertex} outside the cluster grid")
        self.vertex = vertex


def quotients(verts, origin, cell):
    """q (V,3) float32: (p - origin) / cell, either operation rounded on its own."""
    p = np.asarray(verts, F32).reshape(-1, 3)
    o = np.asarray(origin, F32).reshape(3)
    with np.errstate(all="ignore"):
        return ((p - o[None, :]).astype(F32) / F32(cell)).astype(F32)


def cell_keys(verts, origin, cell):
    """int64 key of every vertex, or OutOfGrid."""
    q = quotients(verts, origin, cell)
    i = np.floor(q)
    ok = (i >= F32(-HALF)) & (i < F32(HALF))                      # false for inf and NaN
    bad = np.flatnonzero(~ok.all(axis=1))
    if len(bad):
        raise OutOfGrid(int(bad[0]))
    ii = i.astype(np.int64) + HALF                                # -0.0 -> 0
    return (ii[:, 2] << 42) | (ii[:, 1] << 21) | ii[:, 0]


def clusters(keys):
    """(cluster of every vertex (V,), members in cluster order then ascending id (V,), start (C + 1,), keys (C,))."""
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    head = np.ones(len(sk), bool)
    head[1:] = sk[1:] != sk[:-1]
    cid = np.cumsum(head) - 1
    vmap = np.empty(len(keys), np.int64)
    vmap[order] = cid
    start = np.append(np.flatnonzero(head), len(sk)).astype(np.int64)
    return vmap, order, start, sk[head]


def representatives(verts, colors, order, start):
    p = np.asarray(verts, F32).reshape(-1, 3)
    c = np.asarray(colors, np.uint8).reshape(-1, 3).astype(np.int64)
    count = np.diff(start)
    s = np.zeros((len(count), 3), F32)
    for r in range(int(count.max()) if len(count) else 0):
        rows = np.flatnonzero(count > r)
        s[rows] = (s[rows] + p[order[start[rows] + r]]).astype(F32)
    pos = (s / count.astype(F32)[:, None]).astype(F32)
    if len(count):
        csum = np.add.reduceat(c[order], start[:-1], axis=0)
        col = ((2 * csum + count[:, None]) // (2 * count[:, None])).astype(np.uint8)
    else:
        col = np.zeros((0, 3), np.uint8)
    return pos, col


def face_decision(g):
    """g (F,3) int64: the faces in cluster ids.  (keep (F,) bool, info): which faces stay, and the counters."""
    n = len(g)
    keep = np.zeros(n, bool)
    info = dict(degenerate=0, groups=0, mixed_groups=0, mixed_kept=0, same_wound_duplicates=0, net={})
    if n == 0:
        return keep, info
    deg = (g[:, 0] == g[:, 1]) | (g[:, 0] == g[:, 2]) | (g[:, 1] == g[:, 2])
    info["degenerate"] = int(deg.sum())
    cand = np.flatnonzero(~deg)
    if len(cand) == 0:
        return keep, info
    t = g[cand]
    k = np.argmin(t, axis=1)
    rows = np.arange(len(t))
    a, b, c = t[rows, k], t[rows, (k + 1) % 3], t[rows, (k + 2) % 3]
    even = b < c                                                   # the winding (a, lo, hi); the other is (a, hi, lo)
    lo, hi = np.minimum(b, c), np.maximum(b, c)
    order = np.lexsort((hi, lo, a))                                # stable: ascending face index inside a group
    sa, slo, shi, sev, sf = a[order], lo[order], hi[order], even[order], cand[order]
    head = np.ones(len(order), bool)
    head[1:] = (sa[1:] != sa[:-1]) | (slo[1:] != slo[:-1]) | (shi[1:] != shi[:-1])
    first = np.flatnonzero(head)
    n_even = np.add.reduceat(sev.astype(np.int64), first)
    n_odd = np.add.reduceat((~sev).astype(np.int64), first)
    big = n + 1
    first_even = np.minimum.reduceat(np.where(sev, sf, big), first)
    first_odd = np.minimum.reduceat(np.where(~sev, sf, big), first)
    net = n_even - n_odd
    keep[first_even[net > 0]] = True
    keep[first_odd[net < 0]] = True
    mixed = (n_even > 0) & (n_odd > 0)
    info["groups"] = len(first)
    info["mixed_groups"] = int(mixed.sum())
    info["mixed_kept"] = int((mixed & (net != 0)).sum())
    # faces that share triple AND winding with another face
    info["same_wound_duplicates"] = int(n_even[n_even > 1].sum() + n_odd[n_odd > 1].sum())
    values, counts = np.unique(net, return_counts=True)
    info["net"] = {int(v): int(m) for v, m in zip(values, counts)}
    return keep, info


def decimate(verts, faces, colors, origin, cell, with_info=False):
    """(vertices (V',3) float32, faces (F',3) int32, colours (V',3) uint8[, info]) of the decimated mesh, or OutOfGrid.
    info: the counters of face_decision, and `integral` (components with q == floor(q)), `clusters`, `unused` (clusters
    no kept face uses), `longest` (members of the largest cluster), `keys` (the cell key of every output vertex)."""
    p = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    col = np.asarray(colors, np.uint8).reshape(-1, 3)
    keys = cell_keys(p, origin, cell)
    vmap, order, start, ckeys = clusters(keys)
    pos, ccol = representatives(p, col, order, start)
    g = vmap[f] if len(f) else f
    keep, info = face_decision(g)
    kf = g[keep]
    used = np.zeros(len(pos), bool)
    used[kf.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    out = (pos[used], new_id[kf].astype(np.int32).reshape(-1, 3), ccol[used])
    if not with_info:
        return out
    q = quotients(p, origin, cell)
    info.update(integral=int((q == np.floor(q)).sum()), clusters=len(pos), unused=int((~used).sum()),
                longest=int(np.diff(start).max()) if len(pos) else 0, keys=ckeys[used])
    return out + (info,)


def decimate_slow(verts, faces, colors, origin, cell):
    """The same definition as plain Python loops over clusters and groups (small meshes only)."""
    p = np.asarray(verts, F32).reshape(-1, 3)
    col = np.asarray(colors, np.uint8).reshape(-1, 3)
    o = np.asarray(origin, F32).reshape(3)
    members = {}
    for v in range(len(p)):
        idx = []
        for a in range(3):
            q = F32(F32(p[v, a] - o[a]) / F32(cell))
            i = np.floor(q)
            if not (-HALF <= i < HALF):
                raise OutOfGrid(v)
            idx.append(int(i))
        members.setdefault((idx[2], idx[1], idx[0]), []).append(v)
    cells = sorted(members)
    vmap = {}
    pos, ccol = [], []
    for cid, cl in enumerate(cells):
        s = np.zeros(3, F32)
        total = np.zeros(3, np.int64)
        for v in members[cl]:
            vmap[v] = cid
            s = (s + p[v]).astype(F32)
            total += col[v]
        n = len(members[cl])
        pos.append((s / F32(n)).astype(F32))
        ccol.append((2 * total + n) // (2 * n))
    groups = {}
    mapped = []
    for fi, face in enumerate(np.asarray(faces, np.int64).reshape(-1, 3)):
        t = [vmap[int(v)] for v in face]
        mapped.append(t)
        if len(set(t)) < 3:
            continue
        k = t.index(min(t))
        rot = (t[k], t[(k + 1) % 3], t[(k + 2) % 3])
        groups.setdefault(tuple(sorted(t)), []).append((fi, rot[1] < rot[2]))
    keep = []
    for members_ in groups.values():
        net = sum(1 if e else -1 for _, e in members_)
        if net:
            keep.append(min(fi for fi, e in members_ if e == (net > 0)))
    keep.sort()
    kept = [mapped[fi] for fi in keep]
    used = sorted({c for t in kept for c in t})
    new_id = {c: n for n, c in enumerate(used)}
    out_f = np.array([[new_id[c] for c in t] for t in kept], np.int32).reshape(-1, 3)
    out_v = np.array([pos[c] for c in used], F32).reshape(-1, 3)
    out_c = np.array([ccol[c] for c in used], np.uint8).reshape(-1, 3)
    return out_v, out_f, out_c
