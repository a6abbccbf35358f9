"""NumPy restatement of the decimation with quadric placement (csrc/amvs_mesh_decimate.hip, include/amvs.h
amvs_mesh_decimate_quadric), written from the definition and not from the kernels (a helper module, not a conftest; no
GPU).  The device results are compared with it bit for bit, so every float32 operation is rounded on its own
(`.astype(F32)` after each) and every sum runs in the stated order.

Clusters, faces, colours and the removal of unused clusters are mesh_decimate_restatement's; the vertex -> corner index
and the face normals are mesh_clean_restatement's.  Only the position of a cluster differs, on the OLD mesh:

    mean          m = mesh_decimate_restatement.representatives
    face normal   n = cross(p1 - p0, p2 - p0), not normalised
    vertex v      Qv = 0; for the corners of v in ascending corner index, f the corner's face: e = p[faces[f, 0]] - m,
                  d = (nx ex + ny ey) + nz ez, Qv += (nx nx, nx ny, nx nz, ny ny, ny nz, nz nz, d nx, d ny, d nz)
    cluster       S = 0; S += Qv over the members in ascending old id = (a00 a01 a02 a11 a12 a22 b0 b1 b2)
    solve         t = (a00 + a11) + a22; lam = regularisation t; m00 = a00 + lam; m11 = a11 + lam; m22 = a22 + lam
                  l10 = a01 / m00; l20 = a02 / m00; d1 = m11 - l10 a01; u12 = a12 - l20 a01; l21 = u12 / d1
                  d2 = (m22 - l20 a02) - l21 u12; z1 = b1 - l10 b0; z2 = (b2 - l20 b0) - l21 z1
                  y2 = z2 / d2; y1 = z1 / d1 - l21 y2; y0 = (b0 / m00 - l10 y1) - l20 y2; cand = m + y
    accept        t > 0, d1 > 0, d2 > 0, cand finite, |y| <= 0.5 cell per axis (false for NaN); otherwise m

An ordered sum over a row or a cluster is a loop over the rank r within it: every row (cluster) with more than r
entries adds its r-th one.  The cause of a fallback is the first condition, in the order above, that does not hold.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_restatement as cr  # noqa: E402
import mesh_decimate_restatement as dr  # noqa: E402

F32 = np.float32
CAUSES = ("t", "d1", "d2", "non-finite", "bound")                 # cause code 1 .. 5; 0 = accepted


def vertex_quadrics(p, f, vmap, mean):
    """Qv (V, 9) float32 of every old vertex."""
    nv = len(p)
    q = np.zeros((nv, 9), F32)
    if len(f) == 0:
        return q
    start, corners = cr.corner_index(f, nv)
    fn = cr.face_normals(p, f)
    deg = np.diff(start)
    mv = mean[vmap]
    with np.errstate(all="ignore"):
        for r in range(int(deg.max())):
            rows = np.flatnonzero(deg > r)
            face = corners[start[rows] + r] // 3
            e = (p[f[face, 0]] - mv[rows]).astype(F32)
            n = fn[face]
            d = ((n[:, 0] * e[:, 0]).astype(F32) + (n[:, 1] * e[:, 1]).astype(F32)).astype(F32)
            d = (d + (n[:, 2] * e[:, 2]).astype(F32)).astype(F32)
            terms = np.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2],
                              n[:, 2] * n[:, 2], d * n[:, 0], d * n[:, 1], d * n[:, 2]], -1).astype(F32)
            q[rows] = (q[rows] + terms).astype(F32)
    return q


def cluster_quadrics(q, order, start):
    """S (C, 9): the members' quadrics added in ascending old id."""
    count = np.diff(start)
    s = np.zeros((len(count), 9), F32)
    with np.errstate(all="ignore"):
        for r in range(int(count.max()) if len(count) else 0):
            rows = np.flatnonzero(count > r)
            s[rows] = (s[rows] + q[order[start[rows] + r]]).astype(F32)
    return s


def solve(s, mean, regularisation, cell):
    """(positions (C, 3) float32, cause (C,) int: 0 accepted, else 1 + index into CAUSES, y (C, 3))."""
    a00, a01, a02, a11, a12, a22, b0, b1, b2 = (s[:, i] for i in range(9))
    reg = F32(regularisation)
    with np.errstate(all="ignore"):
        t = ((a00 + a11).astype(F32) + a22).astype(F32)
        lam = (reg * t).astype(F32)
        m00, m11, m22 = (a00 + lam).astype(F32), (a11 + lam).astype(F32), (a22 + lam).astype(F32)
        l10, l20 = (a01 / m00).astype(F32), (a02 / m00).astype(F32)
        d1 = (m11 - (l10 * a01).astype(F32)).astype(F32)
        u12 = (a12 - (l20 * a01).astype(F32)).astype(F32)
        l21 = (u12 / d1).astype(F32)
        d2 = ((m22 - (l20 * a02).astype(F32)).astype(F32) - (l21 * u12).astype(F32)).astype(F32)
        z1 = (b1 - (l10 * b0).astype(F32)).astype(F32)
        z2 = ((b2 - (l20 * b0).astype(F32)).astype(F32) - (l21 * z1).astype(F32)).astype(F32)
        y2 = (z2 / d2).astype(F32)
        y1 = ((z1 / d1).astype(F32) - (l21 * y2).astype(F32)).astype(F32)
        y0 = (((b0 / m00).astype(F32) - (l10 * y1).astype(F32)).astype(F32) - (l20 * y2).astype(F32)).astype(F32)
        y = np.stack([y0, y1, y2], -1).astype(F32)
        cand = (mean + y).astype(F32)
        half = F32(F32(0.5) * F32(cell))
        checks = [t > 0, d1 > 0, d2 > 0, np.isfinite(cand).all(axis=1), (np.abs(y) <= half).all(axis=1)]
    cause = np.zeros(len(s), np.int64)
    for code in range(len(checks), 0, -1):                        # the first failing condition wins
        cause[~checks[code - 1]] = code
    pos = np.where((cause == 0)[:, None], cand, mean).astype(F32)
    return pos, cause, y


class Prepared:
    """Everything of a decimation that does not depend on the regularisation: the clusters, their means, colours and
    quadrics, the faces that stay and the clusters they use."""

    def __init__(self, verts, faces, colors, origin, cell):
        p = np.asarray(verts, F32).reshape(-1, 3)
        f = np.asarray(faces, np.int64).reshape(-1, 3)
        col = np.asarray(colors, np.uint8).reshape(-1, 3)
        self.cell = F32(cell)
        keys = dr.cell_keys(p, origin, cell)
        self.vmap, self.order, self.start, _ = dr.clusters(keys)
        self.mean, self.colors = dr.representatives(p, col, self.order, self.start)
        g = self.vmap[f] if len(f) else f
        keep, _ = dr.face_decision(g)
        kf = g[keep]
        self.used = np.zeros(len(self.mean), bool)
        self.used[kf.reshape(-1)] = True
        new_id = np.cumsum(self.used) - 1
        self.faces = new_id[kf].astype(np.int32).reshape(-1, 3)
        self.quadrics = cluster_quadrics(vertex_quadrics(p, f, self.vmap, self.mean), self.order, self.start)

    def place(self, regularisation, with_info=False):
        """(vertices, faces, colours, n_fallback[, info]); info: `causes` (name -> clusters), `cause`, `mean`, `y`,
        `position` of every cluster of step 2 and `used` (those that stay)."""
        pos, cause, y = solve(self.quadrics, self.mean, regularisation, self.cell)
        out = (pos[self.used], self.faces, self.colors[self.used], int((cause != 0).sum()))
        if not with_info:
            return out
        info = dict(causes={name: int((cause == k + 1).sum()) for k, name in enumerate(CAUSES)}, cause=cause, mean=self.mean,
                    y=y, position=pos, used=self.used, clusters=len(pos))
        return out + (info,)


def decimate_quadric(verts, faces, colors, origin, cell, regularisation=1e-3, with_info=False):
    """(vertices (V',3) float32, faces (F',3) int32, colours (V',3) uint8, n_fallback[, info]), or dr.OutOfGrid."""
    return Prepared(verts, faces, colors, origin, cell).place(regularisation, with_info)


def _solve_one(s, m, reg, cell):
    a00, a01, a02, a11, a12, a22, b0, b1, b2 = (F32(x) for x in s)
    t = F32(F32(a00 + a11) + a22)
    lam = F32(reg * t)
    m00, m11, m22 = F32(a00 + lam), F32(a11 + lam), F32(a22 + lam)
    l10, l20 = F32(a01 / m00), F32(a02 / m00)
    d1 = F32(m11 - F32(l10 * a01))
    u12 = F32(a12 - F32(l20 * a01))
    l21 = F32(u12 / d1)
    d2 = F32(F32(m22 - F32(l20 * a02)) - F32(l21 * u12))
    z1 = F32(b1 - F32(l10 * b0))
    z2 = F32(F32(b2 - F32(l20 * b0)) - F32(l21 * z1))
    y2 = F32(z2 / d2)
    y1 = F32(F32(z1 / d1) - F32(l21 * y2))
    y0 = F32(F32(F32(b0 / m00) - F32(l10 * y1)) - F32(l20 * y2))
    y = (y0, y1, y2)
    cand = [F32(m[a] + y[a]) for a in range(3)]
    half = F32(F32(0.5) * F32(cell))
    ok = bool(t > 0 and d1 > 0 and d2 > 0 and all(np.isfinite(c) for c in cand) and all(abs(v) <= half for v in y))
    return (cand if ok else [F32(x) for x in m]), ok


def decimate_quadric_slow(verts, faces, colors, origin, cell, regularisation=1e-3):
    """The same definition as plain Python loops (small meshes only): (vertices, faces, colours, n_fallback)."""
    p = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    col = np.asarray(colors, np.uint8).reshape(-1, 3)
    o = np.asarray(origin, F32).reshape(3)
    members = {}
    for v in range(len(p)):
        idx = [int(np.floor(F32(F32(p[v, a] - o[a]) / F32(cell)))) for a in range(3)]
        members.setdefault((idx[2], idx[1], idx[0]), []).append(v)
    cells = sorted(members)
    cluster_of = {v: c for c, cl in enumerate(cells) for v in members[cl]}
    rows = [[] for _ in range(len(p))]
    for fi, face in enumerate(f):
        for k in range(3):
            rows[int(face[k])].append(fi)                         # ascending 3 fi + k: fi ascending, a vertex once per face
    reg = F32(regularisation)
    pos, n_fallback = [], 0
    with np.errstate(all="ignore"):
        for cl in cells:
            s = np.zeros(3, F32)
            for v in members[cl]:
                s = (s + p[v]).astype(F32)
            m = (s / F32(len(members[cl]))).astype(F32)
            total = [F32(0)] * 9
            for v in members[cl]:
                q = [F32(0)] * 9
                for fi in rows[v]:
                    p0, p1, p2 = (p[int(f[fi, k])] for k in range(3))
                    a = [F32(p1[i] - p0[i]) for i in range(3)]
                    b = [F32(p2[i] - p0[i]) for i in range(3)]
                    n = [F32(F32(a[1] * b[2]) - F32(a[2] * b[1])), F32(F32(a[2] * b[0]) - F32(a[0] * b[2])),
                         F32(F32(a[0] * b[1]) - F32(a[1] * b[0]))]
                    e = [F32(p0[i] - m[i]) for i in range(3)]
                    d = F32(F32(F32(n[0] * e[0]) + F32(n[1] * e[1])) + F32(n[2] * e[2]))
                    terms = [n[0] * n[0], n[0] * n[1], n[0] * n[2], n[1] * n[1], n[1] * n[2], n[2] * n[2], d * n[0], d * n[1], d * n[2]]
                    q = [F32(q[i] + F32(terms[i])) for i in range(9)]
                total = [F32(total[i] + q[i]) for i in range(9)]
            x, ok = _solve_one(total, m, reg, cell)
            n_fallback += 0 if ok else 1
            pos.append(np.array(x, F32))
    mv, mf, mc = dr.decimate_slow(p, f, col, origin, cell)
    # decimate_slow's vertices are the used clusters in ascending cell order: the same ones, other positions
    used = sorted({cluster_of[int(v)] for v in _kept_old_vertices(f, cluster_of)})
    assert len(used) == len(mv)
    out_v = np.array([pos[c] for c in used], F32).reshape(-1, 3)
    return out_v, mf, mc, n_fallback


def _kept_old_vertices(f, cluster_of):
    """Old vertex ids of the faces that the decimation keeps (the definition of dr.decimate_slow, by cluster id)."""
    groups, mapped = {}, []
    for fi, face in enumerate(f):
        t = [cluster_of[int(v)] for v in face]
        mapped.append(face)
        if len(set(t)) < 3:
            continue
        k = t.index(min(t))
        rot = (t[k], t[(k + 1) % 3], t[(k + 2) % 3])
        groups.setdefault(tuple(sorted(t)), []).append((fi, rot[1] < rot[2]))
    out = []
    for g in groups.values():
        net = sum(1 if e else -1 for _, e in g)
        if net:
            out += list(mapped[min(fi for fi, e in g if e == (net > 0))])
    return out
