"""NumPy restatement of the mesh rasteriser, the visibility counts and the visibility filter (include/amvs.h
amvs_mesh_render, amvs_mesh_visibility, amvs_mesh_filter_visible; csrc/amvs_mesh_render.hip), written from the
definition in the header and not from the kernels (a helper module, not a conftest; no GPU).  Every float operation is
a float32 NumPy operation rounded on its own, the coverage test is exact in int64, and the resolve is a minimum over
64-bit keys, so the device result must equal this one bit for bit.

    project(verts, K, pose, near)            zc, u, v, iz, usable, sx, sy of every vertex
    render(verts, faces, K, poses, near, H, W)   depth (n,H,W) float32, face (n,H,W) int32, n_skipped (n,) int64
    render_loops(...)                        the same by plain per-vertex, per-face, per-pixel Python loops with a projection
                                             of their own (small inputs only)
    visibility(verts, K, poses, near, depth, tolerance)      counts (V,) int32
    filter_visible(verts, faces, colors, counts, min_views)  the filtered mesh
"""
import numpy as np

F32 = np.float32
LIMIT = F32(2.0 ** 20)            # |u|, |v| of a usable vertex
SUB = 256                         # fixed-point steps per pixel
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
CHUNK = 1 << 21                   # (face, pixel) pairs expanded at a time


def _cam(K, pose):
    return np.asarray(K, F32).reshape(9), np.asarray(pose, F32).reshape(12)


def project(verts, K, pose, near):
    """(a): camera depth zc, image position u, v, inverse depth iz, the usable flag and the fixed-point position."""
    k, P = _cam(K, pose)
    p = np.asarray(verts, F32).reshape(-1, 3)
    X, Y, Z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        zc = ((P[6] * X + P[7] * Y) + P[8] * Z) + P[11]
        xc = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[9]
        yc = ((P[3] * X + P[4] * Y) + P[5] * Z) + P[10]
        pu = (k[0] * xc + k[1] * yc) + k[2] * zc
        pv = (k[3] * xc + k[4] * yc) + k[5] * zc
        pw = (k[6] * xc + k[7] * yc) + k[8] * zc
        u, v = pu / pw, pv / pw
        iz = F32(1.0) / zc
        usable = (zc > F32(near)) & (np.abs(u) <= LIMIT) & (np.abs(v) <= LIMIT)
        sx = np.rint(np.where(usable, u, F32(0)) * F32(SUB)).astype(np.int64)
        sy = np.rint(np.where(usable, v, F32(0)) * F32(SUB)).astype(np.int64)
    return zc, u, v, iz, usable, sx, sy


def _inside(w, dx, dy):
    return (w > 0) | ((w == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))


def _ceil_div(a):
    return -(np.negative(a) // SUB)


class Setup:
    """(b) of one view: the faces that draw, corners in the order the coverage uses, and their clamped boxes."""

    def __init__(self, verts, faces, K, pose, near, H, W):
        f = np.asarray(faces, np.int64).reshape(-1, 3)
        _, _, _, iz, usable, sx, sy = project(verts, K, pose, near)
        ok = usable[f].all(axis=1) if len(f) else np.zeros(0, bool)
        self.n_skipped = int((~ok).sum())
        i0, i1, i2 = f[:, 0], f[:, 1], f[:, 2]
        area = (sx[i1] - sx[i0]) * (sy[i2] - sy[i0]) - (sy[i1] - sy[i0]) * (sx[i2] - sx[i0])
        swap = area < 0
        i1, i2 = np.where(swap, i2, i1), np.where(swap, i1, i2)
        area = np.abs(area)
        ids = np.stack([i0, i1, i2], axis=1)
        x, y = sx[ids], sy[ids]
        # pixels px with SUB * px inside [min, max]: ceil(min / SUB) .. floor(max / SUB), clamped to the image
        lo_x = np.maximum(_ceil_div(x.min(axis=1)), 0)
        hi_x = np.minimum(x.max(axis=1) // SUB, W - 1)
        lo_y = np.maximum(_ceil_div(y.min(axis=1)), 0)
        hi_y = np.minimum(y.max(axis=1) // SUB, H - 1)
        bw, bh = np.maximum(hi_x - lo_x + 1, 0), np.maximum(hi_y - lo_y + 1, 0)
        draw = ok & (area != 0) & (bw > 0) & (bh > 0)
        self.usable_face, self.area_all, self.box_all = ok, area, np.where(ok & (area != 0), bw * bh, 0)
        keep = np.flatnonzero(draw)
        self.face = keep
        self.ids, self.x, self.y, self.area = ids[keep], x[keep], y[keep], area[keep]
        self.iz = iz[ids[keep]]
        self.lo_x, self.lo_y, self.bw, self.bh = lo_x[keep], lo_y[keep], bw[keep], bh[keep]


def _fragments(s, sel, px, py):
    """(c), (d), (e) for the pairs (face sel[i] of the set-up, pixel (px[i], py[i])): (covered, keys)."""
    Px, Py = px * SUB, py * SUB
    w = []
    ins = np.ones(len(sel), bool)
    for a, b in ((1, 2), (2, 0), (0, 1)):
        ax, ay, bx, by = s.x[sel, a], s.y[sel, a], s.x[sel, b], s.y[sel, b]
        dx, dy = bx - ax, by - ay
        wi = dx * (Py - ay) - dy * (Px - ax)
        ins &= _inside(wi, dx, dy)
        w.append(wi)
    area = s.area[sel].astype(F32)
    with np.errstate(all="ignore"):
        b0, b1, b2 = (wi.astype(F32) / area for wi in w)
        iz = s.iz[sel]
        z = F32(1.0) / ((b0 * iz[:, 0] + b1 * iz[:, 1]) + b2 * iz[:, 2])
        ins &= np.isfinite(z) & (z > 0)
    key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | s.face[sel].astype(np.uint64)
    return ins, key


def render_keys(verts, faces, K, pose, near, H, W):
    """The key map (H*W,) uint64 of one view (all ones where nothing was drawn) and the faces skipped."""
    s = Setup(verts, faces, K, pose, near, H, W)
    keys = np.full(H * W, NO_KEY, np.uint64)
    n_pix = s.bw * s.bh
    ends = np.cumsum(n_pix)
    first = 0
    while first < len(n_pix):
        last = int(np.searchsorted(ends, (ends[first - 1] if first else 0) + CHUNK, side="right"))
        last = max(last, first + 1)
        cnt = n_pix[first:last]
        sel = np.repeat(np.arange(first, last), cnt)
        within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        px = s.lo_x[sel] + within % s.bw[sel]
        py = s.lo_y[sel] + within // s.bw[sel]
        ins, key = _fragments(s, sel, px, py)
        np.minimum.at(keys, (py * W + px)[ins], key[ins])
        first = last
    return keys, s.n_skipped


def split_keys(keys, H, W):
    drawn = keys != NO_KEY
    depth = np.where(drawn, (keys >> np.uint64(32)).astype(np.uint32), np.uint32(0)).view(F32)
    face = np.where(drawn, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return depth.reshape(H, W), face.reshape(H, W)


def render(verts, faces, K, poses, near, H, W):
    poses = np.asarray(poses, F32).reshape(-1, 12)
    depth = np.empty((len(poses), H, W), F32)
    face = np.empty((len(poses), H, W), np.int32)
    skipped = np.empty(len(poses), np.int64)
    for m, pose in enumerate(poses):
        keys, skipped[m] = render_keys(verts, faces, K, pose, near, H, W)
        depth[m], face[m] = split_keys(keys, H, W)
    return depth, face, skipped


def _project_scalar(point, K, pose, near):
    """(a) for one vertex, stated on its own and not through project(): the rotation as a 3 x 3 matrix and a
    translation, the rows' dot products accumulated left to right in float32 scalars, the fixed-point position with
    Python's round() (ties to even) on the exact product.  Returns (iz, usable, sx, sy)."""
    Km = np.asarray(K, F32).reshape(3, 3)
    R, t = np.asarray(pose, F32)[:9].reshape(3, 3), np.asarray(pose, F32)[9:]

    def row(m, x, extra=None):
        acc = m[0] * x[0] + m[1] * x[1]
        acc = acc + m[2] * x[2]
        return acc if extra is None else acc + extra

    with np.errstate(all="ignore"):
        x = [F32(c) for c in point]
        cam = [row(R[r], x, t[r]) for r in range(3)]
        pu, pv, pw = (row(Km[r], cam) for r in range(3))
        u, v, iz = pu / pw, pv / pw, F32(1.0) / cam[2]
    usable = bool(cam[2] > F32(near)) and bool(abs(u) <= 2.0 ** 20) and bool(abs(v) <= 2.0 ** 20)
    if not usable:
        return iz, False, 0, 0
    return iz, True, round(float(u) * 256.0), round(float(v) * 256.0)


def render_loops(verts, faces, K, poses, near, H, W):
    """render() by plain loops over vertices, faces and EVERY pixel of the image (no bounding box): its own scalar
    projection, Python integers for the coverage, float32 scalars for the depth."""
    poses = np.asarray(poses, F32).reshape(-1, 12)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    depth = np.zeros((len(poses), H, W), F32)
    face = np.full((len(poses), H, W), -1, np.int32)
    skipped = np.zeros(len(poses), np.int64)
    pts3 = np.asarray(verts, F32).reshape(-1, 3)
    for m, pose in enumerate(poses):
        cam = [_project_scalar(p, K, pose, near) for p in pts3]
        iz, usable = [c[0] for c in cam], [c[1] for c in cam]
        sx, sy = [c[2] for c in cam], [c[3] for c in cam]
        best = {}
        for fi, tri in enumerate(f):
            if not all(usable[i] for i in tri):
                skipped[m] += 1
                continue
            c = [int(i) for i in tri]
            pts = [(int(sx[i]), int(sy[i])) for i in c]
            area = (pts[1][0] - pts[0][0]) * (pts[2][1] - pts[0][1]) - (pts[1][1] - pts[0][1]) * (pts[2][0] - pts[0][0])
            if area == 0:
                continue
            if area < 0:
                c[1], c[2], pts[1], pts[2], area = c[2], c[1], pts[2], pts[1], -area
            for py in range(H):
                for px in range(W):
                    w, inside = [], True
                    for a, b in ((1, 2), (2, 0), (0, 1)):
                        dx, dy = pts[b][0] - pts[a][0], pts[b][1] - pts[a][1]
                        wi = dx * (SUB * py - pts[a][1]) - dy * (SUB * px - pts[a][0])
                        inside = inside and (wi > 0 or (wi == 0 and (dy < 0 or (dy == 0 and dx > 0))))
                        w.append(wi)
                    if not inside:
                        continue
                    with np.errstate(all="ignore"):
                        b = [F32(np.int64(wi)) / F32(np.int64(area)) for wi in w]
                        z = F32(1.0) / ((b[0] * iz[c[0]] + b[1] * iz[c[1]]) + b[2] * iz[c[2]])
                    if not (np.isfinite(z) and z > 0):
                        continue
                    key = (int(np.asarray(z, F32).view(np.uint32)) << 32) | fi
                    if key < best.get((py, px), 1 << 64):
                        best[(py, px)] = key
        for (py, px), key in best.items():
            depth[m, py, px] = np.asarray(key >> 32, np.uint32).view(F32)
            face[m, py, px] = key & 0xFFFFFFFF
    return depth, face, skipped


def visibility(verts, K, poses, near, depth, tolerance):
    """counts[v]: the views in which vertex v lies in front of `near`, inside the image, and not behind the rendered
    depth at its nearest pixel by more than the tolerance (or where nothing was drawn)."""
    poses = np.asarray(poses, F32).reshape(-1, 12)
    depth = np.asarray(depth, F32)
    _, H, W = depth.shape
    counts = np.zeros(len(np.asarray(verts).reshape(-1, 3)), np.int32)
    tol = F32(tolerance)
    for m, pose in enumerate(poses):
        zc, u, v, _, _, _, _ = project(verts, K, pose, near)
        with np.errstate(all="ignore"):
            fx, fy = np.floor(u + F32(0.5)), np.floor(v + F32(0.5))
            inimg = (fx >= 0) & (fx < F32(W)) & (fy >= 0) & (fy < F32(H))
            ok = (zc > F32(near)) & inimg
            px = np.where(ok, fx, 0).astype(np.int64)
            py = np.where(ok, fy, 0).astype(np.int64)
            d = depth[m][py, px]
            seen = ok & ((d == 0) | (zc <= d + tol))
        counts += seen.astype(np.int32)
    return counts


def filter_visible(verts, faces, colors, counts, min_views):
    """The faces whose three vertices all have counts >= min_views, in their order; the vertices no face uses leave,
    the others keep their order.  A mesh that loses every face is empty."""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    colors = np.asarray(colors, np.uint8).reshape(-1, 3)
    keep = (np.asarray(counts)[f] >= min_views).all(axis=1) if len(f) else np.zeros(0, bool)
    f = f[keep]
    if len(f) == 0:
        return np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint8)
    used = np.zeros(len(verts), bool)
    used[f.ravel()] = True
    new_id = np.cumsum(used) - 1
    return verts[used], new_id[f].astype(np.int32), colors[used]
