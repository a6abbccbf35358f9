"""NumPy restatement of the texture from the views and of the textured render (include/amvs.h amvs_mesh_texture,
amvs_fetch_mesh_texture, amvs_fetch_render_texture; csrc/amvs_mesh_texture.hip), written from the definition in the
header and not from the kernels (a helper module, not a conftest; no GPU).  Every float operation is a float32 NumPy
operation rounded on its own, the edge functions are exact in int64, so the device result must equal this one byte for
byte.

    layout(F, N, cells_per_row)              (cols, rows, Wt, Ht)
    face_texels(N)                           the texel set of a face, (T,2) int64 rows (i, j)
    atlas_position(f, i, j, N, cols)         atlas (X, Y) of texel (i, j) of face f (arrays)
    uvs(F, N, cells_per_row)                 (F,3,2) float32
    texture(verts, faces, colors, K, poses, near, depth, images_bgr, tolerance, min_cos, best_view, N, cells_per_row)
                                             (atlas (Ht,Wt,3) uint8 RGB, uv, n_texels, n_textured); `miss` names a
                                             near-miss of the definition (NEAR_MISSES), `counters` (a dict) receives what
                                             the texels ran into
    texture_loops(...)                       the same by plain Python loops with a scalar projection of their own
    render_texture(verts, faces, atlas, K, poses, near, depth, face, N, cells_per_row)      (n,H,W,3) uint8 RGB
    render_texture_loops(...)                the same by plain per-pixel loops
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_render_restatement as rr  # noqa: E402

F32 = np.float32
MAX_TEXELS, MAX_SIDE = 64, 16384
NEAR_MISSES = ("vertex normals", "b0 = 1 - (b1 + b2)", "gutter left black", "odd face not mirrored", "g not exchanged back",
               "no pull-back", "v not flipped")
COUNTERS = ("reached", "fallen back", "gutter reached", "gutter fallen back", "pull-back", "corner clamp", "exchanged", "outside set")


def _byte(q):
    """floorf(q + 0.5f) clamped to 0 .. 255."""
    q = np.asarray(q, F32)
    with np.errstate(invalid="ignore"):
        return np.minimum(F32(255), np.maximum(F32(0), np.floor(q + F32(0.5)))).astype(np.uint8)


def layout(F, N, cells_per_row=0):
    assert 1 <= N <= MAX_TEXELS and cells_per_row >= 0
    C, n_cells = N + 3, (F + 1) // 2
    if n_cells == 0:
        return 0, 0, 0, 0
    cols = cells_per_row
    if cols == 0:
        cols = int(np.ceil(np.sqrt(n_cells)))
        while cols * cols < n_cells:
            cols += 1
        while cols > 1 and (cols - 1) * (cols - 1) >= n_cells:
            cols -= 1
    rows = -(-n_cells // cols)
    return cols, rows, cols * C, rows * C


def face_texels(N):
    return np.array([(i, j) for j in range(N + 1) for i in range(N + 1) if i + j <= N + 1], np.int64).reshape(-1, 2)


def atlas_position(f, i, j, N, cols, mirror=True):
    C = N + 3
    cell = f // 2
    cx, cy = (cell % cols) * C, (cell // cols) * C
    odd = (f % 2 == 1) & mirror
    return np.where(odd, cx + C - 1 - i, cx + i), np.where(odd, cy + C - 1 - j, cy + j)


def uvs(F, N, cells_per_row=0, miss=None):
    cols, _, Wt, Ht = layout(F, N, cells_per_row)
    out = np.zeros((F, 3, 2), F32)
    f = np.arange(F, dtype=np.int64)
    for k, (i, j) in enumerate(((0, 0), (N, 0), (0, N))):
        if F == 0:
            break
        X, Y = atlas_position(f, i, j, N, cols, mirror=miss != "odd face not mirrored")
        out[:, k, 0] = (X.astype(F32) + F32(0.5)) / F32(Wt)
        t = (Y.astype(F32) + F32(0.5)) / F32(Ht)
        out[:, k, 1] = t if miss == "v not flipped" else F32(1.0) - t
    return out


def _walk(p, nrm, K, poses, near, depth, images, tol, mc, best_view):
    """Steps a to f of amvs_mesh_color_views for the points p with the normals nrm: (q (P,3) B, G, R, reached (P,))."""
    k = np.asarray(K, F32).reshape(9)
    n, H, W = depth.shape
    P_ = len(p)
    X, Y, Z = p[:, 0], p[:, 1], p[:, 2]
    S, Wsum, reached = np.zeros((P_, 3), F32), np.zeros(P_, F32), np.zeros(P_, bool)
    with np.errstate(all="ignore"):
        for m in range(n):
            P = poses[m]
            zc = ((P[6] * X + P[7] * Y) + P[8] * Z) + P[11]
            xc = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[9]
            yc = ((P[3] * X + P[4] * Y) + P[5] * Z) + P[10]
            pu = (k[0] * xc + k[1] * yc) + k[2] * zc
            pv = (k[3] * xc + k[4] * yc) + k[5] * zc
            pw = (k[6] * xc + k[7] * yc) + k[8] * zc
            u, v = pu / pw, pv / pw
            x0, y0 = np.floor(u), np.floor(v)
            ok = (zc > near) & (x0 >= 0) & (x0 < F32(W - 1)) & (y0 >= 0) & (y0 < F32(H - 1))
            at = np.flatnonzero(ok)                             # the rest of the view only for the points inside it
            ix, iy = x0[at].astype(np.int64), y0[at].astype(np.int64)
            d = np.stack([depth[m][iy, ix], depth[m][iy, ix + 1], depth[m][iy + 1, ix], depth[m][iy + 1, ix + 1]], axis=1)
            z = zc[at, None]
            clear = ((d > 0) & (z <= d + tol) & (d <= z + tol)).all(axis=1)
            nn = nrm[at]
            ncx = (P[0] * nn[:, 0] + P[1] * nn[:, 1]) + P[2] * nn[:, 2]
            ncy = (P[3] * nn[:, 0] + P[4] * nn[:, 1]) + P[5] * nn[:, 2]
            ncz = (P[6] * nn[:, 0] + P[7] * nn[:, 1]) + P[8] * nn[:, 2]
            dot = (ncx * xc[at] + ncy * yc[at]) + ncz * zc[at]
            c = (-dot) / np.sqrt((xc[at] * xc[at] + yc[at] * yc[at]) + zc[at] * zc[at])
            keep = clear & (c > mc)
            at, ix, iy, c = at[keep], ix[keep], iy[keep], c[keep]
            img = images[m].astype(F32)
            f00, f10, f01, f11 = img[iy, ix], img[iy, ix + 1], img[iy + 1, ix], img[iy + 1, ix + 1]
            a, b = (u[at] - x0[at])[:, None], (v[at] - y0[at])[:, None]
            top = f00 + a * (f10 - f00)
            bot = f01 + a * (f11 - f01)
            val = top + b * (bot - top)
            if best_view:
                take = ~reached[at] | (c > Wsum[at])
                S[at[take]], Wsum[at[take]] = val[take], c[take]
            else:
                S[at] = S[at] + c[:, None] * val
                Wsum[at] = Wsum[at] + c
            reached[at] = True
        q = S if best_view else S / Wsum[:, None]
    return q, reached


def _face_frames(verts, faces):
    """Corners (F,3,3) and unit face normals (F,3) as (c) of the definition forms them."""
    p = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    c = p[f]
    a, b = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
    n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)
    with np.errstate(all="ignore"):
        l = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        unit = np.where((l > 0)[:, None], n / l[:, None], F32(0)).astype(F32)
    return c, unit


def texture(verts, faces, colors, K, poses, near, depth, images_bgr, tolerance, min_cos, best_view, N, cells_per_row=0, miss=None,
            counters=None, vertex_normals=None):
    assert miss is None or miss in NEAR_MISSES
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(f)
    cols, rows, Wt, Ht = layout(F, N, cells_per_row)
    assert Wt <= MAX_SIDE and Ht <= MAX_SIDE
    atlas = np.zeros((Ht, Wt, 3), np.uint8)
    uv = uvs(F, N, cells_per_row, miss)
    tex = face_texels(N)
    T = len(tex)
    if F == 0:
        return atlas, uv, 0, 0
    poses = np.asarray(poses, F32).reshape(-1, 12)
    depth = np.asarray(depth, F32)
    images = np.asarray(images_bgr, np.uint8)
    corners, unit = _face_frames(verts, f)
    if miss == "vertex normals":
        unit = np.asarray(vertex_normals, F32).reshape(-1, 3)[f[:, 0]]
    col = np.asarray(colors, np.uint8).reshape(-1, 3).astype(F32)[f]           # (F,3,3) corner, channel
    fi = np.repeat(np.arange(F, dtype=np.int64), T)
    ti, tj = np.tile(tex[:, 0], F), np.tile(tex[:, 1], F)
    b1, b2 = ti.astype(F32) / F32(N), tj.astype(F32) / F32(N)
    b0 = F32(1.0) - (b1 + b2) if miss == "b0 = 1 - (b1 + b2)" else (F32(1.0) - b1) - b2
    c = corners[fi]
    pts = (b0[:, None] * c[:, 0] + b1[:, None] * c[:, 1]) + b2[:, None] * c[:, 2]
    q, reached = _walk(pts, unit[fi], K, poses, F32(near), depth, images, F32(tolerance), F32(min_cos), best_view)
    cf = col[fi]
    fallback = (b0[:, None] * cf[:, 0] + b1[:, None] * cf[:, 1]) + b2[:, None] * cf[:, 2]
    out = np.where(reached[:, None], _byte(q)[:, ::-1], _byte(fallback))
    gutter = ti + tj == N + 1
    if miss == "gutter left black":
        out[gutter] = 0
    X, Y = atlas_position(fi, ti, tj, N, cols, mirror=miss != "odd face not mirrored")
    atlas[Y, X] = out
    if counters is not None:
        for name, value in (("reached", reached & ~gutter), ("fallen back", ~reached & ~gutter), ("gutter reached", reached & gutter),
                            ("gutter fallen back", ~reached & gutter)):
            counters[name] = counters.get(name, 0) + int(value.sum())
    return atlas, uv, F * T, int(reached.sum())


def _camera_scalar(point, K, pose):
    """Projection (a) for one point, stated on its own: R as a 3 x 3 matrix and t, rows accumulated left to right in
    float32 scalars.  Returns (xc, yc, zc, u, v)."""
    Km = np.asarray(K, F32).reshape(3, 3)
    R, t = np.asarray(pose, F32)[:9].reshape(3, 3), np.asarray(pose, F32)[9:]
    x = [F32(c) for c in point]
    cam = []
    for r in range(3):
        acc = R[r, 0] * x[0] + R[r, 1] * x[1]
        acc = acc + R[r, 2] * x[2]
        cam.append(acc + t[r])
    h = []
    for r in range(3):
        acc = Km[r, 0] * cam[0] + Km[r, 1] * cam[1]
        h.append(acc + Km[r, 2] * cam[2])
    return cam[0], cam[1], cam[2], h[0] / h[2], h[1] / h[2]


def _round(q):
    return min(255, max(0, int(np.floor(F32(q) + F32(0.5)))))


def texture_loops(verts, faces, colors, K, poses, near, depth, images_bgr, tolerance, min_cos, best_view, N, cells_per_row=0):
    """texture() one face, one texel and one view at a time, in float32 scalars (small inputs only)."""
    poses = np.asarray(poses, F32).reshape(-1, 12)
    depth = np.asarray(depth, F32)
    images = np.asarray(images_bgr, np.uint8)
    n, H, W = depth.shape
    tol, mc, near = F32(tolerance), F32(min_cos), F32(near)
    pts = np.asarray(verts, F32).reshape(-1, 3)
    col = np.asarray(colors, np.uint8).reshape(-1, 3)
    tris = np.asarray(faces, np.int64).reshape(-1, 3)
    F, C = len(tris), N + 3
    n_cells = (F + 1) // 2
    if n_cells == 0:
        return np.zeros((0, 0, 3), np.uint8), np.zeros((0, 3, 2), F32), 0, 0
    cols = cells_per_row
    while cols * cols < n_cells and cells_per_row == 0:
        cols += 1
    rows = (n_cells + cols - 1) // cols
    Wt, Ht = cols * C, rows * C
    atlas = np.zeros((Ht, Wt, 3), np.uint8)
    uv = np.zeros((F, 3, 2), F32)
    n_texels = n_textured = 0
    with np.errstate(all="ignore"):
        for fi, tri in enumerate(tris):
            cx, cy = ((fi // 2) % cols) * C, ((fi // 2) // cols) * C

            def place(i, j):
                return (cx + C - 1 - i, cy + C - 1 - j) if fi % 2 else (cx + i, cy + j)

            for k, (i, j) in enumerate(((0, 0), (N, 0), (0, N))):
                X, Y = place(i, j)
                uv[fi, k, 0] = (F32(X) + F32(0.5)) / F32(Wt)
                uv[fi, k, 1] = F32(1.0) - (F32(Y) + F32(0.5)) / F32(Ht)
            p0, p1, p2 = (pts[v] for v in tri)
            a, b = p1 - p0, p2 - p0
            nv = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
            l = np.sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2])
            nv = [c / l for c in nv] if l > 0 else [F32(0)] * 3
            for j in range(N + 1):
                for i in range(N + 1):
                    if i + j > N + 1:
                        continue
                    n_texels += 1
                    b1, b2 = F32(i) / F32(N), F32(j) / F32(N)
                    b0 = (F32(1.0) - b1) - b2
                    point = [(b0 * p0[ax] + b1 * p1[ax]) + b2 * p2[ax] for ax in range(3)]
                    total, weight, best, best_w = [F32(0)] * 3, F32(0), None, None
                    for m in range(n):
                        xc, yc, zc, u, v = _camera_scalar(point, K, poses[m])
                        if not zc > near:
                            continue
                        x0, y0 = np.floor(u), np.floor(v)
                        if not (x0 >= 0 and x0 < W - 1 and y0 >= 0 and y0 < H - 1):
                            continue
                        ax_, ay_ = u - x0, v - y0
                        ix, iy = int(x0), int(y0)
                        taps = [(iy, ix), (iy, ix + 1), (iy + 1, ix), (iy + 1, ix + 1)]
                        if not all(depth[m][t] > 0 and zc <= depth[m][t] + tol and depth[m][t] <= zc + tol for t in taps):
                            continue
                        R = poses[m][:9].reshape(3, 3)
                        nc = [(R[r, 0] * nv[0] + R[r, 1] * nv[1]) + R[r, 2] * nv[2] for r in range(3)]
                        dot = (nc[0] * xc + nc[1] * yc) + nc[2] * zc
                        c = (-dot) / np.sqrt((xc * xc + yc * yc) + zc * zc)
                        if not c > mc:
                            continue
                        val = []
                        for ch in range(3):
                            f00, f10, f01, f11 = (F32(images[m][t][ch]) for t in taps)
                            top = f00 + ax_ * (f10 - f00)
                            bot = f01 + ax_ * (f11 - f01)
                            val.append(top + ay_ * (bot - top))
                        if best_view:
                            if best is None or c > best_w:
                                best, best_w = val, c
                        else:
                            total = [total[ch] + c * val[ch] for ch in range(3)]
                            weight = weight + c
                            best = total
                    X, Y = place(i, j)
                    if best is None:
                        for ch in range(3):
                            atlas[Y, X, ch] = _round((b0 * F32(col[tri[0], ch]) + b1 * F32(col[tri[1], ch])) + b2 * F32(col[tri[2], ch]))
                        continue
                    n_textured += 1
                    q = best if best_view else [total[ch] / weight for ch in range(3)]
                    for ch in range(3):
                        atlas[Y, X, 2 - ch] = _round(q[ch])
    return atlas, uv, n_texels, n_textured


def lookup(g1, g2, N, miss=None):
    """The texel lookup of the textured render from g_1, g_2 (float32 arrays): (i, j, ax, ay, pulled back, clamped)."""
    fn = F32(N)
    with np.errstate(all="ignore"):
        x = np.minimum(np.maximum(g1 * fn, F32(0)), fn)
        y = np.minimum(np.maximum(g2 * fn, F32(0)), fn)
        fx, fy = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    clamped = (fx > N - 1) | (fy > N - 1)
    i, j = np.minimum(fx, N - 1), np.minimum(fy, N - 1)
    ax, ay = x - i.astype(F32), y - j.astype(F32)
    pull = i + j >= N
    if miss != "no pull-back":
        j = np.where(pull, N - 1 - i, j)
        ay = np.where(pull, F32(1.0), ay).astype(F32)
    return i, j, ax, ay, pull, clamped


def render_texture(verts, faces, atlas, K, poses, near, depth, face, N, cells_per_row=0, miss=None, counters=None):
    assert miss is None or miss in NEAR_MISSES
    poses = np.asarray(poses, F32).reshape(-1, 12)
    depth, face = np.asarray(depth, F32), np.asarray(face, np.int32)
    n, H, W = face.shape
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    cols = layout(len(f), N, cells_per_row)[0]
    tex = np.asarray(atlas, np.uint8).astype(F32)
    C = N + 3
    member = np.zeros((N + 2, N + 2), bool)
    member[tuple(face_texels(N).T)] = True
    out = np.zeros((n, H, W, 3), np.uint8)
    for m in range(n):
        py, px = np.nonzero(face[m] >= 0)
        if len(py) == 0:
            continue
        _, _, _, iz, _, sx, sy = rr.project(verts, K, poses[m], near)
        fid = face[m][py, px].astype(np.int64)
        tri = f[fid]
        i0, i1, i2 = tri[:, 0], tri[:, 1], tri[:, 2]
        area = (sx[i1] - sx[i0]) * (sy[i2] - sy[i0]) - (sy[i1] - sy[i0]) * (sx[i2] - sx[i0])
        swap = area < 0
        i1, i2 = np.where(swap, i2, i1), np.where(swap, i1, i2)
        area = np.abs(area)
        ids = (i0, i1, i2)
        Px, Py = px.astype(np.int64) * rr.SUB, py.astype(np.int64) * rr.SUB
        w = []
        for a, b in ((1, 2), (2, 0), (0, 1)):
            ax_, ay_, bx_, by_ = sx[ids[a]], sy[ids[a]], sx[ids[b]], sy[ids[b]]
            w.append((bx_ - ax_) * (Py - ay_) - (by_ - ay_) * (Px - ax_))
        with np.errstate(all="ignore"):
            fa = area.astype(F32)
            z = depth[m][py, px]
            e1 = z * ((w[1].astype(F32) / fa) * iz[ids[1]])
            e2 = z * ((w[2].astype(F32) / fa) * iz[ids[2]])
        back = swap & (miss != "g not exchanged back")
        g1, g2 = np.where(back, e2, e1), np.where(back, e1, e2)
        i, j, ax, ay, pull, clamped = lookup(g1, g2, N, miss)
        q = []
        taps_ok = np.ones(len(fid), bool)
        for di, dj in ((0, 0), (1, 0), (0, 1), (1, 1)):
            taps_ok &= member[i + di, j + dj]
            X, Y = atlas_position(fid, i + di, j + dj, N, cols)
            q.append(tex[Y, X])
        with np.errstate(all="ignore"):
            top = q[0] + ax[:, None] * (q[1] - q[0])
            bot = q[2] + ax[:, None] * (q[3] - q[2])
            val = top + ay[:, None] * (bot - top)
        out[m][py, px] = _byte(val)
        if counters is not None:
            for name, value in (("pull-back", pull), ("corner clamp", clamped), ("exchanged", swap), ("outside set", ~taps_ok)):
                counters[name] = counters.get(name, 0) + int(value.sum())
    return out


def render_texture_loops(verts, faces, atlas, K, poses, near, depth, face, N, cells_per_row=0):
    """render_texture() one pixel at a time: the render restatement's scalar projection, Python integers for the edge
    functions, float32 scalars for the rest."""
    poses = np.asarray(poses, F32).reshape(-1, 12)
    depth, face = np.asarray(depth, F32), np.asarray(face, np.int32)
    n, H, W = face.shape
    tris = np.asarray(faces).reshape(-1, 3)
    pts3 = np.asarray(verts, F32).reshape(-1, 3)
    cols = layout(len(tris), N, cells_per_row)[0]
    C = N + 3
    out = np.zeros((n, H, W, 3), np.uint8)
    for m in range(n):
        cache = {}
        for py in range(H):
            for px in range(W):
                fi = int(face[m, py, px])
                if fi < 0:
                    continue
                c = [int(i) for i in tris[fi]]
                for i in c:
                    if i not in cache:
                        cache[i] = rr._project_scalar(pts3[i], K, poses[m], near)
                pts = [(int(cache[i][2]), int(cache[i][3])) for i in c]
                area = (pts[1][0] - pts[0][0]) * (pts[2][1] - pts[0][1]) - (pts[1][1] - pts[0][1]) * (pts[2][0] - pts[0][0])
                flip = area < 0
                if flip:
                    c[1], c[2], pts[1], pts[2], area = c[2], c[1], pts[2], pts[1], -area
                w = []
                for a, b in ((1, 2), (2, 0), (0, 1)):
                    dx, dy = pts[b][0] - pts[a][0], pts[b][1] - pts[a][1]
                    w.append(dx * (rr.SUB * py - pts[a][1]) - dy * (rr.SUB * px - pts[a][0]))
                with np.errstate(all="ignore"):
                    z = depth[m, py, px]
                    g = [z * ((F32(np.int64(w[k])) / F32(np.int64(area))) * cache[c[k]][0]) for k in range(3)]
                    if flip:
                        g[1], g[2] = g[2], g[1]
                    x = min(max(g[1] * F32(N), F32(0)), F32(N))
                    y = min(max(g[2] * F32(N), F32(0)), F32(N))
                    i, j = min(int(np.floor(x)), N - 1), min(int(np.floor(y)), N - 1)
                    ax, ay = F32(x) - F32(i), F32(y) - F32(j)
                    if i + j >= N:
                        j, ay = N - 1 - i, F32(1.0)
                    cx, cy = ((fi // 2) % cols) * C, ((fi // 2) // cols) * C

                    def tap(ti, tj):
                        X, Y = (cx + C - 1 - ti, cy + C - 1 - tj) if fi % 2 else (cx + ti, cy + tj)
                        return atlas[Y, X].astype(F32)

                    f00, f10, f01, f11 = tap(i, j), tap(i + 1, j), tap(i, j + 1), tap(i + 1, j + 1)
                    for ch in range(3):
                        top = f00[ch] + ax * (f10[ch] - f00[ch])
                        bot = f01[ch] + ax * (f11[ch] - f01[ch])
                        out[m, py, px, ch] = _round(top + ay * (bot - top))
    return out
