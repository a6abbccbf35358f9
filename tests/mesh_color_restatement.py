"""NumPy restatement of the colours from the views and of the colour render (include/amvs.h amvs_mesh_color_views,
amvs_fetch_render_color; csrc/amvs_mesh_color.hip), written from the definition in the header and not from the kernels
(a helper module, not a conftest; no GPU).  Every float operation is a float32 NumPy operation rounded on its own, the
edge functions are exact in int64, so the device result must equal this one byte for byte.

    color_views(verts, normals, colors, K, poses, near, depth, images_bgr, tolerance, min_cos, best_view)
                                             (colours (V,3) uint8 RGB, n_colored); `miss` names a near-miss of the
                                             definition (NEAR_MISSES) that the tests must tell from it; `counters` (a
                                             dict) receives what every (vertex, view) pair ran into
    color_views_loops(...)                   the same by plain Python loops with a scalar projection of their own
    render_color(verts, faces, colors, K, poses, near, depth, face)      (n,H,W,3) uint8 RGB
    render_color_loops(...)                  the same by plain per-pixel loops
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_render_restatement as rr  # noqa: E402

F32 = np.float32
NEAR_MISSES = ("nearest pixel", "undrawn admitted", "nearer test only", "cosine >=", "bgr not swapped", "unweighted mean",
               "descending views", "truncation", "ties to the last", "fused sample")
COUNTERS = ("reached", "behind near", "border", "undrawn", "nearer", "farther", "cosine")


def _byte(q, truncate=False):
    """(g): floorf(q + 0.5f) clamped to 0 .. 255."""
    q = np.asarray(q, F32)
    with np.errstate(invalid="ignore"):         # a near-miss may divide 0 by 0; the definition never rounds a NaN
        r = np.floor(q) if truncate else np.floor(q + F32(0.5))
        return np.minimum(F32(255), np.maximum(F32(0), r)).astype(np.uint8)


def _fused(a, b, c):
    """a * b + c with one rounding (through float64, where the product of two float32 is exact)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def color_views(verts, normals, colors, K, poses, near, depth, images_bgr, tolerance, min_cos, best_view, miss=None,
                counters=None):
    assert miss is None or miss in NEAR_MISSES
    k = np.asarray(K, F32).reshape(9)
    poses = np.asarray(poses, F32).reshape(-1, 12)
    p = np.asarray(verts, F32).reshape(-1, 3)
    nrm = np.asarray(normals, F32).reshape(-1, 3)
    depth = np.asarray(depth, F32)
    images = np.asarray(images_bgr, np.uint8)
    n, H, W = depth.shape
    assert images.shape == (n, H, W, 3) and len(poses) == n
    tol, mc, near = F32(tolerance), F32(min_cos), F32(near)
    V = len(p)
    X, Y, Z = p[:, 0], p[:, 1], p[:, 2]
    S = np.zeros((V, 3), F32)                   # B, G, R sums, or the best view's values
    Wsum = np.zeros(V, F32)                     # sum of the weights, or the best weight
    reached = np.zeros(V, bool)
    count = dict.fromkeys(COUNTERS, 0)
    order = range(n - 1, -1, -1) if miss == "descending views" else range(n)
    with np.errstate(all="ignore"):
        for m in order:
            P = poses[m]
            zc = ((P[6] * X + P[7] * Y) + P[8] * Z) + P[11]
            xc = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[9]
            yc = ((P[3] * X + P[4] * Y) + P[5] * Z) + P[10]
            pu = (k[0] * xc + k[1] * yc) + k[2] * zc
            pv = (k[3] * xc + k[4] * yc) + k[5] * zc
            pw = (k[6] * xc + k[7] * yc) + k[8] * zc
            u, v = pu / pw, pv / pw
            front = zc > near
            x0, y0 = np.floor(u), np.floor(v)
            inside = (x0 >= 0) & (x0 < F32(W - 1)) & (y0 >= 0) & (y0 < F32(H - 1))
            ok = front & inside
            ax, ay = u - x0, v - y0
            ix, iy = np.where(ok, x0, 0).astype(np.int64), np.where(ok, y0, 0).astype(np.int64)
            d = np.stack([depth[m][iy, ix], depth[m][iy, ix + 1], depth[m][iy + 1, ix], depth[m][iy + 1, ix + 1]], axis=1)
            drawn = (d > 0).all(axis=1)
            z = zc[:, None]
            not_behind = (z <= d + tol).all(axis=1)
            not_before = (d <= z + tol).all(axis=1)
            if miss == "undrawn admitted":
                und = ~(d > 0)
                drawn = np.ones(V, bool)
                not_behind = ((z <= d + tol) | und).all(axis=1)
                not_before = ((d <= z + tol) | und).all(axis=1)
            if miss == "nearer test only":
                not_before = np.ones(V, bool)
            clear = drawn & not_behind & not_before
            ncx = (P[0] * nrm[:, 0] + P[1] * nrm[:, 1]) + P[2] * nrm[:, 2]
            ncy = (P[3] * nrm[:, 0] + P[4] * nrm[:, 1]) + P[5] * nrm[:, 2]
            ncz = (P[6] * nrm[:, 0] + P[7] * nrm[:, 1]) + P[8] * nrm[:, 2]
            dot = (ncx * xc + ncy * yc) + ncz * zc
            length = np.sqrt((xc * xc + yc * yc) + zc * zc)
            c = (-dot) / length
            facing = (c >= mc) if miss == "cosine >=" else (c > mc)
            use = ok & clear & facing
            count["behind near"] += int((~front).sum())
            count["border"] += int((front & ~inside).sum())
            count["undrawn"] += int((ok & ~drawn).sum())
            count["nearer"] += int((ok & drawn & ~not_behind).sum())
            count["farther"] += int((ok & drawn & not_behind & ~not_before).sum())
            count["cosine"] += int((ok & clear & ~facing).sum())
            count["reached"] += int(use.sum())
            w = np.ones(V, F32) if miss == "unweighted mean" else c
            img = images[m].astype(F32)
            f00, f10, f01, f11 = img[iy, ix], img[iy, ix + 1], img[iy + 1, ix], img[iy + 1, ix + 1]
            a, b = ax[:, None], ay[:, None]
            if miss == "nearest pixel":
                jx = np.where(ok, np.floor(u + F32(0.5)), 0).astype(np.int64)
                jy = np.where(ok, np.floor(v + F32(0.5)), 0).astype(np.int64)
                val = img[jy, jx]
            elif miss == "fused sample":
                top = _fused(np.broadcast_to(a, f00.shape), f10 - f00, f00)
                bot = _fused(np.broadcast_to(a, f00.shape), f11 - f01, f01)
                val = _fused(np.broadcast_to(b, f00.shape), bot - top, top)
            else:
                top = f00 + a * (f10 - f00)
                bot = f01 + a * (f11 - f01)
                val = top + b * (bot - top)
            if best_view:
                better = (w >= Wsum) if miss == "ties to the last" else (w > Wsum)
                take = use & (~reached | better)
                S[take] = val[take]
                Wsum[take] = w[take]
            else:
                S[use] = S[use] + w[use, None] * val[use]
                Wsum[use] = Wsum[use] + w[use]
            reached |= use
        q = S if best_view else S / Wsum[:, None]
    out = np.array(np.asarray(colors, np.uint8).reshape(-1, 3))
    bgr = _byte(q[reached], truncate=miss == "truncation")
    out[reached] = bgr if miss == "bgr not swapped" else bgr[:, ::-1]
    if counters is not None:
        for name in COUNTERS:
            counters[name] = counters.get(name, 0) + count[name]
    return out, int(reached.sum())


def _camera_scalar(point, K, pose):
    """(a) for one point, stated on its own: R as a 3 x 3 matrix and t, rows accumulated left to right in float32
    scalars.  Returns (xc, yc, zc, u, v)."""
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


def color_views_loops(verts, normals, colors, K, poses, near, depth, images_bgr, tolerance, min_cos, best_view):
    """color_views() one vertex and one view at a time, in float32 scalars (small inputs only)."""
    poses = np.asarray(poses, F32).reshape(-1, 12)
    depth = np.asarray(depth, F32)
    images = np.asarray(images_bgr, np.uint8)
    n, H, W = depth.shape
    tol, mc, near = F32(tolerance), F32(min_cos), F32(near)
    out = np.array(np.asarray(colors, np.uint8).reshape(-1, 3))
    nrm = np.asarray(normals, F32).reshape(-1, 3)
    n_colored = 0
    with np.errstate(all="ignore"):
        for vi, point in enumerate(np.asarray(verts, F32).reshape(-1, 3)):
            total, weight, best, best_w = [F32(0)] * 3, F32(0), None, None
            for m in range(n):
                xc, yc, zc, u, v = _camera_scalar(point, K, poses[m])
                if not zc > near:
                    continue
                x0, y0 = np.floor(u), np.floor(v)
                if not (x0 >= 0 and x0 < W - 1 and y0 >= 0 and y0 < H - 1):
                    continue
                ax, ay = u - x0, v - y0
                ix, iy = int(x0), int(y0)
                taps = [(iy, ix), (iy, ix + 1), (iy + 1, ix), (iy + 1, ix + 1)]
                if not all(depth[m][t] > 0 and zc <= depth[m][t] + tol and depth[m][t] <= zc + tol for t in taps):
                    continue
                R = poses[m][:9].reshape(3, 3)
                nc = [(R[r, 0] * nrm[vi, 0] + R[r, 1] * nrm[vi, 1]) + R[r, 2] * nrm[vi, 2] for r in range(3)]
                dot = (nc[0] * xc + nc[1] * yc) + nc[2] * zc
                c = (-dot) / np.sqrt((xc * xc + yc * yc) + zc * zc)
                if not c > mc:
                    continue
                val = []
                for ch in range(3):
                    f00, f10, f01, f11 = (F32(images[m][t][ch]) for t in taps)
                    top = f00 + ax * (f10 - f00)
                    bot = f01 + ax * (f11 - f01)
                    val.append(top + ay * (bot - top))
                if best_view:
                    if best is None or c > best_w:
                        best, best_w = val, c
                else:
                    total = [total[ch] + c * val[ch] for ch in range(3)]
                    weight = weight + c
                    best = total
            if best is None:
                continue
            n_colored += 1
            q = best if best_view else [total[ch] / weight for ch in range(3)]
            for ch in range(3):
                out[vi, 2 - ch] = min(255, max(0, int(np.floor(F32(q[ch]) + F32(0.5)))))
    return out, n_colored


def render_color(verts, faces, colors, K, poses, near, depth, face):
    poses = np.asarray(poses, F32).reshape(-1, 12)
    depth, face = np.asarray(depth, F32), np.asarray(face, np.int32)
    n, H, W = face.shape
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    col = np.asarray(colors, np.uint8).reshape(-1, 3).astype(F32)
    out = np.zeros((n, H, W, 3), np.uint8)
    for m in range(n):
        py, px = np.nonzero(face[m] >= 0)
        if len(py) == 0:
            continue
        _, _, _, iz, _, sx, sy = rr.project(verts, K, poses[m], near)
        tri = f[face[m][py, px]]
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
            t = [(w[i].astype(F32) / fa) * iz[ids[i]] for i in range(3)]
            z = depth[m][py, px]
            q = z[:, None] * ((t[0][:, None] * col[i0] + t[1][:, None] * col[i1]) + t[2][:, None] * col[i2])
        out[m][py, px] = _byte(q)
    return out


def render_color_loops(verts, faces, colors, K, poses, near, depth, face):
    """render_color() one pixel at a time: the render restatement's scalar projection, Python integers for the edge
    functions, float32 scalars for the rest."""
    poses = np.asarray(poses, F32).reshape(-1, 12)
    depth, face = np.asarray(depth, F32), np.asarray(face, np.int32)
    n, H, W = face.shape
    col = np.asarray(colors, np.uint8).reshape(-1, 3)
    pts3 = np.asarray(verts, F32).reshape(-1, 3)
    out = np.zeros((n, H, W, 3), np.uint8)
    for m in range(n):
        cache = {}
        for py in range(H):
            for px in range(W):
                fi = int(face[m, py, px])
                if fi < 0:
                    continue
                c = [int(i) for i in np.asarray(faces).reshape(-1, 3)[fi]]
                for i in c:
                    if i not in cache:
                        cache[i] = rr._project_scalar(pts3[i], K, poses[m], near)
                pts = [(int(cache[i][2]), int(cache[i][3])) for i in c]
                area = (pts[1][0] - pts[0][0]) * (pts[2][1] - pts[0][1]) - (pts[1][1] - pts[0][1]) * (pts[2][0] - pts[0][0])
                if area < 0:
                    c[1], c[2], pts[1], pts[2], area = c[2], c[1], pts[2], pts[1], -area
                w = []
                for a, b in ((1, 2), (2, 0), (0, 1)):
                    dx, dy = pts[b][0] - pts[a][0], pts[b][1] - pts[a][1]
                    w.append(dx * (rr.SUB * py - pts[a][1]) - dy * (rr.SUB * px - pts[a][0]))
                with np.errstate(all="ignore"):
                    t = [(F32(np.int64(w[i])) / F32(np.int64(area))) * cache[c[i]][0] for i in range(3)]
                    for ch in range(3):
                        q = depth[m, py, px] * ((t[0] * F32(col[c[0], ch]) + t[1] * F32(col[c[1], ch])) + t[2] * F32(col[c[2], ch]))
                        out[m, py, px, ch] = min(255, max(0, int(np.floor(F32(q) + F32(0.5)))))
    return out
