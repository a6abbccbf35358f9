"""Normals from the depth maps written out from their definition (a helper module, not a conftest; no GPU): the text of
include/amvs.h under "oriented normals for the cloud", restated twice.

    fit_normals, cloud_normals            Python floats (IEEE double, one rounding per operation, nothing contracted) and
                                          Python integers, pixel by pixel and point by point
    fit_normals_np, cloud_normals_np      the vectorised NumPy twin for larger inputs: the same operations in the same
                                          order, element-wise over all pixels / points

tests/test_cloud_normals_cpu.py shows that the two agree bit for bit; tests/test_hip_cloud_normals.py compares the device
with them.  Both take variant=: None is the definition, a name of VARIANTS one deliberate near-miss in its place.  The
near-misses exist only so that the CPU test can show that the input family tells each of them from the definition.

Both return branch counters, one per guard and per exact edge of the definition (FIT_COUNTERS, CLOUD_COUNTERS).
"""
import math

import numpy as np

VARIANTS = ("swap_loops", "q_from_centre", "lt_jump", "lt_tolerance", "rint_pixel", "no_c_guard", "unit_weight",
            "gt_min_views", "f32_Sq", "K_not_transposed")
FLT_MAX = float(np.finfo(np.float32).max)

FIT_COUNTERS = ("centre_invalid", "nbr_outside", "nbr_invalid", "jump_rejected", "jump_equal", "few_points",
                "n_eq_min_points", "n_eq_min_points_minus_1", "det_zero", "c_not_positive", "len_bad", "normal")
CLOUD_COUNTERS = ("behind", "xc2_zero", "outside", "u_eq_minus_half", "u_eq_w_minus_half", "pixel_tie", "no_normal_pixel",
                  "depth_rejected", "depth_equal", "backfacing", "added", "few_views", "seen_eq_min_views_minus_1", "l_zero",
                  "normal")


def _check(variant):
    if variant is not None and variant not in VARIANTS:
        raise ValueError(f"unknown variant {variant!r}")


def _rows(a, shape):
    return [[float(v) for v in row] for row in np.asarray(a, np.float64).reshape(shape)]


def _poses(poses):
    return ([_rows(R, (3, 3)) for R, _ in poses], [[float(v) for v in np.asarray(t, np.float64).reshape(3)] for _, t in poses])


def _valid(d, c, thr):
    return d > 0.0 and d <= FLT_MAX and c >= thr           # (float32 values widened: the same comparisons; NaN fails each)


def _f32(v):
    with np.errstate(over="ignore"):                      # (a sum beyond FLT_MAX rounds to infinity, as on the device)
        return float(np.float32(v))


# ------------------------------------------------------------------------------------------------- the fit ---
def fit_normals(depth, conf, K, poses, min_confidence, radius, jump, min_points, world, variant=None):
    """(normals (n, H, W, 3) float32, pixels with a normal, counters) of the stacked (n, H, W) float32 maps."""
    _check(variant)
    depth, conf = np.asarray(depth, np.float32), np.asarray(conf, np.float32)
    n_maps, H, W = depth.shape
    Kr = _rows(K, (3, 3))
    Rs, _ = _poses(poses)
    thr, jmp = _f32(min_confidence), _f32(jump)
    out = np.zeros((n_maps, H, W, 3), np.float32)
    cnt = dict.fromkeys(FIT_COUNTERS, 0)
    offsets = [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]
    if variant == "swap_loops":
        offsets = [(dy, dx) for dx in range(-radius, radius + 1) for dy in range(-radius, radius + 1)]
    for j in range(n_maps):
        D = [[float(v) for v in row] for row in depth[j]]
        Cf = [[float(v) for v in row] for row in conf[j]]
        R = Rs[j]
        for y0 in range(H):
            for x0 in range(W):
                dc = D[y0][x0]
                if not _valid(dc, Cf[y0][x0], thr):
                    cnt["centre_invalid"] += 1
                    continue
                lim = jmp * dc
                n = sx = sy = sxx = sxy = syy = 0
                Sq = Sxq = Syq = 0.0
                for dy, dx in offsets:
                    y, x = y0 + dy, x0 + dx
                    if y < 0 or y >= H or x < 0 or x >= W:
                        cnt["nbr_outside"] += 1
                        continue
                    dn = D[y][x]
                    if not _valid(dn, Cf[y][x], thr):
                        cnt["nbr_invalid"] += 1
                        continue
                    gap = math.fabs(dn - dc)
                    if gap == lim and (dy or dx):
                        cnt["jump_equal"] += 1
                    if not (gap < lim if variant == "lt_jump" and (dy or dx) else gap <= lim):
                        cnt["jump_rejected"] += 1
                        continue
                    q = 1.0 / (dc if variant == "q_from_centre" else dn)
                    n += 1; sx += dx; sy += dy; sxx += dx * dx; sxy += dx * dy; syy += dy * dy
                    Sq = _f32(Sq + q) if variant == "f32_Sq" else Sq + q
                    Sxq = Sxq + float(dx) * q
                    Syq = Syq + float(dy) * q
                C00, C01, C02 = syy * n - sy * sy, sx * sy - sxy * n, sxy * sy - sx * syy
                C11, C12, C22 = sxx * n - sx * sx, sxy * sx - sxx * sy, sxx * syy - sxy * sxy
                det = sxx * C00 + sxy * C01 + sx * C02
                cnt["n_eq_min_points"] += n == min_points
                cnt["n_eq_min_points_minus_1"] += n == min_points - 1
                if n < min_points:
                    cnt["few_points"] += 1
                    continue
                if det == 0:
                    cnt["det_zero"] += 1
                    continue
                assert det > 0 and abs(det) < 2 ** 53
                a = (float(C00) * Sxq + float(C01) * Syq) + float(C02) * Sq
                b = (float(C01) * Sxq + float(C11) * Syq) + float(C12) * Sq
                c = (float(C02) * Sxq + float(C12) * Syq) + float(C22) * Sq
                if not c > 0.0:
                    cnt["c_not_positive"] += 1
                    if variant != "no_c_guard":
                        continue
                cp = (c - a * float(x0)) - b * float(y0)
                if variant == "K_not_transposed":
                    m = [(Kr[i][0] * a + Kr[i][1] * b) + Kr[i][2] * cp for i in range(3)]
                else:
                    m = [(Kr[0][i] * a + Kr[1][i] * b) + Kr[2][i] * cp for i in range(3)]
                s = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
                ln = math.sqrt(s) if s >= 0.0 else float("nan")
                if not (ln > 0.0 and ln <= 1.7976931348623157e308):
                    cnt["len_bad"] += 1
                    continue
                v = [-m[0] / ln, -m[1] / ln, -m[2] / ln]
                if world:
                    v = [(R[0][i] * v[0] + R[1][i] * v[1]) + R[2][i] * v[2] for i in range(3)]
                out[j, y0, x0] = v
                cnt["normal"] += 1
    return out, cnt["normal"], cnt


def fit_normals_np(depth, conf, K, poses, min_confidence, radius, jump, min_points, world, variant=None):
    """The twin of fit_normals: every operation element-wise over all pixels, in the same order."""
    _check(variant)
    depth, conf = np.asarray(depth, np.float32), np.asarray(conf, np.float32)
    n_maps, H, W = depth.shape
    Kr = np.asarray(K, np.float64).reshape(3, 3)
    Rs = np.stack([np.asarray(R, np.float64).reshape(3, 3) for R, _ in poses])
    thr, jmp = np.float32(min_confidence), np.float64(np.float32(jump))
    cnt = dict.fromkeys(FIT_COUNTERS, 0)
    with np.errstate(all="ignore"):
        valid = (depth > np.float32(0)) & (depth <= np.float32(FLT_MAX)) & (conf >= thr)
        D = depth.astype(np.float64)
        lim = jmp * D
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        zi = np.zeros((n_maps, H, W), np.int64)
        n, sx, sy, sxx, sxy, syy = (zi.copy() for _ in range(6))
        Sq, Sxq, Syq = (np.zeros((n_maps, H, W), np.float64) for _ in range(3))
        offsets = [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]
        if variant == "swap_loops":
            offsets = [(dy, dx) for dx in range(-radius, radius + 1) for dy in range(-radius, radius + 1)]
        for dy, dx in offsets:
            inside = ((ys + dy >= 0) & (ys + dy < H) & (xs + dx >= 0) & (xs + dx < W))[None] & valid
            cnt["nbr_outside"] += int((valid & ~inside).sum())
            yy, xx = np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1)
            dn, vn = D[:, yy, xx], valid[:, yy, xx]
            cnt["nbr_invalid"] += int((inside & ~vn).sum())
            cand = inside & vn
            gap = np.abs(dn - D)
            off = bool(dy or dx)
            if off:
                cnt["jump_equal"] += int((cand & (gap == lim)).sum())
            used = cand & ((gap < lim) if variant == "lt_jump" and off else (gap <= lim))
            cnt["jump_rejected"] += int((cand & ~used).sum())
            q = 1.0 / (D if variant == "q_from_centre" else dn)
            n += used; sx += used * dx; sy += used * dy; sxx += used * (dx * dx); sxy += used * (dx * dy); syy += used * (dy * dy)
            if variant == "f32_Sq":
                Sq = np.where(used, (Sq + q).astype(np.float32).astype(np.float64), Sq)
            else:
                Sq = np.where(used, Sq + q, Sq)
            Sxq = np.where(used, Sxq + np.float64(dx) * q, Sxq)
            Syq = np.where(used, Syq + np.float64(dy) * q, Syq)
        C00, C01, C02 = syy * n - sy * sy, sx * sy - sxy * n, sxy * sy - sx * syy
        C11, C12, C22 = sxx * n - sx * sx, sxy * sx - sxx * sy, sxx * syy - sxy * sxy
        det = sxx * C00 + sxy * C01 + sx * C02
        cnt["centre_invalid"] = int((~valid).sum())
        cnt["n_eq_min_points"] = int((valid & (n == min_points)).sum())
        cnt["n_eq_min_points_minus_1"] = int((valid & (n == min_points - 1)).sum())
        few = valid & (n < min_points)
        cnt["few_points"] = int(few.sum())
        live = valid & ~few
        cnt["det_zero"] = int((live & (det == 0)).sum())
        live = live & (det != 0)
        f = np.float64
        a = (C00.astype(f) * Sxq + C01.astype(f) * Syq) + C02.astype(f) * Sq
        b = (C01.astype(f) * Sxq + C11.astype(f) * Syq) + C12.astype(f) * Sq
        c = (C02.astype(f) * Sxq + C12.astype(f) * Syq) + C22.astype(f) * Sq
        bad_c = live & ~(c > 0.0)
        cnt["c_not_positive"] = int(bad_c.sum())
        if variant != "no_c_guard":
            live = live & ~bad_c
        cp = (c - a * xs.astype(f)[None]) - b * ys.astype(f)[None]
        if variant == "K_not_transposed":
            m = [(Kr[i, 0] * a + Kr[i, 1] * b) + Kr[i, 2] * cp for i in range(3)]
        else:
            m = [(Kr[0, i] * a + Kr[1, i] * b) + Kr[2, i] * cp for i in range(3)]
        ln = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        good = (ln > 0.0) & (ln <= np.finfo(f).max)
        cnt["len_bad"] = int((live & ~good).sum())
        live = live & good
        v = [-m[0] / ln, -m[1] / ln, -m[2] / ln]
        if world:
            Rm = Rs[:, :, :, None, None]
            v = [(Rm[:, 0, i] * v[0] + Rm[:, 1, i] * v[1]) + Rm[:, 2, i] * v[2] for i in range(3)]
        out = np.zeros((n_maps, H, W, 3), np.float32)
        for i in range(3):
            out[..., i] = np.where(live, v[i], 0.0).astype(np.float32)
    cnt["normal"] = int(live.sum())
    return out, cnt["normal"], cnt


# ------------------------------------------------------------------------------------------- cloud normals ---
def _round_pixel(u, variant):
    if variant == "rint_pixel":
        return float(np.rint(u)) if math.isfinite(u) else float("nan")
    return math.floor(u + 0.5) * 1.0 if math.isfinite(u + 0.5) else float("nan")


def cloud_normals(points, depth, normal_maps, K, poses, depth_tolerance, min_views, variant=None):
    """(normals (N, 3) float32, seen (N,) int32, points with a normal, counters): `normal_maps` are the WORLD-frame maps
    of fit_normals for the same stacked depth maps."""
    _check(variant)
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    depth, nm = np.asarray(depth, np.float32), np.asarray(normal_maps, np.float32)
    n_maps, H, W = depth.shape
    Kr = _rows(K, (3, 3))
    Rs, ts = _poses(poses)
    tol = _f32(depth_tolerance)
    out = np.zeros((len(pts), 3), np.float32)
    seen_out = np.zeros(len(pts), np.int32)
    cnt = dict.fromkeys(CLOUD_COUNTERS, 0)
    for p in range(len(pts)):
        X = [float(v) for v in pts[p]]
        s = [0.0, 0.0, 0.0]
        seen = 0
        for j in range(n_maps):
            R, t = Rs[j], ts[j]
            Xc = [((R[i][0] * X[0] + R[i][1] * X[1]) + R[i][2] * X[2]) + t[i] for i in range(3)]
            uvw = [(Kr[i][0] * Xc[0] + Kr[i][1] * Xc[1]) + Kr[i][2] * Xc[2] for i in range(3)]
            if not (uvw[2] > 0.0 and Xc[2] > 0.0):
                cnt["behind"] += 1
                cnt["xc2_zero"] += Xc[2] == 0.0
                continue
            u, v = uvw[0] / uvw[2], uvw[1] / uvw[2]
            cnt["u_eq_minus_half"] += u == -0.5
            cnt["u_eq_w_minus_half"] += u == W - 0.5
            px, py = _round_pixel(u, variant), _round_pixel(v, variant)
            if not (0.0 <= px < float(W) and 0.0 <= py < float(H)):
                cnt["outside"] += 1
                continue
            cnt["pixel_tie"] += (u + 0.5 == math.floor(u + 0.5)) or (v + 0.5 == math.floor(v + 0.5))
            px, py = int(px), int(py)
            n = [float(c) for c in nm[j, py, px]]
            if not (n[0] != 0.0 or n[1] != 0.0 or n[2] != 0.0):
                cnt["no_normal_pixel"] += 1
                continue
            d = float(depth[j, py, px])
            gap, lim = math.fabs(d - Xc[2]), tol * d
            cnt["depth_equal"] += gap == lim
            if not (gap < lim if variant == "lt_tolerance" else gap <= lim):
                cnt["depth_rejected"] += 1
                continue
            nc = [(R[i][0] * n[0] + R[i][1] * n[1]) + R[i][2] * n[2] for i in range(3)]
            w = (-((nc[0] * Xc[0] + nc[1] * Xc[1]) + nc[2] * Xc[2])) / math.sqrt((Xc[0] * Xc[0] + Xc[1] * Xc[1]) + Xc[2] * Xc[2])
            if not w > 0.0:
                cnt["backfacing"] += 1
                continue
            if variant == "unit_weight":
                w = 1.0
            s = [s[i] + w * n[i] for i in range(3)]
            seen += 1
            cnt["added"] += 1
        L = math.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
        seen_out[p] = seen
        cnt["seen_eq_min_views_minus_1"] += seen == min_views - 1
        enough = seen > min_views if variant == "gt_min_views" else seen >= min_views
        if not enough:
            cnt["few_views"] += 1
        elif not L > 0.0:
            cnt["l_zero"] += 1
        else:
            out[p] = [s[0] / L, s[1] / L, s[2] / L]
            cnt["normal"] += 1
    return out, seen_out, cnt["normal"], cnt


def cloud_normals_np(points, depth, normal_maps, K, poses, depth_tolerance, min_views, variant=None):
    """The twin of cloud_normals: the maps in ascending order, every operation element-wise over all points."""
    _check(variant)
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    depth, nm = np.asarray(depth, np.float32), np.asarray(normal_maps, np.float32)
    n_maps, H, W = depth.shape
    Kr = np.asarray(K, np.float64).reshape(3, 3)
    tol = np.float64(np.float32(depth_tolerance))
    N = len(pts)
    X = [pts[:, i] for i in range(3)]
    s = [np.zeros(N) for _ in range(3)]
    seen = np.zeros(N, np.int32)
    cnt = dict.fromkeys(CLOUD_COUNTERS, 0)
    with np.errstate(all="ignore"):
        for j in range(n_maps):
            R = np.asarray(poses[j][0], np.float64).reshape(3, 3)
            t = np.asarray(poses[j][1], np.float64).reshape(3)
            Xc = [((R[i, 0] * X[0] + R[i, 1] * X[1]) + R[i, 2] * X[2]) + t[i] for i in range(3)]
            uvw = [(Kr[i, 0] * Xc[0] + Kr[i, 1] * Xc[1]) + Kr[i, 2] * Xc[2] for i in range(3)]
            front = (uvw[2] > 0.0) & (Xc[2] > 0.0)
            cnt["behind"] += int((~front).sum())
            cnt["xc2_zero"] += int((~front & (Xc[2] == 0.0)).sum())
            u, v = uvw[0] / uvw[2], uvw[1] / uvw[2]
            cnt["u_eq_minus_half"] += int((front & (u == -0.5)).sum())
            cnt["u_eq_w_minus_half"] += int((front & (u == W - 0.5)).sum())
            if variant == "rint_pixel":
                px, py = np.rint(u), np.rint(v)
            else:
                px, py = np.floor(u + 0.5), np.floor(v + 0.5)
            inside = front & (px >= 0.0) & (px < float(W)) & (py >= 0.0) & (py < float(H))
            cnt["outside"] += int((front & ~inside).sum())
            cnt["pixel_tie"] += int((inside & ((u + 0.5 == np.floor(u + 0.5)) | (v + 0.5 == np.floor(v + 0.5)))).sum())
            ix = np.where(inside, px, 0.0).astype(np.int64)
            iy = np.where(inside, py, 0.0).astype(np.int64)
            n = [nm[j, iy, ix, i].astype(np.float64) for i in range(3)]
            has = inside & ((n[0] != 0.0) | (n[1] != 0.0) | (n[2] != 0.0))
            cnt["no_normal_pixel"] += int((inside & ~has).sum())
            d = depth[j, iy, ix].astype(np.float64)
            gap, lim = np.abs(d - Xc[2]), tol * d
            cnt["depth_equal"] += int((has & (gap == lim)).sum())
            near = has & ((gap < lim) if variant == "lt_tolerance" else (gap <= lim))
            cnt["depth_rejected"] += int((has & ~near).sum())
            nc = [(R[i, 0] * n[0] + R[i, 1] * n[1]) + R[i, 2] * n[2] for i in range(3)]
            w = (-((nc[0] * Xc[0] + nc[1] * Xc[1]) + nc[2] * Xc[2])) / np.sqrt((Xc[0] * Xc[0] + Xc[1] * Xc[1]) + Xc[2] * Xc[2])
            add = near & (w > 0.0)
            cnt["backfacing"] += int((near & ~add).sum())
            if variant == "unit_weight":
                w = np.ones(N)
            s = [np.where(add, s[i] + w * n[i], s[i]) for i in range(3)]
            seen = seen + add.astype(np.int32)
            cnt["added"] += int(add.sum())
        L = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
        enough = (seen > min_views) if variant == "gt_min_views" else (seen >= min_views)
        ok = enough & (L > 0.0)
        out = np.zeros((N, 3), np.float32)
        for i in range(3):
            out[:, i] = np.where(ok, s[i] / L, 0.0).astype(np.float32)
    cnt["seen_eq_min_views_minus_1"] = int((seen == min_views - 1).sum())
    cnt["few_views"] = int((~enough).sum())
    cnt["l_zero"] = int((enough & ~(L > 0.0)).sum())
    cnt["normal"] = int(ok.sum())
    return out, seen.astype(np.int32), cnt["normal"], cnt
