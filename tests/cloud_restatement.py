"""The point-cloud stage written out from its definition (a helper module, not a conftest; no GPU): include/amvs.h and
the header comments of csrc/amvs_fusion.hip / csrc/amvs_knn.hip, restated with Python floats (IEEE double, one rounding
per operation, nothing contracted) and integer loops.  tests/test_cloud_restatement_cpu.py shows that it gives the
reference's own clouds (g10, g12) bit for bit; tests/test_hip_cloud.py compares the device with it.

    select_fuse / select_stereo   which pixels of the stacked maps become points (float32 comparisons), row-major,
                                  map after map, with the per-map counts
    project                       the selected pixels in world space, float64, the two 3-term products as fused
                                  chains; colours BGR -> RGB
    filter_points                 95th-percentile radius cut around the per-axis median, then the 1 cm voxel grid
    voxel_downsample, take        the two steps on a resident cloud
    knn_mean                      mean distance to the k-1 nearest other points, brute force

The fused multiply-add is exact: fma(a, b, c) = float(Fraction(a) * Fraction(b) + Fraction(c)), one correct rounding.

Every function takes variant=: None is the definition, a name of VARIANTS one deliberate near-miss in its place.  The
near-misses exist only so that the CPU test can show that the input family tells each of them from the definition.
"""
import math
from fractions import Fraction

import numpy as np

VARIANTS = ("reciprocal_voxel", "trunc_voxel", "last_of_run", "input_order_output", "le_percentile",
            "single_branch_lerp", "upper_median", "unfused_project", "gt_conf", "ge_depth", "pose_of_map0", "bgr_kept",
            "knn_keep_self", "knn_plain_sum")
FILTER_VOXEL = 0.01


def _check(variant):
    if variant is not None and variant not in VARIANTS:
        raise ValueError(f"unknown variant {variant!r}")


def fma(a, b, c):
    """a * b + c with one rounding."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


# ---------------------------------------------------------------------------------------------- selection ---
def _per_map(sel, n_maps, hw):
    counts = [0] * n_maps
    for g in sel:
        counts[g // hw] += 1
    return counts


def select_fuse(conf, min_views, variant=None):
    """(flat indices into the stacked maps, ascending; points per map): confidence >= min_views in float32."""
    _check(variant)
    conf = np.asarray(conf, np.float32)
    thr = np.float32(min_views)
    flag = conf > thr if variant == "gt_conf" else conf >= thr
    sel = [int(g) for g in np.flatnonzero(flag.reshape(-1))]
    return sel, _per_map(sel, conf.shape[0], conf[0].size)


def select_stereo(conf, depth, min_confidence, variant=None):
    """confidence >= float32(min_confidence) and depth > 0, both in float32."""
    _check(variant)
    conf, depth = np.asarray(conf, np.float32), np.asarray(depth, np.float32)
    thr = np.float32(min_confidence)
    flag = conf > thr if variant == "gt_conf" else conf >= thr
    flag = flag & ((depth >= np.float32(0)) if variant == "ge_depth" else (depth > np.float32(0)))
    sel = [int(g) for g in np.flatnonzero(flag.reshape(-1))]
    return sel, _per_map(sel, conf.shape[0], conf[0].size)


# --------------------------------------------------------------------------------------------- projection ---
def project(sel, depth, bgr, K_inv, poses, variant=None):
    """Pixel sel[i] of the stacked (n, H, W) maps -> points[i] (float64), colours[i] (RGB):
    ray_j = fma(1, Kinv[j,2], fma(y, Kinv[j,1], x*Kinv[j,0])), c_j = ray_j*d - t_j,
    X_j = fma(c2, R[2,j], fma(c1, R[1,j], c0*R[0,j]))."""
    _check(variant)
    depth = np.asarray(depth, np.float32)
    n_maps, H, W = depth.shape
    bgr = np.asarray(bgr, np.uint8).reshape(n_maps, H * W, 3)
    flat = depth.reshape(-1)
    Ki = [[float(v) for v in row] for row in np.asarray(K_inv, np.float64).reshape(3, 3)]
    Rs = [[[float(v) for v in row] for row in np.asarray(R, np.float64).reshape(3, 3)] for R, _ in poses]
    ts = [[float(v) for v in np.asarray(t, np.float64).reshape(3)] for _, t in poses]
    pts = np.empty((len(sel), 3), np.float64)
    rgb = np.empty((len(sel), 3), np.uint8)
    for i, g in enumerate(sel):
        m, p = divmod(g, H * W)
        y, x = divmod(p, W)
        y, x, d = float(y), float(x), float(flat[g])
        pm = 0 if variant == "pose_of_map0" else m
        R, t = Rs[pm], ts[pm]
        c = [0.0] * 3
        for j in range(3):
            if variant == "unfused_project":
                ray = (x * Ki[j][0] + y * Ki[j][1]) + Ki[j][2]
            else:
                ray = fma(1.0, Ki[j][2], fma(y, Ki[j][1], x * Ki[j][0]))
            c[j] = ray * d - t[j]
        for j in range(3):
            if variant == "unfused_project":
                pts[i, j] = (c[0] * R[0][j] + c[1] * R[1][j]) + c[2] * R[2][j]
            else:
                pts[i, j] = fma(c[2], R[2][j], fma(c[1], R[1][j], c[0] * R[0][j]))
        b = bgr[m, p]
        rgb[i] = b if variant == "bgr_kept" else b[::-1]
    return pts, rgb


# ------------------------------------------------------------------------------------------------ filter ---
def median(values, variant=None):
    """np.median: the middle of the sorted values, (a + b) / 2 of the two middle ones for an even count."""
    s = sorted(values)
    m = len(s)
    if m % 2:
        return s[m // 2]
    return s[m // 2] if variant == "upper_median" else (s[m // 2 - 1] + s[m // 2]) / 2.0


def percentile95(values, variant=None):
    """np.percentile(values, 95), method 'linear': virtual index 0.95*(m-1) and NumPy's _lerp (a + diff*t, replaced
    by b - diff*(1-t) where t >= 0.5)."""
    s = sorted(values)
    m = len(s)
    vi = (95.0 / 100.0) * float(m - 1)
    prev = min(int(math.floor(vi)), m - 1)
    nxt = min(prev + 1, m - 1)
    t = vi - float(prev)
    a, b = s[prev], s[nxt]
    diff = b - a
    if t >= 0.5 and variant != "single_branch_lerp":
        return b - diff * (1.0 - t)
    return a + diff * t


def distances(points, variant=None):
    """Distance of every point to the per-axis median: sqrt((dx*dx + dy*dy) + dz*dz)."""
    P = [[float(v) for v in row] for row in np.asarray(points, np.float64).reshape(-1, 3)]
    c = [median([p[a] for p in P], variant) for a in range(3)]
    out = []
    for p in P:
        dx, dy, dz = p[0] - c[0], p[1] - c[1], p[2] - c[2]
        out.append(math.sqrt((dx * dx + dy * dy) + dz * dz))
    return out


def radius_keep(points, variant=None):
    """(indices kept by the radius cut, threshold, distances); the cut is strict."""
    dist = distances(points, variant)
    thr = percentile95(dist, variant)
    if variant == "le_percentile":
        return [i for i, d in enumerate(dist) if d <= thr], thr, dist
    return [i for i, d in enumerate(dist) if d < thr], thr, dist


def voxel_index(p, voxel, variant=None):
    q = p * (1.0 / voxel) if variant == "reciprocal_voxel" else p / voxel
    return math.trunc(q) if variant == "trunc_voxel" else math.floor(q)


def voxel_key(point, voxel, variant=None):
    """ix*10**9 + iy*10**6 + iz as a signed 64-bit integer."""
    ix, iy, iz = (voxel_index(float(v), voxel, variant) for v in point)
    key = ix * 10 ** 9 + iy * 10 ** 6 + iz
    return (key + 2 ** 63) % 2 ** 64 - 2 ** 63


def voxel_pick(points, idx, voxel, variant=None):
    """Of the points idx (in that order), the first of every voxel key, in ascending key order."""
    head = {}
    for i in idx:
        k = voxel_key(points[i], voxel, variant)
        if variant == "last_of_run" or k not in head:
            head[k] = i
    if variant == "input_order_output":
        return sorted(head.values())
    return [head[k] for k in sorted(head)]


def filter_points(points, colors, variant=None):
    _check(variant)
    points, colors = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(colors).reshape(-1, 3)
    if len(points) == 0:
        return points.copy(), colors.copy()
    keep, _, _ = radius_keep(points, variant)
    pick = voxel_pick(points, keep, FILTER_VOXEL, variant)
    return points[pick], colors[pick]


def voxel_downsample(points, colors, voxel, keep=None, variant=None):
    _check(variant)
    points, colors = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(colors).reshape(-1, 3)
    idx = [i for i in range(len(points)) if keep is None or keep[i]]
    pick = voxel_pick(points, idx, float(voxel), variant)
    return points[pick], colors[pick]


def take(points, colors, idx):
    idx = [int(i) for i in idx]
    points, colors = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(colors).reshape(-1, 3)
    n = len(points)
    if any(i < 0 or i >= n for i in idx):
        raise IndexError("index outside the cloud")
    return points[idx].reshape(-1, 3), colors[idx].reshape(-1, 3)


def fuse_filter(case, do_filter=True, variant=None):
    """(points, colours, raw count) of a cloud_inputs.MapCase through select_fuse, project and filter_points."""
    sel, _ = select_fuse(case.conf, case.threshold, variant)
    pts, rgb = project(sel, case.depth, case.bgr, case.K_inv, case.poses, variant)
    if do_filter:
        pts, rgb = filter_points(pts, rgb, variant)
    return pts, rgb, len(sel)


def backproject(case, variant=None):
    """(points, colours, per-map counts) of a cloud_inputs.MapCase through select_stereo and project."""
    sel, per = select_stereo(case.conf, case.depth, case.threshold, variant)
    pts, rgb = project(sel, case.depth, case.bgr, case.K_inv, case.poses, variant)
    return pts, rgb, per


# --------------------------------------------------------------------------------------------------- kNN ---
def pairwise_sum(v):
    """NumPy's pairwise summation of fewer than 128 values, along the last axis of v."""
    n = v.shape[-1]
    if n < 8:
        res = np.zeros(v.shape[:-1])
        for i in range(n):
            res = res + v[..., i]
        return res
    r = [v[..., j].copy() for j in range(8)]
    body = n - n % 8
    for i in range(8, body, 8):
        for j in range(8):
            r[j] = r[j] + v[..., i + j]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for i in range(body, n):
        res = res + v[..., i]
    return res


def knn_mean(points, k, queries=None, variant=None, chunk=256):
    """For every query (all points, or the rows `queries`): all ((dx*dx)+(dy*dy))+(dz*dz) to every point, the k
    smallest, their square roots ascending, the first (the query itself) dropped, the rest summed in NumPy's pairwise
    order and divided by k-1.  NumPy's elementwise float64 operations round once each and fuse nothing."""
    _check(variant)
    P = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    n = len(P)
    if not 2 <= k <= n:
        raise ValueError("needs 2 <= k <= n")
    q_idx = np.arange(n) if queries is None else np.asarray(queries, np.int64)
    out = np.empty(len(q_idx), np.float64)
    for s in range(0, len(q_idx), chunk):
        Q = P[q_idx[s:s + chunk]]
        dx = Q[:, None, 0] - P[None, :, 0]
        d2 = dx * dx
        dy = Q[:, None, 1] - P[None, :, 1]
        d2 = d2 + dy * dy
        dz = Q[:, None, 2] - P[None, :, 2]
        d2 = d2 + dz * dz
        small = np.sort(np.partition(d2, k - 1, axis=1)[:, :k], axis=1)
        d = np.sqrt(small)
        rest = d[:, :k - 1] if variant == "knn_keep_self" else d[:, 1:]
        if variant == "knn_plain_sum":
            tot = np.zeros(len(Q))
            for i in range(k - 1):
                tot = tot + rest[:, i]
        else:
            tot = pairwise_sum(rest)
        out[s:s + chunk] = tot / float(k - 1)
    return out
