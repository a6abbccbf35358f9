"""The cross-view depth-map filter restated from the text of include/amvs_depth.h (a helper module, not a conftest; no GPU,
no library): depth_filter() in plain Python loops over Python floats (IEEE float64, one rounding per operation, nothing
contracted) and depth_filter_np(), a NumPy twin that walks the neighbours in the same order with whole images as operands
(elementwise float64 only: no `@`, no matmul, no einsum -- BLAS contracts).  tests/test_depth_filter_cpu.py holds the two
to each other bit for bit; tests/test_hip_depth_filter.py holds csrc/amvs_depth_filter.hip to them.

Both return (depth_out (n,H,W) float32, count_out (n,H,W) float32, (valid input pixels, pixels kept), counters).  The
counters say how often each guard and each exact edge of the definition was met, so that the CPU test can hold the input
family to reaching every one of them:

    centre_depth_nonpositive, centre_depth_nonfinite, centre_conf_low   an invalid centre pixel, by its first cause
    Xi_behind, uvw_behind                                               steps 3 and 4: Xi_2 <= 0, uvw_2 <= 0
    outside_left, outside_right, outside_top, outside_bottom            step 4, by the first side that fails
    nbr_depth_nonpositive, nbr_depth_nonfinite, nbr_conf_low            step 5, by its first cause
    Y_behind, back_uvw_behind                                           steps 6 and 7: Y_2 <= 0, uvw_2 <= 0
    e2_fail, e2_tie                                                     step 8: e2 above the bound; exactly on it
    depth_fail, depth_tie                                               step 8: the depth apart by more; exactly the bound
    consistent                                                          step 8 passed
    cnt_just_below, cnt_at_min                                          valid pixels with cnt == min_consistent - 1; == min_consistent

`variant` names a near-miss of the definition (VARIANTS): what a plausible implementation would do instead.  The CPU test
shows that the input family tells every one of them from the definition.
"""
import math

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)

COUNTERS = ("centre_depth_nonpositive", "centre_depth_nonfinite", "centre_conf_low", "Xi_behind", "uvw_behind",
            "outside_left", "outside_right", "outside_top", "outside_bottom", "nbr_depth_nonpositive", "nbr_depth_nonfinite",
            "nbr_conf_low", "Y_behind", "back_uvw_behind", "e2_fail", "e2_tie", "depth_fail", "depth_tie", "consistent",
            "cnt_just_below", "cnt_at_min")
TIE_COUNTERS = ("e2_tie", "depth_tie")

VARIANTS = (
    "lt_for_le",               # step 8 with < for <=
    "truncate",                # step 4 with truncation toward zero for floor(. + 0.5)
    "backproject_uv",          # step 6 from the unrounded (u, v) instead of the integer pixel
    "mean_without_centre",     # the refined depth as the mean of the agreeing depths alone
    "reverse_order",           # the neighbours of a row visited last to first
    "count_after_threshold",   # the count zeroed with the depth (the definition stores it before the threshold)
    "float32",                 # all arithmetic in float32
)


def neighbour_rows(n_maps, neighbours):
    """The rows the definition walks: the given [n_maps][n_nbr] list, or every other map in ascending index."""
    if neighbours is None:
        return [[i for i in range(n_maps) if i != j] for j in range(n_maps)]
    rows = np.asarray(neighbours, np.int64).reshape(n_maps, -1)
    return [[int(i) for i in row] for row in rows]


def _check(variant):
    if variant is not None and variant not in VARIANTS:
        raise ValueError(f"unknown variant {variant!r}")


def _invalid_cause(d, c, mc):
    """None for a VALID pixel (float32 values widened exactly, so float64 comparisons are the float32 ones), else the
    first cause."""
    if not d > 0.0:
        return "depth_nonpositive"
    if not d <= FLT_MAX:
        return "depth_nonfinite"
    if not c >= mc:
        return "conf_low"
    return None


# ------------------------------------------------------------------------------------------------ the loops ---
def _reproject(Ki, A, B, x, y, d):
    """Steps 1 to 3: pixel (x, y) at depth d of the camera with pose A = (R, t) into the camera with pose B."""
    RA, tA = A
    RB, tB = B
    Q = [0.0] * 3
    for c in range(3):
        r = (Ki[c][0] * x + Ki[c][1] * y) + Ki[c][2]
        P = r * d
        Q[c] = P - tA[c]
    Xw = [(RA[0][c] * Q[0] + RA[1][c] * Q[1]) + RA[2][c] * Q[2] for c in range(3)]
    return [((RB[c][0] * Xw[0] + RB[c][1] * Xw[1]) + RB[c][2] * Xw[2]) + tB[c] for c in range(3)]


def _project(K, X):
    return [(K[c][0] * X[0] + K[c][1] * X[1]) + K[c][2] * X[2] for c in range(3)]


def _floor(q, F):
    if F is float:
        return float(math.floor(q)) if math.isfinite(q) else q
    return np.floor(q)


def _trunc(q, F):
    if F is float:
        return float(math.trunc(q)) if math.isfinite(q) else q
    return np.trunc(q)


def depth_filter(depth, conf, K, K_inv, poses, neighbours, min_confidence, max_px, max_rel, min_consistent, refine,
                 variant=None):
    _check(variant)
    F = np.float32 if variant == "float32" else float            # the number type of every operation below
    depth = np.ascontiguousarray(depth, np.float32)
    conf = np.ascontiguousarray(conf, np.float32)
    n, H, W = depth.shape
    dl, cl = depth.astype(np.float64).tolist(), conf.astype(np.float64).tolist()      # (exact widening)
    mc = float(np.float32(min_confidence))
    Kf = [[F(v) for v in row] for row in np.asarray(K, np.float64).reshape(3, 3)]
    Ki = [[F(v) for v in row] for row in np.asarray(K_inv, np.float64).reshape(3, 3)]
    P = [([[F(v) for v in row] for row in np.asarray(R, np.float64).reshape(3, 3)],
          [F(v) for v in np.asarray(t, np.float64).reshape(3)]) for R, t in poses]
    px_bound = F(np.float32(max_px)) * F(np.float32(max_px))
    rel = F(np.float32(max_rel))
    half, zero = F(0.5), F(0.0)
    rows = neighbour_rows(n, neighbours)
    depth_out = np.zeros((n, H, W), np.float32)
    count_out = np.zeros((n, H, W), np.float32)
    k = dict.fromkeys(COUNTERS, 0)
    n_valid = n_kept = 0
    with np.errstate(all="ignore"):
        for j in range(n):
            row = rows[j][::-1] if variant == "reverse_order" else rows[j]
            for y0 in range(H):
                for x0 in range(W):
                    cause = _invalid_cause(dl[j][y0][x0], cl[j][y0][x0], mc)
                    if cause is not None:
                        k["centre_" + cause] += 1
                        continue
                    n_valid += 1
                    d, x, y = F(dl[j][y0][x0]), F(x0), F(y0)
                    lim = rel * d
                    cnt = 0
                    s = zero if variant == "mean_without_centre" else d
                    for i in row:
                        if i < 0:
                            continue
                        Xi = _reproject(Ki, P[j], P[i], x, y, d)
                        if not Xi[2] > zero:
                            k["Xi_behind"] += 1
                            continue
                        uvw = _project(Kf, Xi)
                        if not uvw[2] > zero:
                            k["uvw_behind"] += 1
                            continue
                        if variant == "truncate":
                            px, py = _trunc(uvw[0] / uvw[2], F), _trunc(uvw[1] / uvw[2], F)
                        else:
                            px, py = _floor(uvw[0] / uvw[2] + half, F), _floor(uvw[1] / uvw[2] + half, F)
                        if not px >= zero:
                            k["outside_left"] += 1
                            continue
                        if not px < F(W):
                            k["outside_right"] += 1
                            continue
                        if not py >= zero:
                            k["outside_top"] += 1
                            continue
                        if not py < F(H):
                            k["outside_bottom"] += 1
                            continue
                        ix, iy = int(px), int(py)
                        cause = _invalid_cause(dl[i][iy][ix], cl[i][iy][ix], mc)
                        if cause is not None:
                            k["nbr_" + cause] += 1
                            continue
                        di = F(dl[i][iy][ix])
                        if variant == "backproject_uv":
                            Y = _reproject(Ki, P[i], P[j], uvw[0] / uvw[2], uvw[1] / uvw[2], di)
                        else:
                            Y = _reproject(Ki, P[i], P[j], px, py, di)
                        if not Y[2] > zero:
                            k["Y_behind"] += 1
                            continue
                        uvw = _project(Kf, Y)
                        if not uvw[2] > zero:
                            k["back_uvw_behind"] += 1
                            continue
                        eu, ev = uvw[0] / uvw[2] - x, uvw[1] / uvw[2] - y
                        e2 = eu * eu + ev * ev
                        if e2 == px_bound:
                            k["e2_tie"] += 1
                        if not (e2 < px_bound if variant == "lt_for_le" else e2 <= px_bound):
                            k["e2_fail"] += 1
                            continue
                        apart = abs(Y[2] - d)
                        if apart == lim:
                            k["depth_tie"] += 1
                        if not (apart < lim if variant == "lt_for_le" else apart <= lim):
                            k["depth_fail"] += 1
                            continue
                        k["consistent"] += 1
                        cnt += 1
                        s = s + Y[2]
                    k["cnt_just_below"] += cnt == min_consistent - 1
                    k["cnt_at_min"] += cnt == min_consistent
                    keep = cnt >= min_consistent
                    if keep or variant != "count_after_threshold":
                        count_out[j, y0, x0] = np.float32(cnt)
                    if not keep:
                        continue
                    n_kept += 1
                    if not refine:
                        depth_out[j, y0, x0] = depth[j, y0, x0]
                    elif variant == "mean_without_centre":
                        depth_out[j, y0, x0] = np.float32(s / F(cnt))
                    else:
                        depth_out[j, y0, x0] = np.float32(s / F(cnt + 1))
    return depth_out, count_out, (n_valid, n_kept), k


# ------------------------------------------------------------------------------------------------- the twin ---
def _reproject_np(Ki, A, B, x, y, d):
    RA, tA = A
    RB, tB = B
    Q = []
    for c in range(3):
        r = (Ki[c, 0] * x + Ki[c, 1] * y) + Ki[c, 2]
        P = r * d
        Q.append(P - tA[c])
    Xw = [(RA[0, c] * Q[0] + RA[1, c] * Q[1]) + RA[2, c] * Q[2] for c in range(3)]
    return [((RB[c, 0] * Xw[0] + RB[c, 1] * Xw[1]) + RB[c, 2] * Xw[2]) + tB[c] for c in range(3)]


def _project_np(K, X):
    return [(K[c, 0] * X[0] + K[c, 1] * X[1]) + K[c, 2] * X[2] for c in range(3)]


def _causes_np(d32, c32, mc32):
    """(valid, nonpositive, nonfinite, conf_low) masks of float32 maps, each invalid pixel under its first cause."""
    pos = d32 > np.float32(0)
    fin = d32 <= np.float32(FLT_MAX)
    ok = c32 >= mc32
    return pos & fin & ok, ~pos, pos & ~fin, pos & fin & ~ok


def depth_filter_np(depth, conf, K, K_inv, poses, neighbours, min_confidence, max_px, max_rel, min_consistent, refine,
                    variant=None):
    _check(variant)
    T = np.float32 if variant == "float32" else np.float64
    depth = np.ascontiguousarray(depth, np.float32)
    conf = np.ascontiguousarray(conf, np.float32)
    n, H, W = depth.shape
    mc = np.float32(min_confidence)
    Kf, Ki = np.asarray(K, np.float64).reshape(3, 3).astype(T), np.asarray(K_inv, np.float64).reshape(3, 3).astype(T)
    P = [(np.asarray(R, np.float64).reshape(3, 3).astype(T), np.asarray(t, np.float64).reshape(3).astype(T)) for R, t in poses]
    px_bound = T(np.float32(max_px)) * T(np.float32(max_px))
    rel = T(np.float32(max_rel))
    half, zero = T(0.5), T(0.0)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x, y = xs.astype(T), ys.astype(T)
    rows = neighbour_rows(n, neighbours)
    depth_out = np.zeros((n, H, W), np.float32)
    count_out = np.zeros((n, H, W), np.float32)
    k = dict.fromkeys(COUNTERS, 0)
    n_valid = n_kept = 0
    flat_d, flat_c = depth.reshape(n, -1), conf.reshape(n, -1)

    def tally(name, mask):
        k[name] += int(mask.sum())

    with np.errstate(all="ignore"):
        for j in range(n):
            valid, c0, c1, c2 = _causes_np(depth[j], conf[j], mc)
            tally("centre_depth_nonpositive", c0)
            tally("centre_depth_nonfinite", c1)
            tally("centre_conf_low", c2)
            n_valid += int(valid.sum())
            d = depth[j].astype(T)
            lim = rel * d
            cnt = np.zeros((H, W), np.int64)
            s = np.zeros((H, W), T) if variant == "mean_without_centre" else d.copy()
            row = rows[j][::-1] if variant == "reverse_order" else rows[j]
            for i in row:
                if i < 0:
                    continue
                m = valid
                Xi = _reproject_np(Ki, P[j], P[i], x, y, d)
                g = Xi[2] > zero
                tally("Xi_behind", m & ~g)
                m = m & g
                uvw = _project_np(Kf, Xi)
                g = uvw[2] > zero
                tally("uvw_behind", m & ~g)
                m = m & g
                u, v = uvw[0] / uvw[2], uvw[1] / uvw[2]
                if variant == "truncate":
                    px, py = np.trunc(u), np.trunc(v)
                else:
                    px, py = np.floor(u + half), np.floor(v + half)
                for name, g in (("outside_left", px >= zero), ("outside_right", px < T(W)), ("outside_top", py >= zero),
                                ("outside_bottom", py < T(H))):
                    tally(name, m & ~g)
                    m = m & g
                at = np.where(m, py, zero).astype(np.int64) * W + np.where(m, px, zero).astype(np.int64)
                di32, ci32 = flat_d[i][at], flat_c[i][at]
                ok, c0, c1, c2 = _causes_np(di32, ci32, mc)
                tally("nbr_depth_nonpositive", m & c0)
                tally("nbr_depth_nonfinite", m & c1)
                tally("nbr_conf_low", m & c2)
                m = m & ok
                di = di32.astype(T)
                Y = _reproject_np(Ki, P[i], P[j], u, v, di) if variant == "backproject_uv" else _reproject_np(Ki, P[i], P[j], px, py, di)
                g = Y[2] > zero
                tally("Y_behind", m & ~g)
                m = m & g
                uvw = _project_np(Kf, Y)
                g = uvw[2] > zero
                tally("back_uvw_behind", m & ~g)
                m = m & g
                eu, ev = uvw[0] / uvw[2] - x, uvw[1] / uvw[2] - y
                e2 = eu * eu + ev * ev
                tally("e2_tie", m & (e2 == px_bound))
                g = e2 < px_bound if variant == "lt_for_le" else e2 <= px_bound
                tally("e2_fail", m & ~g)
                m = m & g
                apart = np.abs(Y[2] - d)
                tally("depth_tie", m & (apart == lim))
                g = apart < lim if variant == "lt_for_le" else apart <= lim
                tally("depth_fail", m & ~g)
                m = m & g
                tally("consistent", m)
                cnt = cnt + m
                s = np.where(m, s + Y[2], s)
            tally("cnt_just_below", valid & (cnt == min_consistent - 1))
            tally("cnt_at_min", valid & (cnt == min_consistent))
            keep = valid & (cnt >= min_consistent)
            n_kept += int(keep.sum())
            stored = keep if variant == "count_after_threshold" else valid
            count_out[j] = np.where(stored, cnt, 0).astype(np.float32)
            if not refine:
                fused = depth[j]
            elif variant == "mean_without_centre":
                fused = (s / np.maximum(cnt, 1).astype(T)).astype(np.float32)
            else:
                fused = (s / (cnt + 1).astype(T)).astype(np.float32)
            depth_out[j] = np.where(keep, fused, np.float32(0))
    return depth_out, count_out, (n_valid, n_kept), k
