"""The lens undistortion restated from the text of include/amvs_lens.h alone (a helper module, not a conftest; no GPU, no
library): undistort() in plain Python loops over Python floats (IEEE float64, one rounding per operation, nothing
contracted) with Python ints for the integer part, and undistort_np(), a NumPy twin with whole images as operands
(elementwise float64 only) for the large case.  tests/test_undistort_cpu.py holds the two to each other byte for byte;
tests/test_hip_undistort.py holds csrc/amvs_undistort.hip to them.

Both return (image (h, w, 3) uint8, n_outside, counters); counters = {"partial": inside pixels with at least one tap
outside the image, "fractional": inside pixels with a non-zero fraction on either axis}.
"""
import math

import numpy as np


def lens(K, dist):
    """(fx, fy, cx, cy), (k1, k2, p1, p2, k3, k4, k5, k6) as Python floats: the entries the header reads, absent ones 0."""
    K = np.asarray(K, np.float64).reshape(9)
    d = [float(v) for v in np.asarray(dist, np.float64).reshape(-1)]
    assert len(d) in (4, 5, 8)
    d += [0.0] * (8 - len(d))
    return (float(K[0]), float(K[4]), float(K[2]), float(K[5])), tuple(d)


def _div(a, b):
    """IEEE float64 division (Python raises on a zero divisor)."""
    if b != 0.0 or math.isnan(a) or math.isnan(b):
        return a / b
    if a == 0.0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _rint(v):
    """Round to nearest, halves to even; NaN and the infinities stay."""
    return float(round(v)) if math.isfinite(v) else v


def source_coordinates(j, i, cam, d):
    """(fu, fv) of the destination pixel at column j and row i: the header's map, operation by operation."""
    fx, fy, cx, cy = cam
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    x = _div(float(j) - cx, fx)
    y = _div(float(i) - cy, fy)
    x2 = x * x
    y2 = y * y
    r2 = x2 + y2
    xy2 = (2.0 * x) * y
    num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2
    kr = _div(num, den)
    xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2)
    yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2
    u = fx * xd + cx
    v = fy * yd + cy
    return _rint(u * 32.0), _rint(v * 32.0)


def undistort(src, K, dist):
    src = np.ascontiguousarray(src, np.uint8)
    h, w = src.shape[:2]
    cam, d = lens(K, dist)
    rows = src.tolist()
    out = np.zeros((h, w, 3), np.uint8)
    n_outside = partial = fractional = 0
    for i in range(h):
        for j in range(w):
            fu, fv = source_coordinates(j, i, cam, d)
            if not (-32.0 <= fu < 32.0 * w and -32.0 <= fv < 32.0 * h):       # (NaN fails every comparison)
                n_outside += 1
                continue
            iu, iv = int(fu), int(fv)
            sx, ax = iu >> 5, iu & 31                                         # (Python's >> floors)
            sy, ay = iv >> 5, iv & 31
            taps = (((sx, sy), (32 - ax) * (32 - ay)), ((sx + 1, sy), ax * (32 - ay)),
                    ((sx, sy + 1), (32 - ax) * ay), ((sx + 1, sy + 1), ax * ay))
            assert sum(wt for _, wt in taps) == 1024
            acc = [512, 512, 512]
            inside = 0
            for (tx, ty), wt in taps:
                if 0 <= tx < w and 0 <= ty < h:
                    inside += 1
                    px = rows[ty][tx]
                    for c in range(3):
                        acc[c] += wt * px[c]
            partial += inside < 4
            fractional += (ax != 0) or (ay != 0)
            out[i, j] = [a >> 10 for a in acc]
    return out, n_outside, {"partial": partial, "fractional": fractional}


def source_coordinates_np(h, w, cam, d):
    """The map for every pixel at once: (fu, fv), each (h, w) float64."""
    fx, fy, cx, cy = (np.float64(v) for v in cam)
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(v) for v in d)
    two, one = np.float64(2.0), np.float64(1.0)
    with np.errstate(all="ignore"):
        x = np.broadcast_to(((np.arange(w, dtype=np.float64) - cx) / fx)[None, :], (h, w))
        y = np.broadcast_to(((np.arange(h, dtype=np.float64) - cy) / fy)[:, None], (h, w))
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        xy2 = (two * x) * y
        num = one + ((k3 * r2 + k2) * r2 + k1) * r2
        den = one + ((k6 * r2 + k5) * r2 + k4) * r2
        kr = num / den
        xd = (x * kr + p1 * xy2) + p2 * (r2 + two * x2)
        yd = (y * kr + p1 * (r2 + two * y2)) + p2 * xy2
        u = fx * xd + cx
        v = fy * yd + cy
        return np.rint(u * np.float64(32.0)), np.rint(v * np.float64(32.0))


def undistort_np(src, K, dist):
    src = np.ascontiguousarray(src, np.uint8)
    h, w = src.shape[:2]
    cam, d = lens(K, dist)
    fu, fv = source_coordinates_np(h, w, cam, d)
    with np.errstate(invalid="ignore"):
        inside = (fu >= -32.0) & (fu < 32.0 * w) & (fv >= -32.0) & (fv < 32.0 * h)
    iu = np.where(inside, fu, 0.0).astype(np.int64)
    iv = np.where(inside, fv, 0.0).astype(np.int64)
    sx, ax = iu >> 5, iu & 31
    sy, ay = iv >> 5, iv & 31
    acc = np.full((h, w, 3), 512, np.int64)
    taps_inside = np.zeros((h, w), np.int64)
    wide = src.astype(np.int64)
    for tx, ty, wt in ((sx, sy, (32 - ax) * (32 - ay)), (sx + 1, sy, ax * (32 - ay)),
                       (sx, sy + 1, (32 - ax) * ay), (sx + 1, sy + 1, ax * ay)):
        ok = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
        px = wide[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)]               # (a tap that is not ok is never used)
        acc += np.where(ok, wt, 0)[..., None] * px
        taps_inside += ok
    out = np.where(inside[..., None], acc >> 10, 0).astype(np.uint8)
    counters = {"partial": int((inside & (taps_inside < 4)).sum()), "fractional": int((inside & ((ax != 0) | (ay != 0))).sum())}
    return out, int((~inside).sum()), counters
