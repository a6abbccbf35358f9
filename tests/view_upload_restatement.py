"""An independent restatement of the view-upload stage (a helper module, not a conftest; no GPU, and no import of
core/imageprep.py): what amvs_set_view_bgr8 has to leave on the device, written from the definitions in the header of
csrc/amvs_prep.hip and from OpenCV's documented 8-bit algorithm, one pixel at a time.

  resize   cv.resize(img, (W, H)), INTER_LINEAR, 8-bit, 3 channels (imgproc/resize.cpp: the table set-up of resize_,
           HResizeLinear, VResizeLinear<uchar>).  Per destination index d of an axis:
               f = (float)((d + 0.5) * scale - 0.5),  scale = 1.0 / ((double)n_dst / n_src)
               s = floor(f);  f -= s                                                      (float32)
               columns only:  s < 0 -> s = 0, f = 0;  s >= n_src - 1 -> s = n_src - 1, f = 0
               w0 = cvRound((1.f - f) * 2048),  w1 = cvRound(f * 2048)                    (float32, half to even)
           rows keep their weights and have the two row indices s, s + 1 clamped into the image instead.
               horizontal   D = S[x0] * a0 + S[x1] * a1
               vertical     dst = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2
           A destination of the source's size is a copy.
  gray     cv.cvtColor(BGR2GRAY), 8-bit: (B * 3735 + G * 19235 + R * 9798 + 16384) >> 15
  float    gray.astype(np.float32) / 255.0
  pack     code = rint(g * 255) clamped to [0, 255] (NaN -> 0); a view is lossless iff every pixel equals
           float32(code) / float32(255)

The coordinate and weight arithmetic uses np.float32 scalars, the fixed-point passes Python integers.  `resize` also
counts the edges a test family has to reach (COUNTERS).  `resize_np` is the same restatement vectorised, for the one
shape too large for the loops; tests/test_view_upload_cpu.py holds it to the loops.  `bilinear64` is the mathematics the
fixed-point chain approximates, and `bilinear_bounds` how far the chain may stray from it.

`variant=` restates a near miss of the kernel instead (VARIANTS), with `poison` standing for whatever a tap outside the
staging buffer would read; the CPU test shows that the family tells each of them from the definition.
"""
import math

import numpy as np

F32 = np.float32
COEF_BITS = 11
COEF_ONE = 1 << COEF_BITS                    # 2048
ACC_MAX = 255 * COEF_ONE
GRAY_B, GRAY_G, GRAY_R, GRAY_HALF, GRAY_SHIFT = 3735, 19235, 9798, 16384, 15

COUNTERS = ("row_ofs_minus1", "row_clamp_bottom", "col_clamp_first", "col_clamp_last", "weights_not_2048", "acc_max")
VARIANTS = ("sy0_unclamped", "cols_unclamped", "bgr_swapped", "shift_after_multiply")


def _round_half_even(x):
    """cvRound of a float32 that is known to be finite: Python's round() is round-half-to-even on the exact value."""
    return int(round(float(x)))


def axis_table(n_dst, n_src, columns):
    """[(s, w0, w1, clamped)] of one axis.  `clamped` is -1 / +1 where the column rule moved the tap and zeroed a
    non-zero fraction (0 elsewhere, and always 0 for rows)."""
    scale = 1.0 / (float(n_dst) / float(n_src))
    table = []
    for d in range(n_dst):
        f = F32((d + 0.5) * scale - 0.5)
        s = int(math.floor(float(f)))
        f = F32(f - F32(s))
        clamped = 0
        if columns:
            if s < 0:
                clamped = -1
                s, f = 0, F32(0.0)
            if s >= n_src - 1:
                if f != 0 or s > n_src - 1:
                    clamped = 1
                s, f = n_src - 1, F32(0.0)
        w0 = _round_half_even(F32(F32(1.0) - f) * F32(2048.0))
        w1 = _round_half_even(f * F32(2048.0))
        table.append((s, w0, w1, clamped))
    return table


def _raw_column_table(n_dst, n_src):
    """The column table without the clamp rule (the near miss cols_unclamped)."""
    return [(s, w0, w1, 0) for s, w0, w1, _ in axis_table(n_dst, n_src, False)]


def resize(src, H, W, variant=None, poison=0):
    """-> (dst (H, W, 3) uint8, counters).  src (h, w, 3) uint8."""
    if variant is not None and variant not in VARIANTS:
        raise ValueError(f"unknown variant {variant!r}")
    h, w = src.shape[:2]
    counters = dict.fromkeys(COUNTERS, 0)
    if (h, w) == (H, W):
        return src.copy(), counters
    cols = _raw_column_table(W, w) if variant == "cols_unclamped" else axis_table(W, w, True)
    rows = axis_table(H, h, False)
    px = src.tolist()

    def tap(y, x, c):
        return px[y][x][c] if 0 <= y < h and 0 <= x < w else poison

    for s, w0, w1, clamped in cols:
        counters["col_clamp_first"] += clamped < 0
        counters["col_clamp_last"] += clamped > 0
        counters["weights_not_2048"] += w0 + w1 != COEF_ONE
    dst = np.zeros((H, W, 3), np.uint8)
    for dy, (sy, b0, b1, _) in enumerate(rows):
        counters["weights_not_2048"] += b0 + b1 != COEF_ONE
        counters["row_ofs_minus1"] += sy == -1 and b0 > 0
        counters["row_clamp_bottom"] += sy + 1 > h - 1 and b1 > 0
        y0 = sy if variant == "sy0_unclamped" else min(max(sy, 0), h - 1)
        y1 = min(max(sy + 1, 0), h - 1)
        for dx, (sx, a0, a1, _) in enumerate(cols):
            x0, x1 = sx, min(sx + 1, w - 1)
            for c in range(3):
                d0 = tap(y0, x0, c) * a0 + tap(y0, x1, c) * a1
                d1 = tap(y1, x0, c) * a0 + tap(y1, x1, c) * a1
                counters["acc_max"] += (d0 == ACC_MAX) + (d1 == ACC_MAX)
                if variant == "shift_after_multiply":
                    v = ((((b0 * d0) >> 4) >> 16) + (((b1 * d1) >> 4) >> 16) + 2) >> 2
                else:
                    v = (((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2
                dst[dy, dx, c] = v & 0xFF                            # the kernel's (unsigned char) cast
    return dst, counters


def gray_codes(bgr, variant=None):
    """(H, W) uint8 gray codes of an (H, W, 3) uint8 BGR image."""
    H, W = bgr.shape[:2]
    out = np.zeros((H, W), np.uint8)
    kb, kr = (GRAY_R, GRAY_B) if variant == "bgr_swapped" else (GRAY_B, GRAY_R)
    px = bgr.tolist()
    for y in range(H):
        for x in range(W):
            b, g, r = px[y][x]
            out[y, x] = (b * kb + g * GRAY_G + r * kr + GRAY_HALF) >> GRAY_SHIFT
    return out


def gray_float(codes):
    """codes.astype(np.float32) / 255.0, one float32 division per pixel."""
    H, W = codes.shape
    out = np.zeros((H, W), F32)
    for y in range(H):
        for x in range(W):
            out[y, x] = F32(int(codes[y, x])) / F32(255.0)
    return out


def prepare(src, H, W, variant=None, poison=0):
    """What amvs_set_view_bgr8 leaves for a source image: {'color', 'codes', 'gray', 'counters'}."""
    color, counters = resize(src, H, W, variant, poison)
    codes = gray_codes(color, variant)
    return {"color": color, "codes": codes, "gray": gray_float(codes), "counters": counters}


# ------------------------------------------------------------------------------ the vectorised form (large shape) ---
def _axis_arrays(n_dst, n_src, columns):
    t = axis_table(n_dst, n_src, columns)                  # the tables are the loops' own: one entry per row / column
    return (np.array([e[0] for e in t], np.int64), np.array([e[1] for e in t], np.int64),
            np.array([e[2] for e in t], np.int64))


def resize_np(src, H, W):
    h, w = src.shape[:2]
    if (h, w) == (H, W):
        return src.copy()
    x0, a0, a1 = _axis_arrays(W, w, True)
    y0, b0, b1 = _axis_arrays(H, h, False)
    x1 = np.minimum(x0 + 1, w - 1)
    r0, r1 = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    s = src.astype(np.int64)
    out = np.zeros((H, W, 3), np.uint8)
    for lo in range(0, H, 64):                             # in bands of rows: a few MB of int64 at a time
        hi = min(lo + 64, H)
        top, bot = s[r0[lo:hi]], s[r1[lo:hi]]
        d0 = top[:, x0] * a0[None, :, None] + top[:, x1] * a1[None, :, None]
        d1 = bot[:, x0] * a0[None, :, None] + bot[:, x1] * a1[None, :, None]
        p0 = (b0[lo:hi, None, None] * (d0 >> 4)) >> 16
        p1 = (b1[lo:hi, None, None] * (d1 >> 4)) >> 16
        out[lo:hi] = ((p0 + p1 + 2) >> 2) & 0xFF
    return out


def gray_codes_np(bgr):
    b = bgr.astype(np.int64)
    return ((b[:, :, 0] * GRAY_B + b[:, :, 1] * GRAY_G + b[:, :, 2] * GRAY_R + GRAY_HALF) >> GRAY_SHIFT).astype(np.uint8)


def prepare_np(src, H, W):
    color = resize_np(src, H, W)
    codes = gray_codes_np(color)
    return {"color": color, "codes": codes, "gray": codes.astype(F32) / F32(255.0)}


class PixelRestater:
    """resize + gray of single destination pixels with the loop form's scalar arithmetic (tables built once)."""

    def __init__(self, src, H, W):
        self.src, self.H, self.W = src, H, W
        self.h, self.w = src.shape[:2]
        self.copy = (self.h, self.w) == (H, W)
        if not self.copy:
            self.cols = axis_table(W, self.w, True)
            self.rows = axis_table(H, self.h, False)

    def color(self, dy, dx):
        if self.copy:
            return [int(v) for v in self.src[dy, dx]]
        sx, a0, a1, _ = self.cols[dx]
        sy, b0, b1, _ = self.rows[dy]
        y0, y1 = min(max(sy, 0), self.h - 1), min(max(sy + 1, 0), self.h - 1)
        x0, x1 = sx, min(sx + 1, self.w - 1)
        out = []
        for c in range(3):
            d0 = int(self.src[y0, x0, c]) * a0 + int(self.src[y0, x1, c]) * a1
            d1 = int(self.src[y1, x0, c]) * a0 + int(self.src[y1, x1, c]) * a1
            out.append(((((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2) & 0xFF)
        return out

    def code(self, dy, dx):
        b, g, r = self.color(dy, dx)
        return (b * GRAY_B + g * GRAY_G + r * GRAY_R + GRAY_HALF) >> GRAY_SHIFT


# ------------------------------------------------------------------------------------- the mathematics behind it ---
def bilinear64(src, H, W):
    """True bilinear interpolation in float64: the half-pixel centre mapping x = (dx + 0.5) * w / W - 0.5, the two taps
    floor(x) and floor(x) + 1 clamped into the image, no fixed point and no rounding.  -> (H, W, 3) float64."""
    h, w = src.shape[:2]
    s = src.astype(np.float64)
    out = np.zeros((H, W, 3), np.float64)
    for dy in range(H):
        fy = (dy + 0.5) * h / H - 0.5
        y0 = math.floor(fy)
        ty = fy - y0
        ya, yb = min(max(y0, 0), h - 1), min(max(y0 + 1, 0), h - 1)
        for dx in range(W):
            fx = (dx + 0.5) * w / W - 0.5
            x0 = math.floor(fx)
            tx = fx - x0
            xa, xb = min(max(x0, 0), w - 1), min(max(x0 + 1, 0), w - 1)
            top = s[ya, xa] * (1.0 - tx) + s[ya, xb] * tx
            bot = s[yb, xa] * (1.0 - tx) + s[yb, xb] * tx
            out[dy, dx] = top * (1.0 - ty) + bot * ty
    return out


def bilinear_bounds(h, w):
    """(lowest, highest) value of fixed-point result minus float64 bilinear value, in gray codes, for a source of h x w;
    derived in the docstring of tests/test_view_upload_cpu.py::test_fixed_point_stays_within_the_derived_bound."""
    eps_x = float(np.spacing(F32(w))) / 2                  # float32 rounding of a coordinate below w
    eps_y = float(np.spacing(F32(h))) / 2
    coord = 255.0 * (eps_x + eps_y)
    e_axis = 255.0 * (2.0 ** -11 + 2.0 ** -25)            # two weights, each half a unit of 1/2048 off; 1.f - f rounds
    wsum = 2049.0 / 2048.0
    weights = e_axis * wsum + e_axis
    shift4 = wsum * 15.0 / 2048.0
    slack = 1e-9                                           # the float64 arithmetic of both sides
    return -(0.5 + 0.5 + shift4 + weights + coord + slack), 0.5 + weights + coord + slack


# ------------------------------------------------------------------------------------------------------ the pack ---
def pack(gray):
    """-> (codes (H, W) uint8, lossless bool) of one float32 gray image."""
    g = np.asarray(gray)
    assert g.dtype == np.float32
    H, W = g.shape
    codes = np.zeros((H, W), np.uint8)
    lossless = True
    for y in range(H):
        for x in range(W):
            v = g[y, x]
            if np.isnan(v):
                code = 0                                   # rint(NaN) converts to 0 on the device; NaN equals nothing
            else:
                with np.errstate(over="ignore"):
                    p = np.rint(v * F32(255.0))            # float32 product, round half to even; +-inf stay
                code = 0 if p <= 0 else 255 if p >= 255 else int(p)
            codes[y, x] = code
            if not (F32(code) / F32(255.0) == v):
                lossless = False
    return codes, lossless


def pack_views(grays):
    """[lossless] per view; the context samples the packed maps iff all() of the uploaded views."""
    return [pack(g)[1] for g in grays]
