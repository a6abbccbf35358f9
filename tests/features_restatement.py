"""CLAHE and the SIFT scale space, restated in NumPy from the text of include/amvs_features.h alone (not from the
kernels): the yardstick tests/test_hip_features.py holds the device to, bit for bit.

float32 stages are float32 arrays and np.float32 scalars, one NumPy operation per written operation, so every operation
rounds once and nothing is fused; the host's float64 stages (sigmas, taps, exp64) are Python floats, which are float64.
"""
import math

import numpy as np

F = np.float32
LAYERS, GAUSS, DOG = 3, 6, 5
K3 = 1.2599210498948732


def fold(i, n):
    """reflect-101 folded as often as needed; i an integer array (or integer), n >= 1."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)                       # into 0 .. p - 1 (NumPy's mod of a positive p is never negative)
    return np.where(m < n, m, p - m)


# ------------------------------------------------------------------------------------------------------ CLAHE ---
def clahe_limit(clip_limit, area):
    """The integer limit of a bin, or 0 when the clipping is off."""
    clip = F(clip_limit)
    if clip == F(0):
        return 0
    t = (clip * F(area)) / F(256)
    if t >= F(area):
        return 0
    return max(1, int(t))


def clahe_luts(gray, clip_limit, grid_x, grid_y):
    """(lut [grid_y][grid_x][256] uint8, tw, th, counters) -- steps 1 to 5."""
    h, w = gray.shape
    wp, hp = -(-w // grid_x) * grid_x, -(-h // grid_y) * grid_y
    padded = gray[fold(np.arange(hp), h)[:, None], fold(np.arange(wp), w)[None, :]]
    tw, th = wp // grid_x, hp // grid_y
    area = tw * th
    limit = clahe_limit(clip_limit, area)
    scale = F(255) / F(area)
    lut = np.empty((grid_y, grid_x, 256), np.uint8)
    counters = {"clipped_tiles": 0, "residual_tiles": 0, "unclipped_tiles": 0}
    for ty in range(grid_y):
        for tx in range(grid_x):
            tile = padded[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
            hist = np.bincount(tile.reshape(-1), minlength=256).astype(np.int64)
            if limit > 0:
                excess = int(np.maximum(hist - limit, 0).sum())
                hist = np.minimum(hist, limit)
                batch = excess // 256
                residual = excess - 256 * batch
                hist = hist + batch
                if residual > 0:
                    step = max(256 // residual, 1)
                    for k in range(residual):
                        hist[k * step] += 1
                    counters["residual_tiles"] += 1
                counters["clipped_tiles" if excess else "unclipped_tiles"] += 1
            c = np.cumsum(hist)
            lut[ty, tx] = np.minimum(255, np.rint(c.astype(F) * scale).astype(np.int64)).astype(np.uint8)
    return lut, tw, th, counters


def clahe(gray, clip_limit=2.0, grid_x=8, grid_y=8, want_counters=False):
    gray = np.ascontiguousarray(gray, np.uint8)
    h, w = gray.shape
    lut, tw, th, counters = clahe_luts(gray, clip_limit, grid_x, grid_y)
    half, one = F(0.5), F(1)
    fy = np.arange(h).astype(F) * (one / F(th)) - half
    fx = np.arange(w).astype(F) * (one / F(tw)) - half
    y1f, x1f = np.floor(fy), np.floor(fx)
    ya, xa = (fy - y1f)[:, None], (fx - x1f)[None, :]
    ya1, xa1 = one - ya, one - xa
    y1, x1 = y1f.astype(np.int64), x1f.astype(np.int64)
    y2, x2 = np.minimum(y1 + 1, grid_y - 1)[:, None], np.minimum(x1 + 1, grid_x - 1)[None, :]
    y1, x1 = np.maximum(y1, 0)[:, None], np.maximum(x1, 0)[None, :]
    v = gray.astype(np.int64)
    l11, l12 = lut[y1, x1, v].astype(F), lut[y1, x2, v].astype(F)
    l21, l22 = lut[y2, x1, v].astype(F), lut[y2, x2, v].astype(F)
    r = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya
    assert r.dtype == F
    out = np.clip(np.rint(r).astype(np.int64), 0, 255).astype(np.uint8)
    return (out, counters) if want_counters else out


# ------------------------------------------------------------------------------------------------ scale space ---
def octaves(h, w):
    m = min(h, w)
    L = (m * m).bit_length() - 1
    return (L - 3) // 2 + 1


def sigmas(sigma):
    """[s_base, s_1 .. s_5] in float64."""
    s = [math.sqrt(max(sigma * sigma - 1.0, 0.01))]
    prev = float(sigma)
    for _ in range(1, 6):
        total = prev * K3
        s.append(math.sqrt(total * total - prev * prev))
        prev = total
    return s


def exp64(x):
    n = float(np.rint(x * 1.4426950408889634))
    t = (x - n * 0.693147180369123816490) - n * 1.90821492927058770002e-10
    fact = [1.0]
    for k in range(1, 14):
        fact.append(fact[-1] * float(k))
    q = 1.0 / fact[13]
    for k in range(12, -1, -1):
        q = q * t + 1.0 / fact[k]
    return math.ldexp(q, int(n))


def taps(s):
    """float32 taps [2 r + 1] of a blur of sigma s."""
    n_taps = int(np.rint(8.0 * s + 1.0)) | 1
    r = n_taps // 2
    d = 2.0 * s * s
    e = [exp64(-(float((j - r) * (j - r))) / d) for j in range(2 * r + 1)]
    total = e[0]
    for j in range(1, 2 * r + 1):
        total = total + e[j]
    return np.array([e[j] / total for j in range(2 * r + 1)], np.float64).astype(F)


def upsample(gray):
    g = np.ascontiguousarray(gray, np.uint8).astype(F)
    h, w = g.shape

    def near_far(n):
        d = np.arange(2 * n)
        k = d // 2
        return k, np.where(d % 2 == 0, np.maximum(k - 1, 0), np.minimum(k + 1, n - 1))

    ny, fy = near_far(h)
    nx, fx = near_far(w)
    a, b = F(0.75), F(0.25)
    row = a * g[:, nx] + b * g[:, fx]                    # row(yy, x) for every source row yy
    return a * row[ny, :] + b * row[fy, :]


def blur(img, tap):
    """Two passes, each pixel one serial float32 sum in tap order."""
    assert img.dtype == F and tap.dtype == F
    h, w = img.shape
    r = (len(tap) - 1) // 2
    xs, ys = np.arange(w), np.arange(h)
    acc = tap[0] * img[:, fold(xs - r, w)]
    for j in range(1, 2 * r + 1):
        acc = acc + tap[j] * img[:, fold(xs - r + j, w)]
    t = acc
    acc = tap[0] * t[fold(ys - r, h), :]
    for j in range(1, 2 * r + 1):
        acc = acc + tap[j] * t[fold(ys - r + j, h), :]
    assert acc.dtype == F
    return acc


def scale_space(gray, sigma=1.6):
    """(gauss, dog): gauss[o] a list of 6 float32 images, dog[o] of 5."""
    h, w = gray.shape
    tp = [taps(s) for s in sigmas(sigma)]
    gauss, dog = [], []
    for o in range(octaves(h, w)):
        g = [blur(upsample(gray), tp[0])] if o == 0 else [np.ascontiguousarray(gauss[o - 1][LAYERS][::2, ::2][:gauss[o - 1][0].shape[0] // 2,
                                                                                                          :gauss[o - 1][0].shape[1] // 2])]
        for i in range(1, GAUSS):
            g.append(blur(g[i - 1], tp[i]))
        gauss.append(g)
        dog.append([g[i + 1] - g[i] for i in range(DOG)])
    return gauss, dog


# ------------------------------------------------------------------------- the float32 functions of the header ---
LN2_HI, LN2_LO, LOG2E = F(0.693359375), F(-2.12194440e-4), F(1.44269504)
EXP_COEF = [F(1) / F(k) for k in (720, 120, 24, 6, 2, 1, 1)]            # 1/6! .. 1/0!
ATAN_COEF = [F(-0.01172120), F(0.05265332), F(-0.11643287), F(0.19354346), F(-0.33262347), F(0.99997726)]
SIN_COEF = [F(-1) / F(39916800), F(1) / F(362880), F(-1) / F(5040), F(1) / F(120), F(-1) / F(6), F(1)]
DEG, RAD, HALF_PI = F(57.29578), F(0.017453292), F(1.5707964)
FIX = F(1048576.0)                                                       # 2^20, the histograms' fixed point
EPS = F(1.1920929e-07)


def expf(x):
    """exp of a float32 array, -80 <= x <= 80; 0 below -80."""
    x = np.asarray(x, F)
    n = np.rint(x * LOG2E)
    t = (x - n * LN2_HI) - n * LN2_LO
    q = EXP_COEF[0]
    for c in EXP_COEF[1:]:
        q = q * t + c
    out = np.ldexp(q, n.astype(np.int32)).astype(F)
    return np.where(x < F(-80), F(0), out).astype(F)


def atan2deg(y, x):
    """The angle of (x, y) in degrees, 0 .. 360, float32 arrays."""
    y, x = np.asarray(y, F), np.asarray(x, F)
    ax, ay = np.abs(x), np.abs(y)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    a = mn / np.where(mx == 0, F(1), mx)
    s = a * a
    p = ATAN_COEF[0]
    for c in ATAN_COEF[1:]:
        p = p * s + c
    r = (p * a) * DEG
    r = np.where(ay > ax, F(90) - r, r)
    r = np.where(x < 0, F(180) - r, r)
    r = np.where(y < 0, F(360) - r, r)
    return np.where(mx == 0, F(0), r).astype(F)


def _sinp(t):
    s = t * t
    p = SIN_COEF[0]
    for c in SIN_COEF[1:]:
        p = p * s + c
    return p * t


def sincosdeg(a):
    """(sin, cos) of a float32 angle in degrees, 0 <= a < 360."""
    a = F(a)
    q = min(int(a * (F(1) / F(90))), 3)
    rr = (a - F(90) * F(q)) * RAD
    s, c = _sinp(rr), _sinp(HALF_PI - rr)
    return [(s, c), (c, -s), (-s, -c), (-c, s)][q]


# ------------------------------------------------------------------------------------------------- keypoints ---
BORDER, MAX_STEPS, ORI_BINS = 5, 5, 36


def pre_threshold(contrast_threshold):
    return F(math.floor(0.5 * float(F(contrast_threshold)) / 3.0 * 255.0))


def candidates(dog_octave, pre):
    """[(i, r, c)] of one octave's 26-neighbour extrema, in (i, r, c) order."""
    out = []
    h, w = dog_octave[0].shape
    if h <= 2 * BORDER or w <= 2 * BORDER:
        return out
    for i in range(1, LAYERS + 1):
        v = dog_octave[i][BORDER:h - BORDER, BORDER:w - BORDER]
        ge, le = np.ones(v.shape, bool), np.ones(v.shape, bool)
        for l in (i - 1, i, i + 1):
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    nb = dog_octave[l][BORDER + dr:h - BORDER + dr, BORDER + dc:w - BORDER + dc]
                    ge &= v >= nb
                    le &= v <= nb
        hit = ((v > pre) & ge) | ((v < -pre) & le)
        out += [(i, int(r) + BORDER, int(c) + BORDER) for r, c in np.argwhere(hit)]
    return out


def refine(dog_octave, o, cand, contrast_threshold, edge_threshold, sigma):
    """None, or the refined keypoint of a candidate: a dict."""
    i, r, c = cand
    h, w = dog_octave[0].shape
    ct, edge, one = F(contrast_threshold), F(edge_threshold), F(1)
    img_scale = one / F(255)
    deriv, second, cross = img_scale * F(0.5), img_scale, img_scale * F(0.25)
    converged = False
    for _ in range(MAX_STEPS):
        p, q, n = dog_octave[i - 1], dog_octave[i], dog_octave[i + 1]
        gx = (q[r, c + 1] - q[r, c - 1]) * deriv
        gy = (q[r + 1, c] - q[r - 1, c]) * deriv
        gs = (n[r, c] - p[r, c]) * deriv
        v2 = q[r, c] * F(2)
        dxx = (q[r, c + 1] + q[r, c - 1] - v2) * second
        dyy = (q[r + 1, c] + q[r - 1, c] - v2) * second
        dss = (n[r, c] + p[r, c] - v2) * second
        dxy = (q[r + 1, c + 1] - q[r + 1, c - 1] - q[r - 1, c + 1] + q[r - 1, c - 1]) * cross
        dxs = (n[r, c + 1] - n[r, c - 1] - p[r, c + 1] + p[r, c - 1]) * cross
        dys = (n[r + 1, c] - n[r - 1, c] - p[r + 1, c] + p[r - 1, c]) * cross
        c00 = dyy * dss - dys * dys
        c01 = dxs * dys - dxy * dss
        c02 = dxy * dys - dxs * dyy
        det = dxx * c00 + dxy * c01 + dxs * c02
        if det == 0:
            return None
        c11 = dxx * dss - dxs * dxs
        c12 = dxy * dxs - dxx * dys
        c22 = dxx * dyy - dxy * dxy
        with np.errstate(all="ignore"):
            xc = -((c00 * gx + c01 * gy + c02 * gs) / det)
            xr = -((c01 * gx + c11 * gy + c12 * gs) / det)
            xi = -((c02 * gx + c12 * gy + c22 * gs) / det)
        big = F(1e6)
        if not (abs(xc) <= big and abs(xr) <= big and abs(xi) <= big):
            return None
        if abs(xc) < F(0.5) and abs(xr) < F(0.5) and abs(xi) < F(0.5):
            converged = True
            break
        c, r, i = c + int(np.rint(xc)), r + int(np.rint(xr)), i + int(np.rint(xi))
        if i < 1 or i > LAYERS or c < BORDER or c >= w - BORDER or r < BORDER or r >= h - BORDER:
            return None
    if not converged:
        return None
    t = gx * xc + gy * xr + gs * xi
    contr = q[r, c] * img_scale + t * F(0.5)
    if abs(contr) * F(LAYERS) < ct:
        return None
    tr, det2 = dxx + dyy, dxx * dyy - dxy * dxy
    if det2 <= 0 or tr * tr * edge >= (edge + one) * (edge + one) * det2:
        return None
    e = (F(i) + xi) * (one / F(3))
    scl = F(sigma) * expf(e * F(0.6931472))
    po = F(2 ** o) * F(0.5)
    return dict(o=o, i=i, r=r, c=c, cand=cand, x=(F(c) + xc) * po, y=(F(r) + xr) * po, size=F(scl) * F(2 ** o), scl=F(scl),
                response=abs(contr))


def _gradients(img, y, x):
    """dx, dy, angle in degrees and magnitude at integer pixel arrays inside the image's 1-pixel border."""
    dx = img[y, x + 1] - img[y, x - 1]
    dy = img[y - 1, x] - img[y + 1, x]
    return atan2deg(dy, dx), np.sqrt(dx * dx + dy * dy)


def _fixed(v):
    return np.rint(v * FIX).astype(np.int64)


def orientation_histogram(img, r, c, scl):
    """The 36 integer bins (fixed point 2^20)."""
    h, w = img.shape
    radius = int(np.rint(F(4.5) * scl))
    sp = F(1.5) * scl
    es = F(-1) / ((F(2) * sp) * sp)
    d = np.arange(-radius, radius + 1)
    di, dj = [a.reshape(-1) for a in np.meshgrid(d, d, indexing="ij")]
    y, x = r + di, c + dj
    keep = (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    di, dj, y, x = di[keep], dj[keep], y[keep], x[keep]
    ori, mag = _gradients(img, y, x)
    wgt = expf((di * di + dj * dj).astype(F) * es)
    b = np.rint(ori * F(0.1)).astype(np.int64)
    b = np.where(b >= ORI_BINS, b - ORI_BINS, b)
    b = np.where(b < 0, b + ORI_BINS, b)
    hist = np.zeros(ORI_BINS, np.int64)
    np.add.at(hist, b, _fixed(wgt * mag))
    return hist


def orientations(img, r, c, scl):
    """[(bin k, angle in degrees)] of a keypoint, ascending k."""
    hq = orientation_histogram(img, r, c, scl).astype(F) * (F(1) / FIX)
    k = np.arange(ORI_BINS)
    g = lambda s: hq[(k + s) % ORI_BINS]          # noqa: E731
    sm = (g(-2) + g(2)) * F(0.0625) + (g(-1) + g(1)) * F(0.25) + hq * F(0.375)
    thr = F(0.8) * sm.max()
    out = []
    for b in range(ORI_BINS):
        lf, ct, rt = sm[(b - 1) % ORI_BINS], sm[b], sm[(b + 1) % ORI_BINS]
        if ct > lf and ct > rt and ct >= thr:
            bf = F(b) + (F(0.5) * (lf - rt)) / ((lf - F(2) * ct) + rt)
            if bf < 0:
                bf = bf + F(ORI_BINS)
            if bf >= F(ORI_BINS):
                bf = bf - F(ORI_BINS)
            ang = F(360) - F(10) * bf
            if abs(ang - F(360)) < EPS:
                ang = F(0)
            out.append((b, F(ang)))
    return out


def descriptor(img, r, c, scl, angle):
    """The 128 uint8 of a keypoint with angle `angle` (the keypoint's, degrees)."""
    h, w = img.shape
    a = F(360) - F(angle)
    if abs(a - F(360)) < EPS:
        a = F(0)
    sn, cs = sincosdeg(a)
    hw = F(3) * scl
    radius = min(int(np.rint(hw * F(1.4142135) * F(2.5))), h + w)
    cs, sn = cs / hw, sn / hw
    d = np.arange(-radius, radius + 1)
    di, dj = [v.reshape(-1) for v in np.meshgrid(d, d, indexing="ij")]
    fi, fj = di.astype(F), dj.astype(F)
    c_rot, r_rot = fj * cs - fi * sn, fj * sn + fi * cs
    rbin, cbin = r_rot + F(1.5), c_rot + F(1.5)
    y, x = r + di, c + dj
    keep = (rbin > -1) & (rbin < 4) & (cbin > -1) & (cbin < 4) & (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    c_rot, r_rot, rbin, cbin, y, x = c_rot[keep], r_rot[keep], rbin[keep], cbin[keep], y[keep], x[keep]
    ori, mag = _gradients(img, y, x)
    wgt = expf((c_rot * c_rot + r_rot * r_rot) * F(-0.125))
    obin = (ori - a) * F(0.022222223)
    m = mag * wgt
    r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
    fr, fc, fo = rbin - r0, cbin - c0, obin - o0
    r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), np.mod(o0.astype(np.int64), 8)
    v1 = m * fr
    v0 = m - v1
    v11 = v1 * fc
    v10 = v1 - v11
    v01 = v0 * fc
    v00 = v0 - v01
    hist = np.zeros(128, np.int64)
    for (dr, dc, vrc) in ((0, 0, v00), (0, 1, v01), (1, 0, v10), (1, 1, v11)):
        hi = vrc * fo
        lo = vrc - hi
        rr, cc = r0 + dr, c0 + dc
        ok = (rr >= 0) & (rr <= 3) & (cc >= 0) & (cc <= 3)
        for (do, v) in ((0, lo), (1, hi)):
            np.add.at(hist, ((rr * 4 + cc) * 8 + (o0 + do) % 8)[ok], _fixed(v)[ok])
    dst = hist.astype(F) * (F(1) / FIX)

    def norm2(v):
        acc = v[0] * v[0]
        for k in range(1, 128):
            acc = acc + v[k] * v[k]
        return acc

    dst = np.minimum(dst, np.sqrt(norm2(dst)) * F(0.2))
    scale = F(512) / max(np.sqrt(norm2(dst)), EPS)
    return np.minimum(255, np.rint(dst * scale).astype(np.int64)).astype(np.uint8)


def extract(gray, n_features=0, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6, stages=None):
    """(keypoints [n][6] float32, descriptors [n][128] uint8) of a gray uint8 image; `stages`, a dict, receives the
    intermediate results (candidates, refined, oriented)."""
    gauss, dog = scale_space(gray, sigma)
    pre = pre_threshold(contrast_threshold)
    oriented, n_cand, n_refined = [], 0, 0
    for o in range(len(dog)):
        for cand in candidates(dog[o], pre):
            n_cand += 1
            kp = refine(dog[o], o, cand, contrast_threshold, edge_threshold, sigma)
            if kp is None:
                continue
            n_refined += 1
            for b, ang in orientations(gauss[o][kp["i"]], kp["r"], kp["c"], kp["scl"]):
                oriented.append(dict(kp, bin=b, angle=ang, key=(o,) + cand + (b,)))
    oriented.sort(key=lambda k: k["key"])                                # the canonical order
    if n_features > 0 and len(oriented) > n_features:
        best = sorted(range(len(oriented)), key=lambda j: (-float(oriented[j]["response"]), j))[:n_features]
        oriented = [oriented[j] for j in sorted(best)]
    kps = np.zeros((len(oriented), 6), F)
    desc = np.zeros((len(oriented), 128), np.uint8)
    for j, k in enumerate(oriented):
        kps[j] = (k["x"], k["y"], k["size"], k["angle"], k["response"], F(k["o"] + 256 * k["i"]))
        desc[j] = descriptor(gauss[k["o"]][k["i"]], k["r"], k["c"], k["scl"], k["angle"])
    if stages is not None:
        stages.update(n_candidates=n_cand, n_refined=n_refined, oriented=oriented)
    return kps, desc


# -------------------------------------------------------------------- plain loops, to hold the array forms to ---
def blur_loops(img, tap):
    h, w = img.shape
    r = (len(tap) - 1) // 2

    def f(i, n):
        if n == 1:
            return 0
        p = 2 * (n - 1)
        m = i % p
        return m if m < n else p - m

    t = np.empty_like(img)
    for y in range(h):
        for x in range(w):
            acc = tap[0] * img[y, f(x - r, w)]
            for j in range(1, 2 * r + 1):
                acc = F(acc + F(tap[j] * img[y, f(x - r + j, w)]))
            t[y, x] = acc
    out = np.empty_like(img)
    for y in range(h):
        for x in range(w):
            acc = tap[0] * t[f(y - r, h), x]
            for j in range(1, 2 * r + 1):
                acc = F(acc + F(tap[j] * t[f(y - r + j, h), x]))
            out[y, x] = acc
    return out


def first_difference(stage, got, want):
    """None, or a sentence naming the first differing element of two arrays of a stage."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{stage}: shape / dtype {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    same = (got == want) | ((got != got) & (want != want))
    if same.all():
        return None
    where = tuple(int(v) for v in np.argwhere(~same)[0])
    return f"{stage}: first difference at pixel {where}: device {got[where]!r}, restatement {want[where]!r}; {int((~same).sum())} differ"
