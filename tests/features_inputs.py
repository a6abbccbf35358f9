"""The small inputs of the CLAHE / scale-space tests (tests/test_features_cpu.py, tests/test_hip_features.py), the second
family for what only larger or crowded images reach (tests/test_hip_features_scale.py), and the restatement's results
for them, computed once and shared.

The textures are band-limited and procedural: a sum of sinusoids with periods of 7 pixels and more, plus smooth noise
(random values on a grid of 6-pixel cells, interpolated by a raised cosine), quantised to 8 bits."""
import collections

import numpy as np

import features_restatement as fr

Case = collections.namedtuple("Case", "name gray")


def texture_function(x, y, seed=0):
    """The texture at real coordinates (arrays of one shape), 0 .. 1."""
    rng = np.random.RandomState(1000 + seed)
    v = np.zeros(np.broadcast(x, y).shape)
    for _ in range(6):
        period = rng.uniform(7.0, 40.0)
        ang = rng.uniform(0, np.pi)
        v = v + rng.uniform(0.5, 1.0) * np.sin(2 * np.pi * (x * np.cos(ang) + y * np.sin(ang)) / period + rng.uniform(0, 2 * np.pi))
    cell = 6.0
    grid = rng.uniform(-1.5, 1.5, (64, 64))
    gx, gy = x / cell, y / cell
    ix, iy = np.floor(gx).astype(int), np.floor(gy).astype(int)
    fx, fy = 0.5 - 0.5 * np.cos(np.pi * (gx - ix)), 0.5 - 0.5 * np.cos(np.pi * (gy - iy))
    g = lambda a, b: grid[np.mod(a, 64), np.mod(b, 64)]    # noqa: E731
    v = v + (g(iy, ix) * (1 - fx) + g(iy, ix + 1) * fx) * (1 - fy) + (g(iy + 1, ix) * (1 - fx) + g(iy + 1, ix + 1) * fx) * fy
    return (v - v.min()) / max(v.max() - v.min(), 1e-9)


def texture(h, w, seed=0):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.round(30 + 200 * texture_function(xx, yy, seed)).astype(np.uint8)


def blobs(h, w, centres, sigma, amplitude=110.0, base=90.0):
    """Gaussian blobs of one sigma at (row, column, sign) centres on a flat ground."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    v = np.full((h, w), base)
    for cy, cx, sign in centres:
        v = v + sign * amplitude * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * sigma * sigma))
    return np.clip(np.round(v), 0, 255).astype(np.uint8)


def planted():
    """Blobs whose extrema lie 5 and 6 pixels from each border of octave 0 (the doubled image: 2.25 and 2.75 input pixels
    in) and of octave 1 (5 and 6 input pixels in), dark and bright alternating."""
    h, w = 44, 52
    centres = []
    for k, d in enumerate((2.25, 2.75)):
        centres += [(d, 12 + 20 * k, 1), (h - 1 - d, 12 + 20 * k, -1), (12 + 14 * k, d, -1), (12 + 14 * k, w - 1 - d, 1)]
    small = blobs(h, w, centres, 1.1)
    centres = []
    for k, d in enumerate((5.0, 6.0)):
        centres += [(d, 14 + 22 * k, 1), (h - 1 - d, 14 + 22 * k, -1), (14 + 16 * k, d, -1), (14 + 16 * k, w - 1 - d, 1)]
    return small, blobs(h, w, centres, 2.2)


def lattice(h=96, w=96, period=16):
    """The same blob at every node of a lattice: away from the borders the keypoints tie in response, bit for bit."""
    return blobs(h, w, [(cy, cx, 1) for cy in range(period // 2, h, period) for cx in range(period // 2, w, period)], 2.0)


def blob_between_bars(h=48, w=48):
    """A blob between two vertical bars: its gradients are two-fold symmetric, the histogram has two peaks 180 degrees apart."""
    g = blobs(h, w, [(h / 2 - 0.5, w / 2 - 0.5, 1)], 2.0).astype(np.int64)
    g[:, w // 2 - 9:w // 2 - 6] += 100
    g[:, w // 2 + 6:w // 2 + 9] += 100
    return np.clip(g, 0, 255).astype(np.uint8)


def cases():
    """name, gray.  Sizes are rows x columns."""
    step = np.full((32, 40), 60, np.uint8)
    step[:, 20:] = 190
    return [
        Case("texture 48x64", texture(48, 64, 0)),
        Case("texture 47x61 (odd: halving drops a row and a column)", texture(47, 61, 1)),
        Case("texture 53x37 (no multiple of the grid)", texture(53, 37, 2)),
        Case("texture 45x50 (the last side with 4 octaves)", texture(45, 50, 3)),
        Case("texture 46x50 (the first side with 5 octaves)", texture(46, 50, 4)),
        Case("texture 24x24 (last octaves narrower than the radius)", texture(24, 24, 5)),
        Case("texture 70x150 (several tiles of the row and column passes)", texture(70, 150, 6)),
        Case("constant 32x40", np.full((32, 40), 77, np.uint8)),
        Case("step edge 32x40", step),
        Case("sliver 3x5 (padding folds more than once)", texture(3, 5, 7)),
        Case("planted 44x52 (extrema 5 and 6 pixels from the borders of octave 0)", planted()[0]),
        Case("planted 44x52 (extrema 5 and 6 pixels from the borders of octave 1)", planted()[1]),
        Case("lattice 96x96 (keypoints that tie in response)", lattice()),
        Case("blob between bars 48x48 (two orientations)", blob_between_bars()),
    ]


# clip_limit, (grid_x, grid_y)
CLAHE_PARAMS = [(2.0, (8, 8)), (3.0, (8, 8)), (40.0, (8, 8)), (0.0, (8, 8)), (300.0, (4, 2)), (2.0, (1, 1)), (2.0, (3, 5))]
SIGMAS = [1.6, 1.4]

# n_features (0: all), contrast_threshold, edge_threshold, sigma: SIFT_create's defaults and the dense mode's values
EXTRACT_PARAMS = [(0, 0.04, 10.0, 1.6), (0, 0.01, 20.0, 1.4), (7, 0.03, 15.0, 1.6)]

_CLAHE, _SPACE, _EXTRACT = {}, {}, {}


def restated_extract(case, params):
    """(keypoints, descriptors, stages) of the restatement."""
    key = (case.name, params)
    if key not in _EXTRACT:
        stages = {}
        kps, desc = fr.extract(case.gray, *params, stages=stages)
        _EXTRACT[key] = (kps, desc, stages)
    return _EXTRACT[key]


def tie_cut(case):
    """n_features that cuts through the largest group of equal responses of a case's keypoints (defaults otherwise)."""
    kps, _, _ = restated_extract(case, EXTRACT_PARAMS[0])
    resp = np.sort(kps[:, 4])[::-1]
    values, first, counts = np.unique(-resp, return_index=True, return_counts=True)
    g = int(np.argmax(counts))
    assert counts[g] >= 4, "no tie to cut"
    return int(first[g] + counts[g] // 2)


# ------------------------------------------------------------------------------------------ the second family ---
# Inputs for what only larger images, crowded images and the ends of the sigma range reach (tests/test_features_cpu.py
# states the condition each one is there for; tests/test_hip_features_scale.py compares them on the device).  They are
# kept out of cases(): every test parametrised over that list would run them too.
BUSY_PARAMS = (0, 0.023, 10.0, 0.5)         # pre-threshold floor(0.5 * 0.023 / 3 * 255) = 0: every non-zero extremum is a candidate
WIDE_PARAMS = (0, 0.01, 20.0, 4.0)          # the largest sigma: orientation radius up to 40, descriptor radius up to 95
FINE_PARAMS = (0, 0.0, 1e6, 0.3)            # orientation radius 1 or 2, nothing rejected for contrast or edge
CLIP_PARAMS = (0, 0.005, 50.0, 4.0)         # of the search for the descriptor radius clip
CUT = 3000                                  # the fixed n_features of the crowded image
EXTREMA_PASS = 8192 * 256                   # lanes of one pass of the extrema search's grid


def noise(h, w, seed=5):
    """Full-range noise about 128, every pixel independent."""
    return np.clip(128 + np.random.RandomState(seed).randint(-60, 61, (h, w)), 0, 255).astype(np.uint8)


def blobs_in_noise(h=220, w=220):
    """Three blobs on a flat ground plus integer noise in -2 .. 2: tens of thousands of extrema, nearly all too weak."""
    g = blobs(h, w, [(40, 40, 1), (100, 90, -1), (70, 120, 1)], 2.0).astype(np.int64)
    return np.clip(g + np.random.RandomState(17).randint(-2, 3, (h, w)), 0, 255).astype(np.uint8)


def seam_pixel(h, w):
    """(layer, row, column) in octave 0 of an h x w image of the last interior pixel of the extrema search's first pass:
    the one a grid stride one short would visit a second time."""
    ih, iw = 2 * h - 10, 2 * w - 10
    layer, rem = divmod(EXTREMA_PASS - 1, ih * iw)
    return 1 + layer, 5 + rem // iw, 5 + rem % iw


def texture_with_seam_blob(h=520, w=700, seed=12):
    """The texture plus one blob of sigma 1.4 centred on seam_pixel()'s place in the image: its extremum is a candidate of
    layer 2 exactly there (pixel (r, c) of the doubled image lies at ((r - 0.5) / 2, (c - 0.5) / 2) of the image)."""
    _, r, c = seam_pixel(h, w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    blob = 110.0 * np.exp(-((yy - (r - 0.5) / 2) ** 2 + (xx - (c - 0.5) / 2) ** 2) / (2.0 * 1.4 * 1.4))
    return np.clip(np.round(texture(h, w, seed) + blob), 0, 255).astype(np.uint8)


def scale_cases():
    """name -> (Case, extraction parameters), built once.  The names are distinct from those of cases(): the memo is
    keyed by them."""
    if not _SCALE:
        _SCALE.update(_scale_cases())
    return _SCALE


_SCALE = {}


def _scale_cases():
    return {
        "wrap": (Case("texture 520x520 (the extrema search wraps)", texture(520, 520, 12)), EXTRACT_PARAMS[0]),
        "wrap, mid-layer": (Case("texture 520x700 (the first pass of the extrema search ends half-way through layer 2, on a keypoint)",
                                 texture_with_seam_blob()), EXTRACT_PARAMS[0]),
        "clip": (Case("blob 14x30 at sigma 4 (descriptor radius beyond rows + columns of octave 1)", clip_image(CLIP_RECIPE)), CLIP_PARAMS),
        "candidates": (Case("blobs in noise 220x220 (more candidates than the first array holds)", blobs_in_noise()), BUSY_PARAMS),
        "crowd": (Case("noise 150x150 (thousands of keypoints, ties everywhere)", noise(150, 150)), BUSY_PARAMS),
        "wide": (Case("texture 70x150 at sigma 4", texture(70, 150, 6)), WIDE_PARAMS),
        "fine": (Case("noise 60x60 at sigma 0.3", np.ascontiguousarray(noise(150, 150)[:60, :60])), FINE_PARAMS),
        "busy": (Case("texture 70x150 at sigma 0.5", texture(70, 150, 6)), BUSY_PARAMS),
    }


SPACE_CASE = Case("texture 70x300 (three row tiles, ten by three column tiles in octave 0)", texture(70, 300, 6))
SPACE_SIGMAS = [4.0, 0.5, 0.1]


def extrema_index(cand, h, w):
    """The index the extrema search gives candidate (i, r, c) of an h x w octave: layer, row, column of the interior."""
    i, r, c = cand
    return (i - 1) * (h - 10) * (w - 10) + (r - 5) * (w - 10) + (c - 5)


def tie_cut_near(kps, around):
    """The first n_features >= around that cuts between two keypoints of equal response."""
    resp = np.sort(kps[:, 4])[::-1]
    for n in range(around, len(resp)):
        if resp[n - 1] == resp[n]:
            return n
    raise AssertionError("no tie to cut")


def cut_by_hand(kps, desc, n):
    """The n strongest of keypoints in canonical order: the strictly stronger ones, then the first of the tie."""
    bound = np.sort(kps[:, 4])[::-1][n]
    keep = [j for j in range(len(kps)) if kps[j, 4] > bound]
    keep += [j for j in range(len(kps)) if kps[j, 4] == bound][:n - len(keep)]
    return kps[sorted(keep)], desc[sorted(keep)]


def descriptor_radius(scl):
    """The descriptor window's radius before the clip, as the header computes it (float32)."""
    f = np.float32
    return int(np.rint(f(3) * f(scl) * f(1.4142135) * f(2.5)))


def clip_recipes():
    """The bounded, seeded search space for an input on which the descriptor radius clip decides: both sides <= 40,
    off-centre blobs of sigma 4 to 8 on square and non-square sides, then 200 smooth-noise textures."""
    sides = [(14, 30), (30, 14), (16, 40), (40, 16), (12, 24), (24, 12), (20, 20), (22, 38), (38, 22), (18, 18), (12, 12), (40, 40)]
    out = []
    for h, w in sides:
        for s in (4.0, 5.0, 6.0, 7.0, 8.0):
            for fy, fx in ((0.5, 0.35), (0.45, 0.6), (0.55, 0.5)):
                for sign in (1, -1):
                    out.append(("blob", h, w, s, round(fy * (h - 1), 2), round(fx * (w - 1), 2), sign))
    for seed in range(200):
        h, w = sides[seed % len(sides)]
        out.append(("texture", h, w, 100 + seed))
    return out


def clip_image(recipe):
    if recipe[0] == "blob":
        _, h, w, s, cy, cx, sign = recipe
        return blobs(h, w, [(cy, cx, sign)], s)
    _, h, w, seed = recipe
    return texture(h, w, seed)


def clipped_keypoints(gray, params=CLIP_PARAMS):
    """The oriented keypoints of an image whose descriptor radius exceeds h + w of their octave."""
    stages = {}
    fr.extract(gray, *params, stages=stages)
    h, w = gray.shape
    return [k for k in stages["oriented"] if descriptor_radius(k["scl"]) > (2 * h >> k["o"]) + (2 * w >> k["o"])]


# what clip_search() returns, frozen: recipe 19 (from 0) of clip_recipes(), found in 0.3 s
CLIP_RECIPE = ("blob", 14, 30, 7.0, 6.5, 10.15, -1)


def clip_search(limit=None):
    """(recipe, number of clipped keypoints) of the first recipe with one, or None."""
    for recipe in clip_recipes()[:limit]:
        hits = clipped_keypoints(clip_image(recipe))
        if hits:
            return recipe, len(hits)
    return None


def rotated_pair(n=128, angle_deg=30.0, scale=1.4, seed=20):
    """(image, the same texture rotated by angle_deg about the centre and magnified by scale, the map of positions):
    both rendered from texture_function, nothing is resampled."""
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    th, c = np.deg2rad(angle_deg), (n - 1) / 2.0
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    inv = R.T / scale
    u, v = xx - c, yy - c
    a = texture_function(xx + 40, yy + 40, seed)
    b = texture_function(c + inv[0, 0] * u + inv[0, 1] * v + 40, c + inv[1, 0] * u + inv[1, 1] * v + 40, seed)
    to8 = lambda t: np.round(30 + 200 * t).astype(np.uint8)        # noqa: E731
    return to8(a), to8(b), (lambda p: c + scale * (np.asarray(p, np.float64) - c) @ R.T)


def restated_clahe(case, clip, grid):
    key = (case.name, clip, grid)
    if key not in _CLAHE:
        _CLAHE[key] = fr.clahe(case.gray, clip, grid[0], grid[1], want_counters=True)
    return _CLAHE[key]


def restated_space(case, sigma):
    key = (case.name, sigma)
    if key not in _SPACE:
        _SPACE[key] = fr.scale_space(case.gray, sigma)
    return _SPACE[key]
