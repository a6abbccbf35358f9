"""The small inputs of the CLAHE / scale-space tests (tests/test_features_cpu.py, tests/test_hip_features.py), and the
restatement's results for them, computed once and shared.

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
