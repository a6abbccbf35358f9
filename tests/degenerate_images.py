"""Degenerate image content for the parity tests (a helper module, not a conftest).

Every GPU parity test elsewhere draws its images from synthetic.make_scene, whose texture makes every window well
conditioned.  Photographs have sky, plain walls, blown-out highlights and black borders, and on a flat window the
reference's variance E[x^2] - E[x]^2 (mvs_patchmatch.py:405-411, dense_stereo.py:340-345) is rounding noise, often
negative: the PatchMatch cost turns NaN and the plane sweep's NCC turns NaN or follows the sign of a rounded
covariance.  The functions here turn a make_scene into such content, seeded and 8-bit exact (gray = code / 255):

    texture       make_scene as is (the control)
    flat          one rectangle at a given code, at the same image rectangle in every view, so that flat
                  reference windows project into flat source windows
    saturated     contrast stretched x4 about mid-gray and clipped
    border        black borders of random width on random sides of every view
    const_source  one source view entirely constant
    checker       a 0/255 checkerboard rectangle in the reference view, flat (code >= 128) in the sources
    float         flat rectangles and noise at values that are not code / 255 (the exact mode's f32 sampling)

draw_pm_case / draw_sweep_case draw the configuration space as tools/fuzz_parity.py does, plus a content class.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CLASSES = ("texture", "flat", "saturated", "border", "const_source", "checker", "float")
DEGENERATE = CLASSES[1:]
FLAT_CODES = (0, 26, 128, 230, 255)


class Case:
    """Images of one scene after a content class: grays (float32, [0,1]), colors (BGR u8), the flat mask per view
    (True where the content class made the image constant) and a description for assertion messages."""

    def __init__(self, scene, content, grays, colors, flat, ref, desc):
        self.scene, self.content, self.grays, self.colors, self.flat, self.ref, self.desc = \
            scene, content, grays, colors, flat, ref, desc
        self.n = len(grays)
        self.H, self.W = grays[0].shape
        self.K = scene.camera.K.astype(np.float32)
        self.R = [scene.poses[i].R for i in range(self.n)]
        self.t = [scene.poses[i].t for i in range(self.n)]

    def images(self):
        return [{"image": c} for c in self.colors]

    def poses(self):
        return dict(self.scene.poses)

    def is_u8(self):
        return all(np.array_equal(np.round(g * 255.0) / np.float32(255.0), g) for g in self.grays)

    def oracle_ctx(self, ref, srcs, k, mode="exact"):
        from oracle import oracle
        return oracle.ViewContext(self.K, self.grays[ref], self.R[ref], self.t[ref], [self.grays[i] for i in srcs],
                                  [self.R[i] for i in srcs], [self.t[i] for i in srcs], k, mode=mode)

    def engine(self, mode="exact"):
        import amvs
        eng = amvs.Engine(self.H, self.W, self.n, self.K, mode=mode)
        for i in range(self.n):
            eng.set_view(i, self.grays[i], self.R[i], self.t[i])
        return eng


def codes_of(scene):
    """The scene's grays as 8-bit codes (n, H, W) uint8."""
    return np.stack([np.round(g * 255.0).clip(0, 255).astype(np.uint8) for g in scene.grays])


def grays_of(codes):
    return [c.astype(np.float32) / np.float32(255.0) for c in codes]


def colors_of(codes):
    """BGR images whose channels follow the gray code as make_scene's do; a flat gray area is flat in colour."""
    c = codes.astype(np.float32)
    bgr = np.stack([np.clip(c * 0.9, 0, 255), c, np.clip(c * 0.8 + 20, 0, 255)], axis=-1)
    return [np.ascontiguousarray(x) for x in bgr.astype(np.uint8)]


def flat_rect(H, W, rng, frac=0.5):
    """A rectangle over about `frac` of the image, at a random place: (y0, y1, x0, x1)."""
    h = max(1, int(round(H * np.sqrt(frac))))
    w = max(1, int(round(W * np.sqrt(frac))))
    y0 = int(rng.integers(0, H - h + 1))
    x0 = int(rng.integers(0, W - w + 1))
    return y0, y0 + h, x0, x0 + w


def _mask(H, W, rect):
    m = np.zeros((H, W), bool)
    y0, y1, x0, x1 = rect
    m[y0:y1, x0:x1] = True
    return m


def apply_flat(codes, rect, code):
    codes = codes.copy()
    y0, y1, x0, x1 = rect
    codes[:, y0:y1, x0:x1] = np.uint8(code)
    return codes


def apply_saturate(codes, gain=4):
    return np.clip((codes.astype(np.int32) - 128) * gain + 128, 0, 255).astype(np.uint8)


def apply_border(codes, rng, max_frac=0.25):
    """Black borders of random width (1 .. max_frac of the side) on a random non-empty set of sides, per view."""
    codes = codes.copy()
    n, H, W = codes.shape
    flat = np.zeros((n, H, W), bool)
    for v in range(n):
        sides = rng.random(4) < 0.5
        if not sides.any():
            sides[int(rng.integers(0, 4))] = True
        for s in np.flatnonzero(sides):
            ext = H if s < 2 else W
            w = int(rng.integers(1, max(2, int(ext * max_frac) + 1)))
            sl = [(slice(0, w), slice(None)), (slice(H - w, H), slice(None)),
                  (slice(None), slice(0, w)), (slice(None), slice(W - w, W))][s]
            codes[v][sl] = 0
            flat[v][sl] = True
    return codes, flat


def checker(H, W, rect, cell):
    """0/255 checkerboard codes over rect (cells of `cell` pixels), None elsewhere (a mask-and-values pair)."""
    y0, y1, x0, x1 = rect
    yy, xx = np.mgrid[y0:y1, x0:x1]
    return np.where(((yy // cell) + (xx // cell)) % 2 == 0, 0, 255).astype(np.uint8)


def make_case(content, n, H, W, seed, ref=0, code=None, arc_step_deg=10.0, rect_frac=0.5):
    """The scene make_scene(n, H, W, seed) with `content` applied; everything that is drawn comes from `seed`."""
    from amvs.synthetic import make_scene
    if content not in CLASSES:
        raise ValueError(content)
    sc = make_scene(n, H, W, seed=seed, arc_step_deg=arc_step_deg)
    rng = np.random.default_rng([seed, CLASSES.index(content)])
    codes = codes_of(sc)
    flat = np.zeros((n, H, W), bool)
    desc = f"{content} {n}x{H}x{W} scene seed {seed}"
    if code is None:
        code = int(rng.choice(FLAT_CODES))
    if content == "flat":
        rect = flat_rect(H, W, rng, rect_frac)
        codes = apply_flat(codes, rect, code)
        flat[:] = _mask(H, W, rect)
        desc += f" code {code} rect {rect}"
    elif content == "saturated":
        codes = apply_saturate(codes)
        flat[:] = (codes == 0) | (codes == 255)
    elif content == "border":
        codes, flat = apply_border(codes, rng)
    elif content == "const_source":
        v = (ref + 1 + int(rng.integers(0, n - 1))) % n
        codes[v] = np.uint8(code)
        flat[v] = True
        desc += f" view {v} at code {code}"
    elif content == "checker":
        code = max(code, 128)
        rect = flat_rect(H, W, rng, rect_frac)
        cell = int(rng.choice([1, 2, 3]))
        codes = apply_flat(codes, rect, code)
        y0, y1, x0, x1 = rect
        codes[ref, y0:y1, x0:x1] = checker(H, W, rect, cell)
        flat[:] = _mask(H, W, rect)
        flat[ref] = False
        desc += f" sources at code {code}, cell {cell} rect {rect}"
    grays = grays_of(codes)
    if content == "float":
        # not 8-bit: a flat rectangle at an off-grid value and a small off-grid perturbation elsewhere
        rect = flat_rect(H, W, rng, rect_frac)
        val = np.float32(rng.uniform(0.05, 0.95))
        m = _mask(H, W, rect)
        for v in range(n):
            g = grays[v] + rng.uniform(-0.4, 0.4, (H, W)).astype(np.float32) / np.float32(255.0)
            g = np.clip(g, 0.0, 1.0).astype(np.float32)
            g[m] = val
            grays[v] = g
        flat[:] = m
        desc += f" value {float(val)!r} rect {rect}"
    return Case(sc, content, grays, colors_of(codes), flat, ref, desc)


# fixed PatchMatch edge cases of tests/test_hip_degenerate.py, 5 views of 96 x 128 (make_case seed 3, reference 2):
# (content, code, mode, k, S, schedule, one iteration per call); the oracle leaves >= 5 % NaN costs at its final depth
PM_FIXED = [("flat", 26, "exact", 5, 4, "auto", False), ("flat", 230, "exact", 11, 4, "view-major", False),
            ("flat", 230, "fast", 5, 4, "paired", False), ("flat", 26, "fast", 7, 4, "split", False),
            ("flat", 255, "fast", 5, 3, "auto", True), ("const_source", 128, "fast", 11, 4, "auto", False),
            ("checker", 230, "fast", 5, 4, "view-major", False), ("float", None, "exact", 5, 4, "auto", False),
            ("flat", 26, "exact", 21, 4, "auto", False), ("flat", 26, "fast", 31, 4, "auto", False)]

# fixed plane-sweep cases, same scenes, 24 planes: (content, code, mode, k, thresh)
SWEEP_FIXED = [("flat", 26, "exact", 5, 0.0), ("flat", 230, "exact", 11, 0.0), ("flat", 26, "fast", 5, 0.0),
               ("flat", 230, "fast", 11, -0.3), ("flat", 230, "exact", 5, 0.8), ("flat", 26, "fast", 5, 0.0005),
               ("checker", 128, "exact", 21, 0.8), ("checker", 230, "exact", 11, 2.0 ** -10),
               ("checker", 230, "fast", 5, 0.3), ("checker", 128, "fast", 21, 0.0),
               ("float", None, "exact", 5, 0.0), ("border", None, "exact", 7, 1.5)]

ODD_K = (3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31)


def draw_pm_case(rng, content=None):
    """One random PatchMatch configuration (the space of tools/fuzz_parity.py) and a content class."""
    n = int(rng.integers(3, 8))
    c = dict(n=n, H=int(rng.integers(9, 151)), W=int(rng.integers(9, 201)), k=int(rng.choice(ODD_K)),
             S=int(rng.integers(2, min(n - 1, 6) + 1)), iters=int(rng.integers(2, 4)), samples=int(rng.integers(1, 4)),
             mode=str(rng.choice(["fast", "exact"])), vpl=int(rng.choice([0, 1, 2])), rows=int(rng.choice([0, 3, 8, 17])),
             scene_seed=int(rng.integers(1, 1000)), arc=float(rng.choice([4.0, 10.0, 25.0])),
             pm_seed=int(rng.integers(0, 2 ** 31)), content=content or str(rng.choice(DEGENERATE)),
             code=int(rng.choice(FLAT_CODES)))
    c["schedule"] = str(rng.choice(["auto", "paired", "view-major", "split"] if c["mode"] == "fast"
                                   else ["auto", "paired", "view-major"]))
    c["split"] = (int(rng.choice([0, 1, 2])), int(rng.choice([0, 1, 4])), 0) if c["schedule"] == "split" else None
    # continue the sweep one iteration per call (first_iteration) instead of one call for all (the split schedule
    # cannot resume a sweep)
    c["one_per_call"] = bool(rng.random() < 0.25) and c["schedule"] != "split"
    return c


def draw_sweep_case(rng, content=None):
    """One random plane-sweep configuration: D crosses the 8-bit keys' 32-plane limit, thresholds inside, on the edge
    of and outside the exact vote gate's range [2^-10, 2^10), wide arcs put planes behind sources."""
    n = int(rng.integers(3, 8))
    return dict(n=n, H=int(rng.integers(9, 151)), W=int(rng.integers(9, 201)),
                k=int(rng.choice([3, 5, 7, 9, 11, 13, 17, 21, 25, 31])), S=int(rng.integers(2, min(n - 1, 6) + 1)),
                D=int(rng.integers(1, 81)), mode=str(rng.choice(["fast", "exact"])),
                thresh=float(rng.choice([0.8, 0.3, 2.0 ** -10, 0.0005, 0.0, -0.3, 1.5])),
                rows=int(rng.choice([0, 5, 13, 32, 47, 64])), ppw=int(rng.choice([0, 1, 3, 7, 32, 40])),
                scene_seed=int(rng.integers(1, 1000)), arc=float(rng.choice([4.0, 10.0, 40.0])),
                batch=bool(rng.random() < 0.3), content=content or str(rng.choice(DEGENERATE)),
                code=int(rng.choice(FLAT_CODES)))


def case_from_draw(c):
    """The images of a drawn configuration (float content forces the exact mode: fast mode takes 8-bit images only)."""
    if c["content"] == "float":
        c["mode"] = "exact"
        if c.get("schedule") == "split":
            c["schedule"], c["split"] = "auto", None
    return make_case(c["content"], c["n"], c["H"], c["W"], c["scene_seed"], ref=0, code=c["code"],
                     arc_step_deg=c["arc"])


def sweep_depths(scene, D):
    """Planes from well in front of the scene to beyond it (as tools/fuzz_parity.py --sweep)."""
    return (1.0 / np.linspace(1 / (scene.depth_max * 3), 1 / (scene.depth_min * 0.2), D)).astype(np.float32)


def mismatches(a, b):
    """Elements that differ, with NaN equal to NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())
