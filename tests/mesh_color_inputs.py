"""Inputs of the vertex-colour tests (a helper module, not a conftest; seeded, no GPU): images, hand-built cases and the
family both tests/test_mesh_color_cpu.py and tests/test_hip_mesh_color.py walk, over the meshes of
mesh_volumes.small_volumes(), mesh_clean_inputs.hand_built() and mesh_render_inputs.hand_built() in the cameras of
mesh_render_inputs.views_for.

Images are random 8-bit noise, so that every misplaced tap changes a byte; of three or more images the fourth is
constant 0 and the fifth constant 255.

The hand-built cases are flat sheets seen by the hand-built camera of mesh_render_inputs (K_HAND, identity pose, image
24 x 32): a sheet is a grid of vertices at chosen pixel positions (at_pixel, exact in float32) and constant depth, wound
to face the camera, so a vertex's footprint is known exactly.  A ColorCase is a mesh_render_inputs.Case with images, a
depth tolerance and `focus`: the vertices the case was built for, by name.

    integer_u        a vertex with u exactly an integer (ax = 0) and one on the optical axis (weight exactly 1); a vertex
                     that no face uses lies on the sheet: zero normal
    borders          a sheet larger than the image with vertices at x0 = 0, -1, W - 2, W - 1 and the same on y
    one_undrawn      an L-shaped sheet: the footprint of the vertex at its inner corner has exactly one undrawn pixel
    two_sheets       a near sheet before a far one: far vertices behind the near sheet, near vertices on its outline
    twin_cameras     the sheet of integer_u in two identical cameras with different images
    twin_constant    the same with constant images 10 and 11
    grazing          a sheet seen at cosines from 0.7 down to 0.4, so that min_cos 0.5 cuts through it
    fused_tap        a sample whose byte differs when the interpolation is contracted into a fused multiply-add
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_inputs as ci  # noqa: E402
import mesh_clean_restatement as cr  # noqa: E402
import mesh_render_inputs as ri  # noqa: E402
import mesh_render_restatement as rr  # noqa: E402
import mesh_volumes as mv  # noqa: E402

F32 = np.float32
SIZES = ((24, 32), (37, 53))
MIN_COS = (F32(0.0), F32(0.5))


def images_for(n, H, W, seed):
    img = np.random.default_rng(7000 + seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    if n >= 5:
        img[3] = 0
        img[4] = 255
    return img


class ColorCase(ri.Case):
    def __init__(self, name, verts, faces, focus, images=None, tolerance=0.0, seed=0, **kw):
        super().__init__(name, verts, faces, seed=seed, **kw)
        self.images = images_for(len(self.poses), self.H, self.W, seed) if images is None else np.asarray(images, np.uint8)
        self.tolerance = F32(tolerance)
        self.focus = focus                     # name -> vertex id
        self.normals = cr.normals(self.verts, self.faces)


def sheet(xs, ys, z, skip=lambda x, y: False):
    """Vertices at at_pixel(x, y, z) for x in xs, y in ys (row-major, y outer) and two faces per cell, wound so that the
    normal looks back at the camera (-z); skip(x, y) leaves out the cell whose top-left vertex is (x, y).  Returns
    (verts, faces, index) with index[(x, y)] the vertex id."""
    verts = [ri.at_pixel(x, y, z) for y in ys for x in xs]
    index = {(x, y): j * len(xs) + i for j, y in enumerate(ys) for i, x in enumerate(xs)}
    faces = []
    for j in range(len(ys) - 1):
        for i in range(len(xs) - 1):
            if skip(xs[i], ys[j]):
                continue
            a, b = j * len(xs) + i, j * len(xs) + i + 1
            c, d = a + len(xs), b + len(xs)
            faces += [(a, c, b), (b, c, d)]
    return verts, faces, index


def integer_u(name="integer u", poses=ri.IDENTITY, images=None, seed=1):
    xs, ys = [4, 7, 8, 9.5, 12], [3, 6, 6.25, 9]
    verts, faces, at = sheet(xs, ys, 2.0)
    verts = verts + [ri.at_pixel(9.25, 5.5, 2.0)]                   # on the sheet, used by no face
    focus = {"integer u": at[(7, 6.25)], "on the axis": at[(8, 6)], "zero normal": len(verts) - 1, "right edge": at[(12, 6)]}
    return ColorCase(name, verts, faces, focus, images=images, poses=poses, seed=seed)


def borders():
    W, H = ri.W, ri.H
    xs = [-3, -1, -0.5, 0, 0.5, 5, W - 2, W - 1.5, W - 1, W + 2]
    ys = [-3, -1, -0.5, 0, 0.5, 5, H - 2, H - 1.5, H - 1, H + 2]
    verts, faces, at = sheet(xs, ys, 2.0)
    focus = {"x0 = 0": at[(0, 5)], "x0 = -1": at[(-0.5, 5)], "x0 = W - 2": at[(W - 1.5, 5)], "x0 = W - 1": at[(W - 1, 5)],
             "x0 = W - 2, integer": at[(W - 2, 5)], "y0 = 0": at[(5, 0)], "y0 = -1": at[(5, -0.5)], "y0 = H - 2": at[(5, H - 1.5)],
             "y0 = H - 1": at[(5, H - 1)]}
    return ColorCase("borders", verts, faces, focus, seed=2)


def one_undrawn():
    xs, ys = [4, 7.5, 8, 12], [3, 5.5, 6, 9]
    verts, faces, at = sheet(xs, ys, 2.0, skip=lambda x, y: x >= 8 and y >= 6)
    return ColorCase("one undrawn pixel", verts, faces, {"inner corner": at[(7.5, 5.5)], "inside": at[(4, 3)]}, seed=3)


def two_sheets():
    far, far_f, far_at = sheet([-2, 2, 8, 10, 13.5, 20, 34], [-2, 3, 7, 11.5, 15, 26], 4.0)
    near, near_f, near_at = sheet([6, 9, 13.5, 14], [5, 8, 12], 2.0)
    off = len(far)
    focus = {"behind the near sheet": far_at[(10, 7)], "far, clear": far_at[(20, 15)], "far, straddling": far_at[(13.5, 11.5)],
             "near, inside": off + near_at[(9, 8)], "near, on the outline": off + near_at[(13.5, 8)],
             "near, right edge": off + near_at[(14, 8)]}
    return ColorCase("two sheets", far + near, far_f + [tuple(i + off for i in f) for f in near_f], focus, seed=4)


def twin_cameras():
    return integer_u("twin cameras", poses=np.stack([ri.IDENTITY, ri.IDENTITY]), seed=5)


def twin_constant():
    img = np.empty((2, ri.H, ri.W, 3), np.uint8)
    img[0], img[1] = 10, 11
    return integer_u("twin cameras, constant 10 and 11", poses=np.stack([ri.IDENTITY, ri.IDENTITY]), images=img, seed=6)


def grazing():
    """A sheet in the plane z = 2 from x = 1 to x = 5 seen by a camera at the origin turned toward it."""
    gx, gy = np.linspace(1.0, 5.0, 17), np.linspace(-1.0, 1.0, 7)
    verts = [(x, y, 2.0) for y in gy for x in gx]
    faces = []
    for j in range(len(gy) - 1):
        for i in range(len(gx) - 1):
            a, b = j * len(gx) + i, j * len(gx) + i + 1
            c, d = a + len(gx), b + len(gx)
            faces += [(a, c, b), (b, c, d)]
    pose = ri.look_at((0.0, 0.0, 0.0), (3.0, 0.0, 2.0), up=(0.0, 1.0, 0.0))
    K = np.array([[12.0, 0, 16.0], [0, 12.0, 12.0], [0, 0, 1]], F32)
    return ColorCase("grazing", verts, faces, {}, K=K, poses=pose, tolerance=0.5, seed=7)


FUSED_AX = F32(0.97826087474823)          # 254 + ax * (1 - 254) is 6.5 with two roundings and just below it with one


def fused_tap():
    """A vertex at u = FUSED_AX, v = 6 exactly (the principal point's column is 0, so u = 16 X / Z with no rounding) over
    the image columns 254 and 1: the sample is 6.5 -> 7 as defined and 6.4999986 -> 6 through a fused multiply-add."""
    K = np.array([[ri.FOCAL, 0, 0.0], [0, ri.FOCAL, ri.CY], [0, 0, 1]], F32)
    xs, ys = [-2.0, float(FUSED_AX), 3.0], [3.0, 6.0, 9.0]
    verts = [(F32(x) * F32(2.0) / F32(ri.FOCAL), (y - ri.CY) * 2.0 / ri.FOCAL, 2.0) for y in ys for x in xs]
    faces = []
    for j in range(2):
        for i in range(2):
            a, b = 3 * j + i, 3 * j + i + 1
            faces += [(a, a + 3, b), (b, a + 3, b + 3)]
    images = images_for(1, ri.H, ri.W, 8)
    images[0, :, 0], images[0, :, 1] = 254, 1
    return ColorCase("fused tap", verts, faces, {"tap": 4}, images=images, K=K, tolerance=0.25, seed=8)


def hand_built():
    return [integer_u(), borders(), one_undrawn(), two_sheets(), twin_cameras(), twin_constant(), grazing(), fused_tap()]


# ---- the family ---------------------------------------------------------------------------------------------

class Member:
    """A mesh of the family with the cameras and images it is coloured from: the maps are rendered once (the
    restatement's) and shared.  n_views lists the numbers of views to run (the first n of the cameras), tolerances the
    depth tolerances."""

    def __init__(self, name, arrays, K, poses, near, H, W, images, n_views, tolerances):
        self.name = name
        self.verts, self.faces, self.colors = arrays
        self.K, self.poses, self.near, self.H, self.W = np.asarray(K, F32), np.asarray(poses, F32).reshape(-1, 12), F32(near), H, W
        self.images, self.n_views, self.tolerances = images, n_views, tolerances
        self._maps = None
        self._normals = None

    @property
    def normals(self):
        if self._normals is None:
            self._normals = cr.normals(self.verts, self.faces) if len(self.verts) else np.zeros((0, 3), F32)
        return self._normals

    def maps(self):
        """(depth, face) of all cameras; view m of a render into the first n cameras is view m of this one."""
        if self._maps is None:
            self._maps = rr.render(self.verts, self.faces, self.K, self.poses, self.near, self.H, self.W)[:2]
        return self._maps


def family(H, W):
    """Large meshes before small ones and the empty one in between, as the grow-only buffers want it."""
    seed = 0
    sources = [(vol.name, vol.extract()) for vol in mv.small_volumes()] + [(m.name, m.arrays()) for m in ci.hand_built()]
    for name, arrays in sources:
        seed += 1
        K, poses, near = ri.views_for(arrays[0], 6, H, W)
        yield Member(name, arrays, K, poses, near, H, W, images_for(6, H, W, seed), (1, 6), (F32(0), F32(near)))
    for case in ri.hand_built() + hand_built():
        seed += 1
        if (case.H, case.W) != (H, W):
            continue
        n = len(case.poses)
        images = case.images if isinstance(case, ColorCase) else images_for(n, H, W, seed)
        tolerances = (F32(0), case.tolerance if isinstance(case, ColorCase) and case.tolerance > 0 else F32(case.near))
        yield Member(case.name, case.arrays(), case.K, case.poses, case.near, H, W, images, (n,), tolerances)


def sphere_case():
    """The analytic-truth scene: the mesh of sphere_volume(33) in six axis views at 48 x 64 (f = 60, distance 3)."""
    H, W, focal, distance, radius = 48, 64, 60.0, 3.0, 0.8
    return ri.sphere_mesh(33), ri.pinhole(focal, H, W), ri.axis_views(distance), F32(0.1), H, W, focal, distance, radius


def sphere_colour(points):
    """A smooth colour function of a point on the unit sphere's directions: (N,3) float64 B, G, R in 40 .. 215."""
    d = np.asarray(points, np.float64)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return np.stack([127.5 + 87.5 * d[..., 0], 127.5 + 87.5 * d[..., 1] * d[..., 2] * 2.0, 127.5 + 87.5 * np.sin(2.0 * d[..., 2])],
                    axis=-1)


def sphere_images():
    """The six images ray-cast from the analytic sphere: (6,H,W,3) uint8 BGR, 0 off the sphere, and the hit masks."""
    _, K, poses, _, H, W, focal, distance, radius = sphere_case()
    Kd = K.astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    rays = np.stack([(xs - Kd[0, 2]) / focal, (ys - Kd[1, 2]) / focal, np.ones((H, W))], -1)
    images = np.zeros((6, H, W, 3), np.uint8)
    hits = np.zeros((6, H, W), bool)
    for m, pose in enumerate(poses.astype(np.float64)):
        R, t = pose[:9].reshape(3, 3), pose[9:]
        eye = -R.T @ t
        d = rays @ R                                                   # world directions: R^T ray
        a, b, c = (d * d).sum(-1), (d @ eye), eye @ eye - radius * radius
        disc = b * b - a * c
        hit = disc > 0
        s = (-b - np.sqrt(np.where(hit, disc, 0))) / a
        points = eye + s[..., None] * d
        col = np.floor(sphere_colour(points) + 0.5)
        images[m] = np.where(hit[..., None], np.clip(col, 0, 255), 0).astype(np.uint8)
        hits[m] = hit
    return images, hits
