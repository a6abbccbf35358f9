"""Inputs of the texture tests (a helper module, not a conftest; seeded, no GPU): the family both
tests/test_mesh_texture_cpu.py and tests/test_hip_mesh_texture.py walk, and the analytic sphere scene.

The family is that of mesh_color_inputs (its meshes up to the 33^3 sphere, its cameras and images) plus the hand-built
cases below, every mesh at N in TEXELS and cells_per_row in CELLS_PER_ROW.  A Job is one texture call: a member, the number
of views, N, cells_per_row, the depth tolerance, min_cos and the combine mode.  The three settings rotate through their
eight combinations from job to job, and the number of views alternates, so every combination meets every N and every
cells_per_row many times without the product of all of them.  A combination whose atlas would exceed the side limit is no
job (the GPU test asserts that it is refused): `refused` lists those.

Hand-built cases, flat sheets in the hand-built camera of mesh_render_inputs (K_HAND, identity pose, 24 x 32):

    hypotenuse        (a) a fronto-parallel face at depth 2 with corners at pixels (12,12), (4,12), (12,4): the midpoint
                      (8,8) of its hypotenuse is a pixel centre the coverage rule gives to it (the edge runs up, dy < 0),
                      there b0 = 0 and g1 = g2 = 0.5 exactly, so i + j = N for even N: the pull-back branch
    corner triangles  (b) six right triangles with the right angle at their top-left vertex A, a pixel centre that the
                      coverage rule gives to them (top and left edge), in the corner orders that make A corner 0, 1 and 2,
                      in both windings: at A g is exactly 1 for A's corner (x = N, i clamped to N - 1) and 0 for the others
    corner sheet      (c) a sheet facing the camera: the image's y runs down, so the set-up exchanges corners 1 and 2 of
                      every face, and the textured pixels must go through the un-exchanged g
    corner sheet, winding reversed
                      the same sheet facing away: no exchange, no view reaches a texel, all fall back
    degenerate        (d) a face of three collinear points (zero normal) beside a sheet: its texels fall back
    two sheets        (e) mesh_color_inputs.two_sheets: far faces half hidden behind the near sheet
    twin constant     (f) mesh_color_inputs.twin_constant: two identical cameras with images of constant 10 and 11
"""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_color_inputs as ki  # noqa: E402
import mesh_decimate_restatement as dr  # noqa: E402
import mesh_render_inputs as ri  # noqa: E402
import mesh_texture_restatement as tr  # noqa: E402
import mesh_volumes as mv  # noqa: E402

F32 = np.float32
SIZES = ki.SIZES
TEXELS = (1, 2, 3, 8)
CELLS_PER_ROW = (0, 1, 3)
MIN_COS = ki.MIN_COS
MAX_FACES = 18408                              # the 33^3 sphere


def hypotenuse():
    verts = [ri.at_pixel(12, 12), ri.at_pixel(4, 12), ri.at_pixel(12, 4), ri.at_pixel(4, 4)]
    return ki.ColorCase("hypotenuse through a pixel centre", verts, [(0, 1, 2), (3, 2, 1)], {"midpoint": (8, 8)}, seed=21)


CORNER_A = [(3 + 9 * k, 3 + 10 * row) for row in range(2) for k in range(3)]       # the owned vertex of every triangle


def corner_triangles():
    verts, faces = [], []
    for t, (x, y) in enumerate(CORNER_A):
        a = len(verts)
        verts += [ri.at_pixel(x, y), ri.at_pixel(x + 6, y), ri.at_pixel(x, y + 6)]
        order = ((0, 1, 2), (2, 0, 1), (1, 2, 0), (0, 2, 1), (1, 0, 2), (2, 1, 0))[t]   # A is corner 0, 1, 2, 0, 1, 2
        faces.append(tuple(a + k for k in order))
    return ki.ColorCase("corner triangles", verts, faces, {}, seed=24)


def corner_sheet(reverse=False):
    verts, faces, at = ki.sheet(list(range(2, 30, 3)), list(range(2, 22, 3)), 2.0)
    faces = np.asarray(faces, np.int32)
    if reverse:
        faces = faces[:, [0, 2, 1]]
    return ki.ColorCase("corner sheet" + (", winding reversed" if reverse else ""), verts, faces, {}, seed=22)


def degenerate():
    verts, faces, at = ki.sheet([3, 9, 15], [3, 9, 15], 2.0)
    n = len(verts)
    verts = verts + [(0.0, 0.0, 2.0), (0.25, 0.125, 2.0), (0.5, 0.25, 2.0)]
    return ki.ColorCase("degenerate face", verts, faces + [(n, n + 1, n + 2)], {"face": len(faces)}, seed=23)


def hand_built():
    return [hypotenuse(), corner_triangles(), corner_sheet(), corner_sheet(True), degenerate(), ki.two_sheets(), ki.twin_constant()]


class Job:
    def __init__(self, mem, n, N, cells_per_row, tolerance, min_cos, best):
        self.mem, self.n, self.N, self.cells_per_row = mem, n, N, cells_per_row
        self.tolerance, self.min_cos, self.best = tolerance, min_cos, best
        self._ref = None

    def __str__(self):
        return (f"{self.mem.name}, {self.mem.H} x {self.mem.W}, {self.n} views, N {self.N}, cells per row {self.cells_per_row}, "
                f"tolerance {self.tolerance}, min_cos {self.min_cos}, best {self.best}")

    def reference(self, counters=None):
        """(atlas, uv, n_texels, n_textured) of the restatement, computed once."""
        if self._ref is None or counters is not None:
            m, n = self.mem, self.n
            depth, _ = m.maps()
            self._ref = tr.texture(m.verts, m.faces, m.colors, m.K, m.poses[:n], m.near, depth[:n], m.images[:n], self.tolerance,
                                   self.min_cos, self.best, self.N, self.cells_per_row, counters=counters)
        return self._ref

    def render_reference(self, counters=None):
        m, n = self.mem, self.n
        depth, face = m.maps()
        return tr.render_texture(m.verts, m.faces, self.reference()[0], m.K, m.poses[:n], m.near, depth[:n], face[:n], self.N,
                                 self.cells_per_row, counters=counters)


def members(H, W):
    for mem in ki.family(H, W):
        if len(mem.faces) <= MAX_FACES:
            yield mem
    if (H, W) == (ri.H, ri.W):
        for case in hand_built()[:5]:                       # the last two are in the colour family already
            yield ki.Member(case.name, case.arrays(), case.K, case.poses, case.near, H, W, case.images, (len(case.poses),),
                            (F32(0), F32(case.near)))


def family(H, W):
    """(jobs, refused): the jobs of one image size, the atlases in descending size within a member (N = 8 first), and the
    (member, N, cells_per_row) whose atlas is over the limit."""
    jobs, refused = [], []
    turn = 0
    settings = list(itertools.product((False, True), (0, 1), (0, 1)))
    for mem in members(H, W):
        for N in reversed(TEXELS):
            for cpr in CELLS_PER_ROW:
                _, _, Wt, Ht = tr.layout(len(mem.faces), N, cpr)
                if Wt > tr.MAX_SIDE or Ht > tr.MAX_SIDE:
                    refused.append((mem, N, cpr))
                    continue
                best, ti, ci_ = settings[turn % 8]
                n = mem.n_views[(turn // 8) % len(mem.n_views)]
                jobs.append(Job(mem, n, N, cpr, mem.tolerances[ti], MIN_COS[ci_], best))
                turn += 1
    return jobs, refused


# ---- the analytic sphere ------------------------------------------------------------------------------------

FINE_PERIOD = 4.0                              # pixels, about: the period of the added term in the images


def sphere_colour(points):
    """mesh_color_inputs.sphere_colour plus a term that varies within a decimated face: a period of about FINE_PERIOD
    pixels at the sphere's image scale (focal 60 at distance 3 - 0.8: 27 pixels per unit, so about 0.147 units)."""
    d = np.asarray(points, np.float64)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    wave = 2.0 * np.pi / (FINE_PERIOD / (60.0 / 2.2) / 0.8)         # per unit of direction on the 0.8 sphere
    fine = np.stack([np.sin(wave * d[..., 1]), np.sin(wave * d[..., 2]), np.sin(wave * d[..., 0])], axis=-1)
    return ki.sphere_colour(points) + 35.0 * fine


def sphere_scene():
    """The mesh of sphere_volume(33) decimated at 2 voxels, the six axis views of the colour section's sphere test and the
    images ray-cast from the analytic sphere with sphere_colour above: a dict."""
    (v, f, c), K, poses, near, H, W, focal, distance, radius = ki.sphere_case()
    vol = mv.sphere_volume(33)
    v, f, c = dr.decimate(v, f, c, vol.origin, F32(2) * vol.voxel)[:3]
    Kd = K.astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    rays = np.stack([(xs - Kd[0, 2]) / focal, (ys - Kd[1, 2]) / focal, np.ones((H, W))], -1)
    images = np.zeros((6, H, W, 3), np.uint8)
    for m, pose in enumerate(poses.astype(np.float64)):
        R, t = pose[:9].reshape(3, 3), pose[9:]
        eye = -R.T @ t
        d = rays @ R
        a, b, cc = (d * d).sum(-1), (d @ eye), eye @ eye - radius * radius
        disc = b * b - a * cc
        hit = disc > 0
        s = (-b - np.sqrt(np.where(hit, disc, 0))) / a
        col = np.floor(sphere_colour(eye + s[..., None] * d) + 0.5)
        images[m] = np.where(hit[..., None], np.clip(col, 0, 255), 0).astype(np.uint8)
    return dict(v=v, f=f, c=c, K=K, poses=poses, near=near, H=H, W=W, images=images, voxel=vol.voxel, radius=radius)
