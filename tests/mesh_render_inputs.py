"""Hand-built inputs for the mesh rendering tests (a helper module, not a conftest; seeded, no GPU), next to the meshes
of mesh_volumes.small_volumes() and mesh_clean_inputs.hand_built().  A Case is a mesh with the cameras it is drawn
into: verts (V,3) float32, faces (F,3) int32, colors (V,3) uint8, K (3,3) float32, poses (n,12) float32 (R row-major,
t), near, H, W.

The hand-built cases look down +z from the origin through K = [[16, 0, CX], [0, 16, CY], [0, 0, 1]]: a vertex meant for
pixel (u, v) at depth Z (2 or 4) sits at ((u - CX) Z / 16, (v - CY) Z / 16, Z), all exact in float32, so the pixel
positions are exact integers and edges run exactly through pixel centres.

    shared_edges     two quads side by side, each cut along a diagonal: the diagonals, the common vertical edge and the
                     outline all pass through pixel centres; depths differ from corner to corner
    coincident       the same three vertices three times, the second copy wound the other way: equal depth everywhere
    behind_near      one face with a vertex behind `near` next to one that is drawn
    beyond_limit     one face with a vertex that projects beyond 2^20 pixels next to one that is drawn
    zero_area        faces whose three screen positions are collinear or coincide (their 3-D area is not zero)
    whole_image      one face that covers the image and reaches thousands of pixels outside it
    off_image        faces entirely to the left of, above, and below-right of the image
    everything       all of the above in one mesh
    reversed_winding(case)   the same mesh with every face's second and third corner exchanged

views_for(verts, n, H, W) are the cameras the bulk family is drawn into, concentric_spheres() and axis_views() the
scene of the visibility tests.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_volumes as mv  # noqa: E402

F32 = np.float32
H, W = 24, 32
CX, CY, FOCAL = 8.0, 6.0, 16.0
K_HAND = np.array([[FOCAL, 0, CX], [0, FOCAL, CY], [0, 0, 1]], F32)
IDENTITY = np.concatenate([np.eye(3).reshape(9), np.zeros(3)]).astype(F32)
NEAR = F32(0.5)


class Case:
    def __init__(self, name, verts, faces, K=K_HAND, poses=IDENTITY, near=NEAR, H=H, W=W, seed=0):
        self.name = name
        self.verts = np.ascontiguousarray(verts, F32).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        self.colors = np.random.default_rng(2000 + seed).integers(0, 256, self.verts.shape, dtype=np.uint8)
        self.K = np.asarray(K, F32).reshape(3, 3)
        self.poses = np.ascontiguousarray(poses, F32).reshape(-1, 12)
        self.near, self.H, self.W = F32(near), int(H), int(W)

    def arrays(self):
        return self.verts, self.faces, self.colors

    def pose_list(self):
        return [(p[:9].reshape(3, 3), p[9:]) for p in self.poses]


def at_pixel(u, v, z=2.0):
    """The point that projects exactly to pixel (u, v) at depth z (a power of two)."""
    return ((u - CX) * z / FOCAL, (v - CY) * z / FOCAL, z)


SHARED_QUADS = ((2, 2, 10, 10), (10, 2, 18, 10))         # (x0, y0, x1, y1) in pixels, sharing the edge x = 10


def shared_edges():
    verts, faces = [], []
    for q, (x0, y0, x1, y1) in enumerate(SHARED_QUADS):
        base = len(verts)
        depths = (2.0, 4.0, 2.0, 2.0) if q == 0 else (4.0, 2.0, 2.0, 2.0)
        verts += [at_pixel(x, y, z) for (x, y), z in zip(((x0, y0), (x1, y0), (x1, y1), (x0, y1)), depths)]
        # the first quad is cut along (x0, y0) - (x1, y1), the second along the other diagonal, wound the other way
        faces += [(base, base + 1, base + 2), (base, base + 2, base + 3)] if q == 0 else \
                 [(base + 1, base, base + 3), (base + 1, base + 3, base + 2)]
    return Case("shared edges", verts, faces, seed=1)


def coincident():
    v = [at_pixel(3, 3, 2.0), at_pixel(15, 4, 4.0), at_pixel(6, 14, 2.0)]
    return Case("coincident faces", v + v, [(3, 4, 5), (0, 2, 1), (0, 1, 2)], seed=2)


def behind_near():
    v = [at_pixel(2, 2), at_pixel(12, 3), at_pixel(4, 11), at_pixel(20, 15), at_pixel(28, 16), (0.5, 0.5, 0.25)]
    return Case("vertex behind near", v, [(0, 1, 2), (3, 4, 5)], seed=3)


def beyond_limit():
    v = [at_pixel(2, 2), at_pixel(12, 3), at_pixel(4, 11), at_pixel(20, 15), at_pixel(28, 16), (3.0e5, 0.0, 2.0)]
    return Case("vertex beyond 2^20 pixels", v, [(0, 1, 2), (3, 5, 4)], seed=4)


def zero_area():
    v = [at_pixel(2, 2, 2.0), at_pixel(6, 4, 4.0), at_pixel(10, 6, 2.0),          # collinear on the screen
         at_pixel(20, 10, 2.0), at_pixel(20, 10, 4.0), at_pixel(25, 3, 2.0)]     # two corners on one ray
    return Case("zero screen area", v, [(0, 1, 2), (3, 4, 5), (0, 2, 1)], seed=5)


def whole_image():
    v = [at_pixel(-3000, -2000, 4.0), at_pixel(5000, -2000, 2.0), at_pixel(-3000, 6000, 2.0)]
    return Case("face over the whole image", v, [(0, 1, 2)], seed=6)


def off_image():
    v = [at_pixel(-40, 2), at_pixel(-3, 5), at_pixel(-20, 20),
         at_pixel(3, -30), at_pixel(20, -2), at_pixel(9, -1),
         at_pixel(W + 1, H + 1), at_pixel(W + 30, H + 4), at_pixel(W + 5, H + 40)]
    return Case("faces off the image", v, [(0, 1, 2), (3, 4, 5), (6, 7, 8)], seed=7)


def everything():
    """All cases in one mesh; the whole-image face goes behind the rest, twice as far away along the same rays."""
    verts, faces, offset = [], [], 0
    for case in (whole_image(), shared_edges(), coincident(), behind_near(), beyond_limit(), zero_area(), off_image()):
        verts.append(case.verts * F32(2.0) if not verts else case.verts)
        faces.append(case.faces + np.int32(offset))
        offset += len(case.verts)
    return Case("every hand-built case in one mesh", np.concatenate(verts), np.concatenate(faces), seed=8)


def reversed_winding(case):
    out = Case(case.name + ", winding reversed", case.verts, case.faces[:, [0, 2, 1]], case.K, case.poses, case.near,
               case.H, case.W)
    out.colors = case.colors
    return out


def hand_built():
    base = [shared_edges(), coincident(), behind_near(), beyond_limit(), zero_area(), whole_image(), off_image(), everything()]
    return base + [reversed_winding(c) for c in (shared_edges(), everything())]


# ---- cameras for any mesh -----------------------------------------------------------------------------------

def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """float32 pose (12,) of a camera at `eye` looking at `target`: rows of R are the camera's axes, t = -R eye."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    up = np.asarray(up, np.float64)
    if abs(float(up @ z)) > 0.99:
        up = np.array([0.0, 1.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return np.concatenate([R.reshape(9), -R @ eye]).astype(F32)


AXES = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


def axis_views(distance):
    """Six cameras on the axes at `distance` from the origin, looking at it."""
    return np.stack([look_at(distance * np.array(a, np.float64), (0.0, 0.0, 0.0)) for a in AXES])


def pinhole(focal, H, W):
    """Principal point at (W / 2, H / 2): with odd sizes it falls between pixel centres."""
    return np.array([[focal, 0, W / 2.0], [0, focal, H / 2.0], [0, 0, 1]], F32)


VIEW_DIRECTIONS = ((0.8, -0.5, 0.33), (-0.3, 0.9, -0.31), (0.1, 0.2, -0.97), (-0.7, -0.6, 0.39), (0.0, 0.0, 1.0))


def views_for(verts, n_views, H, W):
    """(K, poses (n_views,12), near) for a mesh: cameras at 2.5 radii of its bounding box round its centre, from
    directions that are no axis (the fifth is one), the sixth INSIDE the box at 0.3 radii off the centre, where faces
    fall behind `near`, project far outside the image or cover all of it."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    lo, hi = (v.min(axis=0), v.max(axis=0)) if len(v) else (np.zeros(3), np.zeros(3))
    centre = (lo + hi) / 2
    radius = max(float(np.linalg.norm(hi - lo)) / 2, 1e-3)
    poses = []
    for d in VIEW_DIRECTIONS:
        d = np.asarray(d, np.float64)
        poses.append(look_at(centre + 2.5 * radius * d / np.linalg.norm(d), centre))
    poses.append(look_at(centre + 0.3 * radius * np.array([0.6, 0.0, 0.8]), centre + radius * np.array([0.0, 1.0, 0.0])))
    return pinhole(0.9 * W, H, W), np.stack(poses[:n_views]), F32(0.05 * radius)


# ---- the visibility scene -----------------------------------------------------------------------------------

def sphere_mesh(n=33):
    return mv.sphere_volume(n).extract()


def concentric_spheres(n=33, scale=0.5):
    """The extracted sphere and a copy scaled by `scale` inside it (face ids offset): (verts, faces, colors, vertices
    of the outer sphere, faces of the outer sphere)."""
    v, f, c = sphere_mesh(n)
    inner = (v * F32(scale)).astype(F32)
    return (np.concatenate([v, inner]), np.concatenate([f, f + np.int32(len(v))]).astype(np.int32), np.concatenate([c, c]),
            len(v), len(f))
