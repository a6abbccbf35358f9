"""Volumes for the hole-filling tests (amvs_tsdf_fill; a helper module, not a conftest; seeded, no GPU): the smallest
shapes at which the fill can go wrong, and the scenes with an analytic truth.

    family()        (name, Volume) pairs: mesh_volumes.random_sign_family() as it is (ragged point counts, an axis of
                    length 2 in each direction, NaN and garbage behind the unobserved points, +-0.0), where nearly
                    everything fills in the first step; the same shapes with 90 % and 97 % of the points unobserved, so that
                    several steps have work; a plane through a layer of -0.0f with a slab unobserved; constant and
                    all-unobserved volumes, where nothing is ever filled; a single observed point, from which the fill
                    grows as an L1 ball that the grid clips; a sphere with a tube unobserved
    large_sphere()  the 160^3 sphere with the same tube: no multiple of anything convenient, 16 000 workgroups
    STEPS, MIN_NEIGHBOURS   what every member runs at
    sphere_with_tube, axis_scene   the scenes of the analytic tests
    fill_cropped    the restatement on the box of the unobserved points, for the large sphere
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_fill_restatement as fr  # noqa: E402
import mesh_render_inputs as ri  # noqa: E402
import mesh_restatement as mr  # noqa: E402
import mesh_volumes as mv  # noqa: E402
from mesh_color_inputs import sphere_colour  # noqa: E402

F32 = np.float32
STEPS = (1, 2, 5)
MIN_NEIGHBOURS = (1, 2, 3, 6)


def hide(volume, hidden, name):
    """The volume with the points of the mask `hidden` unobserved: weight 0 and NaN behind it."""
    tsdf, weight, color = volume.tsdf.copy(), volume.weight.copy(), volume.color.copy()
    tsdf[hidden] = F32(np.nan)
    weight[hidden] = F32(0.0)
    color[hidden] = F32(np.nan)
    return mv.Volume(name, tsdf, weight, color, volume.origin, volume.voxel)


def sphere_with_tube(n, rho=0.2, trunc=0.05):
    """mesh_volumes.sphere_volume(n) with the tube x^2 + y^2 < rho^2, z > 0 unobserved; also the hidden mask."""
    v = mv.sphere_volume(n, trunc=trunc)
    ax = -1.0 + np.arange(n) * 2.0 / (n - 1)
    X, Y, Z = ax[None, None, :], ax[None, :, None], ax[:, None, None]
    hidden = ((X ** 2 + Y ** 2) < rho ** 2) & (Z > 0) & np.ones(v.tsdf.shape, bool)
    return hide(v, hidden, f"sphere {n}^3 without a tube"), hidden


def plane_with_slab():
    """The plane through a layer of -0.0f (mesh_volumes.grid_plane_volume, sign < 0) with the slab of the layers 6 .. 8
    above it unobserved but for their rim i == 0: the points of layer 6 have the -0.0f layer for their only known
    neighbour at step 1, those next to the rim two."""
    v = mv.grid_plane_volume((9, 8, 11), 2, 5, sign=-1.0)
    hidden = np.zeros(v.tsdf.shape, bool)
    hidden[6:9, :, 1:] = True
    return hide(v, hidden, "plane of -0.0f with an unobserved slab")


def single_point(dims=(5, 4, 6), at=(3, 1, 2)):
    """One observed point (i, j, k) = `at` in an otherwise unobserved grid."""
    nx, ny, nz = dims
    tsdf = np.full((nz, ny, nx), np.nan, F32)
    weight = np.zeros(tsdf.shape, F32)
    color = np.full(tsdf.shape + (3,), np.nan, F32)
    i, j, k = at
    tsdf[k, j, i], weight[k, j, i], color[k, j, i] = -0.375, 3.0, (30.0, 60.0, 90.0)
    return mv.Volume(f"single observed point in {nx}x{ny}x{nz}", tsdf, weight, color, (0.0, 0.0, 0.0), 0.5)


def all_unobserved(dims=(6, 5, 3)):
    nx, ny, nz = dims
    tsdf = np.full((nz, ny, nx), np.nan, F32)
    return mv.Volume("all unobserved", tsdf, np.zeros(tsdf.shape, F32), np.full(tsdf.shape + (3,), np.nan, F32), (0.0, 0.0, 0.0), 0.25)


def family():
    out = [(v.name, v) for v in mv.random_sign_family()]
    for unobserved in (0.9, 0.97):
        for n, d in enumerate(mv.RANDOM_SIGN_SHAPES):
            v = mv.random_sign_volume(d, 2024 + n, unobserved=unobserved)
            out.append((f"{v.name} unobserved {unobserved}", v))
    out.append(("plane -0.0f slab", plane_with_slab()))
    out.append(("constant", mv.constant_volume(0.75)))
    out.append(("all unobserved", all_unobserved()))
    out.append(("single point", single_point()))
    out.append(("sphere 33 tube", sphere_with_tube(33)[0]))
    return out


def large_sphere():
    return sphere_with_tube(160)[0]


def fill_cropped(v, steps, min_neighbours=1):
    """The restatement on the box of the unobserved points grown by one point, put back into the whole volume: a step reads
    nothing but the 6-neighbours of unobserved points, so the rest of a large volume need not be walked."""
    hidden = np.argwhere(~(v.weight > 0))
    lo = np.maximum(hidden.min(axis=0) - 1, 0)
    hi = np.minimum(hidden.max(axis=0) + 2, v.weight.shape)
    box = tuple(slice(a, b) for a, b in zip(lo, hi))
    t, w, c, gen, counts = fr.fill(v.tsdf[box], v.weight[box], v.color[box], steps, min_neighbours)
    out = [v.tsdf.copy(), v.weight.copy(), v.color.copy(), (v.weight > 0).astype(np.uint8)]
    for whole, part in zip(out, (t, w, c, gen)):
        whole[box] = part
    return (*out, counts)


def axis_scene(views=6, n=33, H=96, W=128, focal=120.0, distance=3.0, radius=0.8, hole_cos=0.96, background=10.0):
    """A sphere of `radius` ray-cast analytically into the first `views` of mesh_render_inputs.axis_views(distance), as
    mesh_color_inputs.sphere_images casts it; off the sphere the depth is `background` at confidence 3; confidence 0 at
    every pixel whose hit point p has p . (1,1,1)/sqrt(3) / radius > hole_cos.  A mesh_volumes.Scene on an n^3 grid over
    [-1, 1]^3 with min_views 2 and a truncation of 4 voxels."""
    K = ri.pinhole(focal, H, W)
    poses = ri.axis_views(distance)[:views]
    Kd = K.astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    rays = np.stack([(xs - Kd[0, 2]) / focal, (ys - Kd[1, 2]) / focal, np.ones((H, W))], -1)
    axis = np.ones(3) / np.sqrt(3.0)
    depth = np.zeros((views, H, W), F32)
    conf = np.zeros((views, H, W), F32)
    colors = np.zeros((views, H, W, 3), np.uint8)
    for m, pose in enumerate(poses.astype(np.float64)):
        R, t = pose[:9].reshape(3, 3), pose[9:]
        eye = -R.T @ t
        d = rays @ R                                                   # world directions: R^T ray
        a, b, c = (d * d).sum(-1), (d @ eye), eye @ eye - radius * radius
        disc = b * b - a * c
        hit = disc > 0
        s = (-b - np.sqrt(np.where(hit, disc, 0))) / a                 # the rays have z = 1: s is the depth along z
        points = eye + s[..., None] * d
        depth[m] = np.where(hit, s, background)
        conf[m] = np.where(hit & ((points @ axis) / radius > hole_cos), 0.0, 3.0)
        col = np.clip(np.floor(sphere_colour(points) + 0.5), 0, 255)
        colors[m] = np.where(hit[..., None], col, 0).astype(np.uint8)
    voxel = F32(2.0 / (n - 1))
    return mv.Scene(f"sphere in {views} axis views", depth, conf, colors, K, poses, 2.0, (-1.0, -1.0, -1.0), voxel, (n, n, n),
                    F32(4.0) * voxel)


def mesh_report(tsdf, weight, color, origin, voxel, radius=0.8):
    """Of the extracted mesh: vertices, faces, directed_edge_defects, the worst | |v| - radius | and the number of vertices
    more than 2 voxels off the sphere."""
    V, F, _ = mr.extract(tsdf, weight, color, origin, voxel)
    err = np.abs(np.linalg.norm(V.astype(np.float64), axis=1) - radius) if len(V) else np.zeros(0)
    return dict(vertices=len(V), faces=len(F), defects=mv.directed_edge_defects(F, len(V)),
                worst=float(err.max()) if len(err) else 0.0, far=int((err > 2.0 * float(voxel)).sum()))
