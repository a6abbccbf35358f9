"""Volumes and hand-built scenes for the surface-mesh tests (a helper module, not a conftest; seeded, no GPU).

The bit-exact mesh tests elsewhere fuse depth maps of synthetic.make_scene's smooth height field, seen from one side:
46 of the 84 (Kuhn tetrahedron, sign case) pairs never occur in their volumes, no TSDF value is exactly zero, and
the integration's guards are taken a handful of times or never.  The families here are made to reach what that
leaves out.  Volumes go to the device through the test hook amvs_tsdf_set_volume (Engine.tsdf_set_volume):

    random_sign_volume   TSDF uniform in (-1, 1) with exact 0.0 and -0.0, weights from a small integer set, a quarter
                         of the points unobserved with garbage (negative, NaN) behind them; `closed` instead observes
                         every point and sets the outermost layer outside, so that the surface closes inside the box
    sphere_volume        a fully observed sphere, or the same sphere inverted (negative outside)
    grid_plane_volume    an axis-aligned plane exactly through a layer of grid points: t == 0 or t == 1 on every
                         crossing edge, coincident vertices the rule
    cube_volume          the single cube (2, 2, 2) with a given sign pattern of its 8 corners
    constant_volume, lone_edge_volume, colour_tie_volumes   the corner cases
    tet_case_coverage    how often each (tetrahedron, case) pair occurs among the meshed tetrahedra, written against
                         mesh_restatement.KUHN and not against the kernel

Scenes (maps, cameras and a grid for amvs_tsdf_integrate) are built by hand, not by make_scene: exact_scene (all
arithmetic exact, so that pixel ties, sdf == -trunc and sdf / trunc == 1 are hit on whole columns of grid points),
inside_scene (cameras inside the box), content_scene (0, negative, NaN, inf in the maps) and many_maps_scene.
branch_counts restates the integration's guards and counts how often each is taken.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_restatement as mr  # noqa: E402

F32 = np.float32
WEIGHTS = (1, 2, 3, 5, 7)


class Volume:
    def __init__(self, name, tsdf, weight, color, origin, voxel):
        self.name = name
        self.tsdf = np.ascontiguousarray(tsdf, F32)
        self.weight = np.ascontiguousarray(weight, F32)
        self.color = np.ascontiguousarray(color, F32)
        self.origin = np.asarray(origin, F32)
        self.voxel = F32(voxel)
        assert self.weight.shape == self.tsdf.shape and self.color.shape == self.tsdf.shape + (3,)

    @property
    def dims(self):
        nz, ny, nx = self.tsdf.shape
        return nx, ny, nz

    def arrays(self):
        return self.tsdf, self.weight, self.color, self.origin, self.voxel

    def extract(self):
        return mr.extract(*self.arrays())


def _integer_colours(rng, weight):
    """Colour sums a fusion could have produced: the sum of `weight` 8-bit values per channel."""
    w = weight.astype(np.int64)[..., None]
    return rng.integers(0, 255 * np.broadcast_to(w, w.shape[:-1] + (3,)) + 1).astype(F32)


def random_sign_volume(dims, seed, closed=False, zero=0.03, unobserved=0.25):
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    shape = (nz, ny, nx)
    tsdf = rng.uniform(-1.0, 1.0, shape).astype(F32)
    u = rng.random(shape)
    tsdf[u < zero] = F32(0.0)
    tsdf[(u >= zero) & (u < 2 * zero)] = F32(-0.0)
    weight = rng.choice(np.array(WEIGHTS, F32), shape)
    if closed:
        shell = np.ones(shape, bool)
        shell[1:-1, 1:-1, 1:-1] = False
        tsdf[shell] = np.abs(tsdf[shell])                        # 0.0 and -0.0 are outside as well
        tsdf[shell & (tsdf == 0)] = F32(0.5)
    else:
        weight[rng.random(shape) < unobserved] = F32(0.0)
    color = _integer_colours(rng, weight)
    hidden = weight == 0
    garbage = np.where(rng.random(shape) < 0.5, F32(np.nan), -np.abs(tsdf) - F32(0.25)).astype(F32)
    tsdf[hidden] = garbage[hidden]
    color[hidden] = F32(np.nan)
    origin = rng.uniform(-1.0, 1.0, 3).astype(F32)
    voxel = F32(rng.uniform(0.01, 0.2))
    kind = "closed" if closed else "open"
    return Volume(f"random {kind} {nx}x{ny}x{nz} seed {seed}", tsdf, weight, color, origin, voxel)


# ragged shapes (point counts that are no multiple of 256: all but the last), some with an axis of length 2
RANDOM_SIGN_SHAPES = ((23, 19, 17), (2, 31, 29), (33, 2, 27), (35, 26, 2), (5, 3, 4), (16, 16, 16))


def random_sign_family(seed=2024):
    return [random_sign_volume(d, seed + n) for n, d in enumerate(RANDOM_SIGN_SHAPES)]


def _position_colours(shape, weight):
    k, j, i = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    mean = np.stack([(37 * i + 11 * j) % 256, (53 * j + 7 * k) % 256, (29 * k + 5 * i) % 256], -1)
    return (mean * np.asarray(weight)[..., None]).astype(F32)


def sphere_volume(n, radius=0.8, trunc=0.05, inverted=False, center=(0.0, 0.0, 0.0)):
    """n^3 points on [-1, 1]^3, tsdf = clip((|X - center| - radius) / trunc), negated if inverted."""
    origin = np.array([-1.0, -1.0, -1.0], F32)
    voxel = F32(2.0 / (n - 1))
    ax = [(origin[a] + np.arange(n, dtype=np.int64).astype(F32) * voxel).astype(np.float64) - center[a] for a in range(3)]
    r = np.sqrt(ax[0][None, None, :] ** 2 + ax[1][None, :, None] ** 2 + ax[2][:, None, None] ** 2)
    tsdf = np.clip((r - radius) / trunc, -1.0, 1.0).astype(F32)
    del r
    if inverted:
        tsdf = -tsdf
    weight = np.full(tsdf.shape, 2.0, F32)
    color = _position_colours(tsdf.shape, weight)
    return Volume(f"{'inverted ' if inverted else ''}sphere {n}^3", tsdf, weight, color, origin, voxel)


def grid_plane_volume(dims, axis, layer, sign=1.0):
    """tsdf = sign * (index along axis - layer) / 4, clipped: exactly zero on one whole layer of grid points."""
    nx, ny, nz = dims
    idx = np.arange((nx, ny, nz)[axis], dtype=np.float64) - layer
    prof = np.clip(sign * idx / 4.0, -1.0, 1.0).astype(F32)
    if sign < 0:
        prof[layer] = F32(-0.0)
    shape = [1, 1, 1]
    shape[2 - axis] = len(prof)
    tsdf = np.broadcast_to(prof.reshape(shape), (nz, ny, nx)).copy()
    weight = np.full(tsdf.shape, 3.0, F32)
    color = _position_colours(tsdf.shape, weight)
    return Volume(f"plane axis {axis} layer {layer} sign {sign:+.0f} {nx}x{ny}x{nz}", tsdf, weight, color,
                  (0.25, -0.5, 1.0), 0.125)


def cube_volume(pattern, seed=7):
    """The single cube: corner c (bit 0 = +x, 1 = +y, 2 = +z) is inside iff bit c of pattern is set."""
    rng = np.random.default_rng(seed * 256 + pattern)
    mag = rng.uniform(0.05, 1.0, 8).astype(F32)
    f = np.where([(pattern >> c) & 1 for c in range(8)], -mag, mag).astype(F32).reshape(2, 2, 2)
    weight = rng.choice(np.array(WEIGHTS, F32), (2, 2, 2))
    return Volume(f"cube pattern {pattern:#04x}", f, weight, _integer_colours(rng, weight), (0.0, 0.0, 0.0), 1.0)


def constant_volume(value, dims=(7, 5, 6)):
    nx, ny, nz = dims
    tsdf = np.full((nz, ny, nx), value, F32)
    weight = np.ones(tsdf.shape, F32)
    return Volume(f"constant {value}", tsdf, weight, _position_colours(tsdf.shape, weight), (0.0, 0.0, 0.0), 0.1)


def lone_edge_volume(direction, dims=(5, 4, 6)):
    """Two observed neighbours (along lattice direction 1 .. 7) with a sign change, everything else unobserved: the
    edge crosses, no tetrahedron is complete, pass (d) drops the vertex."""
    nx, ny, nz = dims
    tsdf = np.full((nz, ny, nx), np.nan, F32)
    weight = np.zeros(tsdf.shape, F32)
    color = np.zeros(tsdf.shape + (3,), F32)
    a = (2, 1, 1)
    b = (2 + (direction >> 2), 1 + ((direction >> 1) & 1), 1 + (direction & 1))
    for at, f in ((a, -0.5), (b, 0.25)):
        tsdf[at], weight[at], color[at] = f, 1.0, (10.0, 20.0, 30.0)
    return Volume(f"lone edge direction {direction}", tsdf, weight, color, (0.0, 0.0, 0.0), 0.5)


# (t, per channel (mean colour at f < 0, mean colour at f > 0, expected 8-bit colour)): c0 + t (c1 - c0) lands
# exactly on x.5 (rounded up by floorf(c + 0.5f); 2.5 and 6.5 are where round-half-even differs), on 0 and on 255
COLOUR_TIES = ((0.25, ((10, 12, 11), (0, 2, 1), (255, 253, 255))),
               (0.5, ((2, 3, 3), (254, 255, 255), (0, 1, 1))),
               (0.25, ((0, 0, 0), (255, 255, 255), (6, 8, 7))))


def colour_tie_volumes():
    """x-slabs: f = -t on the layers i <= 1, 1 - t beyond, so t = f0 / (f0 - f1) is exactly 0.25 or 0.5 on every
    crossing edge, with constant mean colours on either side (weights 2 and 3)."""
    out = []
    for n, (t, chans) in enumerate(COLOUR_TIES):
        nx, ny, nz = 4, 3, 3
        tsdf = np.empty((nz, ny, nx), F32)
        tsdf[..., :2], tsdf[..., 2:] = -t, 1.0 - t
        weight = np.empty(tsdf.shape, F32)
        weight[..., :2], weight[..., 2:] = 2.0, 3.0
        color = np.empty(tsdf.shape + (3,), F32)
        for ch, (c0, c1, _) in enumerate(chans):
            color[..., :2, ch], color[..., 2:, ch] = 2.0 * c0, 3.0 * c1
        out.append((Volume(f"colour ties {n}", tsdf, weight, color, (0.0, 0.0, 0.0), 0.25),
                    np.array([c[2] for c in chans], np.uint8)))
    return out


def corner_case_volumes():
    """(volume, expected (V, F) or None)."""
    out = [(constant_volume(0.75), (0, 0)), (constant_volume(-0.75), (0, 0)), (constant_volume(-0.0), (0, 0))]
    out += [(lone_edge_volume(d), (0, 0)) for d in range(1, 8)]
    out += [(v, None) for v, _ in colour_tie_volumes()]
    return out


def small_volumes():
    """Every generated volume small enough to compare with the restatement in bulk (the cubes and the large sphere
    are apart)."""
    vols = random_sign_family()
    vols += [random_sign_volume((14, 11, 9), 5, closed=True), random_sign_volume((19, 23, 21), 6, closed=True)]
    vols += [sphere_volume(33, trunc=0.2), sphere_volume(33, trunc=0.2, inverted=True),
             sphere_volume(30, radius=0.6, trunc=0.15, center=(0.1, -0.05, 0.07), inverted=True)]
    vols += [grid_plane_volume((9, 8, 11), 2, 5), grid_plane_volume((9, 8, 11), 2, 5, sign=-1.0),
             grid_plane_volume((12, 7, 6), 0, 4), grid_plane_volume((6, 13, 5), 1, 7, sign=-1.0)]
    vols += [v for v, _ in corner_case_volumes()]
    return vols


def tet_case_coverage(tsdf, weight):
    """counts[t, case]: how many meshed (all four corners observed) Kuhn tetrahedra t have the sign case `case`
    (bit v = local vertex v, in mesh_restatement.KUHN's order, has f < 0)."""
    inside = np.asarray(tsdf, F32) < 0
    obs = np.asarray(weight, F32) > 0
    nz, ny, nx = inside.shape

    def corner(a, c):
        di, dj, dk = c & 1, (c >> 1) & 1, c >> 2
        return a[dk:nz - 1 + dk, dj:ny - 1 + dj, di:nx - 1 + di]

    counts = np.zeros((6, 16), np.int64)
    for t, tet in enumerate(mr.KUHN):
        ok = np.ones((nz - 1, ny - 1, nx - 1), bool)
        case = np.zeros(ok.shape, np.int64)
        for lv, c in enumerate(tet):
            ok &= corner(obs, c)
            case |= corner(inside, c).astype(np.int64) << lv
        counts[t] = np.bincount(case[ok], minlength=16)
    return counts


# ---- mesh properties ---------------------------------------------------------------------------------------

def directed_edge_defects(faces, n_vertices):
    """(directed edges that occur more than once, directed edges whose opposite does not occur exactly once).  Both
    zero: consistently oriented and closed, every undirected edge on exactly two faces, once in each direction."""
    f = np.asarray(faces, np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    n = max(int(n_vertices), 1)
    fwd, counts = np.unique(a * n + b, return_counts=True)
    back = np.unique(b * n + a)
    return int((counts != 1).sum()), int(len(fwd) - np.isin(fwd, back, assume_unique=True).sum())


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    p0, p1, p2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", p0, np.cross(p1, p2)).sum() / 6.0)


# ---- integration scenes ------------------------------------------------------------------------------------

class Scene:
    """Maps, float32 cameras and a grid for amvs_tsdf_integrate / mesh_restatement.integrate."""

    def __init__(self, name, depth, conf, colors, K, poses, min_views, origin, voxel, dims, trunc):
        self.name = name
        self.depth = np.ascontiguousarray(depth, F32)
        self.conf = np.ascontiguousarray(conf, F32)
        self.colors = np.ascontiguousarray(colors, np.uint8)
        self.K = np.asarray(K, F32).reshape(3, 3)
        self.poses = np.asarray(poses, F32).reshape(-1, 12)
        self.min_views, self.origin, self.voxel = F32(min_views), np.asarray(origin, F32), F32(voxel)
        self.dims, self.trunc = tuple(int(d) for d in dims), F32(trunc)
        self.n, self.H, self.W = self.depth.shape
        assert self.conf.shape == self.depth.shape and self.colors.shape == self.depth.shape + (3,)
        assert len(self.poses) == self.n

    def pose_list(self):
        return [(p[:9].reshape(3, 3), p[9:]) for p in self.poses]

    def integrate(self, order=None):
        o = np.arange(self.n) if order is None else np.asarray(order)
        return mr.integrate(self.depth[o], self.conf[o], self.colors[o], self.K, self.poses[o], self.min_views,
                            self.origin, self.voxel, self.dims, self.trunc)


def _pose(R=None, t=(0.0, 0.0, 0.0)):
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    return np.concatenate([R.reshape(9), np.asarray(t, np.float64)]).astype(F32)


def _rot(ax, ay, az=0.0):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _random_colours(rng, n, H, W):
    return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def exact_scene(cx, seed=1):
    """Identity rotations, focal length 16, principal point (cx, 6) with cx an integer or a half-integer, grid origin
    and voxel, depths and trunc powers of two (or sums of two).  On the layer Z = 2, u = 8 X + cx and v = 8 Y + 6 are
    multiples of 1/2: u + 0.5 is an integer on every other column of grid points (floorf(u + 0.5f) against round-half-
    even), u == -0.5 (pixel 0, inside) and u == W - 0.5 (pixel W, outside) both occur.  Neighbouring pixels hold
    different depths, so the pixel a tie goes to shows in the volume.  Map 0 (depths 2 and 4, trunc 1/4): sdf ==
    -trunc on the layer Z = 2.25 (kept, value -1), sdf / trunc == 1 on Z = 1.75, clamped before it.  Map 1 is map 0
    shifted by a quarter voxel in x and y (other columns tie).  Maps 2 .. 7 look at the layer where zc == 0.5, shifted
    so that they reach the layers Z = 0.5 .. 0.6875 and even as well as odd pixels: there a grid step is two pixels,
    and the depths 0.25 (sdf == -trunc: kept) and 0.25 - 2^-25 (sdf one ulp beyond -trunc: cut) alternate in blocks
    of 2 x 2 pixels, so that the sampled pixels hold both."""
    rng = np.random.default_rng(seed)
    H, W = 12, 16
    K = np.array([[16.0, 0, cx], [0, 16.0, 6.0], [0, 0, 1]], F32)
    voxel = F32(1.0 / 16)
    first_i = int(round((cx + 0.5) * 2))                          # u(i = 0) = -0.5 on the layer Z = 2
    origin = np.array([-first_i / 16.0, -1.0, 0.5], F32)
    dims = (2 * W + 4, 30, 34)                                    # Z = 0.5 .. 2.5625
    near = ((0, 0, 0), (1, 1, 1), (1, 0, 2), (0, 1, 3), (1, 0, 0), (0, 1, 1))   # t = (a / 32, b / 32, -c / 16)
    depth = np.empty((2 + len(near), H, W), F32)
    col, row = np.arange(W)[None, :], np.arange(H)[:, None]
    depth[0] = np.where((col + row) % 2 == 0, 2.0, 4.0)
    depth[1] = np.where((col + row) % 3 == 0, 2.0, 2.125)
    depth[2:] = np.where((col // 2 + row // 2) % 2 == 0, 0.25, 0.25 - 2.0 ** -25)
    conf = np.full(depth.shape, 2.0, F32)
    poses = np.stack([_pose(), _pose(t=(1.0 / 64, 1.0 / 64, 0.0))] +
                     [_pose(t=(a / 32.0, b / 32.0, -c / 16.0)) for a, b, c in near])
    return Scene(f"exact cx={cx}", depth, conf, _random_colours(rng, len(depth), H, W), K, poses, 2.0, origin, voxel,
                 dims, 0.25)


def inside_scene(seed=2):
    """Cameras inside the box.  Map 0: the centre on a grid layer (zc == 0 exactly on it, negative behind it).  Map 1:
    t_z = 2^-100 over a layer at Z = 0, so zc is tiny and pu / pw around 2^100: the float comparison must reject the
    pixel before any cast to int.  Map 2: t_z = 2^-126, where the quotient overflows to inf.  Map 3: a rotated camera
    at a point that is no grid point."""
    rng = np.random.default_rng(seed)
    H, W = 20, 24
    K = np.array([[16.0, 0, 12.0], [0, 16.0, 10.0], [0, 0, 1]], F32)
    voxel = F32(0.125)
    origin = np.array([-1.5, -1.25, 0.0], F32)
    dims = (25, 21, 19)                                           # Z = 0 .. 2.25
    R3 = _rot(0.3, -0.4, 0.2)
    poses = np.stack([_pose(t=(0.0, 0.0, -0.75)), _pose(t=(0.0, 0.0, 2.0 ** -100)), _pose(t=(0.0, 0.0, 2.0 ** -126)),
                      _pose(R3, -R3 @ np.array([0.3, -0.2, 1.1]))])
    depth = rng.uniform(0.4, 1.6, (4, H, W)).astype(F32)
    conf = np.full(depth.shape, 3.0, F32)
    return Scene("camera inside the box", depth, conf, _random_colours(rng, 4, H, W), K, poses, 1.0, origin, voxel, dims, 0.5)


def content_scene(seed=3):
    """Valid views of a wall at depth about 2 whose maps hold, in blocks of pixels, depth 0, -0.0, negative, NaN and
    +inf and confidence NaN, +inf, exactly min_views, and the float just below min_views."""
    rng = np.random.default_rng(seed)
    H, W = 30, 40
    n = 3
    K = np.array([[40.0, 0, 19.5], [0, 40.0, 14.5], [0, 0, 1]], F32)
    depth = (2.0 + 0.05 * rng.standard_normal((n, H, W))).astype(F32)
    conf = rng.choice(np.array([3.0, 4.0, 5.0], F32), (n, H, W))
    mv = F32(3.0)
    bad_depth = (0.0, -0.0, -1.5, np.nan, np.inf)
    bad_conf = (np.nan, np.inf, mv, np.nextafter(mv, F32(0)), 2.0)
    for m in range(n):
        for q in range(24):
            y, x = rng.integers(0, H - 4), rng.integers(0, W - 4)
            if q % 2 == 0:
                depth[m, y:y + 4, x:x + 4] = bad_depth[(q // 2 + m) % 5]
            else:
                conf[m, y:y + 4, x:x + 4] = bad_conf[(q // 2 + m) % 5]
    poses = np.stack([_pose(), _pose(_rot(0.0, 0.1), (-0.2, 0.0, 0.05)), _pose(_rot(-0.08, -0.05), (0.1, 0.1, 0.0))])
    return Scene("depth and confidence content", depth, conf, _random_colours(rng, n, H, W), K, poses, mv,
                 (-0.9, -0.7, 1.6), 0.05, (37, 29, 17), 0.15)


def many_maps_scene(n=17, seed=4):
    """n >= 16 maps of the wall Z = 2, from cameras that slide along x (so that a grid point is seen by any number of
    them from 0 to n) with small rotations: weights up to n, means that divide by 3, 5, 7, ..."""
    rng = np.random.default_rng(seed)
    H, W = 24, 32
    K = np.array([[32.0, 0, 15.5], [0, 32.0, 11.5], [0, 0, 1]], F32)
    Kinv = np.linalg.inv(K.astype(np.float64))
    ys, xs = np.mgrid[0:H, 0:W]
    rays = np.stack([xs, ys, np.ones_like(xs)], -1).reshape(-1, 3) @ Kinv.T
    poses, depth = [], []
    for m in range(n):
        R = _rot(0.02 * rng.standard_normal(), 0.02 * rng.standard_normal(), 0.02 * rng.standard_normal())
        C = np.array([-0.6 + 1.2 * m / (n - 1), 0.05 * rng.standard_normal(), 0.02 * rng.standard_normal()])
        poses.append(_pose(R, -R @ C))
        world = rays @ R                                          # R^T ray, as rows
        lam = (2.0 - C[2]) / world[:, 2]                          # C + lam R^T ray on Z = 2; depth = lam (ray z = 1)
        depth.append(lam.reshape(H, W))
    depth = np.stack(depth).astype(F32)
    conf = np.full(depth.shape, 2.0, F32)
    return Scene(f"{n} maps", depth, conf, _random_colours(rng, n, H, W), K, np.stack(poses), 2.0,
                 (-1.8, -0.4, 1.7), 0.05, (73, 17, 13), 0.2)


def integration_scenes():
    return [exact_scene(8.0), exact_scene(7.5), inside_scene(), content_scene(), many_maps_scene()]


BRANCHES = ("behind", "zc_zero", "huge", "outside", "tie", "tie_first", "tie_last", "no_depth", "depth_neg_zero",
            "depth_nan", "depth_inf", "low_conf", "conf_nan", "conf_below", "conf_at_min", "conf_inf", "cut", "beyond_cut",
            "at_cut", "clamped", "at_one", "kept")


def branch_counts(sc):
    """How often each guard of the integration is taken, and each of its edges met, over all (grid point, map) visits,
    with the restatement's float32 arithmetic.  A visit is counted at a guard only if it passed the guards before it.

        behind      zc <= 0;  zc_zero: zc == 0 exactly, among them
        huge        in front, |u| or |v| at least 2^31 or not finite: a cast to int before the range test would be
                    undefined
        outside     the pixel is outside the image
        tie         in front, u + 0.5 or v + 0.5 exactly an integer while u or v is not: where floorf(x + 0.5f) and
                    round-half-even can part;  tie_first: u or v == -0.5 (pixel 0, inside);  tie_last: u == W - 0.5
                    or v == H - 0.5 (pixel W or H, outside)
        no_depth    depth <= 0 or NaN;  depth_neg_zero, depth_nan: depth -0.0 or NaN, among them;  depth_inf: depth
                    +inf (goes on)
        low_conf    confidence < min_views or NaN;  conf_nan, conf_below: confidence NaN or the float just below
                    min_views, among them;  conf_at_min, conf_inf: confidence exactly min_views or +inf (go on)
        cut         sdf < -trunc;  beyond_cut: sdf exactly one ulp beyond -trunc, among them;  at_cut: sdf == -trunc
                    (kept)
        clamped     sdf / trunc > 1;  at_one: sdf / trunc == 1
        kept        the visits that add to the sums"""
    X, Y, Z = mr.grid_coords(sc.origin, sc.voxel, sc.dims)
    Kf = sc.K.reshape(9)
    out = dict.fromkeys(BRANCHES, 0)
    half = F32(0.5)
    with np.errstate(all="ignore"):
        for m in range(sc.n):
            R = sc.poses[m]
            zc = ((R[6] * X + R[7] * Y) + R[8] * Z) + R[11]
            xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + R[9]
            yc = ((R[3] * X + R[4] * Y) + R[5] * Z) + R[10]
            pu = (Kf[0] * xc + Kf[1] * yc) + Kf[2] * zc
            pv = (Kf[3] * xc + Kf[4] * yc) + Kf[5] * zc
            pw = (Kf[6] * xc + Kf[7] * yc) + Kf[8] * zc
            u, v = pu / pw, pv / pw
            front = zc > 0
            out["behind"] += int((~front).sum())
            out["zc_zero"] += int((zc == 0).sum())
            out["huge"] += int((front & ~((np.abs(u) < F32(2.0 ** 31)) & (np.abs(v) < F32(2.0 ** 31)))).sum())
            tie = np.zeros(front.shape, bool)
            for x in (u, v):
                tie |= np.isfinite(x) & (np.floor(x + half) == x + half) & (np.floor(x) != x)
            out["tie"] += int((front & tie).sum())
            out["tie_first"] += int((front & ((u == -half) | (v == -half))).sum())
            out["tie_last"] += int((front & ((u == F32(sc.W) - half) | (v == F32(sc.H) - half))).sum())
            fx, fy = np.floor(u + half), np.floor(v + half)
            inimg = (fx >= 0) & (fx < F32(sc.W)) & (fy >= 0) & (fy < F32(sc.H))
            out["outside"] += int((front & ~inimg).sum())
            ok = front & inimg
            px = np.where(ok, fx, 0).astype(np.int64)
            py = np.where(ok, fy, 0).astype(np.int64)
            d, c = sc.depth[m][py, px], sc.conf[m][py, px]
            has_d = d > 0
            out["no_depth"] += int((ok & ~has_d).sum())
            out["depth_neg_zero"] += int((ok & (d == 0) & np.signbit(d)).sum())
            out["depth_nan"] += int((ok & np.isnan(d)).sum())
            ok &= has_d
            out["depth_inf"] += int((ok & np.isinf(d)).sum())
            has_c = c >= sc.min_views
            out["low_conf"] += int((ok & ~has_c).sum())
            out["conf_nan"] += int((ok & np.isnan(c)).sum())
            out["conf_below"] += int((ok & (c == np.nextafter(sc.min_views, F32(0)))).sum())
            ok &= has_c
            out["conf_at_min"] += int((ok & (c == sc.min_views)).sum())
            out["conf_inf"] += int((ok & np.isinf(c)).sum())
            sdf = d - zc
            cut = sdf < -sc.trunc
            out["cut"] += int((ok & cut).sum())
            out["beyond_cut"] += int((ok & (sdf == np.nextafter(-sc.trunc, F32(-np.inf)))).sum())
            out["at_cut"] += int((ok & (sdf == -sc.trunc)).sum())
            ok &= ~cut
            q = sdf / sc.trunc
            out["clamped"] += int((ok & (q > 1)).sum())
            out["at_one"] += int((ok & (q == 1)).sum())
            out["kept"] += int(ok.sum())
    return out
