"""Surface mesh on the GPU (csrc/amvs_mesh.hip, include/amvs.h amvs_tsdf_*, PatchMatchMVS.reconstruct_mesh).  No
reference counterpart: the device volume and mesh are compared bit for bit with the NumPy restatement
(tests/mesh_restatement.py) and the geometry with the synthetic scenes' analytic surface."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_restatement as mr  # noqa: E402
from mesh_hip_common import _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

AMP = 0.15                      # make_scene's height field Z = AMP sin(1.3 X) cos(1.7 Y)


def _surface_z(X, Y):
    return AMP * np.sin(1.3 * X) * np.cos(1.7 * Y)


def _poses32(R, t):
    return np.stack([np.concatenate([np.asarray(r, np.float64).reshape(9), np.asarray(tt, np.float64).reshape(3)])
                     for r, tt in zip(R, t)]).astype(np.float32)


def _world_points(depth, K, R, t):
    """GT depth of one view -> world points (float64)."""
    H, W = depth.shape
    ys, xs = np.mgrid[0:H, 0:W]
    rays = np.stack([xs, ys, np.ones_like(xs)], -1).reshape(-1, 3) @ np.linalg.inv(K).T
    Xc = rays * depth.reshape(-1, 1)
    return (Xc - t) @ R


def _check_volume(eng, depth, conf, colors, K, poses, min_views, origin, voxel, dims, trunc, what):
    tsdf, weight, color = eng.tsdf_volume()
    rt, rw, rc = mr.integrate(depth, conf, colors, K, poses, min_views, origin, voxel, dims, trunc)
    assert np.any(rw > 0), f"{what}: nothing observed (test set-up)"
    assert _same_bits(weight, rw), f"{what}: weight differs in {int((weight != rw).sum())} points"
    assert _same_bits(tsdf, rt), f"{what}: tsdf differs in {int((tsdf != rt).sum())} points"
    assert _same_bits(color, rc), f"{what}: colour sums differ"
    return tsdf, weight, color


def _check_mesh(mesh, tsdf, weight, color, origin, voxel, what):
    verts, faces, cols = mesh
    rv, rf, rcol = mr.extract(tsdf, weight, color, origin, voxel)
    assert len(rf) > 0, f"{what}: empty mesh (test set-up)"
    assert verts.shape == rv.shape and faces.shape == rf.shape, f"{what}: {len(verts)}/{len(faces)} vs {len(rv)}/{len(rf)}"
    assert _same_bits(verts, rv), f"{what}: vertex positions differ"
    assert np.array_equal(faces, rf), f"{what}: faces differ"
    assert np.array_equal(cols, rcol), f"{what}: vertex colours differ"


def _scene_a_box(scene_a, pad=0.1):
    pts = np.concatenate([_world_points(scene_a.gt_depth[i], scene_a.K, scene_a.R[i], scene_a.t[i])
                          for i in range(scene_a.n)])
    return pts.min(0) - pad, pts.max(0) + pad


def test_volume_and_mesh_bit_exact_on_ground_truth_maps(scene_a):
    """scene_a's GT depth maps, host and device maps, host and resident colours, a regular and a ragged grid."""
    import torch
    K = scene_a.K32()
    poses = _poses32(scene_a.R, scene_a.t)
    pose_list = [(scene_a.R[i], scene_a.t[i]) for i in range(scene_a.n)]
    depth = scene_a.gt_depth.astype(np.float32)
    conf = np.full(depth.shape, 3.0, np.float32)
    conf[:, :4] = 1.0                                            # a band below min_views
    colors = np.stack(scene_a.colors)
    lo, hi = _scene_a_box(scene_a)
    with scene_a.engine() as eng:
        for dims in ((40, 40, 40), (37, 53, 29)):
            voxel = np.float32((hi - lo).max() / (max(dims) - 1))
            trunc = np.float32(3.0 * voxel)
            origin = lo.astype(np.float32)
            mesh = eng.tsdf_mesh(K, pose_list, 2, origin, voxel, dims, trunc, depth=depth, conf=conf, colors_bgr=colors)
            vol = _check_volume(eng, depth, conf, colors, K, poses, 2, origin, voxel, dims, trunc, f"host maps {dims}")
            _check_mesh(mesh, *vol, origin, voxel, f"host maps {dims}")
        # device maps + resident colour images (view ids in another order than the maps)
        for i in range(scene_a.n):
            eng.set_view_colors(i, colors[i])
        order = [3, 1, 4, 0, 2]
        d_t = torch.from_numpy(depth[order]).cuda()
        c_t = torch.from_numpy(conf[order]).cuda()
        torch.cuda.synchronize()
        mesh = eng.tsdf_mesh(K, [pose_list[i] for i in order], 2, origin, voxel, dims, trunc,
                             device_ptrs=(d_t.data_ptr(), c_t.data_ptr(), len(order)), view_ids=order)
        vol = _check_volume(eng, depth[order], conf[order], colors[order], K, poses[order], 2, origin, voxel, dims, trunc,
                            "device maps, resident colours")
        _check_mesh(mesh, *vol, origin, voxel, "device maps, resident colours")


def test_volume_bit_exact_on_a_box_the_views_see_partly(scene_a):
    K = scene_a.K32()
    poses = _poses32(scene_a.R, scene_a.t)
    pose_list = [(scene_a.R[i], scene_a.t[i]) for i in range(scene_a.n)]
    depth = scene_a.gt_depth.astype(np.float32)
    conf = np.full(depth.shape, 4.0, np.float32)
    colors = np.stack(scene_a.colors)
    lo, hi = _scene_a_box(scene_a)
    size = hi - lo
    lo2, hi2 = lo - 1.5 * size, hi + 0.5 * size                   # most of it outside some frustum or behind the surface
    dims = (31, 26, 33)
    voxel = np.float32((hi2 - lo2).max() / (max(dims) - 1))
    origin = lo2.astype(np.float32)
    trunc = np.float32(2.5 * voxel)
    with scene_a.engine() as eng:
        mesh = eng.tsdf_mesh(K, pose_list, 3, origin, voxel, dims, trunc, depth=depth, conf=conf, colors_bgr=colors)
        tsdf, weight, color = _check_volume(eng, depth, conf, colors, K, poses, 3, origin, voxel, dims, trunc, "partial box")
        assert 0 < (weight == 0).mean() < 1 and len(np.unique(weight)) > 2   # unobserved points and partial view counts
        if len(mesh[1]):
            _check_mesh(mesh, tsdf, weight, color, origin, voxel, "partial box")


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_volume_and_mesh_bit_exact_on_patchmatch_maps(scene_a, mode):
    from amvs.engine import make_pm_params
    K = scene_a.K32()
    poses = _poses32(scene_a.R, scene_a.t)
    colors = np.stack(scene_a.colors)
    refs = [0, 1, 2, 3, 4]
    srcs = [[j for j in range(scene_a.n) if j != r][:4] for r in refs]
    lo, hi = _scene_a_box(scene_a)
    dims = (45, 38, 41)
    voxel = np.float32((hi - lo).max() / (max(dims) - 1))
    origin = lo.astype(np.float32)
    trunc = np.float32(4.0 * voxel)
    with scene_a.engine(mode=mode) as eng:
        p = make_pm_params(7, 2, 4, scene_a.depth_min, scene_a.depth_max)
        depth, _, conf = eng.patchmatch(refs, srcs, p, seed=5)
        mesh = eng.tsdf_mesh(K, [(scene_a.R[i], scene_a.t[i]) for i in refs], 2, origin, voxel, dims, trunc,
                             depth=depth, conf=conf, colors_bgr=colors[refs])
        vol = _check_volume(eng, depth, conf, colors[refs], K, poses[refs], 2, origin, voxel, dims, trunc, f"PatchMatch ({mode})")
        _check_mesh(mesh, *vol, origin, voxel, f"PatchMatch ({mode})")


def _edge_counts(faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0, return_counts=True)


def test_ground_truth_geometry_of_a_height_field():
    """GT depth maps of make_scene: the mesh lies on Z = amp sin(1.3X) cos(1.7Y), is a manifold inside the box
    and faces the cameras."""
    import amvs
    from amvs.synthetic import make_scene
    sc = make_scene(8, 360, 480, seed=5, amp=AMP)
    K = sc.camera.K.astype(np.float32)
    n = len(sc.depths)
    depth = np.stack(sc.depths).astype(np.float32)
    conf = np.full(depth.shape, 3.0, np.float32)
    colors = np.stack(sc.colors)
    voxel = np.float32(0.03)
    origin = np.array([-0.8, -0.6, -0.3], np.float32)
    dims = (54, 41, 21)
    trunc = np.float32(4 * voxel)
    with amvs.Engine(360, 480, n, K) as eng:
        verts, faces, _ = eng.tsdf_mesh(K, [(sc.poses[i].R, sc.poses[i].t) for i in range(n)], 3, origin, voxel, dims,
                                        trunc, depth=depth, conf=conf, colors_bgr=colors)
    v = verts.astype(np.float64)
    hi = origin + (np.array(dims) - 1) * voxel
    margin = 2 * voxel
    inner = ((v[:, 0] > origin[0] + margin) & (v[:, 0] < hi[0] - margin) &
             (v[:, 1] > origin[1] + margin) & (v[:, 1] < hi[1] - margin))
    assert inner.sum() > 1000
    dist = np.abs(v[inner, 2] - _surface_z(v[inner, 0], v[inner, 1]))      # vertical: >= the normal distance
    assert np.median(dist) <= 0.25 * voxel, np.median(dist) / voxel
    assert dist.max() <= 1.0 * voxel, dist.max() / voxel
    edges, counts = _edge_counts(faces)
    interior_edge = inner[edges[:, 0]] & inner[edges[:, 1]]
    assert np.all(counts[interior_edge] == 2)
    assert counts.max() == 2
    nrm = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    fin = inner[faces].all(axis=1)
    assert (nrm[fin, 2] < 0).mean() >= 0.99                            # the cameras are at Z < 0


def _sparse_points(sc, view=0, step=9):
    """A sparse cloud on the surface (what SfM hands the dense stage): GT depth of every step-th pixel of one view."""
    d = sc.depths[view][::step, ::step]
    K = sc.camera.K
    ys, xs = np.mgrid[0:sc.depths[view].shape[0]:step, 0:sc.depths[view].shape[1]:step]
    rays = np.stack([xs, ys, np.ones_like(xs)], -1).reshape(-1, 3) @ np.linalg.inv(K).T
    R, t = sc.poses[view].R, sc.poses[view].t
    return (rays * d.reshape(-1, 1) - t) @ R


@pytest.mark.parametrize("mode", ["exact", "fast", "extended"])
def test_reconstruct_mesh_end_to_end(mode, tmp_path):
    """reconstruct_mesh on the resident path in both arithmetic modes of the reference's algorithm and in the extended
    mode.  The surface is checked against the analytic height field in the extended mode only: the reference's
    algorithm converges on a few per cent of the pixels, and measured on this scene only 13 %
    of its mesh vertices lie within 2 voxels of the surface, against 100 % in the extended mode."""
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    from amvs.core.utils import save_mesh_ply
    from amvs.synthetic import make_scene
    sc = make_scene(8, 120, 160, seed=3, amp=AMP)
    sparse = _sparse_points(sc)

    def make():
        return PatchMatchMVS(sc.camera, scale=1.0, patch_size=7, num_iterations=4, num_samples=6, min_views=3,
                             seed=2, device=0, mode="exact" if mode == "extended" else mode, extended=mode == "extended")

    pm = make()
    verts, faces, cols = pm.reconstruct_mesh(sc.images(), sc.poses, sparse, max_dim=96)
    assert len(verts) > 100 and len(faces) > 100
    assert verts.dtype == np.float32 and faces.dtype == np.int32 and cols.dtype == np.uint8
    assert np.array_equal(np.unique(faces), np.arange(len(verts)))       # every vertex on a face
    save_mesh_ply(verts, faces, cols, str(tmp_path / "mesh.ply"))
    assert os.path.getsize(tmp_path / "mesh.ply") > 15 * len(verts)
    # the mesh leaves reconstruct() as it was: same cloud as a fresh object's
    pts, rgb = pm.reconstruct(sc.images(), sc.poses, sparse)
    pts2, rgb2 = make().reconstruct(sc.images(), sc.poses, sparse)
    assert len(pts) > 0 and np.array_equal(pts, pts2) and np.array_equal(rgb, rgb2)
    if mode != "extended":
        return
    # on the analytic surface, to 2 voxels of the grid reconstruct_mesh chose from that cloud
    voxel = PatchMatchMVS._mesh_grid(pts, None, None, 4.0, 96)[1]
    v = verts.astype(np.float64)
    dist = np.abs(v[:, 2] - _surface_z(v[:, 0], v[:, 1]))
    assert (dist <= 2 * voxel).mean() >= 0.9, ((dist <= 2 * voxel).mean(), voxel)


def test_volume_over_budget_is_a_clear_error(scene_a):
    import amvs
    from amvs import _lib
    K = scene_a.K32()
    depth = scene_a.gt_depth.astype(np.float32)
    conf = np.full(depth.shape, 3.0, np.float32)
    pose_list = [(scene_a.R[i], scene_a.t[i]) for i in range(scene_a.n)]
    with scene_a.engine() as eng:
        for dims in ((1024, 1024, 1024), (513, 512, 512)):
            assert np.prod(dims) > _lib.TSDF_MAX_POINTS
            with pytest.raises(amvs.AmvsError, match="over the budget"):
                eng.tsdf_integrate(K, pose_list, 2, (0, 0, 0), 0.01, dims, 0.04, depth=depth, conf=conf,
                                   colors_bgr=np.stack(scene_a.colors))
        with pytest.raises(amvs.AmvsError, match="no volume"):
            eng.tsdf_extract()
        # the context still works
        mesh = eng.tsdf_mesh(K, pose_list, 2, (-1, -1, 3), 0.1, (21, 21, 21), 0.3, depth=depth, conf=conf,
                             colors_bgr=np.stack(scene_a.colors))
        assert mesh[0].dtype == np.float32
