"""The rendering kernels (csrc/amvs_mesh_render.hip; include/amvs.h amvs_mesh_render, amvs_mesh_visibility,
amvs_mesh_filter_visible) against the NumPy restatement (tests/mesh_render_restatement.py), bit for bit: depth maps as
uint32 views, face ids, skipped faces, visibility counts and the filtered mesh element for element.  The meshes are
what the generated volumes of tests/mesh_volumes.py extract (fed through amvs_tsdf_set_volume + amvs_tsdf_extract), the
hand-built meshes of tests/mesh_clean_inputs.py and the inputs of tests/mesh_render_inputs.py (fed through
amvs_mesh_set), which test_mesh_render_cpu.py checks for what they reach."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_inputs as ci  # noqa: E402
import mesh_clean_restatement as cr  # noqa: E402
import mesh_render_inputs as ri  # noqa: E402
import mesh_render_restatement as rr  # noqa: E402
import mesh_volumes as mv  # noqa: E402
from mesh_hip_common import _scene_a_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = ((24, 32), (37, 53))


def _engine(H, W):
    import amvs
    return amvs.Engine(H, W, 1, ri.K_HAND)


def _poses(p):
    return [(q[:9].reshape(3, 3), q[9:]) for q in np.asarray(p, F32).reshape(-1, 12)]


def _assert_maps_equal(got, ref, what):
    for name, a, b in zip(("depth", "face", "skipped"), got, ref):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {name} {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        same = np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else np.array_equal(a, b)
        assert same, f"{what}: {name} differs at {int((a != b).sum())} places, first {np.argwhere(a != b)[:1]}"


def _assert_mesh_equal(mesh, ref, what):
    verts, faces, cols = mesh[:3]
    rv, rf, rc = ref[:3]
    assert (len(verts), len(faces)) == (len(rv), len(rf)), f"{what}: {len(verts)} / {len(faces)} vs {len(rv)} / {len(rf)}"
    assert verts.shape == (len(rv), 3) and faces.shape == (len(rf), 3) and cols.shape == (len(rv), 3)
    assert np.array_equal(faces, rf), f"{what}: faces differ"
    assert np.array_equal(verts.view(np.uint32), np.ascontiguousarray(rv, F32).view(np.uint32)), f"{what}: positions differ"
    assert np.array_equal(cols, rc), f"{what}: colours differ"


class Source:
    """A mesh of the family and the way it reaches the device."""

    def __init__(self, eng, name, arrays=None, volume=None, cameras=None):
        self.eng, self.name, self.volume, self.cameras = eng, name, volume, cameras
        if volume is not None:
            eng.tsdf_set_volume(*volume.arrays())
            arrays = volume.extract()
        self.v, self.f, self.c = arrays

    def reset(self):
        if self.volume is not None:
            self.eng.tsdf_extract()
        else:
            self.eng.mesh_set(self.v, self.f, self.c)


def _sources(eng, H, W):
    for vol in mv.small_volumes():
        yield Source(eng, vol.name, volume=vol)
    for m in ci.hand_built():
        yield Source(eng, m.name, arrays=m.arrays())
    for case in ri.hand_built():
        if (case.H, case.W) == (H, W):
            yield Source(eng, case.name, arrays=case.arrays(), cameras=(case.K, case.poses, case.near))


@pytest.mark.parametrize("H,W", SIZES)
def test_family_bit_exact_on_one_context(H, W):
    """Every mesh of the family on ONE context per image size (the buffers only grow: large meshes come before small
    ones and the empty one), drawn into 1 and into 6 cameras; the counts at tolerance 0 and at one unit (the near
    distance, a twentieth of the mesh's radius); the filter at min_views 1 and 2."""
    n_runs = n_pixels = n_skipped = n_removed = n_emptied = 0
    with _engine(H, W) as eng:
        for src in _sources(eng, H, W):
            for n_views in (1, 6):
                if src.cameras is not None:
                    K, poses, near = src.cameras
                    if n_views == 6:
                        continue
                else:
                    K, poses, near = ri.views_for(src.v, n_views, H, W)
                what = f"{src.name}, {H} x {W}, {n_views} views"
                ref = rr.render(src.v, src.f, K, poses, near, H, W)
                for tol in (F32(0), F32(near)):
                    ref_counts = rr.visibility(src.v, K, poses, near, ref[0], tol)
                    for min_views in (1, 2):
                        src.reset()
                        got = eng.mesh_render(K, _poses(poses), near=near, skipped=True)
                        _assert_maps_equal(got, ref, what)
                        counts = eng.mesh_visibility(tol)
                        assert counts.dtype == np.int32 and np.array_equal(counts, ref_counts), f"{what}, tolerance {tol}: counts"
                        rv, rf, rc = rr.filter_visible(src.v, src.f, src.c, ref_counts, min_views)
                        assert eng.mesh_filter_visible(min_views) == (len(rv), len(rf)), f"{what}, min_views {min_views}"
                        _assert_mesh_equal(eng.mesh_fetch(), (rv, rf, rc), f"{what}, tolerance {tol}, min_views {min_views}")
                        n_runs += 1
                        n_removed += 0 < len(rf) < len(src.f)
                        n_emptied += len(rf) == 0 and len(src.f) > 0
                n_pixels += int((ref[1] >= 0).sum())
                n_skipped += int(ref[2].sum())
        from amvs import _lib
        assert _lib.index_check()[0] == 0
    assert n_runs >= 300 and n_pixels >= 25_000 and n_skipped >= 100_000 and n_removed >= 50 and n_emptied >= 4


def test_maps_do_not_depend_on_the_large_face_threshold():
    """Every face on the workgroup path (threshold 1), none (a huge threshold) and automatic: the same maps.  The
    decimated sphere and the whole-image face have boxes of hundreds of pixels, the extracted sphere of a few."""
    H, W = 37, 53
    sphere = ri.sphere_mesh(33)
    coarse = _decimated(sphere)
    meshes = [("sphere", sphere, ri.views_for(sphere[0], 6, H, W)), ("decimated sphere", coarse, ri.views_for(coarse[0], 6, H, W))]
    with _engine(H, W) as eng:
        for name, (v, f, c), (K, poses, near) in meshes:
            ref = rr.render(v, f, K, poses, near, H, W)
            eng.mesh_set(v, f, c)
            for large in (1, 2 ** 31 - 1, 0, 7):
                eng.set_render_tuning(large)
                _assert_maps_equal(eng.mesh_render(K, _poses(poses), near=near, skipped=True), ref, f"{name}, threshold {large}")
    with _engine(ri.H, ri.W) as eng:
        for case in ri.hand_built():
            ref = rr.render(case.verts, case.faces, case.K, case.poses, case.near, case.H, case.W)
            eng.mesh_set(*case.arrays())
            for large in (1, 2 ** 31 - 1, 0):
                eng.set_render_tuning(large)
                got = eng.mesh_render(case.K, case.pose_list(), near=case.near, skipped=True)
                _assert_maps_equal(got, ref, f"{case.name}, threshold {large}")
        import amvs
        with pytest.raises(amvs.AmvsError, match="set_render_tuning"):
            eng.set_render_tuning(-1)


def _decimated(mesh):
    """The sphere on cells of 6 voxels, by the decimation's own restatement: faces of hundreds of pixels."""
    import mesh_decimate_restatement as dr
    vol = mv.sphere_volume(33)
    return dr.decimate(*mesh, vol.origin, F32(6) * vol.voxel)


def test_concentric_spheres_end_to_end():
    v, f, c, n_outer_v, n_outer_f = ri.concentric_spheres()
    H, W = 37, 53
    K, poses = ri.pinhole(50.0, H, W), ri.axis_views(3.0)
    voxel = mv.sphere_volume(33).voxel
    ref = rr.render(v, f, K, poses, 0.1, H, W)
    ref_counts = rr.visibility(v, K, poses, 0.1, ref[0], voxel)
    with _engine(H, W) as eng:
        eng.mesh_set(v, f, c)
        _assert_maps_equal(eng.mesh_render(K, _poses(poses), near=0.1, skipped=True), ref, "concentric spheres")
        counts = eng.mesh_visibility(voxel)
        assert np.array_equal(counts, ref_counts)
        assert counts[:n_outer_v].min() >= 1 and counts[n_outer_v:].max() == 0
        assert eng.mesh_filter_visible(1) == (n_outer_v, n_outer_f)
        mesh = eng.mesh_fetch()
    _assert_mesh_equal(mesh, (v[:n_outer_v], f[:n_outer_f], c[:n_outer_v]), "the outer sphere")
    assert mv.directed_edge_defects(mesh[1], len(mesh[0])) == (0, 0) and len(mesh[1]) == 2 * len(mesh[0]) - 4


def _run(eng, mesh, cameras, tol, min_views):
    K, poses, near = cameras
    eng.mesh_set(*mesh)
    maps = eng.mesh_render(K, _poses(poses), near=near, skipped=True)
    counts = eng.mesh_visibility(tol)
    sizes = eng.mesh_filter_visible(min_views)
    return maps + (counts, np.asarray(sizes)) + eng.mesh_fetch()


def test_same_bits_twice_and_on_a_fresh_context():
    """The larger mesh in more views before the smaller in fewer (the buffers only grow), the empty mesh between."""
    H, W = 37, 53
    big = mv.random_sign_volume((19, 23, 21), 6, closed=True).extract()
    small = ci.threshold().arrays()
    empty = ci.empty().arrays()
    jobs = [(big, ri.views_for(big[0], 6, H, W), F32(0.01), 2), (empty, ri.views_for(empty[0], 2, H, W), F32(0), 1),
            (small, ri.views_for(small[0], 1, H, W), F32(0), 1)]
    with _engine(H, W) as eng:
        first = [_run(eng, *job) for job in jobs]
        second = [_run(eng, *job) for job in jobs]
    with _engine(H, W) as eng:
        third = [_run(eng, *job) for job in reversed(jobs)][::-1]
    assert len(first[0][-2]) > 0 and (first[0][1] >= 0).sum() > 1000 and (first[1][1] == -1).all()
    assert first[1][4].tolist() == [0, 0]
    for again in (second, third):
        for a, b in zip(again, first):
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def test_argument_and_attribute_rules():
    import amvs
    H, W = ri.H, ri.W
    case = ri.everything()
    K, poses, near = case.K, case.pose_list(), case.near
    with _engine(H, W) as eng:
        with pytest.raises(amvs.AmvsError, match="mesh_render: no mesh"):
            eng.mesh_render(K, poses, near=near)
        eng.mesh_set(*case.arrays())
        for what, call in (("fetch_render: no current render", lambda: eng.mesh_render_fetch(0, 1)),
                           ("mesh_visibility: no current render", lambda: eng.mesh_visibility(0.0)),
                           ("mesh_filter_visible: no current counts", lambda: eng.mesh_filter_visible(1))):
            with pytest.raises(amvs.AmvsError, match=what):
                call()
        with pytest.raises(amvs.AmvsError, match="fetch_mesh_visibility: no current counts"):
            eng._chk(eng._lib.amvs_fetch_mesh_visibility(eng._h, np.zeros(len(case.verts), np.int32).ctypes.data_as(C.POINTER(C.c_int))))
        # the arguments of the render
        with pytest.raises(amvs.AmvsError, match="mesh_render: n_views must be >= 1"):
            eng.mesh_render(K, [], near=near)
        for bad in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf):
            with pytest.raises(amvs.AmvsError, match="mesh_render: near must be positive and finite"):
                eng.mesh_render(K, poses, near=bad)
        for bad in (np.nan, np.inf):
            Kb = K.copy(); Kb[1, 2] = bad
            with pytest.raises(amvs.AmvsError, match="mesh_render: K must be finite"):
                eng.mesh_render(Kb, poses, near=near)
            R, t = poses[0]
            with pytest.raises(amvs.AmvsError, match="mesh_render: pose 1 is not finite"):
                eng.mesh_render(K, [poses[0], (R, np.array([0.0, bad, 0.0]))], near=near)
        too_many = (2 ** 31 - 1) // (H * W) + 1
        with pytest.raises(amvs.AmvsError, match="mesh_render: .* over the limit"):
            eng._chk(_render_raw(eng, too_many, K, near))
        # a refused render leaves no render behind; a good one does
        with pytest.raises(amvs.AmvsError, match="no current render"):
            eng.mesh_render_fetch(0, 1)
        ref = rr.render(case.verts, case.faces, K, case.poses, near, H, W)
        _assert_maps_equal(eng.mesh_render(K, poses, near=near, skipped=True), ref, case.name)
        for first, count in ((-1, 1), (0, 0), (0, 2), (1, 1)):
            with pytest.raises(amvs.AmvsError, match="fetch_render: views"):
                eng.mesh_render_fetch(first, count)
        for bad in (-1.0, np.nan, np.inf):
            with pytest.raises(amvs.AmvsError, match="mesh_visibility: depth_tolerance"):
                eng.mesh_visibility(bad)
        with pytest.raises(amvs.AmvsError, match="no current counts"):
            eng.mesh_filter_visible(1)
        counts = eng.mesh_visibility(0.0)
        assert np.array_equal(counts, rr.visibility(case.verts, K, case.poses, near, ref[0], 0.0))
        for bad in (0, -1):
            with pytest.raises(amvs.AmvsError, match="mesh_filter_visible: min_views must be >= 1"):
                eng.mesh_filter_visible(bad)
        # normals keep the maps and the counts; a new render drops the counts
        eng.mesh_normals()
        _assert_maps_equal(eng.mesh_render_fetch(0, 1), ref[:2], "after the normals")
        eng.mesh_render(K, poses, near=near)
        with pytest.raises(amvs.AmvsError, match="no current counts"):
            eng.mesh_filter_visible(1)
        # every call that replaces or moves the mesh drops both
        origin = np.full(3, -64.0, F32)
        changes = (lambda: eng.mesh_smooth(1), lambda: eng.mesh_smooth(0), lambda: eng.mesh_filter_components(),
                   lambda: eng.mesh_decimate(origin, 1.0), lambda: eng.mesh_decimate_quadric(origin, 1.0),
                   lambda: eng.mesh_set(*case.arrays()), lambda: eng.mesh_filter_visible(1))
        for n, change in enumerate(changes):
            eng.mesh_set(*case.arrays())
            eng.mesh_filter_components(); eng.mesh_normals()
            eng.mesh_render(K, poses, near=near)
            eng.mesh_visibility(0.0)
            change()
            with pytest.raises(amvs.AmvsError, match="fetch_render: no current render"):
                eng.mesh_render_fetch(0, 1)
            with pytest.raises(amvs.AmvsError, match="no current"):
                eng.mesh_filter_visible(1)
        # the filter itself also drops labels and normals
        for flag in (dict(normals=True), dict(labels=True)):
            with pytest.raises(amvs.AmvsError, match="no current"):
                eng.mesh_fetch(**flag)
        # a refused decimation changes nothing: the maps stay
        eng.mesh_set(*case.arrays())
        eng.mesh_render(K, poses, near=near)
        with pytest.raises(amvs.AmvsError, match="outside the cluster grid"):
            eng.mesh_decimate(np.zeros(3, F32), 1e-7)
        _assert_maps_equal(eng.mesh_render_fetch(0, 1), ref[:2], "after the refused decimation")
        # the clean-up works on the filtered mesh as on any other
        counts = eng.mesh_visibility(0.0)
        rv, rf, rc = rr.filter_visible(*case.arrays(), counts, 1)
        assert eng.mesh_filter_visible(1) == (len(rv), len(rf)) and 0 < len(rf) < len(case.faces)
        eng.mesh_smooth(2)
        eng.mesh_normals()
        mesh = eng.mesh_fetch(normals=True)
        sv = cr.smooth(rv, rf, 2)
        _assert_mesh_equal(mesh, (sv, rf, rc), "smoothing after the filter")
        assert np.array_equal(mesh[3].view(np.uint32), cr.normals(sv, rf).view(np.uint32))
        # an empty mesh renders empty maps, has no counts to speak of and filters to nothing
        for mesh_in in (ci.empty().arrays(), ci.vertices_only().arrays()):
            eng.mesh_set(*mesh_in)
            depth, face, skipped = eng.mesh_render(K, poses, near=near, skipped=True)
            assert (depth == 0).all() and (face == -1).all() and skipped.tolist() == [0]
            assert len(eng.mesh_visibility(0.0)) == len(mesh_in[0])
            assert eng.mesh_filter_visible(1) == (0, 0)
            assert [a.shape for a in eng.mesh_fetch()] == [(0, 3), (0, 3), (0, 3)]
        from amvs import _lib
        assert _lib.index_check()[0] == 0


def _render_raw(eng, n_views, K, near):
    """amvs_mesh_render with more views than fit the limit, which is refused before any pose is read: one pose is
    passed."""
    Kf = np.ascontiguousarray(K, F32).reshape(9)
    poses = np.ascontiguousarray(ri.IDENTITY, F32)
    f32p = C.POINTER(C.c_float)
    return eng._lib.amvs_mesh_render(eng._h, n_views, Kf.ctypes.data_as(f32p), poses.ctypes.data_as(f32p), float(near), None)


def test_reconstruct_mesh_visibility_culling(scene_a, capsys):
    """On scene_a: min_visible_views=0 returns what the call without the keyword returns, array for array;
    min_visible_views=2 equals the Engine calls made by hand on that mesh, and with the component filter after it the
    restatements chained; the line is printed."""
    import amvs
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    camera, images, poses, sparse = _scene_a_inputs(scene_a)
    pm = PatchMatchMVS(camera, scale=1.0, patch_size=7, num_iterations=4, num_samples=6, min_views=2, seed=2, device=0)
    base = pm.reconstruct_mesh(images, poses, sparse, max_dim=64)
    capsys.readouterr()
    zero = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, min_visible_views=0)
    assert "visibility" not in capsys.readouterr().out
    assert len(base) == len(zero) == 3
    _assert_mesh_equal(zero, base, "min_visible_views=0")
    v, f, c = base
    assert len(f) > 100
    got = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, min_visible_views=2)
    line = [ln for ln in capsys.readouterr().out.splitlines() if "visibility >=" in ln]
    origin, voxel = pm.last_mesh_grid[:2]
    cams = [(poses[i].R, poses[i].t) for i in pm.last_mesh_views]
    assert len(cams) >= 3
    tol = F32(1.0) * F32(voxel)
    with amvs.Engine(scene_a.H, scene_a.W, 1, pm.K_scaled) as eng:
        eng.mesh_set(v, f, c)
        eng.mesh_render(pm.K_scaled, cams, near=F32(voxel))
        counts = eng.mesh_visibility(tol)
        sizes = eng.mesh_filter_visible(2)
        by_hand = eng.mesh_fetch()
    assert sizes == (len(by_hand[0]), len(by_hand[1])) and len(got) == 3
    _assert_mesh_equal(got, by_hand, "min_visible_views=2")
    # and the hand-made calls are the restatement's
    pp = np.stack([np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)]) for R, t in cams])
    Kf = np.asarray(pm.K_scaled, np.float64).astype(F32)
    depth = rr.render(v, f, Kf, pp.astype(F32), F32(voxel), scene_a.H, scene_a.W)[0]
    ref_counts = rr.visibility(v, Kf, pp.astype(F32), F32(voxel), depth, tol)
    assert np.array_equal(counts, ref_counts)
    ref = rr.filter_visible(v, f, c, ref_counts, 2)
    _assert_mesh_equal(got, ref, "min_visible_views=2 against the restatement")
    print(f"scene_a: {len(f)} faces -> {len(ref[1])} seen by two views")
    assert 0 < len(ref[1]) <= len(f)
    assert len(line) == 1 and f"visibility >= 2 views: {len(f):,} faces -> {len(ref[1]):,}" in line[0], line
    # the component filter runs on what the culling leaves
    both = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, min_visible_views=2, min_component_faces=50)
    _assert_mesh_equal(both, cr.filter(*ref, 50)[1:4], "culling, then the component filter")
    for bad in (-1, 1.5, np.nan):
        with pytest.raises(ValueError, match="min_visible_views"):
            pm.reconstruct_mesh(images, poses, sparse, max_dim=64, min_visible_views=bad)
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="visibility_tolerance_voxels"):
            pm.reconstruct_mesh(images, poses, sparse, max_dim=64, min_visible_views=1, visibility_tolerance_voxels=bad)
