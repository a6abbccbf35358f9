"""The texture kernels (csrc/amvs_mesh_texture.hip; include/amvs.h amvs_mesh_texture, amvs_fetch_mesh_texture,
amvs_fetch_render_texture) against the NumPy restatement (tests/mesh_texture_restatement.py), byte for byte: the atlas,
the UVs, both counts and the textured render.  The family is that of tests/mesh_texture_inputs.py, which
test_mesh_texture_cpu.py checks for what it reaches; every mesh goes to the device through amvs_mesh_set, the maps are
the device's own (compared with their restatement in test_hip_mesh_render.py)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_restatement as cr  # noqa: E402
import mesh_color_inputs as ki  # noqa: E402
import mesh_color_restatement as kr  # noqa: E402
import mesh_render_inputs as ri  # noqa: E402
import mesh_render_restatement as rr  # noqa: E402
import mesh_texture_inputs as ti  # noqa: E402
import mesh_texture_restatement as tr  # noqa: E402
from mesh_hip_common import _assert_mesh_equal, _scene_a_inputs, _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
SLOTS = 6                                       # resident colour images of a context


def _engine(H, W):
    import amvs
    return amvs.Engine(H, W, SLOTS, ri.K_HAND)


def _poses(p):
    return [(q[:9].reshape(3, 3), q[9:]) for q in np.asarray(p, F32).reshape(-1, 12)]


@functools.lru_cache(maxsize=None)
def _family(H, W):
    return ti.family(H, W)


def _index_clean():
    from amvs import _lib
    assert _lib.index_check()[0] == 0


def _assert_texture(got, ref, what):
    atlas, uv, n_textured = got
    assert atlas.dtype == np.uint8 and atlas.shape == ref[0].shape, f"{what}: atlas {atlas.shape} vs {ref[0].shape}"
    assert np.array_equal(atlas, ref[0]), f"{what}: {int((atlas != ref[0]).any(axis=2).sum())} texels differ"
    assert _same_bits(uv, ref[1]), f"{what}: UVs differ"
    assert n_textured == ref[3], f"{what}: n_textured {n_textured} vs {ref[3]}"


@pytest.mark.parametrize("H,W", ti.SIZES)
def test_family_byte_exact_on_one_context(H, W):
    """Every job of the family on ONE context per image size, the calls chained: atlases of all sizes follow each other in
    the same grow-only buffers, the largest of a mesh first.  Host images and resident ones (uploaded in reversed slot
    order, so that the view ids matter) alternate.  Every texture is followed by the textured render of all its views and
    of the last alone."""
    import amvs
    jobs, refused = _family(H, W)
    n_textured = n_fallen = n_pixels = 0
    with _engine(H, W) as eng:
        current = None
        for turn, job in enumerate(jobs):
            mem, n = job.mem, job.n
            if current != (id(mem), n):
                if current is None or current[0] != id(mem):
                    eng.mesh_set(mem.verts, mem.faces, mem.colors)
                    for j in range(len(mem.images)):
                        eng.set_view_colors(SLOTS - 1 - j, mem.images[j])
                eng.mesh_render(mem.K, _poses(mem.poses[:n]), near=mem.near, fetch=False)
                current = (id(mem), n)
            src = dict(view_ids=[SLOTS - 1 - j for j in range(n)]) if turn % 2 else dict(colors_bgr=mem.images[:n])
            got = eng.mesh_texture(job.tolerance, job.N, job.min_cos, job.best, job.cells_per_row, **src)
            ref = job.reference()
            _assert_texture(got, ref, str(job))
            assert eng.last_texture_texels == ref[2] == len(mem.faces) * ((job.N + 1) * (job.N + 2) // 2 + job.N), str(job)
            pic = job.render_reference()
            out = eng.mesh_render_texture(0, n)
            assert out.dtype == np.uint8 and out.shape == pic.shape and np.array_equal(out, pic), f"{job}: textured render"
            assert np.array_equal(eng.mesh_render_texture(n - 1, 1), pic[n - 1:])
            n_textured += ref[3]
            n_fallen += ref[2] - ref[3]
            n_pixels += int(pic.any(axis=3).sum())
        for mem, N, cpr in refused[:6]:
            eng.mesh_set(mem.verts, mem.faces, mem.colors)
            eng.mesh_render(mem.K, _poses(mem.poses[:1]), near=mem.near, fetch=False)
            with pytest.raises(amvs.AmvsError, match="mesh_texture: an atlas of .* is over the limit"):
                eng.mesh_texture(0.0, N, cells_per_row=cpr, colors_bgr=mem.images[:1])
        _index_clean()
    assert len(jobs) >= 400 and len(refused) >= 6 and n_textured >= 100_000 and n_fallen >= 100_000 and n_pixels >= 10_000


def _sphere_job():
    import mesh_volumes as mv
    H, W = 37, 53
    v, f, c = ri.sphere_mesh(33)
    K, poses, near = ri.views_for(v, 6, H, W)
    vol = mv.sphere_volume(33)
    return H, W, v, f, c, K, poses, near, ki.images_for(6, H, W, 78), vol.origin, vol.voxel


def test_argument_rules():
    import amvs
    H, W, v, f, c, K, poses, near, images, origin, voxel = _sphere_job()
    with _engine(H, W) as eng:
        eng.mesh_set(v, f, c)
        with pytest.raises(amvs.AmvsError, match="mesh_texture: no current render"):
            eng.mesh_texture(voxel, colors_bgr=images[:0].reshape(0, H, W, 3))
        eng.mesh_render(K, _poses(poses), near=near, fetch=False)
        with pytest.raises(amvs.AmvsError, match="fetch_render_texture: no current texture"):
            eng.mesh_render_texture(0, 1)
        import ctypes as C
        with pytest.raises(amvs.AmvsError, match="fetch_mesh_texture: no current texture"):
            eng._chk(eng._lib.amvs_fetch_mesh_texture(eng._h, None, None))
        with pytest.raises(amvs.AmvsError, match="mesh_texture: give exactly one colour source"):
            eng.mesh_texture(voxel)
        for j in range(5):
            eng.set_view_colors(j, images[j])
        with pytest.raises(amvs.AmvsError, match="mesh_texture: give exactly one colour source"):
            eng.mesh_texture(voxel, view_ids=list(range(5)) + [0], colors_bgr=images)
        for bad in ([0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, SLOTS], [0, 1, 2, 3, 4, -1]):   # slot 5 has no colour image yet
            with pytest.raises(amvs.AmvsError, match="mesh_texture: view .* has no resident colour image"):
                eng.mesh_texture(voxel, view_ids=bad)
        for bad in (-1.0, np.nan, np.inf):
            with pytest.raises(amvs.AmvsError, match="mesh_texture: depth_tolerance"):
                eng.mesh_texture(bad, colors_bgr=images)
        for bad in (-0.1, 1.0, 1.5, np.nan, np.inf, -np.inf):
            with pytest.raises(amvs.AmvsError, match="mesh_texture: min_cos"):
                eng.mesh_texture(voxel, min_cos=bad, colors_bgr=images)
        for bad in (0, -1, 65, 1000):
            with pytest.raises(amvs.AmvsError, match="mesh_texture: texels must lie in 1 .. 64"):
                eng.mesh_texture(voxel, bad, colors_bgr=images)
        with pytest.raises(amvs.AmvsError, match="mesh_texture: cells_per_row"):
            eng.mesh_texture(voxel, cells_per_row=-1, colors_bgr=images)
        # 9204 cells: one per row is 9204 * 4 texels high even at N = 1, 2000 per row is 2000 * 67 wide at N = 64
        for N, cpr in ((1, 1), (64, 2000), (8, 1490)):
            wt, ht = tr.layout(len(f), N, cpr)[2:]
            assert max(wt, ht) > tr.MAX_SIDE
            with pytest.raises(amvs.AmvsError, match="mesh_texture: an atlas of .* is over the limit"):
                eng.mesh_texture(voxel, N, cells_per_row=cpr, colors_bgr=images)
        wt, ht = tr.layout(len(f), 1, 4096)[2:]                       # exactly 16384 passes
        assert wt == tr.MAX_SIDE
        atlas = eng.mesh_texture(voxel, 1, cells_per_row=4096, colors_bgr=images)[0]
        assert atlas.shape == (ht, wt, 3)
        with pytest.raises(ValueError, match="colors_bgr"):
            eng.mesh_texture(voxel, colors_bgr=images[:5])
        with pytest.raises(ValueError, match="view ids"):
            eng.mesh_texture(voxel, view_ids=[0, 1])
        for first, count in ((-1, 1), (0, 0), (0, 7), (6, 1)):
            with pytest.raises(amvs.AmvsError, match="fetch_render_texture: views"):
                eng.mesh_render_texture(first, count)
        # a mesh without faces: a 0 x 0 atlas and success
        eng.mesh_set(v[:5], np.zeros((0, 3), np.int32), c[:5])
        eng.mesh_render(K, _poses(poses), near=near, fetch=False)
        atlas, uv, n = eng.mesh_texture(voxel, 8, cells_per_row=5, colors_bgr=images)
        assert atlas.shape == (0, 0, 3) and uv.shape == (0, 3, 2) and n == 0 and eng.last_texture_texels == 0
        assert not eng.mesh_render_texture(0, 6).any()
        _index_clean()


def test_what_keeps_and_what_drops_the_texture():
    import amvs
    import ctypes as C
    H, W, v, f, c, K, poses, near, images, origin, voxel = _sphere_job()
    depth, face, _ = rr.render(v, f, K, poses, near, H, W)
    normals = cr.normals(v, f)
    ref = tr.texture(v, f, c, K, poses, near, depth, images, voxel, 0.2, False, 3)
    other = ri.axis_views(3.0)
    depth2, face2, _ = rr.render(v, f, K, other, near, H, W)

    def textured(eng):
        eng.mesh_render(K, _poses(poses), near=near, fetch=False)
        return eng.mesh_texture(voxel, 3, colors_bgr=images)

    def stale(eng, what):
        with pytest.raises(amvs.AmvsError, match="fetch_mesh_texture: no current texture"):
            eng._chk(eng._lib.amvs_fetch_mesh_texture(eng._h, None, None))
        try:
            eng.mesh_render_fetch(0, 1)
        except amvs.AmvsError:
            return
        with pytest.raises(amvs.AmvsError, match="fetch_render_texture: no current texture"):      # the render outlived the call
            eng.mesh_render_texture(0, 1)

    def fetch(eng):
        atlas, uv = np.empty_like(ref[0]), np.empty_like(ref[1])
        eng._chk(eng._lib.amvs_fetch_mesh_texture(eng._h, atlas.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                  uv.ctypes.data_as(C.POINTER(C.c_float))))
        return atlas, uv

    with _engine(H, W) as eng:
        eng.mesh_set(v, f, c)
        eng.mesh_filter_components()                                  # labels
        eng.mesh_normals()
        eng.mesh_render(K, _poses(poses), near=near, fetch=False)
        counts = eng.mesh_visibility(voxel)
        before = eng.mesh_fetch(normals=True, labels=True)
        # mesh_texture leaves everything else current and unchanged
        _assert_texture(eng.mesh_texture(voxel, 3, colors_bgr=images), ref, "sphere")
        after = eng.mesh_fetch(normals=True, labels=True)
        assert _same_bits(after[0], before[0]) and np.array_equal(after[1], before[1]) and np.array_equal(after[2], c)
        assert _same_bits(after[3], normals) and np.array_equal(after[4], before[4])
        got = eng.mesh_render_fetch(0, 6)
        assert _same_bits(got[0], depth) and np.array_equal(got[1], face)
        again = np.empty(len(v), np.int32)
        eng._chk(eng._lib.amvs_fetch_mesh_visibility(eng._h, again.ctypes.data_as(C.POINTER(C.c_int))))
        assert np.array_equal(again, counts)
        # what keeps it: normals, visibility, every fetch, and a render from other cameras
        eng.mesh_normals()
        eng.mesh_visibility(voxel)
        eng.mesh_render_color(0, 2)
        atlas, uv = fetch(eng)
        assert np.array_equal(atlas, ref[0]) and _same_bits(uv, ref[1])
        pic = tr.render_texture(v, f, ref[0], K, poses, near, depth, face, 3)
        assert np.array_equal(eng.mesh_render_texture(0, 6), pic)
        eng.mesh_render(K, _poses(other), near=near, fetch=False)
        assert np.array_equal(eng.mesh_render_texture(1, 4), tr.render_texture(v, f, ref[0], K, other, near, depth2, face2, 3)[1:5])
        assert np.array_equal(fetch(eng)[0], ref[0])
        # what drops it
        eng.mesh_render(K, _poses(poses), near=near, fetch=False)
        eng.mesh_color_views(voxel, colors_bgr=images)
        stale(eng, "mesh_color_views")
        colors = kr.color_views(v, normals, c, K, poses, near, depth, images, voxel, 0.2, False)[0]
        _assert_texture(eng.mesh_texture(voxel, 3, colors_bgr=images), tr.texture(v, f, colors, K, poses, near, depth, images, voxel,
                                                                                  0.2, False, 3), "after recolouring")
        eng.mesh_smooth(0)
        stale(eng, "mesh_smooth(0)")
        textured(eng)
        eng.mesh_filter_components()
        stale(eng, "mesh_filter_components")
        textured(eng)
        eng.mesh_decimate(origin, F32(2) * voxel)
        stale(eng, "mesh_decimate")
        eng.mesh_set(v, f, c)
        textured(eng)
        eng.mesh_set(v, f, c)
        stale(eng, "mesh_set")
        _index_clean()
    # a second context in the opposite order: the texture before normals, labels and counts, from resident images
    with _engine(H, W) as eng:
        eng.mesh_set(v, f, c)
        for j in range(6):
            eng.set_view_colors(j, images[j])
        eng.mesh_render(K, _poses(poses), near=near, fetch=False)
        _assert_texture(eng.mesh_texture(voxel, 3, view_ids=range(6)), ref, "second context")
        eng.mesh_visibility(voxel)
        eng.mesh_normals()
        assert np.array_equal(fetch(eng)[0], ref[0]) and _same_bits(eng.mesh_fetch(normals=True)[3], normals)
        assert np.array_equal(eng.mesh_render_texture(0, 6), pic)


def test_reconstruct_mesh_textures_the_final_mesh(scene_a, capsys, tmp_path):
    """On scene_a through the device-preparation path (resident images) and the host-image path: the atlas and the UVs are
    the restatement's on the fetched mesh, the line says what happened, texture_texels=0 is the call without the argument,
    and the result goes through save_mesh_obj."""
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    from amvs.core.utils import save_mesh_obj
    camera, images, poses, sparse = _scene_a_inputs(scene_a)
    H, W = scene_a.H, scene_a.W
    results = []
    for device_prep in (True, False):
        pm = PatchMatchMVS(camera, scale=1.0, patch_size=7, num_iterations=4, num_samples=6, min_views=2, seed=2, device=0,
                           device_prep=device_prep)
        base = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, decimate_voxels=2.0)
        off = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, decimate_voxels=2.0, texture_texels=0)
        assert len(base) == len(off) == 3
        _assert_mesh_equal(off, base, "texture_texels=0")
        capsys.readouterr()
        got = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, decimate_voxels=2.0, texture_texels=8)
        line = [ln for ln in capsys.readouterr().out.splitlines() if "Clean-up" in ln]
        assert len(got) == 5
        _assert_mesh_equal(got, base, "the mesh beside its texture")
        v, f, c = base
        ids = pm.last_mesh_views
        voxel = pm.last_mesh_grid[1]
        pp = np.stack([np.concatenate([np.asarray(poses[i].R, np.float64).reshape(9), np.asarray(poses[i].t, np.float64).reshape(3)])
                       for i in ids]).astype(F32)
        Kf = np.asarray(pm.K_scaled, np.float64).astype(F32)
        bgr = np.stack([scene_a.colors[i] for i in ids])
        depth = rr.render(v, f, Kf, pp, F32(voxel), H, W)[0]
        ref = tr.texture(v, f, c, Kf, pp, F32(voxel), depth, bgr, F32(1.0) * F32(voxel), 0.2, False, 8)
        assert np.array_equal(got[4], ref[0]) and _same_bits(got[3], ref[1]), f"device_prep {device_prep}"
        assert 0 < ref[3] <= ref[2]
        said = f"texture 8 texels, {ref[0].shape[1]} x {ref[0].shape[0]}: {ref[3]:,} of {ref[2]:,} texels from the views"
        assert len(line) == 1 and said in line[0], line
        results.append(got)
    assert np.array_equal(results[0][4], results[1][4])
    both = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, decimate_voxels=2.0, color_from_views=True, color_best_view=True,
                               with_normals=True, texture_texels=2)
    assert len(both) == 6 and both[3].shape == (len(both[0]), 3) and both[4].shape == (len(both[1]), 3, 2)
    v, f, c = both[:3]
    depth = rr.render(v, f, Kf, pp, F32(voxel), H, W)[0]
    ref = tr.texture(v, f, c, Kf, pp, F32(voxel), depth, bgr, F32(voxel), 0.2, True, 2)
    assert np.array_equal(both[5], ref[0]) and _same_bits(both[4], ref[1])
    save_mesh_obj(v, f, both[4], both[5], tmp_path / "scene.obj", normals=both[3])
    assert all((tmp_path / name).stat().st_size > 0 for name in ("scene.obj", "scene.mtl", "scene.png"))
