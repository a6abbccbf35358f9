"""The colour kernels (csrc/amvs_mesh_color.hip; include/amvs.h amvs_mesh_color_views, amvs_fetch_render_color) against
the NumPy restatement (tests/mesh_color_restatement.py), byte for byte: the vertex colours, the number of recoloured
vertices and the colour render.  The family is that of tests/mesh_color_inputs.py, which test_mesh_color_cpu.py checks
for what it reaches; every mesh goes to the device through amvs_mesh_set, the maps and the normals are the device's own
(compared with their restatements in test_hip_mesh_render.py and test_hip_mesh_clean.py)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_restatement as cr  # noqa: E402
import mesh_color_inputs as ki  # noqa: E402
import mesh_color_restatement as kr  # noqa: E402
import mesh_decimate_restatement as dr  # noqa: E402
import mesh_render_inputs as ri  # noqa: E402
import mesh_render_restatement as rr  # noqa: E402
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
def _members(H, W):
    """The family of one image size with its reference maps, computed once for the tests of this file."""
    return list(ki.family(H, W))


def _index_clean():
    from amvs import _lib
    assert _lib.index_check()[0] == 0


@pytest.mark.parametrize("H,W", ki.SIZES)
def test_family_byte_exact_on_one_context(H, W):
    """Every mesh of the family on ONE context per image size: normals, then the render into 1 and 6 cameras, then the
    colours at tolerance 0 and one unit, min_cos 0 and 0.5, blended and from the best view, from host images and from
    resident ones (uploaded in reversed slot order, so that the view ids matter).  The calls are chained: every one starts
    from the colours the one before left, as the restatement does."""
    n_runs = n_colored = n_kept = 0
    with _engine(H, W) as eng:
        for mem in _members(H, W):
            depth, _ = mem.maps()
            eng.mesh_set(mem.verts, mem.faces, mem.colors)
            eng.mesh_normals()
            for j in range(len(mem.images)):
                eng.set_view_colors(SLOTS - 1 - j, mem.images[j])
            cur = mem.colors
            for n in mem.n_views:
                eng.mesh_render(mem.K, _poses(mem.poses[:n]), near=mem.near, fetch=False)
                for tol in mem.tolerances:
                    for min_cos in ki.MIN_COS:
                        for best in (False, True):
                            for resident in (False, True):
                                src = dict(view_ids=[SLOTS - 1 - j for j in range(n)]) if resident else dict(colors_bgr=mem.images[:n])
                                got = eng.mesh_color_views(tol, min_cos, best, **src)
                                cur, ref = kr.color_views(mem.verts, mem.normals, cur, mem.K, mem.poses[:n], mem.near, depth[:n],
                                                          mem.images[:n], tol, min_cos, best)
                                what = f"{mem.name}, {H} x {W}, {n} views, tolerance {tol}, min_cos {min_cos}, best {best}, resident {resident}"
                                assert got == ref, f"{what}: n_colored {got} vs {ref}"
                                out = eng.mesh_fetch()[2]
                                assert np.array_equal(out, cur), f"{what}: {int((out != cur).any(axis=1).sum())} vertices differ"
                                n_runs += 1
                                n_colored += ref
                                n_kept += len(mem.verts) - ref
        _index_clean()
    assert n_runs >= 1000 and n_colored >= 10_000 and n_kept >= 10_000


@pytest.mark.parametrize("H,W", ki.SIZES)
def test_colour_render_byte_exact(H, W):
    """amvs_fetch_render_color on the same family: with the colours the mesh came with, and after recolouring; all views
    and sub-ranges of them."""
    n_pixels = 0
    with _engine(H, W) as eng:
        for mem in _members(H, W):
            depth, face = mem.maps()
            n = max(mem.n_views)
            eng.mesh_set(mem.verts, mem.faces, mem.colors)
            eng.mesh_render(mem.K, _poses(mem.poses[:n]), near=mem.near, fetch=False)
            ref = kr.render_color(mem.verts, mem.faces, mem.colors, mem.K, mem.poses[:n], mem.near, depth[:n], face[:n])
            got = eng.mesh_render_color(0, n)
            assert got.dtype == np.uint8 and got.shape == ref.shape and np.array_equal(got, ref), f"{mem.name}: before recolouring"
            assert not got[face[:n] < 0].any()
            eng.mesh_normals()
            eng.mesh_color_views(mem.tolerances[1], 0.0, False, colors_bgr=mem.images[:n])
            colors = kr.color_views(mem.verts, mem.normals, mem.colors, mem.K, mem.poses[:n], mem.near, depth[:n], mem.images[:n],
                                    mem.tolerances[1], 0.0, False)[0]
            ref = kr.render_color(mem.verts, mem.faces, colors, mem.K, mem.poses[:n], mem.near, depth[:n], face[:n])
            for first, count in ((0, n), (n - 1, 1)) + (((1, 2), (2, 4)) if n == 6 else ()):
                got = eng.mesh_render_color(first, count)
                assert np.array_equal(got, ref[first:first + count]), f"{mem.name}: views {first} .. {first + count - 1}"
            n_pixels += int((face[:n] >= 0).sum())
        _index_clean()
    assert n_pixels >= 10_000


def _sphere_job():
    import mesh_volumes as mv
    H, W = 37, 53
    v, f, c = ri.sphere_mesh(33)
    K, poses, near = ri.views_for(v, 6, H, W)
    vol = mv.sphere_volume(33)
    return H, W, v, f, c, K, poses, near, ki.images_for(6, H, W, 77), vol.origin, vol.voxel


def test_argument_and_attribute_rules():
    import amvs
    H, W, v, f, c, K, poses, near, images, origin, voxel = _sphere_job()
    depth, face, _ = rr.render(v, f, K, poses, near, H, W)
    normals = cr.normals(v, f)
    with _engine(H, W) as eng:
        eng.mesh_set(v, f, c)
        eng.mesh_normals()
        with pytest.raises(amvs.AmvsError, match="mesh_color_views: no current render"):
            eng.mesh_color_views(voxel, colors_bgr=images[:0].reshape(0, H, W, 3))
        with pytest.raises(amvs.AmvsError, match="fetch_render_color: no current render"):
            eng.mesh_render_color(0, 1)
        eng.mesh_set(v, f, c)
        eng.mesh_render(K, _poses(poses), near=near, fetch=False)
        with pytest.raises(amvs.AmvsError, match="mesh_color_views: no current normals"):
            eng.mesh_color_views(voxel, colors_bgr=images)
        eng.mesh_normals()                                           # keeps the render
        with pytest.raises(amvs.AmvsError, match="mesh_color_views: give exactly one colour source"):
            eng.mesh_color_views(voxel)
        for j in range(5):
            eng.set_view_colors(j, images[j])
        with pytest.raises(amvs.AmvsError, match="mesh_color_views: give exactly one colour source"):
            eng.mesh_color_views(voxel, view_ids=list(range(5)) + [0], colors_bgr=images)
        for bad in ([0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, SLOTS], [0, 1, 2, 3, 4, -1]):   # slot 5 has no colour image yet
            with pytest.raises(amvs.AmvsError, match="mesh_color_views: view .* has no resident colour image"):
                eng.mesh_color_views(voxel, view_ids=bad)
        for bad in (-1.0, np.nan, np.inf):
            with pytest.raises(amvs.AmvsError, match="mesh_color_views: depth_tolerance"):
                eng.mesh_color_views(bad, colors_bgr=images)
        for bad in (-0.1, 1.0, 1.5, np.nan, np.inf, -np.inf):
            with pytest.raises(amvs.AmvsError, match="mesh_color_views: min_cos"):
                eng.mesh_color_views(voxel, min_cos=bad, colors_bgr=images)
        with pytest.raises(ValueError, match="colors_bgr"):
            eng.mesh_color_views(voxel, colors_bgr=images[:5])
        with pytest.raises(ValueError, match="view ids"):
            eng.mesh_color_views(voxel, view_ids=[0, 1])
        for first, count in ((-1, 1), (0, 0), (0, 7), (6, 1)):
            with pytest.raises(amvs.AmvsError, match="fetch_render_color: views"):
                eng.mesh_render_color(first, count)
        assert np.array_equal(eng.mesh_fetch()[2], c)                # no refused call has touched a colour
        # what stays current: everything
        eng.mesh_filter_components()                                  # labels; drops normals and render
        eng.mesh_normals()
        eng.mesh_render(K, _poses(poses), near=near, fetch=False)
        counts = eng.mesh_visibility(voxel)
        before = eng.mesh_fetch(normals=True, labels=True)
        n = eng.mesh_color_views(voxel, 0.2, False, colors_bgr=images)
        colors, ref_n = kr.color_views(v, normals, c, K, poses, near, depth, images, voxel, 0.2, False)
        assert n == ref_n and 0 < n < len(v)
        after = eng.mesh_fetch(normals=True, labels=True)
        assert _same_bits(after[0], before[0]) and np.array_equal(after[1], before[1]) and np.array_equal(after[2], colors)
        assert _same_bits(after[3], before[3]) and np.array_equal(after[4], before[4]) and _same_bits(after[3], normals)
        got = eng.mesh_render_fetch(0, 6)
        assert _same_bits(got[0], depth) and np.array_equal(got[1], face)
        import ctypes as C
        again = np.empty(len(v), np.int32)
        eng._chk(eng._lib.amvs_fetch_mesh_visibility(eng._h, again.ctypes.data_as(C.POINTER(C.c_int))))
        assert np.array_equal(again, counts)
        assert np.array_equal(eng.mesh_render_color(2, 3), kr.render_color(v, f, colors, K, poses, near, depth, face)[2:5])
        # the smoothing moves the mesh: the maps go stale, and with them the colour render and the recolouring
        eng.mesh_smooth(1)
        for what, call in (("fetch_render_color: no current render", lambda: eng.mesh_render_color(0, 1)),
                           ("mesh_color_views: no current render", lambda: eng.mesh_color_views(voxel, colors_bgr=images))):
            with pytest.raises(amvs.AmvsError, match=what):
                call()
        # a later decimation averages the new colours as its restatement says
        eng.mesh_set(v, f, c)
        eng.mesh_render(K, _poses(poses), near=near, fetch=False)
        eng.mesh_normals()
        assert eng.mesh_color_views(voxel, 0.2, True, colors_bgr=images) == ref_n
        best = kr.color_views(v, normals, c, K, poses, near, depth, images, voxel, 0.2, True)[0]
        cell = F32(2) * voxel
        eng.mesh_decimate(origin, cell)
        _assert_mesh_equal(eng.mesh_fetch(), dr.decimate(v, f, best, origin, cell), "decimation after recolouring")
        _index_clean()
    # a second context, the render before the normals, resident images
    with _engine(H, W) as eng:
        eng.mesh_set(v, f, c)
        for j in range(6):
            eng.set_view_colors(j, images[j])
        eng.mesh_render(K, _poses(poses), near=near, fetch=False)
        eng.mesh_normals()
        assert eng.mesh_color_views(voxel, 0.2, False, view_ids=range(6)) == ref_n
        assert np.array_equal(eng.mesh_fetch()[2], colors)


def _without_clock(text):
    """Printed progress with every elapsed time (`0.03s`) blanked."""
    import re
    return re.sub(r"\d+\.\d+s", "#s", text)


def test_reconstruct_mesh_colours_from_the_views(scene_a, capsys):
    """On scene_a: the device-preparation path (resident images) and the host-image path give the same mesh, which is the
    restatement applied to the mesh without the option, the restatement's maps and the prepared images (at scale 1 the
    inputs themselves); with decimation and culling the line says what happened; color_from_views=False is the call
    without the argument."""
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    camera, images, poses, sparse = _scene_a_inputs(scene_a)
    H, W = scene_a.H, scene_a.W
    results = []
    for device_prep in (True, False):
        pm = PatchMatchMVS(camera, scale=1.0, patch_size=7, num_iterations=4, num_samples=6, min_views=2, seed=2, device=0,
                           device_prep=device_prep)
        capsys.readouterr()
        base = pm.reconstruct_mesh(images, poses, sparse, max_dim=64)
        said = capsys.readouterr().out
        off = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, color_from_views=False)
        assert len(base) == len(off) == 3 and "Mesh:" in said and "colours" not in said
        assert _without_clock(capsys.readouterr().out) == _without_clock(said)          # the same lines, the times aside
        _assert_mesh_equal(off, base, "color_from_views=False")
        got = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, color_from_views=True)
        line = [ln for ln in capsys.readouterr().out.splitlines() if "Clean-up" in ln]
        assert pm._resident_colors == device_prep and len(got) == 3
        v, f, c = base
        ids = pm.last_mesh_views
        voxel = pm.last_mesh_grid[1]
        pp = np.stack([np.concatenate([np.asarray(poses[i].R, np.float64).reshape(9), np.asarray(poses[i].t, np.float64).reshape(3)])
                       for i in ids]).astype(F32)
        Kf = np.asarray(pm.K_scaled, np.float64).astype(F32)
        bgr = np.stack([scene_a.colors[i] for i in ids])
        depth = rr.render(v, f, Kf, pp, F32(voxel), H, W)[0]
        colors, n = kr.color_views(v, cr.normals(v, f), c, Kf, pp, F32(voxel), depth, bgr, F32(1.0) * F32(voxel), 0.2, False)
        _assert_mesh_equal(got, (v, f, colors), f"color_from_views, device_prep {device_prep}")
        assert 0 < n <= len(v) and (colors != c).any()
        assert len(line) == 1 and f"colours from {len(ids)} views: {n:,} of {len(v):,} vertices" in line[0], line
        results.append(got)
    _assert_mesh_equal(results[0], results[1], "resident images against host images")
    # best view, with normals, after culling and decimation: the line, and the restatements chained
    both = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, min_visible_views=2, decimate_voxels=2.0, color_from_views=True,
                               color_best_view=True, color_min_cos=0.3, with_normals=True)
    line = [ln for ln in capsys.readouterr().out.splitlines() if "Clean-up" in ln]
    plain = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, min_visible_views=2, decimate_voxels=2.0)
    v, f, c = plain
    depth = rr.render(v, f, Kf, pp, F32(voxel), H, W)[0]
    normals = cr.normals(v, f)
    colors, n = kr.color_views(v, normals, c, Kf, pp, F32(voxel), depth, bgr, F32(voxel), F32(0.3), True)
    assert len(both) == 4 and _same_bits(both[3], normals)
    _assert_mesh_equal(both, (v, f, colors), "culling, decimation, colours from the best view")
    assert len(line) == 1 and "visibility >= 2 views" in line[0] and "decimation at 2 voxels" in line[0], line
    assert line[0].index("decimation") < line[0].index(f"colours from {len(ids)} views: {n:,} of {len(v):,} vertices") < line[0].index("normals")
    for bad in (dict(color_from_views=1), dict(color_from_views=None), dict(color_best_view="yes"), dict(color_min_cos=-0.1),
                dict(color_min_cos=1.0), dict(color_min_cos=np.nan), dict(color_min_cos="a")):
        with pytest.raises(ValueError, match="color_"):
            pm.reconstruct_mesh(images, poses, sparse, max_dim=64, **bad)
