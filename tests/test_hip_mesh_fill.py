"""Hole filling on the device (csrc/amvs_mesh_fill.hip; include/amvs.h amvs_tsdf_fill, amvs_tsdf_fetch_fill) against the
NumPy restatement (tests/mesh_fill_restatement.py), byte for byte: the filled volume at every point that is observed
afterwards, the generations, the per-step counts and the mesh amvs_tsdf_extract makes of it.  The family is that of
tests/mesh_fill_inputs.py, which test_mesh_fill_cpu.py checks for what it reaches; every volume goes to the device through
amvs_tsdf_set_volume."""
import ctypes as C
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_fill_inputs as fi  # noqa: E402
import mesh_fill_restatement as fr  # noqa: E402
import mesh_render_inputs as ri  # noqa: E402
import mesh_restatement as mr  # noqa: E402
import mesh_volumes as mv  # noqa: E402
from mesh_hip_common import K_ANY, _assert_mesh_equal, _engine, _scene_a_inputs, _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
EINVAL = r"\(-1\): "                                       # AMVS_EINVAL, as Engine._chk words it


def _index_clean():
    from amvs import _lib
    assert _lib.index_check()[0] == 0


@functools.lru_cache(maxsize=None)
def _family():
    return fi.family()


_MESHES = {}


def _extract(t, w, c, origin, voxel):
    """mesh_restatement.extract, computed once per volume: many (steps, min_neighbours) pairs leave the same one."""
    key = hashlib.sha1(b"".join(np.ascontiguousarray(a).tobytes() for a in (t, w, c, origin, np.asarray(voxel)))).digest()
    if key not in _MESHES:
        _MESHES[key] = mr.extract(t, w, c, origin, voxel)
    return _MESHES[key]


def _assert_filled(eng, ref, volume, what):
    """The context's volume, generations and last counts against the restatement's `ref`, then the extracted mesh."""
    t, w, c, gen, counts = ref
    assert eng.last_fill_counts == counts, f"{what}: counts {eng.last_fill_counts} vs {counts}"
    got_gen = eng.tsdf_fill_generations()
    assert got_gen.dtype == np.uint8 and np.array_equal(got_gen, gen), f"{what}: {int((got_gen != gen).sum())} generations differ"
    gt, gw, gc = eng.tsdf_volume()
    assert _same_bits(gw, w), f"{what}: weights differ"
    seen = w > 0
    assert _same_bits(gt[seen], t[seen]), f"{what}: tsdf differs at {int((gt[seen] != t[seen]).sum())} observed points"
    assert _same_bits(gc[seen], c[seen]), f"{what}: colour sums differ"
    hidden = ~seen                                                  # nobody writes behind a point that stays unobserved
    assert np.array_equal(gt[hidden].view(np.uint32), volume.tsdf[hidden].view(np.uint32)), f"{what}: an unobserved tsdf changed"
    _assert_mesh_equal(eng.tsdf_extract(), _extract(t, w, c, volume.origin, volume.voxel), what)


@pytest.mark.parametrize("min_neighbours", fi.MIN_NEIGHBOURS)
def test_family_byte_exact_on_one_context(min_neighbours):
    """Every member at every step count on ONE context, the calls chained: volumes of all sizes follow each other in the
    same grow-only buffers, and every fill starts from a freshly set volume."""
    filled = 0
    with _engine() as eng:
        for name, v in _family():
            for steps in fi.STEPS:
                what = f"{name}, {steps} steps, {min_neighbours} neighbours"
                ref = fr.fill(*v.arrays()[:3], steps, min_neighbours)
                eng.tsdf_set_volume(*v.arrays())
                n = eng.tsdf_fill(steps, min_neighbours)
                assert n == sum(ref[4]), what
                filled += n
                _assert_filled(eng, ref, v, what)
        _index_clean()
    assert filled > 0


def test_large_sphere():
    """160^3: 16 000 workgroups, no multiple of anything convenient, after a small volume on the same context.  The
    restatement of the fill runs on the tube's box (test_mesh_fill_cpu.py holds that to the whole volume on the 33^3 sphere);
    the extraction's restatement walks the whole volume and is most of this test's time."""
    v = fi.large_sphere()
    ref = fi.fill_cropped(v, 4)
    assert all(n > 0 for n in ref[4])
    with _engine() as eng:
        small = _family()[0][1]
        eng.tsdf_set_volume(*small.arrays())
        eng.tsdf_fill(1)
        eng.tsdf_set_volume(*v.arrays())
        assert eng.tsdf_fill(4) == sum(ref[4])
        _assert_filled(eng, ref, v, v.name)
        _index_clean()


def test_every_refusal():
    import amvs
    v = _family()[0][1]
    with _engine() as eng:
        gen = np.zeros(v.tsdf.shape, np.uint8)
        with pytest.raises(amvs.AmvsError, match=EINVAL + "tsdf_fill: no volume"):
            eng.tsdf_fill(2)
        with pytest.raises(amvs.AmvsError, match=EINVAL + "tsdf_fetch_fill: no fill of the current volume"):
            eng._chk(eng._lib.amvs_tsdf_fetch_fill(eng._h, gen.ctypes.data_as(C.POINTER(C.c_uint8))))
        eng.tsdf_set_volume(*v.arrays())
        for steps in (0, 65, -1):
            with pytest.raises(amvs.AmvsError, match=EINVAL + "tsdf_fill: steps must lie in 1 .. 64"):
                eng.tsdf_fill(steps)
        for mn in (0, 7, -1):
            with pytest.raises(amvs.AmvsError, match=EINVAL + "tsdf_fill: min_neighbours must lie in 1 .. 6"):
                eng.tsdf_fill(2, mn)
        with pytest.raises(amvs.AmvsError, match=EINVAL + "tsdf_fetch_fill: no fill of the current volume"):
            eng.tsdf_fill_generations()
        # a refused call did no work: the volume is as set, and 64 steps are accepted
        assert all(_same_bits(a[v.weight > 0], b[v.weight > 0]) for a, b in zip(eng.tsdf_volume(), v.arrays()[:3]))
        eng.tsdf_fill(64, 6)
        assert len(eng.last_fill_counts) == 64
        eng.tsdf_fill_generations()
        # NULL outputs are allowed, a NULL generation buffer is not
        eng._chk(eng._lib.amvs_tsdf_fill(eng._h, 1, 1, None, None))
        with pytest.raises(amvs.AmvsError, match=EINVAL + "tsdf_fetch_fill: NULL output"):
            eng._chk(eng._lib.amvs_tsdf_fetch_fill(eng._h, None))
        # a new volume forgets the fill, whichever call makes it
        eng.tsdf_set_volume(*v.arrays())
        with pytest.raises(amvs.AmvsError, match=EINVAL + "tsdf_fetch_fill: no fill of the current volume"):
            eng.tsdf_fill_generations()
        _index_clean()
    sc = mv.many_maps_scene()
    with _engine(sc.H, sc.W, 1, sc.K) as eng:
        eng.tsdf_set_volume(*v.arrays())
        eng.tsdf_fill(1)
        eng.tsdf_integrate(sc.K, sc.pose_list(), sc.min_views, sc.origin, sc.voxel, sc.dims, sc.trunc, depth=sc.depth, conf=sc.conf,
                           colors_bgr=sc.colors)
        with pytest.raises(amvs.AmvsError, match=EINVAL + "tsdf_fetch_fill: no fill of the current volume"):
            eng.tsdf_fill_generations()
        # on an integrated volume
        t, w, c = sc.integrate()
        ref = fr.fill(t, w, c, 3, 2)
        assert eng.tsdf_fill(3, 2) == sum(ref[4]) > 0
        _assert_filled(eng, ref, mv.Volume(sc.name, t, w, c, sc.origin, sc.voxel), sc.name)
        _index_clean()


MESSAGES = {"mesh": "no mesh",
            "normals": EINVAL + "fetch_mesh_attributes: no current normals",
            "labels": EINVAL + "fetch_mesh_attributes: no current labels",
            "render": EINVAL + "fetch_render: no current render",
            "visibility": EINVAL + "fetch_mesh_visibility: no current counts",
            "texture": EINVAL + "fetch_mesh_texture: no current texture"}


def _fetches(eng):
    def counts():
        out = np.empty(max(eng._mesh_counts[0], 1), np.int32)
        eng._chk(eng._lib.amvs_fetch_mesh_visibility(eng._h, out.ctypes.data_as(C.POINTER(C.c_int32))))

    return {"normals": lambda: eng.mesh_fetch(normals=True), "labels": lambda: eng.mesh_fetch(labels=True),
            "render": lambda: eng.mesh_render_fetch(0, 1), "visibility": counts,
            "texture": lambda: eng._chk(eng._lib.amvs_fetch_mesh_texture(eng._h, None, None))}


def test_a_fill_drops_the_mesh_and_every_attribute():
    """The row of csrc/amvs_mesh_state.h: after tsdf_fill nothing of the mesh is current, in either order of making the
    attributes; the extraction that follows meshes the filled volume and brings none of them back."""
    import amvs
    v = fi.sphere_with_tube(17, rho=0.3, trunc=0.2)[0]
    ref = fr.fill(*v.arrays()[:3], 3)
    filled_mesh = mr.extract(*ref[:3], v.origin, v.voxel)
    H, W = 24, 32
    K, poses, near = ri.views_for(v.extract()[0], 2, H, W)
    images = np.random.default_rng(3).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    pose_list = [(q[:9].reshape(3, 3), q[9:]) for q in np.asarray(poses, F32).reshape(-1, 12)]

    def everything(eng, texture_first):
        """Every attribute made current.  The labels come first in either order: mesh_filter_components drops the others."""
        eng.mesh_filter_components()
        if not texture_first:
            eng.mesh_normals()
        eng.mesh_render(K, pose_list, near=near, fetch=False)
        if texture_first:
            eng.mesh_texture(v.voxel, 2, colors_bgr=images)
        eng.mesh_visibility(F32(1e6))
        if texture_first:
            eng.mesh_normals()
        else:
            eng.mesh_texture(v.voxel, 2, colors_bgr=images)
        for fetch in _fetches(eng).values():
            fetch()

    for reverse in (False, True):
        with amvs.Engine(H, W, 2, K) as eng:
            eng.tsdf_set_volume(*v.arrays())
            _assert_mesh_equal(eng.tsdf_extract(), v.extract(), v.name)
            everything(eng, reverse)
            assert eng.tsdf_fill(3) == sum(ref[4])
            with pytest.raises(amvs.AmvsError, match=MESSAGES["mesh"]):
                eng.mesh_fetch()
            for name, fetch in _fetches(eng).items():
                with pytest.raises(amvs.AmvsError):
                    fetch()
            for call in (eng.mesh_normals, lambda: eng.mesh_smooth(1), eng.mesh_filter_components):
                with pytest.raises(amvs.AmvsError, match=MESSAGES["mesh"]):
                    call()
            _assert_mesh_equal(eng.tsdf_extract(), filled_mesh, "the filled volume")
            for name, fetch in _fetches(eng).items():
                with pytest.raises(amvs.AmvsError, match=MESSAGES[name]):
                    fetch()
            everything(eng, not reverse)
            _assert_mesh_equal(eng.mesh_fetch(), filled_mesh, "after the attributes")
            _index_clean()


def test_two_calls_compose_on_the_device():
    """fill(2) then fill(3) leaves the volume of fill(5); the second call's generations count from its own start."""
    with _engine() as eng:
        for index in (0, 6, 12, 21, 22):
            name, v = _family()[index]
            for mn in (1, 2):
                whole = fr.fill(*v.arrays()[:3], 5, mn)
                first = fr.fill(*v.arrays()[:3], 2, mn)
                second = fr.fill(*first[:3], 3, mn)
                eng.tsdf_set_volume(*v.arrays())
                eng.tsdf_fill(2, mn)
                assert eng.last_fill_counts == first[4]
                eng.tsdf_fill(3, mn)
                assert eng.last_fill_counts == second[4] == whole[4][2:], name
                _assert_filled(eng, second, v, f"{name}: two calls")
                got = eng.tsdf_volume()
                seen = whole[1] > 0
                assert all(_same_bits(g[seen], r[seen]) for g, r in zip(got, whole[:3])) and _same_bits(got[1], whole[1]), name
        _index_clean()


def test_reconstruct_mesh_fills_between_fusion_and_extraction(scene_a, capsys):
    """On scene_a through the device-preparation path (resident images) and the host-image path: the generations and the
    volume are the restatement's fill of the same volume with its filled points made unobserved again, the mesh is the
    restatement's extraction of it, the line says what happened, and fill_holes_voxels=0 is the call without the argument."""
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    camera, images, poses, sparse = _scene_a_inputs(scene_a)
    for device_prep in (True, False):
        pm = PatchMatchMVS(camera, scale=1.0, patch_size=7, num_iterations=4, num_samples=6, min_views=2, seed=2, device=0,
                           device_prep=device_prep)
        base = pm.reconstruct_mesh(images, poses, sparse, max_dim=64)
        off = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, fill_holes_voxels=0, fill_min_neighbours=1)
        _assert_mesh_equal(off, base, "fill_holes_voxels=0")
        capsys.readouterr()
        got = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, fill_holes_voxels=2)
        line = [ln for ln in capsys.readouterr().out.splitlines() if "Clean-up" in ln]
        assert len(got) == 3
        eng = pm._engine
        gen = eng.tsdf_fill_generations()
        t, w, c = eng.tsdf_volume()
        origin, voxel, dims, _ = pm.last_mesh_grid
        assert gen.shape == t.shape == tuple(dims[::-1]) and np.array_equal(w > 0, gen > 0)
        filled = gen >= 2
        assert filled.any() and (w[filled] == 1).all()
        t0, w0, c0 = t.copy(), w.copy(), c.copy()
        t0[filled], w0[filled], c0[filled] = np.nan, 0.0, np.nan
        ref = fr.fill(t0, w0, c0, 2)
        seen = w > 0
        assert np.array_equal(ref[3], gen) and _same_bits(ref[1], w), f"device_prep {device_prep}"
        assert _same_bits(ref[0][seen], t[seen]) and _same_bits(ref[2][seen], c[seen]), f"device_prep {device_prep}"
        assert eng.last_fill_counts == ref[4]
        mesh = mr.extract(ref[0], ref[1], ref[2], np.asarray(origin, np.float64).astype(F32), F32(voxel))
        _assert_mesh_equal(got, mesh, f"device_prep {device_prep}: the filled mesh")
        assert len(got[1]) > len(base[1])
        said = f"filled {sum(ref[4]):,} grid points in 2 steps"
        assert len(line) == 1 and said in line[0], line
    # two known neighbours asked for: fewer points, and the other clean-up steps run on the filled mesh
    both = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, fill_holes_voxels=2, fill_min_neighbours=2, min_component_faces=8)
    assert 0 < pm._engine.last_fill_counts[0] < ref[4][0] and len(both) == 3
