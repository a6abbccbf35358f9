"""The surface-mesh kernels (csrc/amvs_mesh.hip) on the volumes and scenes of tests/mesh_volumes.py: every sign
case of every Kuhn tetrahedron, exact zeros, unobserved points, a volume of 4 M points, shrinking buffers, and the
integration's guards at their edges.  Volumes reach the device through the test hook amvs_tsdf_set_volume; volume and
mesh are compared bit for bit with tests/mesh_restatement.py.  test_mesh_cpu.py checks, on the restatement alone,
that these inputs reach all 84 (tetrahedron, case) pairs and every branch of the integration."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_restatement as mr  # noqa: E402
import mesh_volumes as mv  # noqa: E402

pytestmark = pytest.mark.gpu

K_ANY = np.array([[30.0, 0, 16.0], [0, 30.0, 12.0], [0, 0, 1]], np.float32)


def _engine(H=24, W=32, n=1, K=K_ANY):
    import amvs
    return amvs.Engine(H, W, n, K)


def _same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _assert_mesh_equal(mesh, ref, what):
    verts, faces, cols = mesh
    rv, rf, rc = ref
    assert (len(verts), len(faces)) == (len(rv), len(rf)), f"{what}: {len(verts)} / {len(faces)} vs {len(rv)} / {len(rf)}"
    assert verts.shape == (len(rv), 3) and faces.shape == (len(rf), 3) and cols.shape == (len(rv), 3)
    assert np.array_equal(faces, rf), f"{what}: faces differ, first at {np.argwhere(faces != rf)[:1]}"
    assert _same_bits(verts, rv), f"{what}: vertex positions differ"
    assert np.array_equal(cols, rc), f"{what}: vertex colours differ"


def _extract(eng, vol):
    eng.tsdf_set_volume(*vol.arrays())
    return eng.tsdf_extract()


def test_hook_round_trip_and_validation():
    import amvs
    vol = mv.random_sign_volume((7, 5, 3), 11)
    with _engine() as eng:
        with pytest.raises(amvs.AmvsError, match="no volume"):
            eng.tsdf_extract()
        eng.tsdf_set_volume(*vol.arrays())
        tsdf, weight, color = eng.tsdf_volume()                   # NaN and -0.0 come back as they went
        assert _same_bits(tsdf, vol.tsdf) and _same_bits(weight, vol.weight) and _same_bits(color, vol.color)
        _assert_mesh_equal(eng.tsdf_extract(), vol.extract(), vol.name)
        # a new volume drops the mesh
        eng.tsdf_set_volume(*vol.arrays())
        with pytest.raises(amvs.AmvsError, match="no mesh"):
            eng._chk(eng._lib.amvs_fetch_mesh(eng._h, None, None, None))
        t, w, c, o, v = vol.arrays()
        for bad_o, bad_v in (((0, np.nan, 0), v), ((0, 0, np.inf), v), (o, 0.0), (o, -1.0), (o, np.inf), (o, np.nan)):
            with pytest.raises(amvs.AmvsError, match="finite"):
                eng.tsdf_set_volume(t, w, c, bad_o, bad_v)
        with pytest.raises(amvs.AmvsError, match=">= 2"):
            eng.tsdf_set_volume(t[:, :, :1], w[:, :, :1], c[:, :, :1], o, v)
        # over the budget: refused from the dims alone, before any array is read
        f32p = C.POINTER(C.c_float)
        one = np.zeros(3, np.float32)
        dims = np.array([513, 512, 512], np.int32)
        rc = eng._lib.amvs_tsdf_set_volume(eng._h, one.ctypes.data_as(f32p), one.ctypes.data_as(f32p), one.ctypes.data_as(f32p),
                                           one.ctypes.data_as(f32p), 0.1, dims.ctypes.data_as(C.POINTER(C.c_int32)))
        with pytest.raises(amvs.AmvsError, match="over the budget"):
            eng._chk(rc)
        # the context still works, and the refused calls left the volume in place
        _assert_mesh_equal(eng.tsdf_extract(), vol.extract(), vol.name + " after refused calls")


def test_generated_volumes_bit_exact():
    """set_volume -> extract against the restatement, bit for bit, on every small generated volume: the random-sign
    family (all 84 tetrahedron cases, ragged and thin shapes, garbage behind unobserved points), closed random-sign
    surfaces, spheres of both orientations, planes through grid points, and the corner cases (0 vertices and 0 faces
    among them)."""
    empty = 0
    with _engine() as eng:
        for vol in mv.small_volumes():
            ref = vol.extract()
            _assert_mesh_equal(_extract(eng, vol), ref, vol.name)
            empty += len(ref[1]) == 0
    assert empty >= 10
    for vol, expect in mv.colour_tie_volumes():                   # on a fresh context each, nothing left over
        with _engine() as eng:
            mesh = _extract(eng, vol)
            assert np.all(mesh[2] == expect[None, :]), vol.name
            _assert_mesh_equal(mesh, vol.extract(), vol.name)


def test_single_cube_every_sign_pattern():
    with _engine() as eng:
        for pattern in range(256):
            vol = mv.cube_volume(pattern)
            _assert_mesh_equal(_extract(eng, vol), vol.extract(), vol.name)


def test_fetch_mesh_skips_null_outputs():
    vol = mv.random_sign_volume((9, 8, 7), 12)
    rv, rf, rc = vol.extract()
    with _engine() as eng:
        eng.tsdf_set_volume(*vol.arrays())
        nv, nf = C.c_int64(-1), C.c_int64(-1)
        eng._chk(eng._lib.amvs_tsdf_extract(eng._h, C.byref(nv), C.byref(nf)))
        assert (nv.value, nf.value) == (len(rv), len(rf))
        f32p, i32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        eng._chk(eng._lib.amvs_fetch_mesh(eng._h, None, None, None))
        for which in range(3):
            verts = np.full((len(rv), 3), 7.0, np.float32)
            faces = np.full((len(rf), 3), -7, np.int32)
            cols = np.full((len(rv), 3), 7, np.uint8)
            args = [verts.ctypes.data_as(f32p), faces.ctypes.data_as(i32p), cols.ctypes.data_as(u8p)]
            args[which] = None
            eng._chk(eng._lib.amvs_fetch_mesh(eng._h, *args))
            assert np.all(verts == 7.0) if which == 0 else _same_bits(verts, rv)
            assert np.all(faces == -7) if which == 1 else np.array_equal(faces, rf)
            assert np.all(cols == 7) if which == 2 else np.array_equal(cols, rc)
        # an empty mesh: counts 0 and 0, and a fetch that writes nothing
        eng.tsdf_set_volume(*mv.constant_volume(0.75).arrays())
        eng._chk(eng._lib.amvs_tsdf_extract(eng._h, C.byref(nv), C.byref(nf)))
        assert (nv.value, nf.value) == (0, 0)
        eng._chk(eng._lib.amvs_fetch_mesh(eng._h, None, None, None))


LARGE_N = 160


def test_large_volume_then_small_ones_on_the_same_context():
    """A sphere on 160^3 = 4.1 M points (the scans run thousands of tiles), element for element against the
    restatement; then a small random-sign volume on the same context, whose buffers only grow, so that anything the
    large mesh left behind would show; then the same small volume once more."""
    big = mv.sphere_volume(LARGE_N)
    assert int(np.prod(big.dims)) >= 4_000_000
    ref = big.extract()
    assert len(ref[1]) >= 400_000, len(ref[1])
    small = mv.random_sign_volume((23, 19, 17), 2024)
    small_ref = small.extract()
    tiny = mv.cube_volume(0x5a)
    with _engine() as eng:
        _assert_mesh_equal(_extract(eng, big), ref, big.name)
        del ref
        first = _extract(eng, small)
        _assert_mesh_equal(first, small_ref, small.name + " after the large volume")
        second = _extract(eng, small)
        _assert_mesh_equal(second, first, small.name + " a second time")
        _assert_mesh_equal(_extract(eng, tiny), tiny.extract(), tiny.name + " after both")
        _assert_mesh_equal(_extract(eng, mv.constant_volume(-0.75)), (np.zeros((0, 3)),) * 3, "all inside after both")


def test_operating_point_256_cubed_is_a_closed_sphere():
    """The README's operating point, a 256^3 volume (16.7 M points).  Properties only: the NumPy restatement of the
    extraction took 13 s and 3.2 GB at 160^3 and would need four times that here, which the suite's budget does not
    have (the 160^3 test above is the largest element-for-element comparison).  The device mesh of a sphere must be
    closed and consistently oriented (every directed edge once, its opposite once), a topological sphere
    (F == 2 V - 4), outward, and within one voxel of the radius."""
    radius = 0.8
    vol = mv.sphere_volume(256, radius=radius)
    with _engine() as eng:
        verts, faces, cols = _extract(eng, vol)
    assert len(faces) > 1_000_000
    assert faces.min() == 0 and faces.max() == len(verts) - 1
    assert mv.directed_edge_defects(faces, len(verts)) == (0, 0)
    assert len(faces) == 2 * len(verts) - 4
    r = np.linalg.norm(verts.astype(np.float64), axis=1)
    assert np.abs(r - radius).max() <= float(vol.voxel), np.abs(r - radius).max() / float(vol.voxel)
    assert mv.signed_volume(verts, faces) == pytest.approx(4.0 / 3.0 * np.pi * radius ** 3, rel=1e-3)
    assert cols.shape == verts.shape


def _integrate_and_compare(eng, sc, what, order=None, **source):
    o = list(range(sc.n)) if order is None else list(order)
    poses = sc.pose_list()
    mesh = eng.tsdf_mesh(sc.K, [poses[i] for i in o], sc.min_views, sc.origin, sc.voxel, sc.dims, sc.trunc, **source)
    tsdf, weight, color = eng.tsdf_volume()
    rt, rw, rc = sc.integrate(o)
    assert np.any(rw > 0), f"{what}: nothing observed (test set-up)"
    assert _same_bits(weight, rw), f"{what}: weight differs in {int((weight != rw).sum())} points"
    assert _same_bits(tsdf, rt), f"{what}: tsdf differs in {int((tsdf != rt).sum())} points"
    assert _same_bits(color, rc), f"{what}: colour sums differ"
    ref = mr.extract(rt, rw, rc, sc.origin, sc.voxel)
    assert len(ref[1]) > 0, f"{what}: empty mesh (test set-up)"
    _assert_mesh_equal(mesh, ref, what)


@pytest.mark.parametrize("index", range(4), ids=["exact-cx8", "exact-cx7.5", "camera-inside", "content"])
def test_integration_edges_bit_exact(index):
    """Hand-built scenes at the integration's edges (tests/mesh_volumes.py): pixel ties of floorf(u + 0.5f) on whole
    columns, u == -0.5 and u == W - 0.5, sdf == -trunc and one ulp beyond, sdf / trunc == 1; cameras inside the box
    (zc == 0, zc tiny, quotients that overflow); 0, -0.0, negative, NaN and inf in the maps."""
    sc = mv.integration_scenes()[index]
    with _engine(sc.H, sc.W, sc.n, sc.K) as eng:
        _integrate_and_compare(eng, sc, sc.name, depth=sc.depth, conf=sc.conf, colors_bgr=sc.colors)


def test_integration_of_many_maps_bit_exact():
    """17 maps: weights from 0 to 17 and means that divide by every count; host colours in map order, then device
    maps with the resident colour images of permuted views."""
    import torch
    sc = mv.many_maps_scene()
    with _engine(sc.H, sc.W, sc.n, sc.K) as eng:
        _integrate_and_compare(eng, sc, sc.name + ", host", depth=sc.depth, conf=sc.conf, colors_bgr=sc.colors)
        for i in range(sc.n):
            eng.set_view_colors(i, sc.colors[i])
        order = np.random.default_rng(9).permutation(sc.n)
        assert not np.array_equal(order, np.arange(sc.n))
        d_t = torch.from_numpy(sc.depth[order]).cuda()
        c_t = torch.from_numpy(sc.conf[order]).cuda()
        torch.cuda.synchronize()
        _integrate_and_compare(eng, sc, sc.name + ", resident colours", order=order,
                               device_ptrs=(d_t.data_ptr(), c_t.data_ptr(), sc.n), view_ids=[int(i) for i in order])
