"""The decimation kernels (csrc/amvs_mesh_decimate.hip, include/amvs.h amvs_mesh_decimate) against the NumPy
restatement (tests/mesh_decimate_restatement.py), bit for bit: positions as uint32 views, faces and colours element
for element.  The meshes are the ones test_mesh_decimate_cpu.py checks for coverage: what the generated volumes of
tests/mesh_volumes.py extract (fed through amvs_tsdf_set_volume + amvs_tsdf_extract), the hand-built meshes of
tests/mesh_clean_inputs.py and the inputs of tests/mesh_decimate_inputs.py (fed through amvs_mesh_set)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_inputs as ci  # noqa: E402
import mesh_clean_restatement as cr  # noqa: E402
import mesh_decimate_inputs as di  # noqa: E402
import mesh_decimate_restatement as dr  # noqa: E402
import mesh_volumes as mv  # noqa: E402
from mesh_hip_common import K_ANY, _engine, _same_bits, _assert_mesh_equal, _scene_a_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32


class Source:
    """A mesh of the family, the way it reaches the device, and the grids it is decimated on: (origin, cell) pairs."""

    def __init__(self, eng, name, grids, arrays=None, volume=None):
        self.eng, self.name, self.volume, self.grids = eng, name, volume, grids
        if volume is not None:
            eng.tsdf_set_volume(*volume.arrays())
            arrays = volume.extract()
        self.v, self.f, self.c = arrays

    def reset(self):
        if self.volume is not None:
            self.eng.tsdf_extract()
        else:
            self.eng.mesh_set(self.v, self.f, self.c)


def _grids(origin, unit):
    """cells of 2 and 3 units, on the origin and off it"""
    origin, unit = np.asarray(origin, F32), F32(unit)
    off = (origin + F32(0.37) * unit).astype(F32)
    return [(origin, F32(2) * unit), (off, F32(2) * unit), (origin, F32(3) * unit), (off, F32(3) * unit)]


def _sources(eng):
    for vol in mv.small_volumes():
        yield Source(eng, vol.name, _grids(vol.origin, vol.voxel), volume=vol)
    for m in ci.hand_built():
        yield Source(eng, m.name, _grids((0.0, 0.0, 0.0), 0.15), arrays=m.arrays())
    for case in di.accepted_cases():
        yield Source(eng, case.name, [(case.origin, case.cell)] + _grids(case.origin, case.cell)[1:], arrays=case.arrays())


def test_family_bit_exact_on_one_context():
    """Every mesh of the family on ONE context (the buffers only grow: large meshes come before small ones and the
    empty one), on cells of 2 and 3 voxels with the grid's origin on and off the volume's (the hand-built meshes: cells
    of 0.3 and 0.45 at 0 and off it; the new inputs: also their own grid): the returned counts, the mesh, and the
    normals computed on it afterwards."""
    n_runs = n_empty = n_faces_out = 0
    with _engine() as eng:
        for src in _sources(eng):
            for origin, cell in src.grids:
                what = f"{src.name}, origin {origin}, cell {cell}"
                src.reset()
                rv, rf, rc = dr.decimate(src.v, src.f, src.c, origin, cell)
                got = eng.mesh_decimate(origin, cell)
                assert got == (len(rv), len(rf)), f"{what}: {got} vs {(len(rv), len(rf))}"
                _assert_mesh_equal(eng.mesh_fetch(), (rv, rf, rc), what)
                eng.mesh_normals()
                n = eng.mesh_fetch(normals=True)[3]
                assert _same_bits(n, cr.normals(rv, rf)), f"{what}: normals differ"
                n_runs += 1
                n_empty += len(rf) == 0
                n_faces_out += len(rf)
    assert n_runs >= 150 and n_empty >= 40 and n_faces_out >= 30_000


def _closed_sphere(faces, n_vertices):
    return mv.directed_edge_defects(faces, n_vertices) == (0, 0) and len(faces) == 2 * n_vertices - 4


def test_large_sphere_bit_exact_then_a_small_mesh():
    """The 160^3 sphere (455 880 faces, the device's own extraction) once at 2 voxels, then a small mesh on the same
    context."""
    big = mv.sphere_volume(160)
    with _engine() as eng:
        eng.tsdf_set_volume(*big.arrays())
        v, f, c = eng.tsdf_extract()
        assert len(f) >= 400_000
        cell = F32(2) * big.voxel
        ref = dr.decimate(v, f, c, big.origin, cell)
        assert eng.mesh_decimate(big.origin, cell) == (len(ref[0]), len(ref[1])) == (18650, 37296)
        _assert_mesh_equal(eng.mesh_fetch(), ref, big.name)
        assert _closed_sphere(ref[1], len(ref[0]))
        case = di.windings()
        eng.mesh_set(*case.arrays())
        small = dr.decimate(*case.arrays(), case.origin, case.cell)
        assert eng.mesh_decimate(case.origin, case.cell) == (len(small[0]), len(small[1]))
        _assert_mesh_equal(eng.mesh_fetch(), small, case.name + " after the large sphere")


def test_operating_point_256_cubed_sphere_bit_exact_and_closed():
    """The 256^3 sphere (1 173 456 faces) at 2 voxels: bit for bit, closed, F = 2 V - 4."""
    vol = mv.sphere_volume(256, radius=0.8)
    with _engine() as eng:
        eng.tsdf_set_volume(*vol.arrays())
        v, f, c = eng.tsdf_extract()
        assert len(f) > 1_000_000
        cell = F32(2) * vol.voxel
        ref = dr.decimate(v, f, c, vol.origin, cell)
        got = eng.mesh_decimate(vol.origin, cell)
        print(f"256^3 sphere: {len(v):,} vertices, {len(f):,} faces -> {got[0]:,} / {got[1]:,}")
        assert got == (len(ref[0]), len(ref[1]))
        mesh = eng.mesh_fetch()
    _assert_mesh_equal(mesh, ref, vol.name)
    assert _closed_sphere(mesh[1], len(mesh[0]))
    assert len(mesh[1]) <= len(f) / 8


def _run(eng, vol, origin, cell):
    eng.tsdf_set_volume(*vol.arrays())
    eng.tsdf_extract()
    counts = eng.mesh_decimate(origin, cell)
    eng.mesh_normals()
    return counts, eng.mesh_fetch(normals=True)


def test_same_bits_twice_and_on_a_fresh_context():
    vol = mv.random_sign_volume((23, 19, 17), 2024)
    other = mv.sphere_volume(33, trunc=0.2)
    args = (vol, vol.origin + F32(0.37) * vol.voxel, F32(2) * vol.voxel)
    with _engine() as eng:
        first = _run(eng, *args)
        _run(eng, other, other.origin, F32(3) * other.voxel)       # something else in between
        second = _run(eng, *args)
    with _engine() as eng:
        third = _run(eng, *args)
    assert first[0][0] > 0 and first[0][1] > 0
    for again in (second, third):
        assert again[0] == first[0]
        for a, b in zip(again[1], first[1]):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_state_rules_and_errors():
    import amvs
    m = ci.threshold()
    v, f, c = m.arrays()
    origin = np.zeros(3, F32)
    with _engine() as eng:
        with pytest.raises(amvs.AmvsError, match="mesh_decimate: no mesh"):
            eng.mesh_decimate(origin, 1.0)
        eng.mesh_set(v, f, c)
        # the arguments
        nv, nf = C.c_int64(0), C.c_int64(0)
        org = origin.ctypes.data_as(C.POINTER(C.c_float))
        for args in ((org, 1.0, None, C.byref(nf)), (org, 1.0, C.byref(nv), None), (None, 1.0, C.byref(nv), C.byref(nf))):
            with pytest.raises(amvs.AmvsError, match="mesh_decimate: NULL"):
                eng._chk(eng._lib.amvs_mesh_decimate(eng._h, *args))
        for bad in (np.nan, np.inf, -np.inf):
            for axis in range(3):
                o = origin.copy(); o[axis] = bad
                with pytest.raises(amvs.AmvsError, match="mesh_decimate: origin must be finite"):
                    eng.mesh_decimate(o, 1.0)
        for cell in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf):
            with pytest.raises(amvs.AmvsError, match="mesh_decimate: cell must be positive and finite"):
                eng.mesh_decimate(origin, cell)
        _assert_mesh_equal(eng.mesh_fetch(), (v, f, c), "after the refused arguments")
        # labels and normals do not survive a decimation
        eng.mesh_filter_components(); eng.mesh_normals()
        assert len(eng.mesh_fetch(normals=True, labels=True)) == 5
        ref = dr.decimate(v, f, c, origin, 0.5)
        assert eng.mesh_decimate(origin, 0.5) == (len(ref[0]), len(ref[1]))
        for flag in (dict(normals=True), dict(labels=True)):
            with pytest.raises(amvs.AmvsError, match="no current"):
                eng.mesh_fetch(**flag)
        _assert_mesh_equal(eng.mesh_fetch(), ref, m.name)
        # the clean-up works on the decimated mesh as on any other
        n_comp, rv, rf, rc, rlab, rn = cr.pipeline(*ref, 1, False, 2)
        assert eng.mesh_filter_components(1) == (n_comp, len(rv), len(rf))
        eng.mesh_smooth(2)
        eng.mesh_normals()
        mesh = eng.mesh_fetch(normals=True, labels=True)
        _assert_mesh_equal(mesh, (rv, rf, rc), m.name + ", clean-up after the decimation")
        assert _same_bits(mesh[3], rn) and np.array_equal(mesh[4], rlab)
        # a vertex outside the cluster grid: refused, and the mesh with its attributes is as before
        for case in di.refused_cases():
            eng.mesh_set(*case.arrays())
            eng.mesh_filter_components(); eng.mesh_normals()
            before = eng.mesh_fetch(normals=True, labels=True)
            with pytest.raises(amvs.AmvsError, match="mesh_decimate: vertex 3 outside the cluster grid"):
                eng.mesh_decimate(case.origin, case.cell)
            after = eng.mesh_fetch(normals=True, labels=True)
            assert len(after) == 5 and all(a.tobytes() == b.tobytes() for a, b in zip(before, after)), case.name
            eng.mesh_smooth(1)                                    # the index is still the mesh's
            _assert_mesh_equal(eng.mesh_fetch(), (cr.smooth(case.verts, case.faces, 1), case.faces, case.colors), case.name)
        # far from the origin the same mesh is inside a coarser grid
        case = di.refused_cases()[0]
        eng.mesh_set(*case.arrays())
        ref = dr.decimate(*case.arrays(), case.origin, 2.0)
        assert eng.mesh_decimate(case.origin, 2.0) == (len(ref[0]), len(ref[1]))
        _assert_mesh_equal(eng.mesh_fetch(), ref, case.name + ", cell 2")
        # nothing at all, vertices only, and everything collapsed into one cell
        for mesh_in in (ci.empty().arrays(), ci.vertices_only().arrays(), (v, f, c)):
            eng.mesh_set(*mesh_in)
            assert eng.mesh_decimate(origin - F32(50.0), 100.0) == (0, 0)
            assert [a.shape for a in eng.mesh_fetch()] == [(0, 3), (0, 3), (0, 3)]
            eng.mesh_normals()
            assert eng.mesh_decimate(origin, 1.0) == (0, 0)        # and again on the empty result
        from amvs import _lib
        assert _lib.index_check()[0] == 0


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_reconstruct_mesh_decimation_end_to_end(mode, scene_a, capsys):
    """On scene_a (5 views of 96 x 64), in both arithmetic modes: reconstruct_mesh(..., decimate_voxels=2.0,
    smooth_iterations=3, with_normals=True) equals the restatements chained, smooth -> decimate -> normals, on what
    the default call returns, and the default call returns the same mesh after it as before it."""
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    camera, images, poses, sparse = _scene_a_inputs(scene_a)
    pm = PatchMatchMVS(camera, scale=1.0, patch_size=7, num_iterations=4, num_samples=6, min_views=2, seed=2, device=0,
                       mode=mode)
    base = pm.reconstruct_mesh(images, poses, sparse, max_dim=64)
    assert len(base) == 3
    v, f, c = base
    assert len(f) > 100
    capsys.readouterr()
    got = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, decimate_voxels=2.0, smooth_iterations=3,
                              with_normals=True)
    line = [ln for ln in capsys.readouterr().out.splitlines() if "Clean-up" in ln]
    assert len(got) == 4
    origin, voxel = pm.last_mesh_grid[:2]
    sv = cr.smooth(v, f, 3, 0.5, -0.53, True)
    rv, rf, rc = dr.decimate(sv, f, c, np.asarray(origin, np.float64).astype(F32), F32(2.0) * F32(voxel))
    print(f"{mode}: {len(v)} vertices, {len(f)} faces -> {len(rv)} / {len(rf)}")
    assert 0 < len(rf) < len(f)
    _assert_mesh_equal(got, (rv, rf, rc), mode)
    assert _same_bits(got[3], cr.normals(rv, rf)), mode
    assert len(line) == 1 and f"{len(f):,} faces -> {len(rf):,}" in line[0], line
    # with the filter: its part of the line is taken before the decimation
    both = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, min_component_faces=50, decimate_voxels=2.0)
    n_comp, fv, ff, fc, flab = cr.filter(v, f, c, 50)
    line = [ln for ln in capsys.readouterr().out.splitlines() if "Clean-up" in ln]
    ref = dr.decimate(fv, ff, fc, np.asarray(origin, np.float64).astype(F32), F32(2.0) * F32(voxel))
    assert len(both) == 3
    _assert_mesh_equal(both, ref, mode + ", filter and decimation")
    assert len(line) == 1 and f"{n_comp:,} components -> {len(np.unique(flab)):,}, {len(ff):,} faces" in line[0], line
    assert f"{len(ff):,} faces -> {len(ref[1]):,}" in line[0], line
    again = pm.reconstruct_mesh(images, poses, sparse, max_dim=64)
    assert len(again) == 3
    _assert_mesh_equal(again, base, mode + ", the default call again")
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="decimate_voxels"):
            pm.reconstruct_mesh(images, poses, sparse, max_dim=64, decimate_voxels=bad)
