"""The decimation with quadric placement (csrc/amvs_mesh_decimate.hip, include/amvs.h amvs_mesh_decimate_quadric) against
the NumPy restatement (tests/mesh_quadric_restatement.py), bit for bit: positions as uint32 views, faces and colours
element for element, the three counts.  The meshes are the ones test_mesh_quadric_cpu.py checks for coverage: what the
generated volumes of tests/mesh_volumes.py and the rotated box extract (fed through amvs_tsdf_set_volume +
amvs_tsdf_extract), the hand-built meshes of tests/mesh_clean_inputs.py and the inputs of tests/mesh_quadric_inputs.py
(fed through amvs_mesh_set)."""
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
import mesh_quadric_inputs as qi  # noqa: E402
import mesh_quadric_restatement as qr  # noqa: E402
import mesh_volumes as mv  # noqa: E402
from mesh_hip_common import K_ANY, _engine, _same_bits, _scene_a_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
REGS = (1e-3, 0.1)


def _assert_mesh_equal(mesh, ref, what):
    verts, faces, cols = mesh[:3]
    rv, rf, rc = ref[:3]
    assert (len(verts), len(faces)) == (len(rv), len(rf)), f"{what}: {len(verts)} / {len(faces)} vs {len(rv)} / {len(rf)}"
    assert verts.shape == (len(rv), 3) and faces.shape == (len(rf), 3) and cols.shape == (len(rv), 3)
    assert np.array_equal(faces, rf), f"{what}: faces differ, first at {np.argwhere(faces != rf)[:1]}"
    assert _same_bits(verts, rv), (f"{what}: vertex positions differ in "
                                   f"{int((verts.view(np.uint32) != rv.view(np.uint32)).any(axis=1).sum())} vertices")
    assert np.array_equal(cols, rc), f"{what}: vertex colours differ"


class Source:
    """A mesh of the family, the way it reaches the device, and the grids it is decimated on: (origin, cell) pairs;
    `own` is a regularisation to run on the first grid besides REGS."""

    def __init__(self, eng, name, grids, arrays=None, volume=None, own=None):
        self.eng, self.name, self.volume, self.grids, self.own = eng, name, volume, grids, own
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
    for vol in [qi.rotated_box()] + mv.small_volumes():
        yield Source(eng, vol.name, _grids(vol.origin, vol.voxel), volume=vol)
    for m in ci.hand_built():
        yield Source(eng, m.name, _grids((0.0, 0.0, 0.0), 0.15), arrays=m.arrays())
    for case in qi.hand_built():
        yield Source(eng, case.name, [(case.origin, case.cell)] + _grids(case.origin, case.unit)[1:], arrays=case.arrays(),
                     own=case.regularisation)


def _check_quadric(eng, src, prep, origin, cell, reg, what):
    rv, rf, rc, rk = prep.place(reg)
    src.reset()
    got = eng.mesh_decimate_quadric(origin, cell, reg)
    assert got == (len(rv), len(rf), rk), f"{what}: {got} vs {(len(rv), len(rf), rk)}"
    _assert_mesh_equal(eng.mesh_fetch(), (rv, rf, rc), what)
    eng.mesh_normals()
    n = eng.mesh_fetch(normals=True)[3]
    assert _same_bits(n, cr.normals(rv, rf)), f"{what}: normals differ"
    return rk, len(rf)


def test_family_bit_exact_on_one_context():
    """Every mesh of the family on ONE context (the buffers only grow: large meshes come before small ones and the
    empty one), on cells of 2 and 3 units with the grid's origin on and off the mesh's, at regularisation 1e-3 and 0.1
    (and the value a case was built for): the three returned counts, the mesh, and the normals computed on it
    afterwards.  On the first grid of every mesh a plain mesh_decimate between two quadric calls still equals
    mesh_decimate_restatement.decimate: the passes and buffers the two placements share do not leak."""
    n_runs = n_fallback = n_faces_out = n_mean_checks = 0
    with _engine() as eng:
        for src in _sources(eng):
            for g, (origin, cell) in enumerate(src.grids):
                prep = qr.Prepared(src.v, src.f, src.c, origin, cell)
                regs = REGS + ((src.own,) if g == 0 and src.own is not None else ())
                for r, reg in enumerate(regs):
                    what = f"{src.name}, origin {origin}, cell {cell}, regularisation {reg}"
                    rk, nf = _check_quadric(eng, src, prep, origin, cell, reg, what)
                    n_runs += 1
                    n_fallback += rk
                    n_faces_out += nf
                    if g == 0 and r == 0:
                        src.reset()
                        ref = dr.decimate(src.v, src.f, src.c, origin, cell)
                        assert eng.mesh_decimate(origin, cell) == (len(ref[0]), len(ref[1])), what
                        _assert_mesh_equal(eng.mesh_fetch(), ref, what + ", mean placement between two quadric calls")
                        n_mean_checks += 1
        from amvs import _lib
        assert _lib.index_check()[0] == 0
    assert n_runs >= 380 and n_mean_checks >= 40 and n_fallback >= 500 and n_faces_out >= 60_000


def test_large_sphere_bit_exact_then_a_small_mesh():
    """The 160^3 sphere (455 880 faces, the device's own extraction) once at 2 voxels, then a small mesh on the same
    context."""
    big = mv.sphere_volume(160)
    with _engine() as eng:
        eng.tsdf_set_volume(*big.arrays())
        v, f, c = eng.tsdf_extract()
        assert len(f) >= 400_000
        cell = F32(2) * big.voxel
        ref = qr.decimate_quadric(v, f, c, big.origin, cell, 1e-3)
        got = eng.mesh_decimate_quadric(big.origin, cell)
        print(f"160^3 sphere: {got}")
        assert got == (len(ref[0]), len(ref[1]), ref[3]) and got[:2] == (18650, 37296)
        _assert_mesh_equal(eng.mesh_fetch(), ref, big.name)
        case = qi.wedge()
        eng.mesh_set(*case.arrays())
        small = qr.decimate_quadric(*case.arrays(), case.origin, case.cell, 1e-3)
        assert eng.mesh_decimate_quadric(case.origin, case.cell, 1e-3) == (len(small[0]), len(small[1]), small[3])
        assert small[3] >= 1
        _assert_mesh_equal(eng.mesh_fetch(), small, case.name + " after the large sphere")
        from amvs import _lib
        assert _lib.index_check()[0] == 0


def _run(eng, vol, origin, cell, reg):
    eng.tsdf_set_volume(*vol.arrays())
    eng.tsdf_extract()
    counts = eng.mesh_decimate_quadric(origin, cell, reg)
    eng.mesh_normals()
    return counts, eng.mesh_fetch(normals=True)


def test_same_bits_twice_and_on_a_fresh_context():
    vol = mv.random_sign_volume((23, 19, 17), 2024)
    other = mv.sphere_volume(33, trunc=0.2)
    args = (vol, vol.origin + F32(0.37) * vol.voxel, F32(2) * vol.voxel, 1e-3)
    with _engine() as eng:
        first = _run(eng, *args)
        _run(eng, other, other.origin, F32(3) * other.voxel, 0.1)       # something else in between
        second = _run(eng, *args)
    with _engine() as eng:
        third = _run(eng, *args)
    assert first[0][0] > 0 and first[0][1] > 0 and 0 < first[0][2] < first[0][0]
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
        with pytest.raises(amvs.AmvsError, match="mesh_decimate_quadric: no mesh"):
            eng.mesh_decimate_quadric(origin, 1.0)
        eng.mesh_set(v, f, c)
        # the arguments
        nv, nf, nk = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        org = origin.ctypes.data_as(C.POINTER(C.c_float))
        outs = (C.byref(nv), C.byref(nf), C.byref(nk))
        for missing in range(3):
            args = tuple(None if k == missing else o for k, o in enumerate(outs))
            with pytest.raises(amvs.AmvsError, match="mesh_decimate_quadric: NULL output"):
                eng._chk(eng._lib.amvs_mesh_decimate_quadric(eng._h, org, 1.0, 1e-3, *args))
        with pytest.raises(amvs.AmvsError, match="mesh_decimate_quadric: NULL origin"):
            eng._chk(eng._lib.amvs_mesh_decimate_quadric(eng._h, None, 1.0, 1e-3, *outs))
        for bad in (np.nan, np.inf, -np.inf):
            for axis in range(3):
                o = origin.copy(); o[axis] = bad
                with pytest.raises(amvs.AmvsError, match="mesh_decimate_quadric: origin must be finite"):
                    eng.mesh_decimate_quadric(o, 1.0)
        for cell in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf):
            with pytest.raises(amvs.AmvsError, match="mesh_decimate_quadric: cell must be positive and finite"):
                eng.mesh_decimate_quadric(origin, cell)
        for reg in (0.0, -0.0, -1e-3, np.nextafter(F32(1), F32(2)), 2.0, np.nan, np.inf, -np.inf):
            with pytest.raises(amvs.AmvsError, match=r"mesh_decimate_quadric: regularisation must be in \(0, 1\]"):
                eng.mesh_decimate_quadric(origin, 1.0, reg)
        _assert_mesh_equal(eng.mesh_fetch(), (v, f, c), "after the refused arguments")
        # labels and normals do not survive a decimation; regularisation 1 is inside the range
        eng.mesh_filter_components(); eng.mesh_normals()
        assert len(eng.mesh_fetch(normals=True, labels=True)) == 5
        ref = qr.decimate_quadric(v, f, c, origin, 0.5, 1.0)
        assert eng.mesh_decimate_quadric(origin, 0.5, 1.0) == (len(ref[0]), len(ref[1]), ref[3])
        for flag in (dict(normals=True), dict(labels=True)):
            with pytest.raises(amvs.AmvsError, match="no current"):
                eng.mesh_fetch(**flag)
        _assert_mesh_equal(eng.mesh_fetch(), ref, m.name)
        # the clean-up works on the decimated mesh as on any other (the index is rebuilt)
        n_comp, rv, rf, rc, rlab, rn = cr.pipeline(*ref[:3], 1, False, 2)
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
            with pytest.raises(amvs.AmvsError, match="mesh_decimate_quadric: vertex 3 outside the cluster grid"):
                eng.mesh_decimate_quadric(case.origin, case.cell)
            after = eng.mesh_fetch(normals=True, labels=True)
            assert len(after) == 5 and all(a.tobytes() == b.tobytes() for a, b in zip(before, after)), case.name
            eng.mesh_smooth(1)                                    # the index is still the mesh's
            _assert_mesh_equal(eng.mesh_fetch(), (cr.smooth(case.verts, case.faces, 1), case.faces, case.colors), case.name)
        # the same refusal on a mesh whose index was never built
        case = di.refused_cases()[0]
        eng.mesh_set(*case.arrays())
        with pytest.raises(amvs.AmvsError, match="mesh_decimate_quadric: vertex 3 outside the cluster grid"):
            eng.mesh_decimate_quadric(case.origin, case.cell)
        _assert_mesh_equal(eng.mesh_fetch(), case.arrays(), case.name)
        ref = qr.decimate_quadric(*case.arrays(), case.origin, 2.0)
        assert eng.mesh_decimate_quadric(case.origin, 2.0) == (len(ref[0]), len(ref[1]), ref[3])
        _assert_mesh_equal(eng.mesh_fetch(), ref, case.name + ", cell 2")
        # nothing at all, vertices only (every cluster keeps the mean), and everything collapsed into one cell
        for mesh_in in (ci.empty().arrays(), ci.vertices_only().arrays(), (v, f, c)):
            eng.mesh_set(*mesh_in)
            ref = qr.decimate_quadric(*mesh_in, origin - F32(50.0), 100.0)
            assert eng.mesh_decimate_quadric(origin - F32(50.0), 100.0) == (0, 0, ref[3])
            assert ref[3] == min(len(mesh_in[0]), 1) or len(mesh_in[1]) > 0
            assert [a.shape for a in eng.mesh_fetch()] == [(0, 3), (0, 3), (0, 3)]
            eng.mesh_normals()
            assert eng.mesh_decimate_quadric(origin, 1.0) == (0, 0, 0)     # and again on the empty result
        eng.mesh_set(*ci.vertices_only().arrays())
        ref = qr.decimate_quadric(*ci.vertices_only().arrays(), origin, 0.3)
        assert eng.mesh_decimate_quadric(origin, 0.3) == (0, 0, ref[3]) and ref[3] >= 2
        from amvs import _lib
        assert _lib.index_check()[0] == 0


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_reconstruct_mesh_quadric_end_to_end(mode, scene_a, capsys):
    """On scene_a (5 views of 96 x 64), in both arithmetic modes: reconstruct_mesh(..., decimate_voxels=2.0,
    decimate_placement="quadric", smooth_iterations=3, with_normals=True) equals the restatements chained, smooth ->
    quadric decimation -> normals, on what the default call returns; the clean-up line names the placement and the
    clusters that kept the mean; the default call returns the same mesh after it as before it; any other placement
    string is a ValueError."""
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    camera, images, poses, sparse = _scene_a_inputs(scene_a)
    pm = PatchMatchMVS(camera, scale=1.0, patch_size=7, num_iterations=4, num_samples=6, min_views=2, seed=2, device=0,
                       mode=mode)
    base = pm.reconstruct_mesh(images, poses, sparse, max_dim=64)
    assert len(base) == 3
    v, f, c = base
    assert len(f) > 100
    capsys.readouterr()
    got = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, decimate_voxels=2.0, decimate_placement="quadric",
                              smooth_iterations=3, with_normals=True)
    line = [ln for ln in capsys.readouterr().out.splitlines() if "Clean-up" in ln]
    assert len(got) == 4
    origin, voxel = pm.last_mesh_grid[:2]
    org, cell = np.asarray(origin, np.float64).astype(F32), F32(2.0) * F32(voxel)
    sv = cr.smooth(v, f, 3, 0.5, -0.53, True)
    rv, rf, rc, rk = qr.decimate_quadric(sv, f, c, org, cell, 1e-3)
    print(f"{mode}: {len(v)} vertices, {len(f)} faces -> {len(rv)} / {len(rf)}, {rk} kept the mean")
    assert 0 < len(rf) < len(f)
    _assert_mesh_equal(got, (rv, rf, rc), mode)
    assert _same_bits(got[3], cr.normals(rv, rf)), mode
    mean = dr.decimate(sv, f, c, org, cell)
    assert np.array_equal(mean[1], rf) and not _same_bits(mean[0], rv)
    assert len(line) == 1, line
    assert f"decimation at 2 voxels, quadric placement ({rk:,} kept the mean): {len(f):,} faces -> {len(rf):,}" in line[0], line
    # another regularisation reaches the device
    other = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, decimate_voxels=2.0, decimate_placement="quadric",
                                decimate_regularisation=0.1)
    ref = qr.decimate_quadric(v, f, c, org, cell, 0.1)
    assert len(other) == 3
    _assert_mesh_equal(other, ref, mode + ", regularisation 0.1")
    # the default placement prints and returns what it did
    capsys.readouterr()
    plain = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, decimate_voxels=2.0)
    line = [ln for ln in capsys.readouterr().out.splitlines() if "Clean-up" in ln]
    ref = dr.decimate(v, f, c, org, cell)
    _assert_mesh_equal(plain, ref, mode + ", mean placement")
    assert len(line) == 1 and f"decimation at 2 voxels: {len(f):,} faces -> {len(ref[1]):,}" in line[0], line
    again = pm.reconstruct_mesh(images, poses, sparse, max_dim=64)
    assert len(again) == 3
    _assert_mesh_equal(again, base, mode + ", the default call again")
    for bad in ("Quadric", "qem", "", None):
        with pytest.raises(ValueError, match="decimate_placement"):
            pm.reconstruct_mesh(images, poses, sparse, max_dim=64, decimate_voxels=2.0, decimate_placement=bad)
