"""The mesh clean-up kernels (csrc/amvs_mesh_clean.hip, include/amvs.h amvs_mesh_*) against the NumPy restatement
(tests/mesh_clean_restatement.py), bit for bit: positions and normals as uint32 views, faces, colours and labels
element for element.  The meshes are the ones test_mesh_clean_cpu.py checks for coverage: what the generated volumes
of tests/mesh_volumes.py extract (fed through amvs_tsdf_set_volume + amvs_tsdf_extract) and the hand-built meshes of
tests/mesh_clean_inputs.py (fed through amvs_mesh_set)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_inputs as ci  # noqa: E402
import mesh_clean_restatement as cr  # noqa: E402
import mesh_volumes as mv  # noqa: E402
from mesh_hip_common import K_ANY, _engine, _same_bits, _assert_mesh_equal, _scene_a_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

FILTERS = ((0, False), (1, False), (8, False), (10 ** 9, False), (0, True))
ITERATIONS = (0, 1, 3, 10)


def _assert_normals_equal(n, ref, what):
    assert _same_bits(n, ref), f"{what}: normals differ in {int((n != ref).any(axis=1).sum())} of {len(ref)} vertices"


class Source:
    """A mesh of the family and the way it reaches the device: reset() makes it the context's current mesh again."""

    def __init__(self, eng, name, arrays=None, volume=None):
        self.eng, self.name, self.volume = eng, name, volume
        if volume is not None:
            eng.tsdf_set_volume(*volume.arrays())
            arrays = volume.extract()
        self.v, self.f, self.c = arrays

    def reset(self):
        if self.volume is not None:
            mesh = self.eng.tsdf_extract()
        else:
            self.eng.mesh_set(self.v, self.f, self.c)
            mesh = self.eng.mesh_fetch()
        return mesh


def _sources(eng):
    for vol in mv.small_volumes():
        yield Source(eng, vol.name, volume=vol)
    for m in ci.hand_built():
        yield Source(eng, m.name, arrays=m.arrays())


def test_family_bit_exact_on_one_context():
    """Every mesh of the family on ONE context (the buffers only grow: large meshes come before small ones and the
    empty one): labels; the filter at min_faces 0, 1, 8, 10^9 and with keep_largest; smoothing at 0, 1, 3 and 10
    iterations, boundary fixed and free, mu -0.53 and 0; normals before and after; and the pipeline in
    reconstruct_mesh's order."""
    n_meshes = n_empty = 0
    with _engine() as eng:
        for src in _sources(eng):
            v, f, c = src.v, src.f, src.c
            name = src.name
            _assert_mesh_equal(src.reset(), (v, f, c), name + ", as uploaded")
            n_meshes += 1
            n_empty += len(f) == 0
            # normals of the raw mesh
            eng.mesh_normals()
            _assert_normals_equal(eng.mesh_fetch(normals=True)[3], cr.normals(v, f), name + ", raw")
            # labels and filters
            for min_faces, largest in FILTERS:
                src.reset()
                what = f"{name}, min_faces {min_faces}, keep_largest {largest}"
                got = eng.mesh_filter_components(min_faces, largest)
                n_comp, rv, rf, rc, rlab = cr.filter(v, f, c, min_faces, largest)
                assert got == (n_comp, len(rv), len(rf)), f"{what}: {got} vs {(n_comp, len(rv), len(rf))}"
                mesh = eng.mesh_fetch(labels=True)
                _assert_mesh_equal(mesh, (rv, rf, rc), what)
                assert np.array_equal(mesh[3], rlab), f"{what}: labels differ"
                # the filtered mesh is a mesh like any other: normals on the new topology
                eng.mesh_normals()
                _assert_normals_equal(eng.mesh_fetch(normals=True)[3], cr.normals(rv, rf), what)
            # smoothing
            for fix in (False, True):
                for mu in (-0.53, 0.0):
                    ref, done = v, 0
                    for it in ITERATIONS:
                        ref = cr.smooth(ref, f, it - done, 0.5, mu, fix)      # the iterations chain
                        done = it
                        src.reset()
                        eng.mesh_smooth(it, 0.5, mu, fix)
                        what = f"{name}, {it} iterations, mu {mu}, fix_boundary {fix}"
                        _assert_mesh_equal(eng.mesh_fetch(), (ref, f, c), what)
                    eng.mesh_normals()
                    _assert_normals_equal(eng.mesh_fetch(normals=True)[3], cr.normals(ref, f), what)
            # the pipeline
            src.reset()
            n_comp, rv, rf, rc, rlab, rn = cr.pipeline(v, f, c, 8, False, 3, 0.5, -0.53, True)
            assert eng.mesh_filter_components(8)[0] == n_comp
            eng.mesh_smooth(3)
            eng.mesh_normals()
            mesh = eng.mesh_fetch(normals=True, labels=True)
            _assert_mesh_equal(mesh, (rv, rf, rc), name + ", pipeline")
            _assert_normals_equal(mesh[3], rn, name + ", pipeline")
            assert np.array_equal(mesh[4], rlab), name + ", pipeline: labels differ"
    assert n_meshes >= 30 and n_empty >= 10


LARGE_N = 160


def test_large_sphere_pipeline_bit_exact():
    """The 160^3 sphere of test_hip_mesh_volumes.py (455 880 faces): filter, 10 Taubin iterations and normals once
    against the restatement, then a small mesh on the same context."""
    big = mv.sphere_volume(LARGE_N)
    with _engine() as eng:
        eng.tsdf_set_volume(*big.arrays())
        v, f, c = eng.tsdf_extract()
        assert len(f) >= 400_000
        n_comp, rv, rf, rc, rlab, rn = cr.pipeline(v, f, c, 8, True, 10, 0.5, -0.53, True)
        assert n_comp == 1 and len(rf) == len(f)
        assert eng.mesh_filter_components(8, True) == (1, len(v), len(f))
        eng.mesh_smooth(10)
        eng.mesh_normals()
        mesh = eng.mesh_fetch(normals=True, labels=True)
        _assert_mesh_equal(mesh, (rv, rf, rc), big.name)
        _assert_normals_equal(mesh[3], rn, big.name)
        assert np.array_equal(mesh[4], rlab)
        del rv, rf, rc, rn, mesh
        m = ci.threshold()
        eng.mesh_set(*m.arrays())
        ref = cr.pipeline(*m.arrays(), ci.MIN_FACES, False, 3)
        eng.mesh_filter_components(ci.MIN_FACES)
        eng.mesh_smooth(3)
        eng.mesh_normals()
        mesh = eng.mesh_fetch(normals=True, labels=True)
        _assert_mesh_equal(mesh, ref[1:4], m.name + " after the large sphere")
        _assert_normals_equal(mesh[3], ref[5], m.name + " after the large sphere")
        assert np.array_equal(mesh[4], ref[4])


def test_operating_point_256_cubed_sphere_properties():
    """The 256^3 sphere, properties only (its restatement does not fit the suite's budget): one component,
    F = 2 V - 4 kept by the filter, normals within 3 degrees of radial, and 10 Taubin iterations leave the surface
    where it was.

    How far a vertex of a clean sphere moves in 10 iterations was measured on the restatement: at 129^3 (295 968
    faces) the largest displacement is 0.616 voxel (0.556 at 65^3) -- almost all of it along the surface, where the
    vertices of a marching-tetrahedra mesh are unevenly spaced and the umbrella operator evens them out -- and the
    largest change of a vertex's distance from the centre is 0.0093 voxel (0.0157 at 65^3).  The bounds are twice the
    129^3 figures: 1.24 voxel for the displacement, 0.019 voxel for the radial part.  (A bound of 0.05 voxel on the
    whole displacement, proposed before anything was measured, does not hold for the definition: it is the radial
    part that stays that small.)"""
    radius = 0.8
    vol = mv.sphere_volume(256, radius=radius)
    voxel = float(vol.voxel)
    with _engine() as eng:
        eng.tsdf_set_volume(*vol.arrays())
        v, f, _ = eng.tsdf_extract()
        assert len(f) > 1_000_000 and len(f) == 2 * len(v) - 4
        assert eng.mesh_filter_components(8, True) == (1, len(v), len(f))
        kv, kf, _, lab = eng.mesh_fetch(labels=True)
        assert np.array_equal(kf, f) and _same_bits(kv, v) and not lab.any()
        eng.mesh_normals()
        n = eng.mesh_fetch(normals=True)[3].astype(np.float64)
        p = v.astype(np.float64)
        r0 = np.linalg.norm(p, axis=1)
        cos = np.clip((n * p).sum(axis=1) / r0 / np.linalg.norm(n, axis=1), -1, 1)
        angle = np.degrees(np.arccos(cos)).max()
        eng.mesh_smooth(10)
        sv, sf, _ = eng.mesh_fetch()
    assert np.array_equal(sf, f) and len(sf) == 2 * len(sv) - 4
    q = sv.astype(np.float64)
    moved = np.linalg.norm(q - p, axis=1).max() / voxel
    radial = np.abs(np.linalg.norm(q, axis=1) - r0).max() / voxel
    print(f"256^3 sphere: normals within {angle:.3f} degrees of radial; 10 iterations move a vertex by at most "
          f"{moved:.4f} voxel, its distance from the centre by at most {radial:.5f} voxel")
    assert angle <= 3.0
    assert moved <= 1.24
    assert radial <= 0.019


def _run_pipeline(eng, vol):
    eng.tsdf_set_volume(*vol.arrays())
    eng.tsdf_extract()
    counts = eng.mesh_filter_components(2)
    eng.mesh_smooth(5)
    eng.mesh_normals()
    return counts, eng.mesh_fetch(normals=True, labels=True)


def test_same_bits_twice_and_on_a_fresh_context():
    vol = mv.random_sign_volume((23, 19, 17), 2024)
    with _engine() as eng:
        first = _run_pipeline(eng, vol)
        _run_pipeline(eng, mv.sphere_volume(33, trunc=0.2))       # something else in between
        second = _run_pipeline(eng, vol)
    with _engine() as eng:
        third = _run_pipeline(eng, vol)
    assert first[0][0] > first[0][1] > 0 or first[0][0] > 1
    for other in (second, third):
        assert other[0] == first[0]
        for a, b in zip(other[1], first[1]):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_state_rules_and_errors():
    import amvs
    vol = mv.random_sign_volume((9, 8, 7), 12)
    m = ci.threshold()
    v, f, c = m.arrays()
    with _engine() as eng:
        for call in (lambda: eng.mesh_filter_components(1), lambda: eng.mesh_smooth(1), eng.mesh_normals,
                     lambda: eng._chk(eng._lib.amvs_fetch_mesh_attributes(eng._h, None, None))):
            with pytest.raises(amvs.AmvsError, match="no mesh"):
                call()
        eng.mesh_set(v, f, c)
        # attributes before they exist
        with pytest.raises(amvs.AmvsError, match="amvs_mesh_normals"):
            eng.mesh_fetch(normals=True)
        with pytest.raises(amvs.AmvsError, match="amvs_mesh_filter_components"):
            eng.mesh_fetch(labels=True)
        eng.mesh_normals()
        eng.mesh_filter_components()                              # labels only; drops the normals
        with pytest.raises(amvs.AmvsError, match="amvs_mesh_normals"):
            eng.mesh_fetch(normals=True)
        assert np.array_equal(eng.mesh_fetch(labels=True)[3], cr.labels(f, len(v)))
        eng.mesh_normals()
        eng.mesh_smooth(1)                                        # keeps the labels, drops the normals
        assert np.array_equal(eng.mesh_fetch(labels=True)[3], cr.labels(f, len(v)))
        with pytest.raises(amvs.AmvsError, match="amvs_mesh_normals"):
            eng.mesh_fetch(normals=True)
        eng.mesh_normals()
        assert len(eng.mesh_fetch(normals=True, labels=True)) == 5
        # every call that replaces the mesh drops both
        eng.mesh_set(v, f)
        assert not eng.mesh_fetch()[2].any()                      # no colours given: zeros
        for flag in (dict(normals=True), dict(labels=True)):
            with pytest.raises(amvs.AmvsError, match="no current"):
                eng.mesh_fetch(**flag)
        eng.mesh_normals(); eng.mesh_filter_components()
        eng.tsdf_set_volume(*vol.arrays())
        with pytest.raises(amvs.AmvsError, match="no mesh"):
            eng.mesh_normals()
        eng.tsdf_extract()
        for flag in (dict(normals=True), dict(labels=True)):
            with pytest.raises(amvs.AmvsError, match="no current"):
                eng.mesh_fetch(**flag)
        eng.mesh_normals(); eng.mesh_filter_components()
        eng.mesh_normals()
        eng.tsdf_extract()
        for flag in (dict(normals=True), dict(labels=True)):
            with pytest.raises(amvs.AmvsError, match="no current"):
                eng.mesh_fetch(**flag)
        # mesh_set refuses before it copies: the extracted mesh stays
        before = eng.mesh_fetch()
        bad_v = v.copy(); bad_v[3, 1] = np.nan
        inf_v = v.copy(); inf_v[0, 0] = np.inf
        rep = f.copy(); rep[2] = (1, 5, 1)
        high = f.copy(); high[4, 2] = len(v)
        neg = f.copy(); neg[0, 0] = -1
        for args, msg in (((bad_v, f, c), "not finite"), ((inf_v, f, c), "not finite"), ((v, rep, c), "repeated"),
                          ((v, high, c), "out of range"), ((v, neg, c), "out of range")):
            with pytest.raises(amvs.AmvsError, match=msg):
                eng.mesh_set(*args)
        one = np.zeros(9, np.float32)
        tri = np.array([0, 1, 2], np.int32)
        f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        for nv, nf in ((3, (2 ** 31) // 3 + 1), (2 ** 31, 1), (-1, 0), (3, -1)):
            rc = eng._lib.amvs_mesh_set(eng._h, one.ctypes.data_as(f32p), nv, tri.ctypes.data_as(i32p), nf, None)
            with pytest.raises(amvs.AmvsError, match="mesh_set"):
                eng._chk(rc)
        after = eng.mesh_fetch()
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        # the smoothing's argument ranges
        for args in ((-1, 0.5, -0.53), (1001, 0.5, -0.53), (1, 0.0, -0.53), (1, -0.5, -0.53), (1, 1.5, -0.53),
                     (1, np.nan, -0.53), (1, 0.5, np.nan), (1, 0.5, np.inf)):
            with pytest.raises(amvs.AmvsError, match="mesh_smooth"):
                eng.mesh_smooth(*args)
        eng.mesh_smooth(0, 1.0, 0.0)                              # the ends of the ranges are inside
        eng.mesh_smooth(1000, 2.0 ** -20, 0.0)
        eng.mesh_smooth(1, 1.0, -1.0)
        # a filter that leaves nothing: empty arrays, and the calls still work on them
        assert eng.mesh_filter_components(10 ** 9)[1:] == (0, 0)
        verts, faces, cols = eng.mesh_fetch()
        assert verts.shape == (0, 3) and faces.shape == (0, 3) and cols.shape == (0, 3)
        eng._chk(eng._lib.amvs_fetch_mesh(eng._h, None, None, None))
        eng.mesh_smooth(2)
        assert eng.mesh_filter_components(1) == (0, 0, 0)
        eng.mesh_normals()
        assert [a.shape for a in eng.mesh_fetch(normals=True, labels=True)] == [(0, 3), (0, 3), (0, 3), (0, 3), (0,)]
        from amvs import _lib
        assert _lib.index_check()[0] == 0


K_FACES = 50                        # from the measured component sizes: see the end-to-end test


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_reconstruct_mesh_clean_up_end_to_end(mode, scene_a):
    """On scene_a (5 views of 96 x 64), in both arithmetic modes: reconstruct_mesh(..., min_component_faces=K_FACES,
    smooth_iterations=3, with_normals=True) equals the restatement applied to what the default call returns, and the
    default call returns the same mesh after it as before it.

    Component sizes of the default call's mesh, measured (faces per component).  Exact: 2 907 vertices, 2 691 faces in
    294 components -- 57 of 1 face, 53 of 2, 24 of 3, 33 of 4, 14 of 5, 21 of 6, 8 of 7, 11 of 8, 64 of 9 to 48, and
    53, 54, 56, 58, 67, 68, 96, 141, 159.  Fast: 2 907 vertices, 2 693 faces in 295 components -- 60 of 1 face, 161
    of 2 to 8, 65 of 9 to 48 (four of them of 48), and 53, 54, 56, 58, 67, 68, 96, 141, 146.  K_FACES = 50 lies in the
    gap between 48 and 53 in both
    modes: 9 components stay, the others go."""
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    camera, images, poses, sparse = _scene_a_inputs(scene_a)
    pm = PatchMatchMVS(camera, scale=1.0, patch_size=7, num_iterations=4, num_samples=6, min_views=2, seed=2, device=0,
                       mode=mode)
    base = pm.reconstruct_mesh(images, poses, sparse, max_dim=64)
    assert len(base) == 3
    v, f, c = base
    lab = cr.labels(f, len(v))
    sizes = np.sort(cr.component_faces(f, lab)[np.unique(lab)])
    print(f"{mode}: {len(v)} vertices, {len(f)} faces in {len(sizes)} components of {sizes.tolist()} faces")
    assert len(f) > 100
    assert sizes[0] < K_FACES <= sizes[-1], sizes
    cleaned = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, min_component_faces=K_FACES, smooth_iterations=3,
                                  with_normals=True)
    assert len(cleaned) == 4
    _, rv, rf, rc, _, rn = cr.pipeline(v, f, c, K_FACES, False, 3, 0.5, -0.53, True)
    assert 0 < len(rf) < len(f)
    _assert_mesh_equal(cleaned, (rv, rf, rc), mode)
    _assert_normals_equal(cleaned[3], rn, mode)
    again = pm.reconstruct_mesh(images, poses, sparse, max_dim=64)
    assert len(again) == 3
    _assert_mesh_equal(again, base, mode + ", the default call again")
    only_normals = pm.reconstruct_mesh(images, poses, sparse, max_dim=64, with_normals=True)
    assert len(only_normals) == 4
    _assert_mesh_equal(only_normals, base, mode + ", normals only")
    _assert_normals_equal(only_normals[3], cr.normals(v, f), mode + ", normals only")
