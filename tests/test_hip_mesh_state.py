"""What of the current mesh's attributes every mesh operation leaves current (csrc/amvs_mesh_state.h, the table above
TsdfState::positions_changed and topology_changed), walked on ONE 24 x 32 context through the Engine methods.  After
every operation each of the normals fetch, the labels fetch, the render fetch, the visibility fetch and
mesh_filter_visible either succeeds or fails with its AMVS_EINVAL message; the index and the pinned flags cannot be
fetched, so a stale one is caught by what the smoother and the normals compute from it, bit for bit against the
restatements.  Expected values come from the table and from the restatement modules, never from a second run of the
library.

The meshes are hand-built ones of tests/mesh_clean_inputs.py: `threshold` (15 faces in two components of 8 and 7, no
isolated vertex) and `isolated` (a quad among three vertices that no face uses), and one volume of
tests/mesh_volumes.small_volumes() where a larger mesh is wanted."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_inputs as ci  # noqa: E402
import mesh_clean_restatement as cr  # noqa: E402
import mesh_decimate_restatement as dr  # noqa: E402
import mesh_quadric_restatement as qr  # noqa: E402
import mesh_render_inputs as ri  # noqa: E402
import mesh_render_restatement as rr  # noqa: E402
import mesh_volumes as mv  # noqa: E402
from mesh_hip_common import K_ANY, _assert_mesh_equal, _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
H, W = 24, 32
N_VIEWS = 2
SEEN_BY_ALL = F32(1e6)              # a tolerance no rendered depth can beat: a vertex counts wherever it projects
NOTHING = dict(normals=False, labels=False, render=False, visibility=False)
EVERYTHING = dict(normals=True, labels=True, render=True, visibility=True)
ONLY_LABELS = dict(NOTHING, labels=True)

EINVAL = r"\(-1\): "                                       # AMVS_EINVAL, as Engine._chk words it
MESSAGES = {"normals": EINVAL + "fetch_mesh_attributes: no current normals",
            "labels": EINVAL + "fetch_mesh_attributes: no current labels",
            "render": EINVAL + "fetch_render: no current render",
            "visibility": EINVAL + "fetch_mesh_visibility: no current counts",
            "filter": EINVAL + "mesh_filter_visible: no current counts"}


@pytest.fixture(scope="module")
def eng():
    import amvs
    with amvs.Engine(H, W, 1, K_ANY) as e:
        yield e
        from amvs import _lib
        assert _lib.index_check()[0] == 0


def _poses(p):
    return [(q[:9].reshape(3, 3), q[9:]) for q in np.asarray(p, F32).reshape(-1, 12)]


def _fetch_counts(eng):
    counts = np.empty(max(eng._mesh_counts[0], 1), np.int32)
    eng._chk(eng._lib.amvs_fetch_mesh_visibility(eng._h, counts.ctypes.data_as(C.POINTER(C.c_int32))))
    return counts[:eng._mesh_counts[0]]


def _expect(eng, what, normals, labels, render, visibility):
    """Each fetch succeeds or fails as the table says.  mesh_filter_visible needs the counts: without them it must
    fail (and change nothing); with them it would change the mesh, so the cases call it where they are done."""
    import amvs
    fetches = {"normals": lambda: eng.mesh_fetch(normals=True), "labels": lambda: eng.mesh_fetch(labels=True),
               "render": lambda: eng.mesh_render_fetch(0, 1), "visibility": lambda: _fetch_counts(eng)}
    current = dict(normals=normals, labels=labels, render=render, visibility=visibility)
    for name, fetch in fetches.items():
        if current[name]:
            fetch()
        else:
            with pytest.raises(amvs.AmvsError, match=MESSAGES[name]):
                fetch()
    if not visibility:
        with pytest.raises(amvs.AmvsError, match=MESSAGES["filter"]):
            eng.mesh_filter_visible(1)


class Current:
    """A mesh on the context with every attribute current, and what the restatements say each of them is."""

    def __init__(self, eng, arrays, tolerance=F32(0)):
        self.v, self.f, self.c = arrays
        self.K, self.poses, self.near = ri.views_for(self.v, N_VIEWS, H, W)
        eng.mesh_filter_components()                          # labels only; it would drop what follows
        eng.mesh_normals()
        self.maps = eng.mesh_render(self.K, _poses(self.poses), near=self.near, skipped=True)
        self.counts = eng.mesh_visibility(tolerance)
        ref_maps = rr.render(self.v, self.f, self.K, self.poses, self.near, H, W)
        for got, ref in zip(self.maps, ref_maps):
            assert got.tobytes() == ref.tobytes()
        assert np.array_equal(self.counts, rr.visibility(self.v, self.K, self.poses, self.near, ref_maps[0], tolerance))
        _expect(eng, "everything current", **EVERYTHING)


def _set_current(eng, mesh, tolerance=F32(0)):
    eng.mesh_set(*mesh)
    return Current(eng, mesh, tolerance)


def _assert_clean_up_matches(eng, v, f, c, what):
    """mesh_smooth(3, fix_boundary) and mesh_normals on the current mesh, which the restatements say is (v, f, c):
    a vertex -> corner index or pinned flags of another topology give other bits."""
    eng.mesh_smooth(3, 0.5, -0.53, True)
    eng.mesh_normals()
    mesh = eng.mesh_fetch(normals=True)
    sv = cr.smooth(v, f, 3, 0.5, -0.53, True)
    _assert_mesh_equal(mesh, (sv, f, c), what + ", smoothed")
    assert _same_bits(mesh[3], cr.normals(sv, f)), what + ": normals differ"
    return sv


def _assert_fetches_work_on_empty(eng, what):
    eng.mesh_normals()
    eng.mesh_smooth(2)
    assert [a.shape for a in eng.mesh_fetch()] == [(0, 3), (0, 3), (0, 3)], what
    eng.mesh_normals()
    assert eng.mesh_fetch(normals=True)[3].shape == (0, 3), what


def test_replacing_the_mesh_leaves_nothing_current(eng):
    import amvs
    m = ci.threshold().arrays()
    vol = mv.random_sign_volume((14, 11, 9), 5, closed=True)
    _set_current(eng, m)
    eng.mesh_set(*m)
    _expect(eng, "mesh_set", **NOTHING)
    Current(eng, m)
    eng.tsdf_set_volume(*vol.arrays())
    for fetch in (lambda: eng.mesh_fetch(normals=True), lambda: eng.mesh_fetch(labels=True)):
        with pytest.raises(amvs.AmvsError, match="no mesh"):
            fetch()
    extracted = vol.extract()
    _assert_mesh_equal(eng.tsdf_extract(), extracted, vol.name)
    _expect(eng, "tsdf_extract", **NOTHING)
    Current(eng, extracted)
    eng.tsdf_extract()
    _expect(eng, "tsdf_extract again", **NOTHING)


def test_components(eng):
    m = ci.threshold().arrays()
    v, f, c = m
    # label only: the mesh is unchanged, yet normals and render go
    _set_current(eng, m)
    n_comp, rv, rf, rc, rlab = cr.filter(v, f, c)
    assert eng.mesh_filter_components() == (n_comp, len(v), len(f)) and n_comp == 2
    _expect(eng, "label only", **ONLY_LABELS)
    mesh = eng.mesh_fetch(labels=True)
    _assert_mesh_equal(mesh, m, "label only")
    assert np.array_equal(mesh[3], rlab)
    # a filter that removes nothing
    eng.mesh_smooth(1, 0.5, -0.53, True)                      # builds the index and the pinned flags
    p1 = cr.smooth(v, f, 1, 0.5, -0.53, True)
    Current(eng, (p1, f, c))
    n_comp, rv, rf, rc, rlab = cr.filter(p1, f, c, 1)
    assert len(rf) == len(f) and len(rv) == len(v)
    assert eng.mesh_filter_components(1) == (n_comp, len(v), len(f))
    _expect(eng, "nothing removed", **ONLY_LABELS)
    mesh = eng.mesh_fetch(labels=True)
    _assert_mesh_equal(mesh, (p1, f, c), "nothing removed")
    assert np.array_equal(mesh[3], rlab)
    _assert_clean_up_matches(eng, p1, f, c, "nothing removed")
    # a filter that removes a component, after the index and the pinned flags of the whole mesh were built
    eng.mesh_set(*m)
    eng.mesh_smooth(1, 0.5, -0.53, True)
    Current(eng, (p1, f, c))
    n_comp, rv, rf, rc, rlab = cr.filter(p1, f, c, ci.MIN_FACES)
    assert 0 < len(rf) < len(f) and 0 < len(rv) < len(v)
    assert eng.mesh_filter_components(ci.MIN_FACES) == (n_comp, len(rv), len(rf))
    _expect(eng, "a component removed", **ONLY_LABELS)
    mesh = eng.mesh_fetch(labels=True)
    _assert_mesh_equal(mesh, (rv, rf, rc), "a component removed")
    assert np.array_equal(mesh[3], rlab)
    _assert_clean_up_matches(eng, rv, rf, rc, "a component removed")


def test_components_only_an_isolated_vertex_leaves(eng):
    """Every face stays and three vertices go: the ids of the others change, so the index and the pinned flags built
    before (two of the quad's four vertices keep a flag that was another vertex's) must not be used again."""
    m = ci.isolated().arrays()
    v, f, c = m
    eng.mesh_set(*m)
    eng.mesh_smooth(1, 0.5, -0.53, True)
    p1 = cr.smooth(v, f, 1, 0.5, -0.53, True)
    assert not np.array_equal(cr.pinned(f, len(v))[:4], cr.pinned(cr.filter(v, f, c, 1)[2], 4))
    Current(eng, (p1, f, c))
    n_comp, rv, rf, rc, rlab = cr.filter(p1, f, c, 1)
    assert len(rf) == len(f) and len(rv) == len(v) - 3
    assert eng.mesh_filter_components(1) == (n_comp, len(rv), len(rf))
    _expect(eng, "isolated vertices removed", **ONLY_LABELS)
    mesh = eng.mesh_fetch(labels=True)
    _assert_mesh_equal(mesh, (rv, rf, rc), "isolated vertices removed")
    assert np.array_equal(mesh[3], rlab)
    _assert_clean_up_matches(eng, rv, rf, rc, "isolated vertices removed")


def test_smoothing_without_iterations(eng):
    m = ci.threshold().arrays()
    cur = _set_current(eng, m)
    eng.mesh_smooth(0)
    _expect(eng, "mesh_smooth(0)", **ONLY_LABELS)
    mesh = eng.mesh_fetch(labels=True)
    _assert_mesh_equal(mesh, m, "mesh_smooth(0)")
    assert np.array_equal(mesh[3], cr.labels(cur.f, len(cur.v)))
    eng.mesh_normals()                                        # normals keep what is there
    _expect(eng, "mesh_normals", **dict(ONLY_LABELS, normals=True))


def test_decimation(eng):
    import amvs
    m = ci.threshold().arrays()
    v, f, c = m
    origin = np.zeros(3, F32)
    # refused for a vertex outside the cluster grid: everything stays current and the mesh is untouched
    cur = _set_current(eng, m)
    before = eng.mesh_fetch(normals=True, labels=True) + eng.mesh_render_fetch(0, N_VIEWS) + (_fetch_counts(eng),)
    with pytest.raises(dr.OutOfGrid):
        dr.decimate(v, f, c, origin, F32(1e-7))
    for refused in (eng.mesh_decimate, eng.mesh_decimate_quadric):
        with pytest.raises(amvs.AmvsError, match="outside the cluster grid"):
            refused(origin, 1e-7)
        _expect(eng, "refused decimation", **EVERYTHING)
        after = eng.mesh_fetch(normals=True, labels=True) + eng.mesh_render_fetch(0, N_VIEWS) + (_fetch_counts(eng),)
        assert len(after) == 8 and all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    _assert_mesh_equal(before, m, "refused decimation")
    assert _same_bits(before[3], cr.normals(v, f)) and np.array_equal(before[4], cr.labels(f, len(v)))
    # ... so mesh_filter_visible, the fifth of the calls, works on those counts
    rv, rf, rc = rr.filter_visible(v, f, c, cur.counts, 1)
    assert eng.mesh_filter_visible(1) == (len(rv), len(rf))
    _assert_mesh_equal(eng.mesh_fetch(), (rv, rf, rc), "the filter after the refused decimation")
    # accepted: nothing stays current
    cell = F32(1.0)
    _set_current(eng, m)
    ref = dr.decimate(v, f, c, origin, cell)
    assert eng.mesh_decimate(origin, cell) == (len(ref[0]), len(ref[1])) and 0 < len(ref[1]) < len(f)
    _expect(eng, "mesh_decimate", **NOTHING)
    _assert_mesh_equal(eng.mesh_fetch(), ref, "mesh_decimate")
    _set_current(eng, m)
    ref = qr.decimate_quadric(v, f, c, origin, cell, 1e-3)
    assert eng.mesh_decimate_quadric(origin, cell, 1e-3) == (len(ref[0]), len(ref[1]), ref[3])
    _expect(eng, "mesh_decimate_quadric", **NOTHING)
    _assert_mesh_equal(eng.mesh_fetch(), ref, "mesh_decimate_quadric")


def test_rendering(eng):
    m = ci.threshold().arrays()
    cur = _set_current(eng, m)
    got = eng.mesh_render(cur.K, _poses(cur.poses), near=cur.near, skipped=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, cur.maps))       # cur.maps equal the restatement's
    _expect(eng, "a second render", **dict(EVERYTHING, visibility=False))
    counts = eng.mesh_visibility(F32(0))
    assert np.array_equal(counts, cur.counts)
    _expect(eng, "mesh_visibility", **EVERYTHING)
    eng.mesh_normals()
    _expect(eng, "mesh_normals", **EVERYTHING)


def test_filter_visible_that_keeps_every_face(eng):
    m = ci.threshold().arrays()
    v, f, c = m
    cur = _set_current(eng, m, SEEN_BY_ALL)
    rv, rf, rc = rr.filter_visible(v, f, c, cur.counts, N_VIEWS)
    assert len(rf) == len(f) and len(rv) == len(v) and cur.counts.min() == N_VIEWS
    assert eng.mesh_filter_visible(N_VIEWS) == (len(v), len(f))
    _expect(eng, "mesh_filter_visible, nothing removed", **NOTHING)
    _assert_mesh_equal(eng.mesh_fetch(), m, "mesh_filter_visible, nothing removed")
    _assert_clean_up_matches(eng, v, f, c, "mesh_filter_visible, nothing removed")


def test_empty_results(eng):
    m = ci.threshold().arrays()
    v, f, c = m
    _set_current(eng, m)
    n_comp = cr.filter(v, f, c, 10 ** 9)[0]
    assert eng.mesh_filter_components(10 ** 9) == (n_comp, 0, 0)
    _expect(eng, "a filter that leaves nothing", **ONLY_LABELS)
    assert eng.mesh_fetch(labels=True)[3].shape == (0,)
    _assert_fetches_work_on_empty(eng, "a filter that leaves nothing")
    cur = _set_current(eng, m)
    rv, rf, rc = rr.filter_visible(v, f, c, cur.counts, N_VIEWS + 1)
    assert len(rf) == 0 and len(rv) == 0
    assert eng.mesh_filter_visible(N_VIEWS + 1) == (0, 0)
    _expect(eng, "a visibility filter that leaves nothing", **NOTHING)
    _assert_fetches_work_on_empty(eng, "a visibility filter that leaves nothing")
    assert eng.mesh_filter_components(1) == (0, 0, 0)


def test_across_stages_no_index_outlives_its_topology(eng):
    """An extracted mesh with its index and pinned flags built, then mesh_decimate_quadric: the clean-up and the render
    of the decimated mesh equal the restatements applied to the restatement's decimated mesh."""
    vol = mv.random_sign_volume((14, 11, 9), 5, closed=True)
    v, f, c = vol.extract()
    eng.tsdf_set_volume(*vol.arrays())
    _assert_mesh_equal(eng.tsdf_extract(), (v, f, c), vol.name)
    eng.mesh_smooth(1, 0.5, -0.53, True)
    p1 = cr.smooth(v, f, 1, 0.5, -0.53, True)
    Current(eng, (p1, f, c))
    origin, cell = vol.origin, F32(2) * vol.voxel
    dv, df, dc, dk = qr.decimate_quadric(p1, f, c, origin, cell, 1e-3)
    assert 0 < len(df) < len(f)
    assert eng.mesh_decimate_quadric(origin, cell, 1e-3) == (len(dv), len(df), dk)
    _expect(eng, "mesh_decimate_quadric", **NOTHING)
    _assert_mesh_equal(eng.mesh_fetch(), (dv, df, dc), vol.name + ", decimated")
    sv = _assert_clean_up_matches(eng, dv, df, dc, vol.name + ", decimated")
    K, poses, near = ri.views_for(sv, N_VIEWS, H, W)
    got = eng.mesh_render(K, _poses(poses), near=near, skipped=True)
    ref = rr.render(sv, df, K, poses, near, H, W)
    assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(got, ref))
    assert (ref[1] >= 0).sum() > 50
    _expect(eng, "a render of the decimated mesh", **dict(NOTHING, normals=True, render=True))
