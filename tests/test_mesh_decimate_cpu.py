"""The mesh decimation on the NumPy restatement alone (tests/mesh_decimate_restatement.py; no GPU): that it says what
a plain loop per cluster and per group says, that the family of meshes the GPU comparison runs on
(test_hip_mesh_decimate.py) reaches what it is meant to reach, and that the definition has the properties it was
chosen for."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_inputs as ci  # noqa: E402
import mesh_decimate_inputs as di  # noqa: E402
import mesh_decimate_restatement as dr  # noqa: E402
import mesh_volumes as mv  # noqa: E402

F32 = np.float32
COUNTERS = ("degenerate", "mixed_groups", "mixed_kept", "same_wound_duplicates", "integral", "unused")
HAND_BUILT_CELL = 0.3


def _same_mesh(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))


@functools.lru_cache(maxsize=None)
def volume_results():
    """(name, info) of every small volume's mesh decimated at its own origin and 2 voxels."""
    out = []
    for vol in mv.small_volumes():
        v, f, c = vol.extract()
        out.append((vol.name, dr.decimate(v, f, c, vol.origin, F32(2) * vol.voxel, with_info=True)[3]))
    return tuple(out)


def _total(infos):
    tot = {k: sum(i[k] for i in infos) for k in COUNTERS}
    tot["longest"] = max([i["longest"] for i in infos] + [0])
    net = {}
    for i in infos:
        for k, n in i["net"].items():
            net[k] = net.get(k, 0) + n
    tot["net"] = net
    return tot


def test_vectorised_restatement_equals_plain_loops():
    cases = [(c.name,) + c.arrays() + (c.origin, c.cell) for c in di.accepted_cases()]
    cases += [(m.name,) + m.arrays() + ((0.0, 0.0, 0.0), HAND_BUILT_CELL) for m in ci.hand_built() if len(m.faces) <= 2000]
    for vol in (mv.random_sign_volume((5, 3, 4), 2028), mv.random_sign_volume((14, 11, 9), 5, closed=True),
                mv.grid_plane_volume((9, 8, 11), 2, 5)):
        cases.append((vol.name,) + tuple(vol.extract()) + (vol.origin, F32(2) * vol.voxel))
        cases.append((vol.name + ", off the grid",) + tuple(vol.extract()) + (vol.origin + F32(0.37) * vol.voxel, F32(3) * vol.voxel))
    n_faces_out = 0
    for name, v, f, c, origin, cell in cases:
        fast, slow = dr.decimate(v, f, c, origin, cell), dr.decimate_slow(v, f, c, origin, cell)
        assert _same_mesh(fast, slow), name
        n_faces_out += len(fast[1])
    assert len(cases) >= 20 and n_faces_out >= 500


def test_range_edges_are_refused_before_anything_else():
    for case in di.range_edges():
        if case.accepted:
            v, f, _ = dr.decimate(*case.arrays(), case.origin, case.cell)
            assert len(f) == 3 and len(v) == 4, case.name
        else:
            for fn in (dr.decimate, dr.decimate_slow):
                with pytest.raises(dr.OutOfGrid, match="vertex 3 outside the cluster grid"):
                    fn(*case.arrays(), case.origin, case.cell)
    assert sum(c.accepted for c in di.range_edges()) == 6 and len(di.refused_cases()) == 6
    # the smallest offending id is the one named
    case = di.refused_cases()[0]
    v = np.concatenate([case.verts, case.verts[3:], case.verts[:1]])
    with pytest.raises(dr.OutOfGrid) as e:
        dr.cell_keys(v, case.origin, case.cell)
    assert e.value.vertex == 3


def test_family_covers_what_it_is_meant_to():
    """The counters over mesh_volumes.small_volumes() at their own origin and 2 voxels, measured on this restatement:
    125 074 degenerate faces, 1 521 mixed groups of which 64 keep a face, 132 faces that share triple and winding with
    another, 35 227 exactly integral quotients, 447 unused clusters, longest cluster 44 (a cell of 2 voxels holds at
    most 8 grid points with 7 edges each: the 478 of a prototype must have counted something else).  The shuffled
    strip at origin 0, cell 0.3: 2 997 mixed groups.  Long clusters and groups with |net| > 1 come from
    mesh_decimate_inputs."""
    vol = _total([i for _, i in volume_results()])
    hand = _total([dr.decimate(*m.arrays(), (0.0, 0.0, 0.0), HAND_BUILT_CELL, with_info=True)[3] for m in ci.hand_built()])
    new = _total([dr.decimate(*c.arrays(), c.origin, c.cell, with_info=True)[3] for c in di.accepted_cases()])
    print("volumes:", vol, "\nhand-built:", hand, "\nnew inputs:", new)
    for k in COUNTERS:
        assert vol[k] + hand[k] >= 50, (k, vol[k], hand[k])
    assert max(vol["longest"], hand["longest"], new["longest"]) >= 256
    assert new["longest"] >= di.PILE and new["same_wound_duplicates"] >= di.PILE
    for net in (-3, -2, 2, 3):
        assert new["net"].get(net, 0) >= 1, (net, new["net"])
    assert new["net"].get(0, 0) >= 2 and new["mixed_kept"] >= 6
    # the face that stays is not always the first of the mesh's faces on its triple
    w = di.windings()
    keys = dr.cell_keys(w.verts, w.origin, w.cell)
    g = dr.clusters(keys)[0][w.faces.astype(np.int64)]
    keep, _ = dr.face_decision(g)
    triple = np.sort(g, axis=1)
    first_of_triple = np.array([np.flatnonzero((triple == t).all(axis=1))[0] for t in triple[keep]])
    assert (first_of_triple != np.flatnonzero(keep)).sum() >= 1
    # indices of either sign, q = -1.0 and q = -0.0
    a = di.around_origin()
    q = dr.quotients(a.verts, a.origin, a.cell)
    assert (np.floor(q) < 0).any(axis=0).all() and (np.floor(q) > 0).any(axis=0).all()
    assert (q[:, 0] == -1.0).any() and ((q[:, 0] == 0) & np.signbit(q[:, 0])).any()
    minus_zero = np.flatnonzero((q[:, 0] == 0) & np.signbit(q[:, 0]))[0]
    assert (dr.cell_keys(a.verts, a.origin, a.cell)[minus_zero] & ((1 << 21) - 1)) == dr.HALF          # cell 0, not -1
    # nothing at all, and vertices without faces
    for m in (ci.empty(), ci.vertices_only()):
        out = dr.decimate(*m.arrays(), (0.0, 0.0, 0.0), HAND_BUILT_CELL)
        assert [x.shape for x in out] == [(0, 3), (0, 3), (0, 3)]


def _euler(faces, n_vertices):
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return n_vertices - len(np.unique(np.sort(e, axis=1), axis=0)) + len(f)


SPHERES = ((65, 2.0, 0.0), (65, 2.0, 0.37), (33, 1.5, 0.0), (33, 1.5, 0.37))


@pytest.mark.parametrize("n,cells,shift", SPHERES)
def test_decimated_sphere_is_closed_and_near_the_sphere(n, cells, shift):
    """sphere_volume(n, trunc=0.1), radius R = 0.8: the result is closed and consistently oriented; at 2 voxels it is
    a sphere (V - E + F = 2) of at most an eighth of the faces (measured: 73 944 -> 6 108 at 65^3, ratio 12.1, largest
    radial error 0.024 voxel; at 1.5 voxels the cells cut the surface into fins and V - E + F is not asked for).  Every
    vertex lies within 0.05 voxel + 3 cell^2 / (8 R) of the radius: the extraction's own 0.05 voxel plus the sagitta of
    a chord of length sqrt(3) cell, the longest a cell holds."""
    R = 0.8
    vol = mv.sphere_volume(n, radius=R, trunc=0.1)
    v, f, c = vol.extract()
    cell = F32(cells) * vol.voxel
    origin = (vol.origin + F32(shift) * vol.voxel).astype(F32)
    dv, df, dc = dr.decimate(v, f, c, origin, cell)
    err = np.abs(np.linalg.norm(dv.astype(np.float64), axis=1) - R).max()
    print(f"{n}^3 at {cells} voxels, shift {shift}: {len(f)} faces -> {len(df)} ({len(f) / len(df):.1f}), {len(dv)} vertices, "
          f"V - E + F = {_euler(df, len(dv))}, radial error {err / float(vol.voxel):.4f} voxel")
    assert mv.directed_edge_defects(df, len(dv)) == (0, 0)
    if cells == 2.0:
        assert _euler(df, len(dv)) == 2
        assert len(df) <= len(f) / 8
    assert err <= 0.05 * float(vol.voxel) + 3.0 * float(cell) ** 2 / (8.0 * R)
    if (n, shift) == (65, 0.0):
        assert (len(df), len(dv)) == (6108, 3056)


def test_decimating_twice_changes_nothing_where_no_representative_left_its_cell():
    """A cluster of one vertex is that vertex (0 + p, p / 1, (2 c + 1) // 2), and faces that survived once are no
    duplicates of one another: a second pass on the same grid is the identity, except where a mean was rounded or
    simply lies outside its cell's run of members into a neighbouring cell -- those vertices merge with that cell's.
    Their number is printed, not bounded."""
    moved_total = 0
    checked = 0
    for vol in mv.small_volumes()[:13] + [mv.sphere_volume(65, trunc=0.1)]:
        v, f, c = vol.extract()
        origin, cell = vol.origin, F32(2) * vol.voxel
        once = dr.decimate(v, f, c, origin, cell, with_info=True)
        if len(once[0]) == 0:
            continue
        keys = dr.cell_keys(once[0], origin, cell)
        moved = int((keys != once[3]["keys"]).sum())
        moved_total += moved
        twice = dr.decimate(*once[:3], origin, cell)
        if moved == 0:
            assert _same_mesh(once, twice), vol.name
            checked += 1
        else:
            # only the moved vertices and the cells they land in are touched
            stay = np.isin(keys, keys[keys != once[3]["keys"]], invert=True)
            kept = once[0][stay]
            assert len(twice[0]) >= len(once[0]) - moved, vol.name
            assert np.isin(kept.view(np.uint32).view([("", np.uint32)] * 3).ravel(),
                           twice[0].view(np.uint32).view([("", np.uint32)] * 3).ravel()).all(), vol.name
    print(f"representatives that left their cell: {moved_total}; meshes unchanged by the second pass: {checked}")
    assert checked >= 3
