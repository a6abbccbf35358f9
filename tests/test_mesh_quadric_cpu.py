"""The decimation with quadric placement on the NumPy restatement alone (tests/mesh_quadric_restatement.py; no GPU): that
it says what plain loops say, that only positions differ from the mean placement, that every fallback is the mean and
every accepted position within half a cell of it, that the family of meshes the GPU comparison runs on
(test_hip_mesh_quadric.py) reaches every cause of a fallback, and that the placement does what it was chosen for."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_inputs as ci  # noqa: E402
import mesh_decimate_restatement as dr  # noqa: E402
import mesh_quadric_inputs as qi  # noqa: E402
import mesh_quadric_restatement as qr  # noqa: E402
import mesh_volumes as mv  # noqa: E402

F32 = np.float32
HAND_BUILT_CELL = 0.3
REG = 1e-3


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_mesh(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))


def _family():
    """(name, vertices, faces, colours, origin, cell, regularisation) of every mesh of the family on its own grid."""
    for vol in mv.small_volumes() + [qi.rotated_box()]:
        yield (vol.name,) + tuple(vol.extract()) + (vol.origin, F32(2) * vol.voxel, REG)
    for m in ci.hand_built():
        yield (m.name,) + m.arrays() + (np.zeros(3, F32), F32(HAND_BUILT_CELL), REG)
    for c in qi.hand_built():
        yield (c.name,) + c.arrays() + (c.origin, c.cell, REG if c.regularisation is None else c.regularisation)


@functools.lru_cache(maxsize=None)
def family_results():
    out = []
    for name, v, f, c, origin, cell, reg in _family():
        out.append((name, (v, f, c, origin, cell, reg), qr.decimate_quadric(v, f, c, origin, cell, reg, with_info=True)))
    return tuple(out)


def _cluster_at(info, origin, cell, point):
    """The cluster of step 2 whose cell holds `point`."""
    keys = dr.cell_keys(info["mean"], origin, cell)
    return int(np.flatnonzero(keys == dr.cell_keys(np.asarray(point, F32).reshape(1, 3), origin, cell)[0])[0])


def test_vectorised_restatement_equals_plain_loops():
    cases = [(c.name,) + c.arrays() + (c.origin, c.cell, r) for c in qi.hand_built()
             for r in {REG, 0.1, c.regularisation or REG}]
    cases += [(m.name,) + m.arrays() + ((0.0, 0.0, 0.0), HAND_BUILT_CELL, REG) for m in ci.hand_built() if len(m.faces) <= 2000]
    for vol in (mv.random_sign_volume((5, 3, 4), 2028), mv.random_sign_volume((14, 11, 9), 5, closed=True),
                mv.grid_plane_volume((9, 8, 11), 2, 5), mv.sphere_volume(17, trunc=0.3)):
        cases.append((vol.name,) + tuple(vol.extract()) + (vol.origin, F32(2) * vol.voxel, REG))
        cases.append((vol.name + ", off the grid",) + tuple(vol.extract()) + (vol.origin + F32(0.37) * vol.voxel, F32(3) * vol.voxel, 0.1))
    n_faces_out = n_fallback = n_accepted = 0
    for name, v, f, c, origin, cell, reg in cases:
        fast = qr.decimate_quadric(v, f, c, origin, cell, reg, with_info=True)
        slow = qr.decimate_quadric_slow(v, f, c, origin, cell, reg)
        assert _same_mesh(fast, slow), name
        assert fast[3] == slow[3], (name, fast[3], slow[3])
        n_faces_out += len(fast[1])
        n_fallback += fast[3]
        n_accepted += fast[4]["clusters"] - fast[3]
    assert len(cases) >= 30 and n_faces_out >= 500 and n_fallback >= 20 and n_accepted >= 500


def test_only_positions_differ_and_they_stay_near_the_mean():
    """Faces and colours are the mean placement's exactly; a cluster that fell back has the mean's bits, an accepted one
    lies within half a cell of it on every axis (one rounding of m + y allowed for)."""
    n_moved = 0
    for name, (v, f, c, origin, cell, reg), (qv, qf, qc, n_fallback, info) in family_results():
        mean = dr.decimate(v, f, c, origin, cell)
        assert np.array_equal(qf, mean[1]) and np.array_equal(qc, mean[2]) and qv.shape == mean[0].shape, name
        back = info["cause"] != 0
        assert n_fallback == int(back.sum()) == sum(info["causes"].values()), name
        assert np.array_equal(_bits(info["position"][back]), _bits(info["mean"][back])), name
        assert np.array_equal(_bits(info["mean"][info["used"]]), _bits(mean[0])), name
        acc = ~back
        with np.errstate(all="ignore"):
            step = np.abs(info["position"][acc].astype(np.float64) - info["mean"][acc].astype(np.float64))
            slack = np.spacing(np.abs(info["position"][acc]).astype(F32)).astype(np.float64)
        assert np.isfinite(info["position"][acc]).all(), name
        assert (step <= 0.5 * float(cell) + slack).all(), name
        assert (np.abs(info["y"][acc]) <= F32(0.5) * F32(cell)).all(), name
        n_moved += int((_bits(info["position"]) != _bits(info["mean"])).any(axis=1).sum())
    assert n_moved >= 10_000


def test_family_covers_every_cause():
    res = {name: (args, out) for name, args, out in family_results()}
    total = {k: sum(out[4]["causes"][k] for _, out in res.values()) for k in qr.CAUSES}
    print("fallbacks by cause over the family:", total, "; clusters:", sum(out[4]["clusters"] for _, out in res.values()))
    for k in qr.CAUSES:
        assert total[k] >= 1, total

    def cause_of(case, point=None):
        args, out = res[case.name]
        k = _cluster_at(out[4], args[3], args[4], case.target if point is None else point)
        code = int(out[4]["cause"][k])
        return (qr.CAUSES[code - 1] if code else "accepted"), k, out[4]

    # a flat cluster is accepted and moves along the common normal only, away from the mean by a good part of 0.25
    cause, k, info = cause_of(qi.flat())
    y = info["y"][k].astype(np.float64)
    along = float(y @ qi.NORMAL)
    print(f"flat cluster: y = {y}, along the normal {along:.6f}, across {np.linalg.norm(y - along * qi.NORMAL):.3g}")
    assert cause == "accepted" and abs(along) >= 0.1
    assert np.linalg.norm(y - along * qi.NORMAL) <= 1e-4 * abs(along)
    assert cause_of(qi.isolated())[0] == "t"
    assert cause_of(qi.zero_area())[0] == "t"
    assert cause_of(qi.wedge())[0] == "bound"
    assert cause_of(qi.singular(), (0.5, 0.5, 0.5))[0] == "d1"
    assert cause_of(qi.singular(), (2.5, 0.5, 0.5))[0] == "d2"
    assert cause_of(qi.overflow_b())[0] == "non-finite"
    args, out = res[qi.overflow_a().name]
    assert out[4]["causes"]["d1"] == out[4]["clusters"] == 6 and np.isinf(qr.Prepared(*args[:5]).quadrics[:, 0]).any()
    cause, k, info = cause_of(qi.pile())
    assert cause == "accepted" and int(np.diff(qr.Prepared(*res[qi.pile().name][0][:5]).start).max()) == 300
    # the same singular inputs at the default regularisation solve
    s = qi.singular()
    assert qr.decimate_quadric(*s.arrays(), s.origin, s.cell, REG)[3] == 0
    # nothing at all, and vertices without faces (every cluster keeps the mean)
    for m, n_clusters in ((ci.empty(), 0), (ci.vertices_only(), None)):
        out = qr.decimate_quadric(*m.arrays(), (0.0, 0.0, 0.0), HAND_BUILT_CELL, with_info=True)
        assert [x.shape for x in out[:3]] == [(0, 3), (0, 3), (0, 3)]
        assert out[3] == out[4]["clusters"] and (n_clusters is None or out[3] == n_clusters)
    assert qr.decimate_quadric(*ci.vertices_only().arrays(), (0.0, 0.0, 0.0), HAND_BUILT_CELL)[3] >= 1


def _euler(faces, n_vertices):
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return n_vertices - len(np.unique(np.sort(e, axis=1), axis=0)) + len(f)


def _max_rms(err, voxel):
    err = np.asarray(err, np.float64) / float(voxel)
    return float(err.max()), float(np.sqrt((err ** 2).mean()))


SPHERE_ROWS = ((2.0, 0.0), (3.0, 0.0), (2.0, 0.37))


def test_sphere_error_against_the_mean_placement():
    """sphere_volume(65, trunc=0.1), R = 0.8, regularisation 1e-3.  Radial error in voxels, mean placement | quadric:
        2 voxels on the origin     3 056 vertices   max 0.0240 rms 0.0142 | max 0.0162 rms 0.0063, 0 kept the mean
        3 voxels                   1 382 vertices   max 0.0431 rms 0.0278 | max 0.0352 rms 0.0191, 0
        2 voxels, shifted 0.37     2 747 vertices   max 0.0214 rms 0.0127 | max 0.0182 rms 0.0085, 0
    The gate (first row): rms <= 0.6 x the mean placement's, max <= the mean placement's; closed, V - E + F = 2."""
    R = 0.8
    vol = mv.sphere_volume(65, radius=R, trunc=0.1)
    v, f, c = vol.extract()
    for cells, shift in SPHERE_ROWS:
        origin = (vol.origin + F32(shift) * vol.voxel).astype(F32)
        cell = F32(cells) * vol.voxel
        mean = dr.decimate(v, f, c, origin, cell)
        quad = qr.decimate_quadric(v, f, c, origin, cell, REG)
        em = _max_rms(np.abs(np.linalg.norm(mean[0].astype(np.float64), axis=1) - R), vol.voxel)
        eq = _max_rms(np.abs(np.linalg.norm(quad[0].astype(np.float64), axis=1) - R), vol.voxel)
        print(f"sphere 65^3 at {cells} voxels, shift {shift}: {len(f)} faces -> {len(quad[1])}, {len(quad[0])} vertices; mean max "
              f"{em[0]:.4f} rms {em[1]:.4f}; quadric max {eq[0]:.4f} rms {eq[1]:.4f}; {quad[3]} kept the mean")
        assert np.array_equal(quad[1], mean[1])
        if (cells, shift) == (2.0, 0.0):
            assert (len(quad[1]), len(quad[0])) == (6108, 3056)
            assert eq[1] <= 0.6 * em[1] and eq[0] <= em[0]
            assert mv.directed_edge_defects(quad[1], len(quad[0])) == (0, 0) and _euler(quad[1], len(quad[0])) == 2


def test_rotated_box_error_against_the_mean_placement_and_the_extraction():
    """The 49^3 rotated box at 2 voxels on the volume's origin, regularisation 1e-3.  Distance to the true box in
    voxels: extraction max 0.52 rms 0.0376; 19 776 faces -> 788 vertices, mean placement max 0.560 rms 0.0695, quadric
    max 0.298 rms 0.0373, 2 clusters kept the mean.  The gate: rms <= 0.65 x the mean placement's and <= 1.1 x the
    extraction's; closed, V - E + F = 2."""
    vol = qi.rotated_box()
    v, f, c = vol.extract()
    cell = F32(2) * vol.voxel
    mean = dr.decimate(v, f, c, vol.origin, cell)
    quad = qr.decimate_quadric(v, f, c, vol.origin, cell, REG)
    e0, em, eq = (_max_rms(qi.box_distance(x), vol.voxel) for x in (v, mean[0], quad[0]))
    print(f"rotated box 49^3: {len(f)} faces, extraction max {e0[0]:.4f} rms {e0[1]:.4f}; -> {len(quad[0])} vertices, "
          f"{len(quad[1])} faces; mean max {em[0]:.4f} rms {em[1]:.4f}; quadric max {eq[0]:.4f} rms {eq[1]:.4f}; "
          f"{quad[3]} kept the mean")
    assert len(f) == 19776 and len(quad[0]) == 788
    assert eq[1] <= 0.65 * em[1] and eq[1] <= 1.1 * e0[1]
    assert mv.directed_edge_defects(quad[1], len(quad[0])) == (0, 0) and _euler(quad[1], len(quad[0])) == 2
