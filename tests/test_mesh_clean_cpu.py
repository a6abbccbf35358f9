"""The mesh clean-up on the NumPy restatement alone (tests/mesh_clean_restatement.py; no GPU): that the family of
meshes the GPU comparison runs on (test_hip_mesh_clean.py) reaches what it is meant to reach, that the definitions
have the properties they were chosen for, and that save_mesh_ply writes normals where asked and today's bytes where
not."""
import functools
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_inputs as ci  # noqa: E402
import mesh_clean_restatement as cr  # noqa: E402
import mesh_volumes as mv  # noqa: E402

F32 = np.float32


@functools.lru_cache(maxsize=None)
def volume_meshes():
    return tuple((vol.name,) + tuple(vol.extract()) for vol in mv.small_volumes())


def family():
    """(name, vertices, faces, colours) of every mesh of the family, the volumes' first."""
    return list(volume_meshes()) + [(m.name,) + m.arrays() for m in ci.hand_built()]


def _zero_area(v, f):
    return int((np.abs(cr.face_normals(v, f)).sum(axis=1) == 0).sum())


# ---- an independent, slow statement of the two ordered sums: plain loops over vertices and corners -------------

def _slow_step(p, faces, factor, pin):
    out = p.copy()
    ids = faces.reshape(-1)
    for v in range(len(p)):
        row = [c for c in range(len(ids)) if ids[c] == v]
        if not row or (pin is not None and pin[v]):
            continue
        s = np.zeros(3, F32)
        for c in row:
            f, k = divmod(c, 3)
            s = (s + p[faces[f, (k + 1) % 3]]).astype(F32)
            s = (s + p[faces[f, (k + 2) % 3]]).astype(F32)
        m = (s / F32(F32(2.0) * F32(len(row)))).astype(F32)
        d = (m - p[v]).astype(F32)
        out[v] = (p[v] + (F32(factor) * d).astype(F32)).astype(F32)
    return out


def _slow_normals(p, faces):
    out = np.zeros_like(p)
    ids = faces.reshape(-1)
    for v in range(len(p)):
        s = np.zeros(3, F32)
        for c in range(len(ids)):
            if ids[c] != v:
                continue
            p0, p1, p2 = (p[i] for i in faces[c // 3])
            a, b = (p1 - p0).astype(F32), (p2 - p0).astype(F32)
            n = np.array([F32(a[1] * b[2]) - F32(a[2] * b[1]), F32(a[2] * b[0]) - F32(a[0] * b[2]),
                          F32(a[0] * b[1]) - F32(a[1] * b[0])], F32)
            s = (s + n).astype(F32)
        l = np.sqrt(F32(F32(F32(s[0] * s[0]) + F32(s[1] * s[1])) + F32(s[2] * s[2])))
        if l > 0:
            out[v] = (s / l).astype(F32)
    return out


def test_vectorised_sums_equal_plain_loops():
    small = [m for m in family() if 0 < len(m[2]) <= 400]
    assert len(small) >= 8
    for name, v, f, _ in small:
        f = np.asarray(f, np.int64)
        pin = cr.pinned(f, len(v))
        for fix in (False, True):
            p = v.copy()
            for factor in (0.5, -0.53, 0.5):
                p = _slow_step(p, f, factor, pin if fix else None)
            ref = cr.smooth(cr.smooth(v, f, 1, 0.5, -0.53, fix), f, 1, 0.5, 0.0, fix)
            assert np.array_equal(p.view(np.uint32), ref.view(np.uint32)), name
        assert np.array_equal(_slow_normals(v, f).view(np.uint32), cr.normals(v, f).view(np.uint32)), name


def test_index_rows_are_ascending_and_complete():
    for name, v, f, _ in family():
        start, corners = cr.corner_index(f, len(v))
        ids = np.asarray(f).reshape(-1)
        assert start[0] == 0 and start[-1] == len(ids) and len(corners) == len(ids), name
        assert np.array_equal(np.sort(corners), np.arange(len(ids))), name
        rows = np.repeat(np.arange(len(v)), np.diff(start))
        assert np.array_equal(ids[corners], rows), name
        same_row = rows[1:] == rows[:-1]
        assert np.all(corners[1:][same_row] > corners[:-1][same_row]), name


def test_family_covers_what_it_is_meant_to():
    fam = family()
    n_pinned = n_free = n_zero_area = 0
    most_components, longest_row, singles = 0, 0, 0
    for name, v, f, _ in volume_meshes():
        f64 = np.asarray(f, np.int64)
        assert np.all((f64[:, 0] != f64[:, 1]) & (f64[:, 0] != f64[:, 2]) & (f64[:, 1] != f64[:, 2])), name
        if len(f):
            assert cr.edge_face_counts(f, len(v))[2].max() <= 2, name      # no edge on three faces
            lab = cr.labels(f, len(v))
            count = cr.component_faces(f, lab)[np.unique(lab)]
            most_components = max(most_components, len(count))
            singles += int((count == 1).sum())
            longest_row = max(longest_row, int(np.diff(cr.corner_index(f, len(v))[0]).max()))
    assert most_components >= 100 and singles >= 1 and 6 <= longest_row <= 16, (most_components, singles, longest_row)
    for name, v, f, _ in fam:
        pin = cr.pinned(f, len(v))
        n_pinned += int(pin.sum())
        n_free += int((~pin).sum())
        n_zero_area += _zero_area(v, f)
    assert n_pinned >= 100 and n_free >= 100, (n_pinned, n_free)
    assert n_zero_area >= 100, n_zero_area
    # zero-length normal sums over faces that have an area
    v, f, _ = ci.coincident().arrays()
    assert _zero_area(v, f) == 0
    s, l = cr.normal_sums(v, f)
    assert np.all(l == 0) and np.all(cr.normals(v, f) == 0)
    # either side of the threshold
    v, f, c = ci.threshold().arrays()
    lab = cr.labels(f, len(v))
    assert sorted(cr.component_faces(f, lab)[np.unique(lab)]) == [ci.MIN_FACES - 1, ci.MIN_FACES]
    n_comp, kv, kf, _, klab = cr.filter(v, f, c, ci.MIN_FACES)
    assert n_comp == 2 and len(kf) == ci.MIN_FACES and len(np.unique(klab)) == 1 and len(kv) == 6
    assert cr.filter(v, f, c, ci.MIN_FACES + 1)[2].shape == (0, 3)
    # the tie: the first faces belong to the component with the larger label, the smaller label wins
    v, f, c = ci.tie().arrays()
    lab = cr.labels(f, len(v))
    assert list(np.unique(lab)) == [0, 4] and lab[f[0, 0]] == 4
    assert list(cr.component_faces(f, lab)[[0, 4]]) == [4, 4]
    _, kv, kf, _, klab = cr.filter(v, f, c, 0, keep_largest=True)
    assert np.array_equal(kv, v[:4]) and len(kf) == 4 and np.all(klab == 0)
    # an unpinned vertex on an edge of three faces
    v, f, _ = ci.closed_book().arrays()
    lo, hi, count = cr.edge_face_counts(f, len(v))
    pin = cr.pinned(f, len(v))
    three = count == 3
    assert three.any() and not pin[lo[three]].any() and not pin[hi[three]].any()
    v, f, _ = ci.open_book().arrays()
    assert cr.edge_face_counts(f, len(v))[2].max() == 3 and cr.pinned(f, len(v)).all()
    # long rows, long chains, nothing at all
    assert np.diff(cr.corner_index(ci.fan().faces, len(ci.fan().verts))[0]).max() >= 1000
    assert len(ci.strip().faces) >= 100_000 and len(np.unique(cr.labels(ci.strip().faces, len(ci.strip().verts)))) == 1
    assert len(ci.empty().faces) == 0 and len(ci.empty().verts) == 0
    v, f, _ = ci.isolated().arrays()
    assert len(np.setdiff1d(np.arange(len(v)), f)) == 3


def _noisy_sphere():
    vol = mv.sphere_volume(65, trunc=0.1)
    v, f, _ = vol.extract()
    rng = np.random.default_rng(0)
    p = v.astype(np.float64)
    r = np.linalg.norm(p, axis=1)
    noisy = p * (1.0 + 0.3 * float(vol.voxel) * rng.standard_normal(len(p)) / r)[:, None]
    return vol, v, f, noisy.astype(F32)


def _radial(p, voxel):
    r = np.linalg.norm(p.astype(np.float64), axis=1) / float(voxel)
    return r.mean(), r.std()


def test_taubin_removes_the_noise_and_keeps_the_radius():
    """sphere_volume(65, trunc=0.1), vertices moved radially by normal noise of sigma 0.3 voxel, 10 iterations at
    lambda 0.5, mu -0.53, boundary fixed.  Measured on this restatement: radial standard deviation 0.300 -> 0.113
    voxel (ratio 0.377), mean radius moved by +0.0012 voxel; 20 plain Laplacian steps (mu = 0) move it by -0.063."""
    vol, _, f, noisy = _noisy_sphere()
    m0, s0 = _radial(noisy, vol.voxel)
    m1, s1 = _radial(cr.smooth(noisy, f, 10, 0.5, -0.53, True), vol.voxel)
    print(f"radial std {s0:.4f} -> {s1:.4f} voxel (ratio {s1 / s0:.3f}), mean radius moved by {m1 - m0:+.5f} voxel")
    assert 0.25 < s0 < 0.35
    assert s1 <= 0.5 * s0
    assert abs(m1 - m0) < 0.01
    m2, _ = _radial(cr.smooth(noisy, f, 20, 0.5, 0.0, True), vol.voxel)
    print(f"20 Laplacian steps move the mean radius by {m2 - m0:+.5f} voxel")
    assert m2 - m0 < -0.03                                         # what Taubin's second step is for


def test_normals_of_a_sphere_are_radial_and_unit():
    """Clean 65^3 sphere.  Measured on this restatement: no zero normal, largest angle to the radial direction
    1.86 degrees, | |n| - 1 | at most 0.53 * 2^-22."""
    _, v, f, _ = _noisy_sphere()
    n = cr.normals(v, f).astype(np.float64)
    length = np.linalg.norm(n, axis=1)
    assert np.all(length > 0)
    p = v.astype(np.float64)
    cos = np.clip((n * p).sum(axis=1) / np.linalg.norm(p, axis=1) / length, -1, 1)
    angle = np.degrees(np.arccos(cos)).max()
    print(f"largest angle to the radial direction {angle:.3f} degrees, | |n| - 1 | <= {np.abs(length - 1).max() * 2 ** 22:.3f} * 2^-22")
    assert angle <= 3.0
    assert np.abs(length - 1).max() <= 2.0 ** -22
    # the inverted sphere's normals point inward: the way the faces do
    vi, fi, _ = mv.sphere_volume(33, trunc=0.2, inverted=True).extract()
    ni = cr.normals(vi, fi).astype(np.float64)
    assert np.all((ni * vi).sum(axis=1) < 0)


def test_keep_largest_of_a_closed_surface_is_closed():
    for vol in (mv.random_sign_volume((14, 11, 9), 5, closed=True), mv.random_sign_volume((19, 23, 21), 6, closed=True)):
        v, f, c = vol.extract()
        assert mv.directed_edge_defects(f, len(v)) == (0, 0), vol.name
        n_comp, kv, kf, kc, lab = cr.filter(v, f, c, 0, keep_largest=True)
        assert n_comp > 1 and 0 < len(kf) < len(f), vol.name
        assert mv.directed_edge_defects(kf, len(kv)) == (0, 0), vol.name
        assert np.all(lab == 0)


FILTERS = ((1, False), (2, False), (8, False), (10 ** 9, False), (0, True), (8, True))


def test_filter_keeps_order_uses_every_vertex_and_labels_afresh():
    kept_some = dropped_some = 0
    for name, v, f, c in family():
        tagged = v.copy()
        tagged[:, 0] = np.arange(len(v))                          # the position tells the old id
        key_in = (f.astype(np.int64) * [len(v) ** 2, len(v), 1]).sum(axis=1) if len(f) else np.zeros(0, np.int64)
        for min_faces, largest in FILTERS:
            n_comp, kv, kf, kc, lab = cr.filter(tagged, f, c, min_faces, largest)
            what = f"{name}, min_faces {min_faces}, keep_largest {largest}"
            assert n_comp == len(np.unique(cr.labels(f, len(v)))), what
            assert np.array_equal(np.unique(kf), np.arange(len(kv))), what          # every vertex on a face
            assert np.array_equal(lab, cr.labels(kf, len(kv))), what
            old = kv[:, 0].astype(np.int64)
            assert np.all(np.diff(old) > 0), what
            assert np.array_equal(kc, c[old]) and np.array_equal(kv[:, 1:], v[old, 1:]), what
            if len(kf):
                key_out = (old[kf] * [len(v) ** 2, len(v), 1]).sum(axis=1)
                assert len(np.unique(key_in)) == len(key_in), what
                order = np.argsort(key_in)
                at = order[np.searchsorted(key_in[order], key_out)]
                assert np.array_equal(key_in[at], key_out) and np.all(np.diff(at) > 0), what    # a subsequence
                count = cr.component_faces(kf, lab)[np.unique(lab)]
                assert count.min() >= min_faces and (not largest or len(count) == 1), what
            kept_some += 0 < len(kf) < len(f)
            dropped_some += len(kf) == 0 and len(f) > 0
        # nothing asked for: nothing changes, isolated vertices included
        n_comp, kv, kf, kc, lab = cr.filter(v, f, c, 0, False)
        assert np.array_equal(kv, v) and np.array_equal(kf, f) and np.array_equal(kc, c) and len(lab) == len(v), name
    assert kept_some >= 10 and dropped_some >= 10


def _read_ply(path):
    """A reader for the two vertex layouts save_mesh_ply writes."""
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n_v = n_f = 0
    props = []
    for ln in lines[2:]:
        w = ln.split()
        if w[:2] == ["element", "vertex"]:
            n_v = int(w[2])
        elif w[:2] == ["element", "face"]:
            n_f = int(w[2])
        elif w and w[0] == "property" and w[1] != "list":
            props.append((w[2], {"float": "<f4", "uchar": "u1"}[w[1]]))
    rec = np.dtype(props)
    verts = np.frombuffer(body, rec, n_v)
    rest = body[n_v * rec.itemsize:]
    assert len(rest) == 13 * n_f
    faces = np.array([struct.unpack_from("<B3i", rest, 13 * i) for i in range(n_f)], np.int64).reshape(-1, 4)
    assert np.all(faces[:, 0] == 3)
    return [p[0] for p in props], verts, faces[:, 1:].astype(np.int32)


def test_save_mesh_ply_with_normals_round_trips(tmp_path):
    from amvs.core.utils import save_mesh_ply
    v, f, c = ci.threshold().arrays()
    n = cr.normals(v, f)
    save_mesh_ply(v, f, c, str(tmp_path / "n.ply"), normals=n)
    names, rec, faces = _read_ply(tmp_path / "n.ply")
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], -1).view(np.uint32), v.view(np.uint32))
    assert np.array_equal(np.stack([rec["nx"], rec["ny"], rec["nz"]], -1).view(np.uint32), n.view(np.uint32))
    assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], -1), c)
    assert np.array_equal(faces, f)
    save_mesh_ply(np.zeros((0, 3)), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint8), str(tmp_path / "e.ply"),
                  normals=np.zeros((0, 3)))
    names, rec, faces = _read_ply(tmp_path / "e.ply")
    assert len(names) == 9 and len(rec) == 0 and len(faces) == 0


def test_save_mesh_ply_without_normals_writes_the_same_bytes_as_before(tmp_path):
    from amvs.core.utils import save_mesh_ply
    v, f, c = ci.isolated().arrays()
    for kwargs in ({}, {"normals": None}):
        save_mesh_ply(v, f, c, str(tmp_path / "m.ply"), **kwargs)
        expect = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\n"
                  "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
                  f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
        for p, col in zip(v, c):
            expect += struct.pack("<3f3B", *p, *col)
        for tri in f:
            expect += struct.pack("<B3i", 3, *tri)
        assert open(tmp_path / "m.ply", "rb").read() == expect
