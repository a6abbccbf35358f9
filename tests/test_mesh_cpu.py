"""Surface mesh without a GPU: the NumPy restatement of csrc/amvs_mesh.hip (tests/mesh_restatement.py) on analytic
signed distance fields, and the binary PLY writer."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_restatement as mr  # noqa: E402
import mesh_volumes as mv  # noqa: E402

import amvs  # noqa: E402,F401


def _edge_counts(faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e = np.sort(e, axis=1)
    uniq, counts = np.unique(e, axis=0, return_counts=True)
    return uniq, counts


def _normals(verts, faces):
    v = verts.astype(np.float64)
    return np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])


def _field(fn, origin, voxel, dims, trunc):
    X, Y, Z = mr.grid_coords(origin, voxel, dims)
    d = fn(X.astype(np.float64), Y.astype(np.float64), Z.astype(np.float64))
    tsdf = np.clip(d / trunc, -1.0, 1.0).astype(np.float32)
    weight = np.ones(tsdf.shape, np.float32)
    color = np.zeros(tsdf.shape + (3,), np.float32)
    color[..., 0] = 200.0
    color[..., 1] = np.float32(100.0)
    color[..., 2] = (np.asarray(X) > 0).astype(np.float32) * 255.0
    return tsdf, weight, color


def test_triangle_table_from_first_principles():
    """Odd sign counts give one triangle, two-two cases two, 0 and 15 none; complementary lone-vertex cases are the
    same triangle wound the other way."""
    def rotations(t):
        return [t[k:] + t[:k] for k in range(3)]

    for case, tris in enumerate(mr.TRI_TABLE):
        bits = bin(case).count("1")
        assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[bits]
        if bits in (1, 3):
            a, b = tris[0], mr.TRI_TABLE[15 - case][0]
            assert [a[0], a[2], a[1]] in rotations(b)


def test_sphere_is_a_closed_outward_manifold():
    voxel, r = 0.1, 1.23
    dims = (32, 30, 31)
    origin = (-1.6, -1.5, -1.55)
    trunc = 3 * voxel
    tsdf, weight, color = _field(lambda x, y, z: np.sqrt(x * x + y * y + z * z) - r, origin, voxel, dims, trunc)
    verts, faces, cols = mr.extract(tsdf, weight, color, origin, voxel)
    assert len(faces) > 1000
    # every vertex is referenced, every edge has exactly 2 faces, V - E + F = 2
    assert np.array_equal(np.unique(faces), np.arange(len(verts)))
    edges, counts = _edge_counts(faces)
    assert np.all(counts == 2)
    assert len(verts) - len(edges) + len(faces) == 2
    # on the sphere to 0.05 voxel, normals outward
    rad = np.linalg.norm(verts.astype(np.float64), axis=1)
    assert np.abs(rad - r).max() <= 0.05 * voxel
    cen = verts[faces].astype(np.float64).mean(axis=1)
    assert np.all(np.einsum("ij,ij->i", _normals(verts, faces), cen) > 0)
    # colours: the corners' means interpolated and rounded
    assert np.all(cols[:, 0] == 200) and np.all(cols[:, 1] == 100)
    assert set(np.unique(cols[:, 2])) <= set(range(256))


def test_plane_is_flat_and_open_only_at_the_box():
    voxel = 0.05
    dims = (21, 17, 19)
    origin = (0.0, 0.0, 0.0)
    trunc = 4 * voxel
    n = np.array([0.2, -0.3, 1.0])
    n /= np.linalg.norm(n)
    c = 0.45
    tsdf, weight, color = _field(lambda x, y, z: n[0] * x + n[1] * y + n[2] * z - c, origin, voxel, dims, trunc)
    verts, faces, _ = mr.extract(tsdf, weight, color, origin, voxel)
    v = verts.astype(np.float64)
    assert np.abs(v @ n - c).max() < 1e-4 * voxel * 100
    # normals along +n (increasing distance)
    nrm = _normals(verts, faces)
    assert np.all(nrm @ n > 0)
    edges, counts = _edge_counts(faces)
    assert counts.max() == 2
    hi = np.array(origin) + (np.array(dims) - 1) * voxel
    border = edges[counts == 1]
    assert len(border) > 0
    ends = v[border.reshape(-1)]
    on_box = np.any((np.abs(ends - np.array(origin)) < 1e-5) | (np.abs(ends - hi) < 1e-5), axis=1)
    assert np.all(on_box)


def test_unobserved_corners_are_not_meshed():
    voxel, r = 0.1, 0.8
    dims = (20, 20, 20)
    origin = (-1.0, -1.0, -1.0)
    tsdf, weight, color = _field(lambda x, y, z: np.sqrt(x * x + y * y + z * z) - r, origin, voxel, dims, 0.3)
    X, _, _ = mr.grid_coords(origin, voxel, dims)
    weight[np.asarray(X) > 0.05] = 0.0
    verts, faces, _ = mr.extract(tsdf, weight, color, origin, voxel)
    assert len(faces) > 0
    assert verts[np.unique(faces)][:, 0].max() <= 0.05 + 1e-6
    _, counts = _edge_counts(faces)
    assert counts.max() == 2


def test_integration_restatement_on_a_fronto_parallel_wall():
    """One camera looking down +z at a wall z = 2: tsdf = clamp((2 - z) / trunc) where observed, 1 behind is cut."""
    H, W = 24, 32
    K = np.array([[30.0, 0, W / 2], [0, 30.0, H / 2], [0, 0, 1]], np.float32)
    depth = np.full((1, H, W), 2.0, np.float32)
    conf = np.full((1, H, W), 3.0, np.float32)
    bgr = np.zeros((1, H, W, 3), np.uint8)
    bgr[..., 0], bgr[..., 1], bgr[..., 2] = 10, 20, 30
    pose = np.concatenate([np.eye(3).reshape(9), np.zeros(3)]).astype(np.float32)[None]
    voxel, trunc = np.float32(0.05), np.float32(0.2)
    dims = (5, 5, 21)
    origin = (-0.1, -0.1, 1.5)
    tsdf, weight, color = mr.integrate(depth, conf, bgr, K, pose, 2, origin, voxel, dims, trunc)
    _, _, Z = mr.grid_coords(origin, voxel, dims)
    Z = np.asarray(Z)
    seen = (2.0 - Z) >= -trunc - 1e-6
    assert np.all(weight[seen & ((2.0 - Z) > -trunc + 1e-6)] == 1)
    assert np.all(weight[(2.0 - Z) < -trunc - 1e-6] == 0)
    obs = weight > 0
    np.testing.assert_allclose(tsdf[obs], np.minimum(1, (2.0 - Z[obs]) / trunc), atol=1e-5)
    assert np.all(color[obs] == np.array([30, 20, 10], np.float32))
    # confidence below min_views: nothing observed
    _, w2, _ = mr.integrate(depth, conf, bgr, K, pose, 4, origin, voxel, dims, trunc)
    assert not np.any(w2)


def _read_ply(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0"
    n_v = int(next(h for h in header if h.startswith("element vertex")).split()[-1])
    n_f = int(next(h for h in header if h.startswith("element face")).split()[-1])
    assert "property list uchar int vertex_indices" in header
    assert header[3:9] == ["property float x", "property float y", "property float z",
                           "property uchar red", "property uchar green", "property uchar blue"]
    vdt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    assert len(data) == end + n_v * vdt.itemsize + n_f * fdt.itemsize
    v = np.frombuffer(data, vdt, n_v, end)
    f = np.frombuffer(data, fdt, n_f, end + n_v * vdt.itemsize)
    assert np.all(f["n"] == 3)
    return (np.stack([v["x"], v["y"], v["z"]], 1), f["v"].copy(), np.stack([v["r"], v["g"], v["b"]], 1))


def test_save_mesh_ply_round_trip(tmp_path):
    from amvs.core.utils import save_mesh_ply
    voxel, r = 0.1, 0.7
    dims = (18, 18, 18)
    origin = (-0.9, -0.9, -0.9)
    tsdf, weight, color = _field(lambda x, y, z: np.sqrt(x * x + y * y + z * z) - r, origin, voxel, dims, 0.3)
    verts, faces, cols = mr.extract(tsdf, weight, color, origin, voxel)
    path = tmp_path / "sub" / "mesh.ply"
    save_mesh_ply(verts, faces, cols, str(path))
    v, f, c = _read_ply(path)
    assert v.shape == verts.shape and f.shape == faces.shape and c.shape == cols.shape
    assert np.array_equal(v.view(np.uint32), verts.view(np.uint32))
    assert np.array_equal(f, faces)
    assert np.array_equal(c, cols)
    # an empty mesh is a valid file as well
    save_mesh_ply(np.zeros((0, 3)), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint8), str(tmp_path / "e.ply"))
    v, f, c = _read_ply(tmp_path / "e.ply")
    assert len(v) == 0 and len(f) == 0
    with pytest.raises(ValueError):
        save_mesh_ply(verts, faces + len(verts), cols, str(tmp_path / "bad.ply"))


def test_mesh_grid_defaults():
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    pts = np.array([[0.0, 0.0, 0.0], [2.0, 1.0, 0.5]])
    origin, voxel, dims, trunc = PatchMatchMVS._mesh_grid(pts, None, None, 4.0, 101)
    assert voxel == pytest.approx(2.0 / (100 - 8))
    assert trunc == pytest.approx(4 * voxel)
    assert dims[0] == 101 and dims[1] < dims[0] and dims[2] < dims[1]
    np.testing.assert_allclose(origin, pts[0] - trunc)
    assert np.all(origin + (np.array(dims) - 1) * voxel >= pts[1] + trunc - 1e-9)
    origin, voxel, dims, trunc = PatchMatchMVS._mesh_grid(pts, ((0, 0, 0), (1, 2, 3)), None, 2.0, 31)
    assert voxel == pytest.approx(0.1) and dims == (11, 21, 31) and trunc == pytest.approx(0.2)
    with pytest.raises(ValueError):
        PatchMatchMVS._mesh_grid(pts, None, None, 4.0, 9)


def test_abi_declares_the_mesh_entry_points():
    from amvs import _lib
    for name in ("amvs_tsdf_integrate", "amvs_tsdf_extract", "amvs_fetch_mesh", "amvs_tsdf_fetch_volume",
                 "amvs_tsdf_set_volume"):
        assert name in _lib.SIGNATURES
    assert hasattr(amvs, "save_mesh_ply") or "save_mesh_ply" in amvs.__all__
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "amvs.h")).read()
    assert f"#define AMVS_TSDF_MAX_POINTS (1ll << {int(np.log2(_lib.TSDF_MAX_POINTS))})" in hdr


# ---- the generated volumes and scenes of tests/mesh_volumes.py, on the restatement alone -------------------------

def test_random_sign_family_reaches_every_tetrahedron_case():
    """The coverage cap of the GPU comparison: over the random-sign family every one of the 84 (Kuhn tetrahedron,
    sign case 1 .. 14) pairs occurs at least 10 times among the meshed tetrahedra (the volumes fused from the
    height-field scenes reach 38 of the 84)."""
    family = mv.random_sign_family()
    total = np.zeros((6, 16), np.int64)
    for vol in family:
        total += mv.tet_case_coverage(vol.tsdf, vol.weight)
    emitting = total[:, 1:15]
    print("hits per (tetrahedron, case 1..14):\n", emitting)
    assert emitting.shape == (6, 14) and emitting.min() >= 10, emitting
    # the recipe: ragged sizes, thin axes, exact zeros of both signs, unobserved points with garbage behind them
    assert sum(int(np.prod(v.dims)) % 256 != 0 for v in family) >= 3
    assert {a for v in family for a in range(3) if v.dims[a] == 2} == {0, 1, 2}
    for vol in family[:1]:
        seen = vol.weight > 0
        zero = vol.tsdf[seen] == 0
        neg = np.signbit(vol.tsdf[seen])
        assert 0.01 < (zero & ~neg).mean() < 0.06 and 0.01 < (zero & neg).mean() < 0.06
        assert 0.15 < (~seen).mean() < 0.35
        assert np.isnan(vol.tsdf[~seen]).any() and (vol.tsdf[~seen] < 0).any()
        assert np.all(np.isfinite(vol.tsdf[seen])) and np.all(vol.color[seen] == np.floor(vol.color[seen]))
        assert np.all(vol.color[seen] <= 255 * vol.weight[seen][:, None])
    # the coverage function against the faces the restatement emits: 1 per odd case, 2 per two-two case
    for vol in family:
        c = mv.tet_case_coverage(vol.tsdf, vol.weight)
        per_case = np.array([len(t) for t in mr.TRI_TABLE])
        assert int((c * per_case[None, :]).sum()) == len(vol.extract()[1])


@pytest.mark.parametrize("dims,seed", [((14, 11, 9), 5), ((19, 23, 21), 6)])
def test_random_sign_surface_is_closed_and_consistently_oriented(dims, seed):
    """A fully observed random-sign volume (exact 0.0 and -0.0 included) whose outermost layer is outside: every
    directed edge of the restatement's mesh occurs exactly once and its opposite exactly once.  Zero-area triangles
    from exact zeros count like any other; coincident vertices keep distinct ids."""
    vol = mv.random_sign_volume(dims, seed, closed=True)
    assert np.all(vol.weight > 0) and (vol.tsdf == 0).sum() > 10 and np.signbit(vol.tsdf[vol.tsdf == 0]).any()
    verts, faces, _ = vol.extract()
    assert len(faces) > 5000
    assert np.array_equal(np.unique(faces), np.arange(len(verts)))
    assert np.all(faces[:, 0] != faces[:, 1]) and np.all(faces[:, 1] != faces[:, 2]) and np.all(faces[:, 0] != faces[:, 2])
    assert mv.directed_edge_defects(faces, len(verts)) == (0, 0)
    assert len(np.unique(verts, axis=0)) < len(verts)              # coincident vertices exist and stay apart


def test_corner_case_volumes():
    for vol, expect in mv.corner_case_volumes():
        verts, faces, cols = vol.extract()
        if expect is not None:
            assert (len(verts), len(faces)) == expect, vol.name
            assert verts.shape == (0, 3) and faces.shape == (0, 3) and cols.shape == (0, 3)
    # colour means that land exactly on x.5, on 0 and on 255
    for vol, expect in mv.colour_tie_volumes():
        verts, faces, cols = vol.extract()
        assert len(verts) == 25 and np.all(cols == expect[None, :]), (vol.name, np.unique(cols, axis=0))
    # the single cube: every pattern but all-outside and all-inside gives faces, complementary patterns the same
    # number of them, and the vertices are the sign-changing ones among the cube's 19 tetrahedron edges
    for pattern in range(256):
        vol = mv.cube_volume(pattern)
        verts, faces, _ = vol.extract()
        assert (len(faces) == 0) == (pattern in (0, 255))
        assert len(faces) == len(mv.cube_volume(255 - pattern).extract()[1])
        crossing = sum(((pattern >> a) & 1) != ((pattern >> b) & 1) for a in range(8) for b in range(a + 1, 8) if a & b == a)
        assert len(verts) == crossing and np.array_equal(np.unique(faces), np.arange(len(verts))), pattern


def test_grid_plane_vertices_coincide_on_the_zero_layer():
    for sign in (1.0, -1.0):
        vol = mv.grid_plane_volume((9, 8, 11), 2, 5, sign=sign)
        assert np.all(vol.tsdf[5] == 0) and np.all(np.signbit(vol.tsdf[5]) == (sign < 0))
        verts, faces, _ = vol.extract()
        assert len(faces) > 0 and np.all(verts[:, 2] == np.float32(1.0) + np.float32(5) * np.float32(0.125))
        assert len(np.unique(verts, axis=0)) == 9 * 8 < len(verts)
        nrm = _normals(verts, faces)
        assert np.all(nrm[:, 2] * sign >= 0) and np.any(nrm[:, 2] != 0) and np.any(np.all(nrm == 0, axis=1))


def test_inverted_sphere_is_closed_and_faces_inward():
    plain = mv.sphere_volume(33, trunc=0.2)
    inverted = mv.sphere_volume(33, trunc=0.2, inverted=True)
    vol = {}
    for name, v in (("plain", plain), ("inverted", inverted)):
        verts, faces, _ = v.extract()
        assert len(faces) > 10000 and mv.directed_edge_defects(faces, len(verts)) == (0, 0)
        assert len(faces) == 2 * len(verts) - 4
        vol[name] = mv.signed_volume(verts, faces)
    ball = 4.0 / 3.0 * np.pi * 0.8 ** 3
    assert vol["plain"] == pytest.approx(ball, rel=0.01) and vol["inverted"] == pytest.approx(-ball, rel=0.01)


def test_integration_scenes_take_every_branch():
    """The branch cap of the GPU comparison: over the hand-built scenes every guard of the integration is taken, and
    every edge mesh_volumes.branch_counts names is met, at least 100 times: zc == 0, pixels u == -0.5 and u == W - 0.5,
    depth -0.0 / NaN / inf, confidence NaN / just below / exactly min_views / inf, sdf == -trunc and one ulp beyond it,
    sdf / trunc == 1, pixel ties."""
    total = dict.fromkeys(mv.BRANCHES, 0)
    scenes = mv.integration_scenes()
    per_scene = []
    for sc in scenes:
        counts = mv.branch_counts(sc)
        per_scene.append(counts)
        print(sc.name, counts)
        for k, n in counts.items():
            total[k] += n
        # the counter agrees with the restatement on what is kept
        assert counts["kept"] == int(sc.integrate()[1].sum()), sc.name
    assert set(total) == set(mv.BRANCHES)
    for k, n in total.items():
        assert n >= 100, (k, n)
    # what each scene is there for, scene by scene
    for counts in per_scene[:2]:                                     # exact arithmetic
        for k in ("tie", "tie_first", "tie_last", "at_cut", "beyond_cut", "clamped", "at_one"):
            assert counts[k] >= 100, (k, counts[k])
    for k in ("behind", "zc_zero", "huge"):                          # cameras inside the box
        assert per_scene[2][k] >= 100, (k, per_scene[2][k])
    for k in ("depth_neg_zero", "depth_nan", "depth_inf", "conf_nan", "conf_below", "conf_at_min", "conf_inf"):
        assert per_scene[3][k] >= 100, (k, per_scene[3][k])          # map content
    # one ulp beyond the cut is outside the volume, sdf == -trunc inside it with the value -1
    sc = scenes[0]
    tsdf, weight, _ = mr.integrate(sc.depth[2:3], sc.conf[2:3], sc.colors[2:3], sc.K, sc.poses[2:3], sc.min_views,
                                   sc.origin, sc.voxel, sc.dims, sc.trunc)
    one = mv.branch_counts(mv.Scene("near map", sc.depth[2:3], sc.conf[2:3], sc.colors[2:3], sc.K, sc.poses[2:3],
                                    sc.min_views, sc.origin, sc.voxel, sc.dims, sc.trunc))
    assert one["beyond_cut"] > 0 and one["kept"] == one["at_cut"] > 0      # the layers behind Z = 0.5 are cut as well
    assert int((weight[0] > 0).sum()) == one["at_cut"] and not np.any(weight[1:])
    assert np.all(tsdf[0][weight[0] > 0] == -1.0)
    # ties on whole columns of the exact scenes, at pixels -0.5 (inside) and W - 0.5 (outside) as well
    for sc in scenes[:2]:
        X, _, Z = mr.grid_coords(sc.origin, sc.voxel, sc.dims)
        u = np.float32(8.0) * np.asarray(X)[np.asarray(Z) == 2.0] + sc.K[0, 2]
        assert u.min() == -0.5 and (u == sc.W - 0.5).any() and mv.branch_counts(sc)["tie"] >= 1000
    # many maps: at least 16, and every weight from 0 to the map count occurs
    many = scenes[-1]
    assert many.n >= 16
    assert np.array_equal(np.unique(many.integrate()[1]), np.arange(many.n + 1))
    # the content scene holds every kind of bad value
    content = scenes[3]
    assert np.isnan(content.depth).any() and np.isinf(content.depth).any() and (content.depth < 0).any()
    assert (content.depth == 0).any() and np.isnan(content.conf).any() and np.isinf(content.conf).any()
    assert (content.conf == content.min_views).any()


def test_branch_counter_on_the_fronto_parallel_wall():
    """branch_counts on a scene small enough to count by hand: one camera at the origin, a wall at depth 2, a
    column of 21 grid points on the optical axis at Z = 1.5 .. 2.5 (trunc 0.25)."""
    H, W = 8, 8
    sc = mv.Scene("axis", np.full((1, H, W), 2.0), np.full((1, H, W), 3.0), np.zeros((1, H, W, 3), np.uint8),
                  [[8.0, 0, 4.0], [0, 8.0, 4.0], [0, 0, 1]], mv._pose()[None], 2.0, (0.0, 0.0, 1.5), 0.0625, (2, 2, 17), 0.25)
    c = mv.branch_counts(sc)
    # Z = 1.5 + k / 16: sdf / trunc > 1 for k < 4, == 1 at k = 4, sdf == -trunc at k = 12, cut for k > 12; 4 points per layer
    assert (c["clamped"], c["at_one"], c["at_cut"], c["cut"], c["kept"]) == (16, 4, 4, 16, 52)
    assert c["behind"] == c["outside"] == c["no_depth"] == c["low_conf"] == 0
