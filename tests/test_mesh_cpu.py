"""Surface mesh without a GPU: the NumPy restatement of csrc/amvs_mesh.hip (tests/mesh_restatement.py) on analytic
signed distance fields, and the binary PLY writer."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_restatement as mr  # noqa: E402

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
    for name in ("amvs_tsdf_integrate", "amvs_tsdf_extract", "amvs_fetch_mesh", "amvs_tsdf_fetch_volume"):
        assert name in _lib.SIGNATURES
    assert hasattr(amvs, "save_mesh_ply") or "save_mesh_ply" in amvs.__all__
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "amvs.h")).read()
    assert f"#define AMVS_TSDF_MAX_POINTS (1ll << {int(np.log2(_lib.TSDF_MAX_POINTS))})" in hdr
