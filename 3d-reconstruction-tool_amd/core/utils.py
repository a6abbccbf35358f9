"""Output helpers around the dense stage (reference: src/core/utils.py).

`save_ply` has the reference's signature (plus optional normals) and writes the same bytes (utils.py:8-37); the per-point
Python `f.write` loop there dominates wall time for multi-million-point clouds, so the formatting
runs in the native library (`amvs_write_ply`, host-only).  `save_mesh_ply` writes the surface mesh of
PatchMatchMVS.reconstruct_mesh as binary little-endian PLY (no reference counterpart).
"""
import ctypes as C
from pathlib import Path

import numpy as np

from .. import _lib


def rows_matmul(rows: np.ndarray, matrix: np.ndarray) -> np.ndarray:
    """rows (m, 3) @ matrix (3, 3) with every row rounded alike: x*b0 + y*b1 + z*b2 as the left-to-right fused
    chain, which is what the device computes (amvs_fusion.hip) and what the BLAS matrix-matrix kernels give.  NumPy
    hands a product of ONE row to the matrix-vector routine instead, whose rounding differs, so a single row is
    multiplied as two.

    This is a deliberate departure from the reference, which writes a plain `@` and so gets the matrix-vector rounding
    for a view with exactly one selected pixel: there the reference's point depends on how many OTHER pixels of the
    view were selected.  The project defines a point by the fused chain alone, on host and device; for one-pixel
    views both are therefore a last bit away from the reference, and equal to each other.  That a two-row product
    rounds like an m-row one is a property of the BLAS in use, not a guarantee: test_cloud_restatement_cpu.py holds
    the host path to the exact fused chain for 1, 2, 3 and 4 rows per view and fails where a BLAS does otherwise."""
    if len(rows) == 1:
        return (np.concatenate([rows, rows]) @ matrix)[:1]
    return rows @ matrix


def nearest_map_neighbours(centers: np.ndarray, k) -> np.ndarray:
    """Neighbour rows of the cross-view depth-map filter (Engine.depth_filter): for each of the n maps the k nearest camera
    centres among the other maps -- the rule and the stable order of DenseStereoReconstructor._find_neighbors (distance
    ascending, ties in map order).  k = None, or a single map: None (every other map in ascending index).  Otherwise
    (n, min(k, n - 1)) int32."""
    centers = np.asarray(centers, np.float64).reshape(-1, 3)
    n = len(centers)
    if k is None or n < 2:
        return None
    k = int(k)
    if k < 1:
        raise ValueError("filter_neighbours must be None or a positive integer")
    rows = []
    for j in range(n):
        ranked = sorted(((i, np.linalg.norm(centers[i] - centers[j])) for i in range(n) if i != j), key=lambda item: item[1])
        rows.append([i for i, _ in ranked[:k]])
    return np.asarray(rows, np.int32)


def save_ply(points: np.ndarray, colors: np.ndarray, output_path: str, normals: np.ndarray = None):
    """Save an (N,3) cloud with (N,3) RGB colours as ASCII PLY.  With normals (N,3) float32 every vertex is
    x y z nx ny nz red green blue (`amvs_write_ply_normals`; no reference counterpart); without, the file is the
    reference's byte for byte."""
    output_path = Path(output_path)
    output_path.parent.mkdir(parents=True, exist_ok=True)
    n = len(points)
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(n, 3))
    cols = np.ascontiguousarray(np.asarray(colors).reshape(n, 3).astype(int).astype(np.int64))
    lib = _lib.load()
    if normals is None:
        name = "amvs_write_ply"
        rc = lib.amvs_write_ply(str(output_path).encode(), pts.ctypes.data_as(C.POINTER(C.c_double)),
                                cols.ctypes.data_as(C.POINTER(C.c_int64)), n)
    else:
        name = "amvs_write_ply_normals"
        nrm = np.ascontiguousarray(np.asarray(normals, dtype=np.float32).reshape(n, 3))
        rc = lib.amvs_write_ply_normals(str(output_path).encode(), pts.ctypes.data_as(C.POINTER(C.c_double)),
                                        nrm.ctypes.data_as(_lib.f32p), cols.ctypes.data_as(C.POINTER(C.c_int64)), n)
    if rc != 0:
        raise _lib.AmvsError(f"{name} failed ({rc}): {lib.amvs_last_error(None).decode()}")
    print(f"Saved {n:,} points to {output_path}")


def save_mesh_ply(vertices: np.ndarray, faces: np.ndarray, colors: np.ndarray, output_path: str, normals: np.ndarray = None):
    """Save a triangle mesh as binary little-endian PLY (read by MeshLab, Open3D and most tools): `element vertex`
    with float x, y, z and uchar red, green, blue; `element face` with `property list uchar int vertex_indices`.
    vertices (V,3), faces (F,3) vertex ids, colors (V,3) RGB in 0..255.  With normals (V,3) the vertex element is
    x y z nx ny nz red green blue (the order MeshLab and Open3D write); without, the file is as it always was."""
    output_path = Path(output_path)
    output_path.parent.mkdir(parents=True, exist_ok=True)
    verts = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    n_v = len(verts)
    tris = np.asarray(faces).reshape(-1, 3)
    cols = np.asarray(colors).reshape(n_v, 3)
    if tris.size and (tris.min() < 0 or tris.max() >= n_v):
        raise ValueError("face vertex ids out of range")
    if cols.size and (cols.min() < 0 or cols.max() > 255):
        raise ValueError("colours must lie in 0..255")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        nrm = np.asarray(normals, dtype=np.float32).reshape(n_v, 3)
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    vrec = np.empty(n_v, dtype=fields + [("r", "u1"), ("g", "u1"), ("b", "u1")])
    vrec["x"], vrec["y"], vrec["z"] = verts[:, 0], verts[:, 1], verts[:, 2]
    if normals is not None:
        vrec["nx"], vrec["ny"], vrec["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    vrec["r"], vrec["g"], vrec["b"] = cols[:, 0], cols[:, 1], cols[:, 2]
    frec = np.empty(len(tris), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"] = 3
    frec["v"] = tris.astype(np.int32)
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {n_v}\n"
              "property float x\nproperty float y\nproperty float z\n"
              + ("property float nx\nproperty float ny\nproperty float nz\n" if normals is not None else "") +
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              f"element face {len(tris)}\n"
              "property list uchar int vertex_indices\n"
              "end_header\n")
    with open(output_path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())
    print(f"Saved mesh with {n_v:,} vertices and {len(tris):,} faces to {output_path}")


def _png_rgb8(image: np.ndarray) -> bytes:
    """An (H,W,3) uint8 RGB image as a PNG file's bytes: 8-bit truecolour, no interlace, every row with filter 0."""
    import struct
    import zlib
    h, w = image.shape[:2]

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    rows = np.zeros((h, 1 + 3 * w), np.uint8)
    rows[:, 1:] = image.reshape(h, 3 * w)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def save_mesh_obj(vertices: np.ndarray, faces: np.ndarray, uv: np.ndarray, atlas: np.ndarray, output_path: str,
                  normals: np.ndarray = None):
    """Save a textured triangle mesh as Wavefront OBJ with its material and texture: name.obj, name.mtl and name.png beside
    each other, `name` being output_path without its suffix.  vertices (V,3), faces (F,3) vertex ids, uv (F,3,2) per corner
    with v up (Engine.mesh_texture's), atlas (Ht,Wt,3) uint8 RGB with row 0 on top.  The OBJ has `v`, one `vt` per corner,
    `vn` with normals (V,3), and `f a/ta` or `f a/ta/na` with ids from 1; the MTL names the PNG as map_Kd.  The PNG is
    written with the standard library alone (8-bit RGB, filter 0)."""
    output_path = Path(output_path)
    output_path.parent.mkdir(parents=True, exist_ok=True)
    stem = output_path.with_suffix("")
    name = stem.name
    verts = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    tris = np.asarray(faces).reshape(-1, 3)
    uvs = np.asarray(uv, dtype=np.float32).reshape(-1, 3, 2)
    img = np.asarray(atlas)
    if tris.size and (tris.min() < 0 or tris.max() >= len(verts)):
        raise ValueError("face vertex ids out of range")
    if len(uvs) != len(tris):
        raise ValueError(f"uv must be ({len(tris)}, 3, 2)")
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise ValueError("atlas must be (Ht, Wt, 3) uint8")
    if len(tris) and img.size == 0:
        raise ValueError("a mesh with faces needs an atlas that is not empty")
    if img.size == 0:
        img = np.zeros((1, 1, 3), np.uint8)                      # a PNG has at least one pixel
    lines = [f"mtllib {name}.mtl", f"usemtl {name}"]
    lines += ["v %.9g %.9g %.9g" % tuple(p) for p in verts.tolist()]
    lines += ["vt %.9g %.9g" % tuple(t) for t in uvs.reshape(-1, 2).tolist()]
    if normals is not None:
        nrm = np.asarray(normals, dtype=np.float32).reshape(len(verts), 3)
        lines += ["vn %.9g %.9g %.9g" % tuple(n) for n in nrm.tolist()]
    for f, (a, b, c) in enumerate(tris.tolist()):
        t = 3 * f + 1
        if normals is None:
            lines.append(f"f {a + 1}/{t} {b + 1}/{t + 1} {c + 1}/{t + 2}")
        else:
            lines.append(f"f {a + 1}/{t}/{a + 1} {b + 1}/{t + 1}/{b + 1} {c + 1}/{t + 2}/{c + 1}")
    stem.with_suffix(".obj").write_text("\n".join(lines) + "\n")
    stem.with_suffix(".mtl").write_text(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    stem.with_suffix(".png").write_bytes(_png_rgb8(np.ascontiguousarray(img)))
    print(f"Saved textured mesh with {len(verts):,} vertices, {len(tris):,} faces and a {img.shape[1]} x {img.shape[0]} texture "
          f"to {stem.with_suffix('.obj')}")


def compute_scene_bounds(points: np.ndarray) -> dict:
    """Axis-aligned bounds, centre and extent of a cloud (reference utils.py:72-86)."""
    lo, hi = points.min(axis=0), points.max(axis=0)
    return {"min": lo, "max": hi, "center": (lo + hi) / 2, "size": hi - lo}
