#!/usr/bin/env python3
"""Device time of the surface-mesh kernels (csrc/amvs_mesh.hip) at the CLI operating point (run on the GPU box):
16 views at 1008 x 756, patch 11, the maps of the extended mode (the reference's algorithm leaves too few correct
depths for a surface) resident on the device, a 256^3 TSDF volume around the fused cloud.  Integration and extraction are timed separately with HIP events on the engine's stream (the extraction
includes its two count read-backs); the first-order bounds of DESIGN.md section 8 are printed next to them.

    python tools/mesh_time.py [n_views W H dim]
"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import amvs  # noqa: E402,F401
from amvs.core.mvs_patchmatch import PatchMatchMVS  # noqa: E402
from amvs.synthetic import make_scene  # noqa: E402

n_views = int(sys.argv[1]) if len(sys.argv) > 1 else 16
W, H = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1008, 756)
dim = int(sys.argv[4]) if len(sys.argv) > 4 else 256
REPS = 5

sc = make_scene(n_views, H, W, device="cuda")
images = [{"image": np.ascontiguousarray(c)} for c in sc.colors]
pm = PatchMatchMVS(sc.camera, scale=1.0, patch_size=11, extended=True)
points, _, maps = pm._reconstruct_maps(images, sc.poses)
lo, hi = points.min(axis=0), points.max(axis=0)
side = float((hi - lo).max()) * 1.05
centre = 0.5 * (lo + hi)
voxel = side / (dim - 1)
origin = centre - 0.5 * side
dims = (dim, dim, dim)
trunc = 4.0 * voxel
ids, src = pm._mesh_inputs(maps)
poses = [(sc.poses[i].R, sc.poses[i].t) for i in ids]
eng = pm._engine
stream = torch.cuda.Stream()
eng.set_stream(stream.cuda_stream)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    t = time.time()
    out = fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), (time.time() - t) * 1e3, out


t_int, t_ext, w_int, w_ext = [], [], [], []
for rep in range(REPS + 1):
    ms, wall, _ = timed(lambda: eng.tsdf_integrate(pm.K_scaled, poses, pm.min_views, origin, voxel, dims, trunc, **src))
    ms2, wall2, mesh = timed(eng.tsdf_extract)
    if rep:                                   # the first round loads the code objects and grows the buffers
        t_int.append(ms); t_ext.append(ms2); w_int.append(wall); w_ext.append(wall2)
eng.set_stream(None)
verts, faces, _ = mesh
tsdf, weight, _ = eng.tsdf_volume()
n_pts = dim ** 3
voxel_views = n_pts * len(ids)
observed = int((weight > 0).sum())
print(f"mesh_time: {len(ids)} maps {W}x{H}, patch 11 (extended mode), grid {dim}^3 = {n_pts:,} points (voxel {voxel:.4g}), "
      f"{observed:,} observed; mesh {len(verts):,} vertices, {len(faces):,} faces")
print(f"  integrate: median {np.median(t_int):.3f} ms device (min {min(t_int):.3f}, wall median {np.median(w_int):.3f} ms)")
print(f"  extract:   median {np.median(t_ext):.3f} ms device (min {min(t_ext):.3f}, wall median {np.median(w_ext):.3f} ms)")
# first-order bounds (estimates; MI355X peaks: 78.6 T FP32 VALU lane-operations/s (157.3 TFLOP/s counting an FMA as 2),
# 8 TB/s HBM)
valu_ms = voxel_views * 30 / 78.6e12 * 1e3
gather_ms = (voxel_views * 11 + n_pts * 20) / 8e12 * 1e3
ext_bytes = n_pts * (8 + 1 + 4 + 4 + 4) * 2 + n_pts * 8 * 2
print(f"  bounds (estimates): integrate VALU {valu_ms:.3f} ms / bytes {gather_ms:.3f} ms "
      f"({voxel_views:,} voxel-views x 30 VALU ops, x 11 B gathered + 20 B written per point); "
      f"extract streaming {ext_bytes / 8e12 * 1e3:.3f} ms ({ext_bytes / n_pts:.0f} B per point)")
