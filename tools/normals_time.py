#!/usr/bin/env python3
"""Device time of the cloud-normal kernels (csrc/amvs_cloud_normals.hip) at the CLI operating point (run on the GPU box), a
sibling of tools/mesh_time.py: 16 views at 1008 x 756, patch 11, the maps resident on the device and the cloud that
reconstruct() yields there.  The fit alone (amvs_depth_normals, the maps stay on the device) and the whole
amvs_cloud_normals call (the fit in the world frame, the cloud kernel, the read-back of the two counts) are timed with HIP
events on the engine's stream, median of 5 after a warm-up, for radius 1 .. 4; first-order byte estimates are printed next
to them (no time gate: there is no earlier code to compare with).

Then, recorded and not asserted anywhere: the angle between the end-to-end normals and the analytic normal of the height
field at the cloud's points, per radius, with the maps' own depth error beside it -- for the reference's algorithm (the
default mode) and for the extended mode.

    python tools/normals_time.py [n_views W H]
"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import torch  # noqa: E402

import amvs  # noqa: E402,F401
import cloud_normals_inputs as ni  # noqa: E402
from amvs.core.mvs_patchmatch import PatchMatchMVS  # noqa: E402
from amvs.synthetic import make_scene  # noqa: E402

n_views = int(sys.argv[1]) if len(sys.argv) > 1 else 16
W, H = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1008, 756)
REPS = 5

sc = make_scene(n_views, H, W, device="cuda")
images = [{"image": np.ascontiguousarray(c)} for c in sc.colors]
gt = np.stack(sc.depths)


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    out = fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), out


for extended in (False, True):
    pm = PatchMatchMVS(sc.camera, scale=1.0, patch_size=11, extended=extended)
    points, colors, maps = pm._reconstruct_maps(images, sc.poses)
    ids, src = pm._mesh_inputs(maps)
    poses = [(sc.poses[i].R, sc.poses[i].t) for i in ids]
    ptrs = src["device_ptrs"][:2]
    eng = pm._engine
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    n_pix = len(ids) * H * W
    depth = maps[1].depth.cpu().numpy().reshape(len(ids), H, W)
    conf = maps[1].confidence.cpu().numpy().reshape(len(ids), H, W)
    sel = conf >= pm.min_views
    rel = np.abs(depth[sel].astype(np.float64) - gt[ids][sel]) / gt[ids][sel]
    mode = "extended mode" if extended else "default mode"
    print(f"normals_time ({mode}): {len(ids)} maps {W}x{H}, patch 11, {int(sel.sum()):,} of {n_pix:,} pixels selected "
          f"(confidence >= {pm.min_views}), cloud {len(points):,} points; relative depth error of the selected pixels: "
          f"median {np.median(rel):.2e}, 90th percentile {np.percentile(rel, 90):.2e}")
    truth = ni.surface_normal(points[:, 0], points[:, 1])
    for radius in (1, 2, 3, 4):
        t_fit, t_all = [], []
        for rep in range(REPS + 1):
            ms, n_fit = timed(stream, lambda: eng.depth_normals(pm.K_scaled, poses, pm.min_views, radius, world=True,
                                                                      device_ptrs=ptrs, fetch=False))
            ms2, counts = timed(stream, lambda: eng.cloud_normals(pm.K_scaled, poses, pm.min_views, radius, device_ptrs=ptrs))
            if rep:                               # the first round loads the code object and grows the buffers
                t_fit.append(ms); t_all.append(ms2)
        normals, seen = eng.fetch_cloud_normals(len(points))
        has = np.any(normals != 0, axis=1)
        ang = np.degrees(np.arccos(np.clip((normals[has].astype(np.float64) * truth[has]).sum(1), -1.0, 1.0)))
        fit_bytes = n_pix * 20
        cloud_bytes = len(points) * 40 + int(seen.sum()) * 16
        print(f"  radius {radius}: fit median {np.median(t_fit):.3f} ms device (min {min(t_fit):.3f}), {n_fit:,} pixels with a normal; "
              f"whole amvs_cloud_normals median {np.median(t_all):.3f} ms (min {min(t_all):.3f}), {counts[1]:,} points with a "
              f"normal, mean {seen.mean():.2f} views a point")
        print(f"    first-order bytes (estimates): fit {fit_bytes / 1e6:.0f} MB (8 B read, 12 B written a pixel) = "
              f"{fit_bytes / 8e12 * 1e3:.3f} ms at 8 TB/s; cloud kernel {cloud_bytes / 1e6:.0f} MB (24 B read, 16 B written a "
              f"point, 16 B gathered a view that adds) = {cloud_bytes / 8e12 * 1e3:.3f} ms")
        print(f"    angle to the analytic normal: median {np.median(ang):.2f}, 90th percentile {np.percentile(ang, 90):.2f}, "
              f"99th {np.percentile(ang, 99):.2f} degrees")
    eng.set_stream(None)
    t0 = time.time()
    pm.reconstruct(images, sc.poses, with_normals=True)
    print(f"  reconstruct(with_normals=True) wall {time.time() - t0:.2f} s")
