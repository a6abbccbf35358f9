#!/usr/bin/env python3
"""Device time of the cross-view depth-map filter (csrc/amvs_depth_filter.hip) at the CLI operating point (run on the GPU
box), a sibling of tools/normals_time.py: 16 maps of 1008 x 756, the extended mode's maps resident on the device.  The whole
amvs_depth_filter call with device inputs and device outputs (the upload of the poses and the neighbour rows, the kernel,
the read-back of the two counts) is timed with HIP events on the engine's stream, median of 5 after a warm-up, for every
other map as neighbour (15) and for the 4 nearest camera centres, with and without refinement.  A first-order bound is
printed next to each time and the measured multiple of it (no time gate: there is no earlier code to compare with):

    bytes       8 B read and 8 B written a pixel, and 8 B gathered a neighbour visit of a valid pixel
    arithmetic  about 190 float64 instructions a neighbour visit that runs to the end -- two reprojections of 51, two
                projections of 15, four divisions of about 12 each, the rounding and the two tests -- none of them fused
                (contraction is off), against the vector FP64 issue rate: half the 78.6 TFLOP/s of the data sheet, which
                counts a fused multiply-add as two.  Twice: for the valid pixels alone, and for every lane of a wave that
                holds a valid pixel -- a wave issues an instruction once for its 64 lanes however many of them are active,
                so that is what sparse valid pixels cost

Then, recorded and not asserted anywhere, end to end on the extended mode's maps: the share of pixels kept, the relative
depth error before and after, and the angle between reconstruct(with_normals=True)'s normals and the analytic normal of the
height field without and with the filter.

    python tools/depth_filter_time.py [n_views W H]
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
from amvs.core.utils import nearest_map_neighbours  # noqa: E402
from amvs.synthetic import make_scene  # noqa: E402

n_views = int(sys.argv[1]) if len(sys.argv) > 1 else 16
W, H = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1008, 756)
REPS = 5
FP64_ISSUE = 78.6e12 / 2          # unfused float64 instructions a second (estimate from the data sheet)
HBM = 6.29e12                     # bytes a second of a float4 copy

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


def angles(points, normals):
    truth = ni.surface_normal(points[:, 0], points[:, 1])
    has = np.any(normals != 0, axis=1)
    return np.degrees(np.arccos(np.clip((normals[has].astype(np.float64) * truth[has]).sum(1), -1.0, 1.0))), int(has.sum())


pm = PatchMatchMVS(sc.camera, scale=1.0, patch_size=11, extended=True)
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
# lanes of the waves that hold a valid pixel: a wave is 64 consecutive pixels of a map (H * W is a multiple of 64 or the
# last wave of a map is ragged; both are counted as 64)
flat = sel.reshape(len(ids), -1)
pad = (-flat.shape[1]) % 64
wave_lanes = 64 * int(np.pad(flat, ((0, 0), (0, pad))).reshape(len(ids), -1, 64).any(axis=2).sum())
rel_err = np.abs(depth.astype(np.float64) - gt[ids]) / gt[ids]
print(f"depth_filter_time (extended mode): {len(ids)} maps {W}x{H}, patch 11, {int(sel.sum()):,} of {n_pix:,} pixels valid "
      f"(confidence >= {pm.min_views}); relative depth error of the valid pixels: median {np.median(rel_err[sel]):.2e}, 90th "
      f"percentile {np.percentile(rel_err[sel], 90):.2e}, RMS {np.sqrt(np.mean(rel_err[sel] ** 2)):.2e}")
od = torch.empty((len(ids), H * W), dtype=torch.float32, device="cuda")
oc = torch.empty_like(od)
torch.cuda.synchronize()
centers = [sc.poses[i].center for i in ids]
for label, k in (("every other map", None), ("4 nearest", 4)):
    rows = nearest_map_neighbours(centers, k)
    n_nbr = len(ids) - 1 if rows is None else rows.shape[1]
    for refine in (False, True):
        times = []
        for rep in range(REPS + 1):
            ms, counts = timed(stream, lambda: eng.depth_filter(pm.K_scaled, poses, pm.min_views, 1.0, 0.01, 2, refine, neighbours=rows,
                                                                device_ptrs=ptrs, out_ptrs=(od.data_ptr(), oc.data_ptr())))
            if rep:                               # the first round loads the code object and grows the scratch
                times.append(ms)
        visits = int(oc.sum().item())             # neighbour visits that ran to the end and agreed (a lower bound of those that ran)
        t_bytes = (n_pix * 16 + counts[0] * n_nbr * 8) / HBM * 1e3
        t_flops = counts[0] * n_nbr * 190 / FP64_ISSUE * 1e3
        t_waves = wave_lanes * n_nbr * 190 / FP64_ISSUE * 1e3
        bound = max(t_bytes, t_flops)
        med = float(np.median(times))
        print(f"  {label} ({n_nbr}), refine {int(refine)}: median {med:.3f} ms device (min {min(times):.3f}); {counts[1]:,} of "
              f"{counts[0]:,} valid pixels kept, {visits:,} agreeing visits")
        print(f"    first-order bound (estimate): bytes {t_bytes:.3f} ms at 6.29 TB/s, float64 issue {t_flops:.3f} ms at "
              f"{FP64_ISSUE / 1e12:.1f} T instructions/s if every visit of a valid pixel ran to the end; measured = "
              f"{med / bound:.2f} x the larger")
        print(f"    the same issue count for all 64 lanes of the {wave_lanes // 64:,} waves that hold a valid pixel ({wave_lanes:,} of "
              f"{n_pix:,} lanes): {t_waves:.3f} ms; measured = {med / max(t_waves, t_bytes):.2f} x")
eng.set_stream(None)

# end to end, recorded only
fd, fc, counts = eng.depth_filter(pm.K_scaled, poses, pm.min_views, 1.0, 0.01, 2, True, device_ptrs=ptrs)
kept = fd > 0
fd_err = np.abs(fd.astype(np.float64) - gt[ids]) / gt[ids]
print(f"end to end (max_px 1, max_rel 0.01, min_consistent 2, every other map): {counts[1]:,} of {counts[0]:,} valid pixels kept "
      f"({counts[1] / max(counts[0], 1):.3f})")
print(f"  relative depth error of the kept pixels before: median {np.median(rel_err[kept]):.2e}, 90th percentile "
      f"{np.percentile(rel_err[kept], 90):.2e}, RMS {np.sqrt(np.mean(rel_err[kept] ** 2)):.2e}; after: median "
      f"{np.median(fd_err[kept]):.2e}, 90th percentile {np.percentile(fd_err[kept], 90):.2e}, RMS {np.sqrt(np.mean(fd_err[kept] ** 2)):.2e}")
for filt in (False, True):
    t0 = time.time()
    pts, cols, nrm = pm.reconstruct(images, sc.poses, with_normals=True, geometric_filter=filt)
    wall = time.time() - t0
    ang, n_has = angles(pts, nrm)
    print(f"  reconstruct(with_normals=True, geometric_filter={filt}): {len(pts):,} points, {n_has:,} with a normal, angle to the "
          f"analytic normal median {np.median(ang):.2f}, 90th percentile {np.percentile(ang, 90):.2f}, 99th {np.percentile(ang, 99):.2f} "
          f"degrees; wall {wall:.2f} s")
