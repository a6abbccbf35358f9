#!/usr/bin/env python3
"""Device time of the lens undistortion (csrc/amvs_undistort.hip, include/amvs_lens.h) at 1920 x 1080 and at the CLI's
source size 4032 x 3024 (run on the GPU box), a sibling of tools/depth_filter_time.py.  The kernel alone is timed by the
library's own events (amvs_undistort_bgr8 records one before and one behind the launch; Engine.timing() returns them),
median of 5 after a warm-up; its upload and download are listed next to it.  The streaming ruler, in the same run: a
device-to-device copy of the same bytes (3 B read and 3 B written a pixel) between two torch tensors, timed by events
around the one copy, and the same bytes at the 6.29 TB/s of a float4 copy.  The kernel does about 35 float64 operations
and one division a pixel on top of its 6 B, so the ratio to the ruler is what is reported; no time is asserted.

Then reconstruct() end to end at the CLI operating point (bench.py cli_defaults: PatchMatchMVS(scale=0.25, 3 iterations,
min_views 3), 16 views of 4032 x 3024 processed at 1008 x 756), undistort off and on, median wall time of 5 calls after
the first.

    python tools/undistort_time.py [n_views]
"""
import contextlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import amvs  # noqa: E402
from amvs.synthetic import make_scene  # noqa: E402

n_views = int(sys.argv[1]) if len(sys.argv) > 1 else 16
REPS = 5
HBM = 6.29e12                     # bytes a second of a float4 copy
DIST = [-0.28, 0.09, 0.001, -0.0015, -0.01]


def lens_matrix(h, w):
    return np.array([[0.85 * w, 0.0, w / 2.0 + 3.3], [0.0, 0.845 * w, h / 2.0 - 2.9], [0.0, 0.0, 1.0]])


def copy_ms(n_bytes):
    src = torch.randint(0, 256, (n_bytes,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    times = []
    for rep in range(REPS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        if rep:
            times.append(a.elapsed_time(b))
    return float(np.median(times)), min(times)


print("undistort_time: the kernel alone (library events), its copies, and the streaming ruler of the same run")
with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as eng:
    for w, h in ((1920, 1080), (4032, 3024)):
        img = np.random.default_rng(w).integers(0, 256, (h, w, 3), dtype=np.uint8)
        K = lens_matrix(h, w)
        rows = []
        for rep in range(REPS + 1):
            _, n_outside = eng.undistort_bgr8(img, K, DIST)
            t = eng.timing()
            if rep:                               # the first round loads the code object and grows the staging blocks
                rows.append((t["sweep_ms"], t["init_ms"], t["confidence_ms"]))
        kernel, up, down = (float(np.median([r[k] for r in rows])) for k in range(3))
        ruler, ruler_min = copy_ms(3 * h * w)
        ideal = 6.0 * h * w / HBM * 1e3
        print(f"  {w} x {h} ({h * w / 1e6:.1f} MP, {n_outside:,} pixels outside): kernel median {kernel:.4f} ms (min "
              f"{min(r[0] for r in rows):.4f}); upload {up:.3f} ms, download {down:.3f} ms (pageable host memory)")
        print(f"    ruler: device-to-device copy of {3 * h * w / 1e6:.1f} MB median {ruler:.4f} ms (min {ruler_min:.4f}); "
              f"6 B a pixel at 6.29 TB/s {ideal:.4f} ms; kernel = {kernel / ruler:.2f} x the copy, {kernel / ideal:.2f} x the bound")

# end to end at the CLI operating point (bench.py run_cli_defaults)
scale, h, w = 0.25, 3024, 4032
H, W = int(h * scale), int(w * scale)
small = make_scene(n_views, H, W, seed=4321, device="cuda")
ids = sorted(small.poses)
images = [{"image": np.ascontiguousarray(np.repeat(np.repeat(small.colors[i], 4, axis=0), 4, axis=1))} for i in ids]
K = small.camera.K.copy()
K[:2] *= 1.0 / scale
cam = amvs.Camera(K=K, dist=np.asarray(DIST))
print(f"reconstruct end to end: PatchMatchMVS(scale=0.25, num_iterations=3, min_views=3), {n_views} views of {w} x {h} -> {W} x {H}")
for undistort in (False, True):
    with open(os.devnull, "w") as sink, contextlib.redirect_stdout(sink):
        pm = amvs.PatchMatchMVS(cam, scale=scale, num_iterations=3, min_views=3, seed=1, undistort=undistort)
        calls = []
        for _ in range(REPS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pts, cols = pm.reconstruct(images, small.poses)
            calls.append(time.perf_counter() - t0)
    print(f"  undistort={undistort}: median {np.median(calls[1:]):.4f} s (first call {calls[0]:.3f} s, the others "
          f"{', '.join(f'{c:.4f}' for c in calls[1:])}); {len(pts):,} points")
