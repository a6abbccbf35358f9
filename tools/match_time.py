#!/usr/bin/env python3
"""Device time of the exact descriptor search (csrc/amvs_match.hip, include/amvs_match.h) at 10 k x 10 k and 100 k x
100 k random uint8 descriptors, and of reconstruct_from_features end to end (run on the GPU box), a sibling of
tools/undistort_time.py.  knn2 is timed by events on the context's stream (amvs_set_stream to a torch stream, one event
before and one behind the call; the call itself synchronises, so the download of the 16 bytes a query is inside the
number and listed beside it from a second, wall-clock figure), median of 5 after a warm-up.

Each time stands next to two bounds:
  matrix   2 * n_q * n_t * 128 integer operations at the int8 peak, 2 x the ~2.5 POP/s of bf16 (MI355X_MICROARCH);
  epilogue 3 vector instructions per output (v_lshl_add_u32, v_med3_u32, v_max_u32: read from the ISA), a wave64
           instruction taking a SIMD 2 cycles when other waves fill in (4 for a wave alone), 1024 SIMDs at 2.4 GHz.
The ISA counts predict the matrix bound, narrowly: per 32 x 32 tile of a wave 4 matrix instructions of 32 cycles (128)
against 48 vector instructions of 2 cycles (96); a wave alone, paying 4 cycles each, would be epilogue-bound (192).

The CPU yardstick is the same search as float64 BLAS + argpartition in NumPy on 16 threads (10 k x 10 k measured, the
100 k figure extrapolated by the pair count).  No time is asserted.

    python tools/match_time.py [--skip-100k]
"""
import contextlib
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np  # noqa: E402

sys.path.insert(0, ".")
import torch  # noqa: E402

import amvs  # noqa: E402

REPS = 5
I8_PEAK = 5.0e15
SIMDS, CLOCK, VALU_PER_OUTPUT, VALU_CYCLES = 1024, 2.4e9, 3, 2.0


def bounds_ms(n_q, n_t):
    matrix = 2.0 * n_q * n_t * 128 / I8_PEAK * 1e3
    epilogue = (n_q * n_t / 64.0) * VALU_PER_OUTPUT * VALU_CYCLES / (SIMDS * CLOCK) * 1e3
    return matrix, epilogue


def cpu_knn2_s(q, t):
    t0 = time.perf_counter()
    a, b = q.astype(np.float64), t.astype(np.float64)
    bn = (b * b).sum(1)
    for r0 in range(0, len(a), 2048):
        s = bn[None, :] - 2.0 * (a[r0:r0 + 2048] @ b.T)
        part = np.argpartition(s, 2, axis=1)[:, :2]
        np.take_along_axis(s, part, 1)
    return time.perf_counter() - t0


print("match_time: knn2 by events on the context's stream, next to the matrix and the epilogue bound")
sizes = [10000] if "--skip-100k" in sys.argv else [10000, 100000]
stream = torch.cuda.Stream()
with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as eng:
    eng.set_stream(stream.cuda_stream)
    for n in sizes:
        rng = np.random.default_rng(n)
        q = rng.integers(0, 256, (n, 128), dtype=np.uint8)
        t = rng.integers(0, 256, (n, 128), dtype=np.uint8)
        t0 = time.perf_counter()
        eng.set_descriptors(0, q)
        eng.set_descriptors(1, t)
        upload = (time.perf_counter() - t0) * 1e3
        ev, wall = [], []
        for rep in range(REPS + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w0 = time.perf_counter()
            a.record(stream)
            eng.knn2(0, 1)
            b.record(stream)
            b.synchronize()
            if rep:
                ev.append(a.elapsed_time(b))
                wall.append((time.perf_counter() - w0) * 1e3)
        matrix, epilogue = bounds_ms(n, n)
        med = float(np.median(ev))
        print(f"  {n:,} x {n:,}: knn2 median {med:.3f} ms (min {min(ev):.3f}, wall {np.median(wall):.3f}); upload of both sets "
              f"{upload:.2f} ms; matrix bound {matrix:.3f} ms, epilogue bound {epilogue:.3f} ms -> {med / matrix:.2f} x the "
              f"matrix bound, {2.0 * n * n * 128 / med / 1e9:.1f} TOP/s")
        if n == 10000:
            cpu = cpu_knn2_s(q, t)
            print(f"    CPU yardstick (float64 BLAS + argpartition, {os.environ['OMP_NUM_THREADS']} threads): {cpu * 1e3:.0f} ms at "
                  f"10 k x 10 k = {cpu * 1e3 / med:.0f} x the device; {cpu * 100:.1f} s extrapolated to 100 k x 100 k")
    eng.set_stream(None)

# reconstruct_from_features end to end: 16 views on an arc, 20 k features each (a quarter matched along the arc), window 8
sys.path.insert(0, "tests")
import match_inputs as mi  # noqa: E402

cam, poses, features, images, planted = mi.dense_scene(n_views=16, n_points=5000, n_distractors=15000, H=756, W=1008, seed=3)
from amvs.core.dense import DenseReconstructor, camera_pairs  # noqa: E402

rec = DenseReconstructor(cam)
calls = []
for _ in range(3):
    with open(os.devnull, "w") as sink, contextlib.redirect_stdout(sink):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pts, cols = rec.reconstruct_from_features(features, images, poses, window=8)
        calls.append(time.perf_counter() - t0)
n_pairs = len(camera_pairs(16, 8))
print(f"reconstruct_from_features: 16 views x 20,000 features, window 8 ({n_pairs} pairs): median {np.median(calls[1:]):.3f} s "
      f"(first call {calls[0]:.3f} s); {len(pts):,} points")
