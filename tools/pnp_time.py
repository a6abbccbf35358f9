#!/usr/bin/env python3
"""Device time of the camera resection (csrc/amvs_pnp.hip, include/amvs_resection.h) on the planted scene of
tests/resection_inputs.py at m = 2 000 and 20 000 correspondences with 50 % outliers and 4096 hypotheses (run on the GPU
box), a sibling of tools/fmat_time.py: pnp_hypotheses (4096 hypotheses), pnp_score (those 4096 on all correspondences),
pnp_refine on the planted inliers and a whole pnp_ransac call, each by events on the context's stream (amvs_set_stream to
a torch stream, one event before and one behind the call), median of 5 after a warm-up.  The entry points take host
arrays and synchronise, so a call's time holds its uploads and downloads; the kernels alone are read from a kernel trace
of this script:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/pnp_time.py --no-cpu

The scoring kernel stands next to two yardsticks:
  float64 bound  32 float64 vector instructions per (wave, hypothesis) -- 17 v_mul_f64, 12 v_add_f64 and 3 v_cmp_*_f64,
                 counted from the gfx950 assembly of pnp_score_kernel (6 of them, the depth and its sign, run for every
                 wave; the other 26 only where a lane has a positive depth) -- at 4 cycles each on a SIMD (16 float64
                 lanes a clock), 1024 SIMDs at 2.4 GHz;
  CPU            tests/resection_restatement.py scoring the same hypotheses in NumPy.
No time is asserted.

    python tools/pnp_time.py [--no-cpu]
"""
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np  # noqa: E402

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import torch  # noqa: E402

import amvs  # noqa: E402
import resection_inputs as ri  # noqa: E402
import resection_restatement as rr  # noqa: E402

REPS = 5
HYPOTHESES = 4096
SIMDS, CLOCK, F64_PER_WAVE_HYPOTHESIS, F64_CYCLES = 1024, 2.4e9, 32, 4.0


def score_bound_ms(n, m):
    waves = -(-m // 64)
    return n * waves * F64_PER_WAVE_HYPOTHESIS * F64_CYCLES / (SIMDS * CLOCK) * 1e3


def timed(stream, call):
    ev = []
    for rep in range(REPS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = call()
        b.record(stream)
        b.synchronize()
        if rep:
            ev.append(a.elapsed_time(b))
    return float(np.median(ev)), min(ev), out


print("pnp_time: calls by events on the context's stream (uploads and downloads inside), median of 5 after a warm-up")
stream = torch.cuda.Stream()
K = ri.K
with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as eng:
    eng.set_stream(stream.cuda_stream)
    for m in (2000, 20000):
        X, x, planted = ri.scene(m, 0.5)
        hyp, hyp_min, (_, R, t) = timed(stream, lambda: eng.pnp_hypotheses(X, x, K, seed=1234, first=0, count=HYPOTHESES))
        sc, sc_min, counts = timed(stream, lambda: eng.pnp_score(R, t, X, x, K, threshold=2.0))
        ref, ref_min, (_, _, steps, cost) = timed(stream, lambda: eng.pnp_refine(X, x, K, *ri.start_pose(), planted))
        ran, ran_min, (Rr, tr, mask, info) = timed(stream, lambda: eng.pnp_ransac(X, x, K, threshold=2.0, max_hypotheses=HYPOTHESES,
                                                                               seed=1234))
        bound = score_bound_ms(HYPOTHESES, m)
        kept = (mask & planted).sum() / planted.sum()
        rot = ri.rotation_error_deg(Rr, ri.true_pose()[0])
        print(f"  m = {m:,}, {HYPOTHESES} hypotheses: pnp_hypotheses {hyp:.3f} ms (min {hyp_min:.3f}); pnp_score {sc:.3f} ms "
              f"(min {sc_min:.3f}), float64 bound of its kernel {bound:.4f} ms; pnp_refine of {planted.sum()} correspondences "
              f"{ref:.3f} ms (min {ref_min:.3f}, {steps} steps); pnp_ransac {ran:.3f} ms (min {ran_min:.3f}): {info['hypotheses']} "
              f"hypotheses run, best keeps {info['best_count']}, {info['n_inliers']} inliers, {100 * kept:.1f} % of the planted "
              f"ones, rotation error {rot:.4f} degrees")
        if "--no-cpu" not in sys.argv:
            t0 = time.perf_counter()
            ref_counts = rr.score(R.reshape(-1, 9), t, X, x, K, 2.0)
            cpu = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(ref_counts, counts)
            print(f"    CPU yardstick (the NumPy restatement scoring the same {HYPOTHESES} hypotheses): {cpu:.0f} ms = "
                  f"{cpu / sc:.0f} x the pnp_score call, the same counts")
    eng.set_stream(None)
