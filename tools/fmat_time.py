#!/usr/bin/env python3
"""Device time of the fundamental-matrix RANSAC (csrc/amvs_fmat.hip, include/amvs_epipolar.h) on the standard scene of
tests/epipolar_inputs.py at m = 2 000 and 20 000 matches with 50 % outliers and 4096 hypotheses (run on the GPU box), a
sibling of tools/match_time.py: fmat_hypotheses (4096 hypotheses), fmat_score (those 4096 on all matches) and a whole
fundamental_ransac call, each by events on the context's stream (amvs_set_stream to a torch stream, one event before and
one behind the call), median of 5 after a warm-up.  The entry points take host arrays and synchronise, so a call's time
holds its uploads and downloads; the kernels alone are read from a kernel trace of this script:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/fmat_time.py --no-cpu

The scoring kernel stands next to two yardsticks:
  float64 bound  38 float64 vector instructions per (wave, hypothesis) -- 19 v_mul_f64, 14 v_add_f64 and 5 v_cmp_*_f64,
                 counted from the gfx950 assembly of fmat_score_kernel -- at 4 cycles each on a SIMD (16 float64 lanes a
                 clock), 1024 SIMDs at 2.4 GHz;
  CPU            tests/epipolar_restatement.py scoring the same hypotheses in NumPy.
No time is asserted.

    python tools/fmat_time.py [--no-cpu]
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
import epipolar_inputs as ei  # noqa: E402
import epipolar_restatement as er  # noqa: E402

REPS = 5
HYPOTHESES = 4096
SIMDS, CLOCK, F64_PER_WAVE_HYPOTHESIS, F64_CYCLES = 1024, 2.4e9, 38, 4.0


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


print("fmat_time: calls by events on the context's stream (uploads and downloads inside), median of 5 after a warm-up")
stream = torch.cuda.Stream()
with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as eng:
    eng.set_stream(stream.cuda_stream)
    for m in (2000, 20000):
        p1, p2, planted = ei.scene(m, 0.5)
        hyp, hyp_min, (_, F) = timed(stream, lambda: eng.fmat_hypotheses(p1, p2, seed=1234, first=0, count=HYPOTHESES))
        sc, sc_min, counts = timed(stream, lambda: eng.fmat_score(F, p1, p2, threshold=2.0))
        ran, ran_min, (Fr, mask, info) = timed(stream, lambda: eng.fundamental_ransac(p1, p2, max_hypotheses=HYPOTHESES, seed=1234))
        bound = score_bound_ms(HYPOTHESES, m)
        kept = (mask & planted).sum() / planted.sum()
        print(f"  m = {m:,}, {HYPOTHESES} hypotheses: fmat_hypotheses {hyp:.3f} ms (min {hyp_min:.3f}); fmat_score {sc:.3f} ms "
              f"(min {sc_min:.3f}), float64 bound of its kernel {bound:.4f} ms; fundamental_ransac {ran:.3f} ms (min {ran_min:.3f}): "
              f"{info['hypotheses']} hypotheses run, best keeps {info['best_count']}, {info['n_inliers']} inliers, "
              f"{100 * kept:.1f} % of the planted ones")
        if "--no-cpu" not in sys.argv:
            t0 = time.perf_counter()
            ref = er.score(F.reshape(-1, 9), p1, p2, 2.0)
            cpu = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(ref, counts)
            print(f"    CPU yardstick (the NumPy restatement scoring the same {HYPOTHESES} hypotheses): {cpu:.0f} ms = "
                  f"{cpu / sc:.0f} x the fmat_score call, the same counts")
    eng.set_stream(None)
