#!/usr/bin/env python3
"""Device time of the two-view start (csrc/amvs_twoview.hip, include/amvs_twoview.h) on the planted pair of
tests/twoview_inputs.py at m = 2 000 and 20 000 matches with 0.5 px of noise and 30 % outliers (run on the GPU box), a
sibling of tools/pnp_time.py: twoview_score with the 4 candidates of the exact F, a whole twoview_pose call and
twoview_triangulate, each by events on the context's stream (amvs_set_stream to a torch stream, one event before and
one behind the call), median of 5 after a warm-up.  The entry points take host arrays and synchronise, so a call's time
holds its uploads and downloads; the kernels alone are read from a kernel trace of this script:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/twoview_time.py --no-cpu

Next to each stands the NumPy restatement (tests/twoview_restatement.py) on the same inputs, whose results must be the
same.  No time is asserted.

    python tools/twoview_time.py [--no-cpu]
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
import twoview_inputs as ti  # noqa: E402
import twoview_restatement as tr  # noqa: E402

REPS = 5


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


def cpu_ms(call):
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


print("twoview_time: calls by events on the context's stream (uploads and downloads inside), median of 5 after a warm-up")
stream = torch.cuda.Stream()
K, I3, Z3 = ti.K, np.eye(3), np.zeros(3)
R0, t0 = ti.true_pose()
F = ti.fundamental(R0, t0)
with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as eng:
    eng.set_stream(stream.cuda_stream)
    R2, tt, _ = eng.twoview_decompose(F, K)
    Rc, tc = tr.candidates(R2, tt)
    for m in (2000, 20000):
        _, p1, p2, planted = ti.scene(m, noise=0.5, outlier_fraction=0.3, seed=m)
        sc, sc_min, counts = timed(stream, lambda: eng.twoview_score(Rc, tc, p1, p2, K))
        po, po_min, (R, t, mask, info) = timed(stream, lambda: eng.twoview_pose(F, K, p1, p2))
        tri, tri_min, (X, valid, cs) = timed(stream, lambda: eng.twoview_triangulate(K, I3, Z3, R, t, p1, p2))
        print(f"  m = {m:,}: twoview_score of 4 poses {sc:.3f} ms (min {sc_min:.3f}), counts {counts.tolist()}; twoview_pose {po:.3f} ms "
              f"(min {po_min:.3f}), {info['n_front']} in front; twoview_triangulate {tri:.3f} ms (min {tri_min:.3f}), {int(valid.sum())} "
              f"valid of which {int((valid & planted).sum())} planted inliers")
        if "--no-cpu" not in sys.argv:
            c_sc, r_counts = cpu_ms(lambda: tr.score(Rc, tc, p1, p2, K))
            c_po, r_pose = cpu_ms(lambda: tr.pose(F, K, p1, p2))
            c_tri, r_tri = cpu_ms(lambda: tr.triangulate(K, I3, Z3, R, t, p1, p2))
            assert np.array_equal(r_counts, counts) and np.array_equal(r_pose[2], mask) and np.array_equal(r_tri[1], valid)
            print(f"    NumPy restatement on the same inputs, the same results: score {c_sc:.0f} ms = {c_sc / sc:.0f} x the call, pose "
                  f"{c_po:.0f} ms = {c_po / po:.0f} x, triangulate {c_tri:.0f} ms = {c_tri / tri:.0f} x")
    eng.set_stream(None)
