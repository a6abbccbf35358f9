#!/usr/bin/env python3
"""Device time of one trial of the bundle adjustment (csrc/amvs_bundle.hip, include/amvs_bundle.h), split by kernel
family, on two synthetic problems: 32 cameras / 5 000 points and 128 cameras / 50 000 points, mean track length about 5,
0.5 px of noise, started a small step off the truth with camera 0 fixed (run on the GPU box).

The library writes the times itself: with AMVS_BA_TIMES=<file> in the environment amvs_ba_solve records a HIP event on
the context's stream behind each kernel family of a trial and appends the milliseconds between them to the file
(csrc/amvs_bundle.hip).  This script runs REPS + 1 calls of three trials each, drops the first call (warm-up: scratch
leases, code objects) and prints the median and the minimum of every family over the remaining trials, with the sizes
(n, N, pairs) and the wall time of the whole call, which holds the host's index lists and the uploads.

    python tools/bundle_time.py [--scipy] [--small-only]

--scipy runs scipy.optimize.least_squares (method trf, a 2-point Jacobian with the exact sparsity pattern over the terms
of tests/bundle_restatement.py, x_scale "jac" and scipy's default tolerances of 1e-8 as in its own bundle adjustment
example, the same fixed camera) on the same inputs on the host instead, for scale, and prints its wall time and final
cost.  No time is asserted."""
import os
import sys
import tempfile
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np  # noqa: E402

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import bundle_inputs as bi  # noqa: E402
import bundle_restatement as br  # noqa: E402

REPS, TRIALS = 5, 3
PROBLEMS = ((32, 5000), (128, 50000))


def problem(C, P):
    sc = bi.scene(C, P, seed=C, noise=0.5, mean_track=5)
    fixed = bi.fixed_mask(C, 0)
    R, t, X = bi.perturbed(sc, fixed != 0, rot=0.003, trans=0.01, pts=0.01, seed=C)
    return sc, fixed, R, t, X


def device(sc, fixed, R, t, X):
    import amvs
    path = os.path.join(tempfile.mkdtemp(), "ba_times.txt")
    os.environ["AMVS_BA_TIMES"] = path
    walls = []
    with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as eng:
        for rep in range(REPS + 1):
            if rep == 1:
                open(path, "w").close()                  # forget the warm-up call
            t0 = time.perf_counter()
            _, _, _, info = eng.ba_solve(R, t, X, sc["cam"], sc["pt"], sc["uv"], bi.K, fixed=fixed, max_trials=TRIALS)
            walls.append((time.perf_counter() - t0) * 1e3)
    del os.environ["AMVS_BA_TIMES"]
    rows = [line.split() for line in open(path)]
    sizes = dict(zip(rows[0][0:8:2], rows[0][1:8:2]))
    names = rows[0][8::2]
    ms = np.array([[float(v) for v in r[9::2]] for r in rows])
    print(f"  n = {sizes['n']}, N = {sizes['N']}, P = {sizes['P']}, pairs = {sizes['pairs']}; {len(rows)} trials; "
          f"cost {info['first_cost']:.4e} -> {info['cost']:.4e} in {info['trials']} trials, {info['kept']} kept")
    for j, name in enumerate(names):
        print(f"    {name:15s} median {np.median(ms[:, j]):9.4f} ms   min {ms[:, j].min():9.4f} ms")
    print(f"    {'a trial':15s} median {np.median(ms.sum(axis=1)):9.4f} ms   min {ms.sum(axis=1).min():9.4f} ms")
    print(f"    the whole call of {TRIALS} trials (lists, uploads, downloads): median {np.median(walls[1:]):.2f} ms wall")


def host_scipy(sc, fixed, R, t, X):
    from scipy.optimize import least_squares
    from scipy.sparse import coo_matrix
    q = br.Problem(sc["cam"], sc["pt"], sc["uv"], bi.K, sc["C"], sc["P"], fixed)
    free = np.flatnonzero(~q.fixed)
    nc = 6 * len(free)

    def state(x):
        Rn, tn = R.copy(), t.copy()
        for a, c in enumerate(free):
            Rn[c], tn[c] = br.pose_update(x[6 * a:6 * a + 6], R[c], t[c])
        return Rn, tn, X + x[nc:].reshape(-1, 3)

    def residuals(x):
        T = br.terms(q, *state(x))
        return np.concatenate([T["rx"], T["ry"]])

    k = np.arange(q.N)
    rows = np.concatenate([np.repeat(k, 3), np.repeat(k + q.N, 3)])
    cols = np.tile((nc + 3 * q.pt[:, None] + np.arange(3)).reshape(-1), 2)
    is_free = q.slot[q.cam] >= 0
    kf = k[is_free]
    rows_c = np.concatenate([np.repeat(kf, 6), np.repeat(kf + q.N, 6)])
    cols_c = np.tile((6 * q.slot[q.cam][is_free][:, None] + np.arange(6)).reshape(-1), 2)
    pattern = coo_matrix((np.ones(len(rows) + len(rows_c)), (np.concatenate([rows, rows_c]), np.concatenate([cols, cols_c]))),
                         shape=(2 * q.N, nc + 3 * q.P)).tocsr()
    t0 = time.perf_counter()
    out = least_squares(residuals, np.zeros(nc + 3 * q.P), jac_sparsity=pattern, method="trf", x_scale="jac")
    wall = time.perf_counter() - t0
    print(f"  scipy least_squares (trf, sparse 2-point Jacobian): {wall:.2f} s wall, {out.nfev} evaluations, cost "
          f"{2.0 * out.cost:.4e} (sum of squares), status {out.status}", flush=True)


if __name__ == "__main__":
    for C, P in PROBLEMS[:1] if "--small-only" in sys.argv else PROBLEMS:
        print(f"bundle_time: {C} cameras, {P} points", flush=True)
        args = problem(C, P)
        (host_scipy if "--scipy" in sys.argv else device)(*args)
