#!/usr/bin/env python3
"""Times the track state of include/amvs_sfm.h and SfMPipeline on a planted scene (default: 128 views on a ring, 8 000
keypoints a view, about 1 000 match rows a pair over the pairs of SfMPipeline's schedule).

    python tools/sfm_time.py                 every step below, each in a child process under its own time limit
    python tools/sfm_time.py --step state    one step in this process

Steps:
  state     half the views are registered through the state (correspondences, register, triangulate each); then the wall
            time of Engine.sfm_scores, sfm_correspondences (median of 20 calls each) and sfm_triangulate (median over the
            views that follow), next to a first-order streaming bound: the rows a call walks times (8 B row + one 4 B
            owner gather, or two for triangulate) plus the per-keypoint arrays it sweeps, at 6.3 TB/s (the measured copy
            rate of the MI355X's HBM).  The times are those of the synchronising entry points, uploads of the segment list
            and read-backs included.
  python    the same three calls on the restatement of tests/sfm_state_restatement.py at the same point: the CPU yardstick
            for what the reference does in Python dictionaries.
  pipeline  SfMPipeline.reconstruct_from_features end to end with planted descriptors, split into descriptor matching and
            verification / RANSAC stages (initial pair, registrations) / track state / bundle adjustment.

Nothing is asserted; the numbers go into README.md and DESIGN.md section 17."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
K = np.array([[1200.0, 0.0, 960.0], [0.0, 1200.0, 540.0], [0.0, 0.0, 1.0]])
HBM_BYTES_PER_S = 6.3e12
LIMITS = {"state": 300, "python": 900, "pipeline": 900}


def scene(V, n_kp, rows_per_pair, seed=1):
    """V cameras on a ring around a ball of points; every view sees n_kp random tracks of T, T chosen so that two views share
    about rows_per_pair; pixels with 0.3 px of noise; the matches of SfMPipeline's pair schedule, one-to-one."""
    from amvs.core.sfm_pipeline import pair_schedule
    rng = np.random.default_rng(seed)
    T = int(n_kp * n_kp / rows_per_pair)
    X = rng.normal(0.0, 1.0, (T, 3))
    poses, kps, tracks = [], [], []
    for v in range(V):
        a = 2 * np.pi * v / V
        c = np.array([8.0 * np.sin(a), 0.3 * np.sin(3 * a), -8.0 * np.cos(a)])
        z = -c / np.linalg.norm(c)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        t = -R @ c
        tr = np.sort(rng.choice(T, n_kp, replace=False))
        pc = X[tr] @ R.T + t
        px = pc[:, :2] / pc[:, 2:3] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]] + rng.normal(0, 0.3, (n_kp, 2))
        poses.append((R, t))
        kps.append(px.astype(np.float32))
        tracks.append(tr)
    matches = {}
    for i, j in pair_schedule(V, min(12, V // 3 + 4)):
        _, ki, kj = np.intersect1d(tracks[i], tracks[j], return_indices=True)
        if len(ki) >= 15:
            matches[(i, j)] = np.stack([ki, kj], 1).astype(np.int32)
    return poses, kps, tracks, matches, T


def median_ms(fn, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def advance(backend, poses, order):
    """Registers the views of `order` through a backend with the methods of the restatement's State."""
    for v in order:
        kp, pid, _, _ = backend.correspondences(v)
        backend.register(v, poses[v][0], poses[v][1], kp, pid)
        backend.triangulate(v, K)


def step_state(args):
    import amvs

    class Device:
        """Engine.sfm_* under the names of the restatement's State."""

        def __init__(self, eng, kps, matches):
            self.eng = eng
            eng.sfm_begin(kps, matches)

        def register(self, view, R, t, kp=(), pid=()):
            return self.eng.sfm_register(view, R, t, kp, pid)

        def correspondences(self, view):
            return self.eng.sfm_correspondences(view)

        def triangulate(self, view, K):
            return self.eng.sfm_triangulate(view, K)

    poses, kps, _, matches, _ = scene(args.views, args.keypoints, args.rows)
    M, G, half = sum(len(m) for m in matches.values()), args.views * args.keypoints, args.views // 2
    with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as eng:
        t0 = time.perf_counter()
        dev = Device(eng, kps, matches)
        begin_ms = (time.perf_counter() - t0) * 1e3
        for v in (0, 1):
            dev.register(v, *poses[v])
        dev.triangulate(1, K)
        t0 = time.perf_counter()
        advance(dev, poses, range(2, half))
        advance_ms = (time.perf_counter() - t0) * 1e3
        reg = set(range(half))
        walked = sum(len(m) for (i, j), m in matches.items() if (i in reg) != (j in reg))
        walked_v = sum(len(m) for (i, j), m in matches.items() if (half in (i, j)) and ((i in reg) != (j in reg)))
        n_points = eng.sfm_counts()[0]
        scores_ms = median_ms(eng.sfm_scores, 20)
        corr_ms = median_ms(lambda: eng.sfm_correspondences(half), 20)
        tri, tri_rows = [], []
        for v in range(half, args.views):
            kp, pid, _, _ = dev.correspondences(v)
            dev.register(v, poses[v][0], poses[v][1], kp, pid)
            t0 = time.perf_counter()
            dev.triangulate(v, K)
            tri.append((time.perf_counter() - t0) * 1e3)
            tri_rows.append(sum(len(m) for (i, j), m in matches.items() if v in (i, j) and i <= v and j <= v))
        tri_ms, rows_tri = float(np.median(tri)), float(np.median(tri_rows))
        counts = eng.sfm_counts()
    bound = {"sfm_scores": (walked * (8 + 4 + 1) + G * (1 + 1 + 4)) / HBM_BYTES_PER_S * 1e3,
             "sfm_correspondences": (walked_v * (8 + 4 + 4) + args.keypoints * 40 + n_points * 4) / HBM_BYTES_PER_S * 1e3,
             "sfm_triangulate": (rows_tri * (8 + 4 + 4 + 16 + 4 + 24)) / HBM_BYTES_PER_S * 1e3}
    out = {"step": "state", "views": args.views, "keypoints": G, "pairs": len(matches), "rows": M, "begin_ms": begin_ms,
           "register_half_ms": advance_ms, "points": counts[0], "observations": counts[2],
           "rows_walked": {"sfm_scores": walked, "sfm_correspondences": walked_v, "sfm_triangulate": rows_tri},
           "ms": {"sfm_scores": scores_ms, "sfm_correspondences": corr_ms, "sfm_triangulate": tri_ms}, "bound_ms": bound}
    out["ratio"] = {k: out["ms"][k] / bound[k] for k in bound}
    print(json.dumps(out))


def step_python(args):
    import sfm_state_restatement as sr
    poses, kps, _, matches, _ = scene(args.views, args.keypoints, args.rows)
    half = args.views // 2
    t0 = time.perf_counter()
    state = sr.State(kps, sorted(matches.items()))
    for v in (0, 1):
        state.register(v, *poses[v])
    state.triangulate(1, K)
    advance(state, poses, range(2, half))
    setup_s = time.perf_counter() - t0
    ms = {"sfm_scores": median_ms(state.scores, 1), "sfm_correspondences": median_ms(lambda: state.correspondences(half), 1)}
    kp, pid, _, _ = state.correspondences(half)
    state.register(half, poses[half][0], poses[half][1], kp, pid)
    ms["sfm_triangulate"] = median_ms(lambda: state.triangulate(half, K), 1)
    print(json.dumps({"step": "python", "views": args.views, "register_half_s": setup_s, "ms": ms}))


def step_pipeline(args):
    import amvs
    from amvs import engine as engine_module
    from amvs.core import ImageFeatures, bundle, geometry, registration
    from amvs.core.camera import Camera
    poses, kps, tracks, _, T = scene(args.views, args.keypoints, args.rows)
    rng = np.random.default_rng(2)
    base = rng.integers(20, 236, (T, 128))
    feats = [ImageFeatures(kp, np.clip(base[tr] + rng.integers(-6, 7, (len(tr), 128)), 0, 255).astype(np.uint8), (1080, 1920))
             for kp, tr in zip(kps, tracks)]
    spent = {"ransac": 0.0, "state": 0.0, "bundle": 0.0}

    def timed(owner, name, bucket):
        fn = getattr(owner, name)

        def wrapper(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                spent[bucket] += time.perf_counter() - t0
        setattr(owner, name, wrapper)

    timed(geometry, "find_best_initial_pair", "ransac")
    timed(registration, "register_view", "ransac")
    timed(bundle, "bundle_adjust", "bundle")
    timed(bundle, "reprojection_errors", "bundle")
    for name in dir(engine_module.Engine):
        if name.startswith("sfm_"):
            timed(engine_module.Engine, name, "state")
    with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as eng:
        pipe = amvs.SfMPipeline(Camera(K), engine=eng)
        t0 = time.perf_counter()
        matches = pipe.match_image_pairs(feats, window_size=min(12, args.views // 3 + 4))
        match_s = time.perf_counter() - t0
        rec = {}
        t0 = time.perf_counter()
        points, _, found = pipe.reconstruct_from_features(feats, matches=matches, record=rec)
        total_s = time.perf_counter() - t0
    print(json.dumps({"step": "pipeline", "views": args.views, "pairs": len(matches), "rows": int(sum(len(m) for m in matches.values())),
                      "registered": len(found), "points": len(points), "bundles": len(rec["bundles"]), "matching_s": match_s,
                      "reconstruct_s": total_s, "ransac_s": spent["ransac"], "state_s": spent["state"], "bundle_s": spent["bundle"],
                      "other_s": total_s - sum(spent.values())}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(LIMITS))
    ap.add_argument("--views", type=int, default=128)
    ap.add_argument("--keypoints", type=int, default=8000)
    ap.add_argument("--rows", type=int, default=1000)
    args = ap.parse_args()
    if args.step:
        return {"state": step_state, "python": step_python, "pipeline": step_pipeline}[args.step](args)
    for step in ("state", "python", "pipeline"):
        cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--views", str(args.views),
               "--keypoints", str(args.keypoints), "--rows", str(args.rows)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print(f"step {step} ended with status {rc}; nothing more is started", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
