#!/usr/bin/env python3
"""Time of the feature extractor (csrc/amvs_clahe.hip, csrc/amvs_sift.hip, csrc/amvs_sift_keypoints.hip,
include/amvs_features.h) on one 1920 x 1080 view of synthetic.make_scene (run on the GPU box), a sibling of
tools/match_time.py: CLAHE, the Gaussian / difference-of-Gaussian scale space, and the whole extraction with the
reference's and with the dense mode's values (the keypoint stages are the difference to the scale space), each by events on the context's stream (amvs_set_stream to a torch stream, one event
before and one behind the call; the calls synchronise, so the upload of the 2 MB image is inside the number, and CLAHE's
download too), median of 5 after a warm-up, with the wall-clock figure beside it.

The scale space stands next to the bytes its passes must move and the time that traffic takes at the bandwidth bench.py
uses for its roofline (HBM_PEAK_GBS).  Per pixel of an octave: the row pass of a blur reads 4 and writes 4 bytes, the
column pass reads 4 and writes 4, and for the five upper images also reads the previous image and writes the difference
(8 more); the first image of octave 0 adds the upsampling (1/4 byte read, 4 written), of a later octave the halving (4
read at a quarter of the pixels, 4 written).  No time is asserted.

    python tools/sift_time.py
"""
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np  # noqa: E402

sys.path.insert(0, ".")
import torch  # noqa: E402

import amvs  # noqa: E402
from amvs.synthetic import make_scene  # noqa: E402

REPS = 5
HBM_PEAK_GBS = 8000.0        # bench.py's ruler


def scale_space_bytes(h, w):
    m = min(h, w)
    n_oct = ((m * m).bit_length() - 4) // 2 + 1
    total, hh, ww = 0.0, 2 * h, 2 * w
    for o in range(n_oct):
        px = hh * ww
        total += (0.25 + 4 + 16) * px if o == 0 else (4 + 4) * px
        total += 5 * 24 * px
        hh, ww = hh // 2, ww // 2
    return total, n_oct


def timed(stream, call):
    ev, wall = [], []
    for rep in range(REPS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        if rep:
            ev.append(a.elapsed_time(b))
            wall.append((time.perf_counter() - w0) * 1e3)
    return float(np.median(ev)), min(ev), float(np.median(wall))


H, W = 1080, 1920
gray = np.round(make_scene(2, H, W, seed=1).grays[0] * 255.0).astype(np.uint8)
print(f"sift_time: one {W} x {H} view, events on the context's stream, median of {REPS}")
stream = torch.cuda.Stream()
with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as eng:
    eng.set_stream(stream.cuda_stream)
    med, low, wall = timed(stream, lambda: eng.clahe(gray, 2.0, (8, 8)))
    print(f"  CLAHE (clip 2, grid 8 x 8), upload and download included: median {med:.3f} ms (min {low:.3f}, wall {wall:.3f})")
    med, low, wall = timed(stream, lambda: eng.sift_scale_space(gray, 1.6))
    moved, n_oct = scale_space_bytes(H, W)
    bound = moved / (HBM_PEAK_GBS * 1e9) * 1e3
    print(f"  scale space (sigma 1.6, {n_oct} octaves), upload included: median {med:.3f} ms (min {low:.3f}, wall "
          f"{wall:.3f}); its passes must move {moved / 1e9:.3f} GB = {bound:.3f} ms at {HBM_PEAK_GBS / 1e3:.1f} TB/s -> {med / bound:.1f} x "
          f"the traffic bound, {moved / med / 1e6:.0f} GB/s")
    med, low, wall = timed(stream, lambda: eng.sift_scale_space(None, 1.6))
    print(f"  scale space of the resident CLAHE result (no upload): median {med:.3f} ms (min {low:.3f}, wall {wall:.3f}) -> "
          f"{med / bound:.1f} x the traffic bound")
    for name, args in (("FeatureExtractor's values (10000 features, contrast 0.03, edge 15, sigma 1.6, CLAHE 2)",
                        (10000, 0.03, 15.0, 1.6, (2.0, (8, 8)))),
                       ("the dense mode's values (100000 features, contrast 0.01, edge 20, sigma 1.4, CLAHE 3)",
                        (100000, 0.01, 20.0, 1.4, (3.0, (8, 8))))):
        n = len(eng.sift_extract(gray, *args[:4], clahe=args[4])[0])
        med, low, wall = timed(stream, lambda: eng.sift_extract(gray, *args[:4], clahe=args[4]))
        print(f"  extract, {name}: {n} keypoints, CLAHE, scale space, keypoints, descriptors and their download: median {med:.3f} ms "
              f"(min {low:.3f}, wall {wall:.3f})")
    eng.set_stream(None)
