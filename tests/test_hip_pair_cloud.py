"""The pair triangulation, the accumulating cloud, the bounds, the grid voxel de-duplication and the chained dense-SIFT
reconstruction on the device (csrc/amvs_triangulate.hip, the grid key of csrc/amvs_fusion.hip, core/dense.py) against
the restatement of tests/match_restatement.py on the inputs of tests/match_inputs.py.

The device's float64 square root is compared with NumPy's on 10^6 seeded values first; it is correctly rounded, so the
accepted points and every accept / reject decision are compared bit for bit, with no candidate left out."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_inputs as mi  # noqa: E402
import match_restatement as mr  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCK = 256                      # lanes per workgroup of the triangulation kernel


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint64), b.view(np.uint64)) if a.dtype == np.float64 else np.array_equal(a, b)


@pytest.fixture(scope="module")
def eng():
    import amvs
    with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as e:
        yield e


_TRI = {}


def restated(beta):
    if beta not in _TRI:
        c = mi.triangulation_case(beta)
        _TRI[beta] = (c,) + mr.triangulate(c["K"], c["R1"], c["t1"], c["R2"], c["t2"], c["pts1"], c["pts2"])
    return _TRI[beta]


def run_pair(eng, c, rows):
    return eng.pair_triangulate(c["K"], c["R1"], c["t1"], c["R2"], c["t2"], c["pts1"][rows], c["pts2"][rows], c["rgb"][rows])


def test_device_square_root_is_correctly_rounded(eng):
    rng = np.random.default_rng(99)
    v = np.concatenate([rng.uniform(0.0, 4.0, 400000), np.exp(rng.uniform(-700.0, 700.0, 400000)),
                        1.0 + rng.uniform(0.0, 1e-12, 100000), rng.uniform(0.0, 1e-300, 99996), [0.0, 1.0, 2.0, np.inf]])
    assert len(v) == 10 ** 6
    assert same(eng.selftest_sqrt(v), np.sqrt(v))


@pytest.mark.parametrize("beta", mi.BASELINES_DEG)
def test_triangulation_bit_for_bit_every_candidate(eng, beta):
    c, X, keep, margin = restated(beta)
    every = np.arange(len(keep))
    eng.pair_cloud_begin()
    assert run_pair(eng, c, every) == int(keep.sum())
    # the decisions, one candidate at a time, are the restatement's: a second pass appends candidate by candidate
    total = eng.pair_cloud_finish()
    pts, rgb = eng.fetch_cloud(total)
    assert same(pts, X[keep]) and same(rgb, c["rgb"][keep])
    for name, (row, expect) in c["planted"].items():
        eng.pair_cloud_begin()
        assert run_pair(eng, c, [row]) == int(expect), name
        eng.pair_cloud_finish()


def test_accumulation_in_candidate_order_and_the_block_edges(eng):
    c, X, keep, _ = restated(10.0)
    n = len(keep)
    assert n > BLOCK + 1
    parts = [np.arange(0), np.arange(1), np.arange(1, BLOCK + 2), np.arange(BLOCK + 2, n), np.arange(0)]   # m = 0, 1, 257, ...
    eng.pair_cloud_begin()
    counts = [run_pair(eng, c, rows) for rows in parts]
    assert counts == [int(keep[rows].sum()) for rows in parts] and counts[0] == 0
    total = eng.pair_cloud_finish()
    assert total == int(keep.sum())
    pts, rgb = eng.fetch_cloud(total)
    assert same(pts, X[keep]) and same(rgb, c["rgb"][keep])
    # the finished cloud is the resident one: the neighbour statistic runs on it where it lies
    stat = eng.cloud_knn_mean_distance(total, 20)
    assert same(stat, eng.knn_mean_distance(pts, 20))
    # several pairs in one cloud, in call order
    c2, X2, keep2, _ = restated(40.0)
    eng.pair_cloud_begin()
    run_pair(eng, c, np.arange(n))
    run_pair(eng, c2, np.arange(len(keep2)))
    total = eng.pair_cloud_finish()
    pts, rgb = eng.fetch_cloud(total)
    assert same(pts, np.vstack([X[keep], X2[keep2]])) and same(rgb, np.vstack([c["rgb"][keep], c2["rgb"][keep2]]))


def test_triangulate_and_finish_need_a_begin(eng):
    import amvs
    c, _, _, _ = restated(10.0)
    eng.pair_cloud_begin()
    eng.pair_cloud_finish()
    with pytest.raises(amvs.AmvsError):
        run_pair(eng, c, [0])
    with pytest.raises(amvs.AmvsError):
        eng.pair_cloud_finish()


@pytest.mark.parametrize("name", sorted(mi.grid_cases()))
def test_bounds_and_grid_bit_for_bit(eng, name):
    p, col, keep, origin, voxel = mi.grid_cases()[name]
    eng.cloud_set(p, col)
    mn, mx = eng.cloud_bounds(keep)
    rmn, rmx = mr.bounds(p, keep)
    assert same(mn, rmn) and same(mx, rmx)
    m = eng.cloud_voxel_downsample_grid(origin, voxel, keep)
    want = mr.voxel_grid(p, col, origin, voxel, keep)
    got = eng.fetch_cloud(m)
    assert m == len(want[0]) and same(got[0], want[0]) and same(got[1], want[1])


def test_grid_parameter_errors_leave_the_cloud(eng):
    import amvs
    p, col, keep, origin, voxel = mi.grid_cases()["one_voxel"]
    eng.cloud_set(p, col)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(amvs.AmvsError):
            eng.cloud_voxel_downsample_grid(origin, bad)
    with pytest.raises(amvs.AmvsError):
        eng.cloud_voxel_downsample_grid([0.0, float("nan"), 0.0], voxel)
    with pytest.raises(amvs.AmvsError):
        eng.cloud_bounds(np.zeros(len(p), bool))                   # no kept point
    with pytest.raises(amvs.AmvsError):
        eng.cloud_voxel_downsample_grid(origin, 1e-300)            # more than 2^62 voxels
    assert same(eng.fetch_cloud(len(p))[0], p)
    # a kept point that is not finite is refused; masked out, it is nobody's business
    bad = p.copy()
    bad[7, 1] = float("nan")
    eng.cloud_set(bad, col)
    with pytest.raises(amvs.AmvsError):
        eng.cloud_voxel_downsample_grid(origin, voxel)
    keep = np.ones(len(p), bool)
    keep[7] = False
    assert eng.cloud_voxel_downsample_grid(origin, voxel, keep) == 1


def test_reconstruct_from_features_equals_the_chained_restatement(eng, capsys):
    from amvs.core import DenseReconstructor
    cam, poses, features, images, planted = mi.dense_scene()
    rp = {i: (p.R, np.ravel(p.t)) for i, p in poses.items()}
    want = mr.reconstruct(cam.K, features, images, rp, window=20, knn_stat=lambda pts, k: eng.knn_mean_distance(pts, k))
    rec = DenseReconstructor(cam)
    got = rec.reconstruct_from_features(features, images, poses, window=20)
    out = capsys.readouterr().out
    assert "DENSE RECONSTRUCTION (HIGH DENSITY MODE)" in out and "Matching 15 camera pairs..." in out
    assert "Statistical filter: kept" in out and "Voxel grid: downsampled to" in out and "Final filtered points:" in out
    assert len(want[0]) > 600
    assert same(got[0], want[0]) and same(got[1], want[1])
    d = np.sqrt(((got[0][:, None, :] - planted[None, :, :]) ** 2).sum(2)).min(1)
    assert (d < 0.01 * 5.0).mean() >= 0.95
    # float32 descriptors holding the same integers, keypoint objects instead of an array, the cross check
    class Kp:
        def __init__(self, xy):
            self.pt = (float(xy[0]), float(xy[1]))
    f2 = {i: {"descriptors": f["descriptors"].astype(np.float32), "keypoints": [Kp(xy) for xy in f["points"]]}
          for i, f in features.items()}
    again = rec.reconstruct_from_features(f2, images, poses, window=20)
    assert same(again[0], want[0]) and same(again[1], want[1])
    want_x = mr.reconstruct(cam.K, features, images, rp, window=1, cross_check=True, ratio=0.8,
                            knn_stat=lambda pts, k: eng.knn_mean_distance(pts, k))
    got_x = rec.reconstruct_from_features(features, images, poses, window=1, ratio=0.8, cross_check=True)
    assert len(want_x[0]) > 100 and same(got_x[0], want_x[0]) and same(got_x[1], want_x[1])
    with pytest.raises(ValueError, match="with_normals"):
        rec.reconstruct_from_features(features, images, poses, with_normals=True)
    assert rec.reconstruct_from_features({}, images, poses)[0].size == 0
