"""The point-cloud stage on the restatement alone (tests/cloud_restatement.py; no GPU): that it gives the clouds the
REFERENCE produced (g10, g12) bit for bit, that the package's host path gives the same on every case of the family the
GPU comparison runs on (tests/cloud_inputs.py, test_hip_cloud.py), that the family tells every named near-miss from
the definition, and that it reaches the edges it is meant to reach."""
import contextlib
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_inputs as ci  # noqa: E402
import cloud_restatement as cr  # noqa: E402
from conftest import GoldenScene, load_golden  # noqa: E402

import amvs  # noqa: E402
from amvs.core.dense_stereo import DenseStereoReconstructor  # noqa: E402
from amvs.core.mvs_patchmatch import DepthNormalMap, PatchMatchMVS  # noqa: E402


def same(a, b):
    """Bit for bit: points as uint64, colours element for element."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == np.float64 and b.dtype == np.float64:
        return np.array_equal(a.view(np.uint64), b.view(np.uint64))
    return np.array_equal(a, b)


def same_cloud(got, want):
    return same(got[0], want[0]) and same(np.asarray(got[1], np.uint8), np.asarray(want[1], np.uint8))


def all_fusion_cases():
    return [c for H, W in ci.SIZES for c in ci.fusion_cases(H, W)] + list(ci.stride_cases("fuse"))


def all_stereo_cases():
    return [c for H, W in ci.SIZES for c in ci.stereo_cases(H, W)] + list(ci.stride_cases("stereo"))


@functools.lru_cache(maxsize=None)
def _fused(name):
    case = next(c for c in all_fusion_cases() if c.name == name)
    raw = cr.fuse_filter(case, do_filter=False)
    return raw, cr.filter_points(raw[0], raw[1])


@functools.lru_cache(maxsize=None)
def _backprojected(name):
    case = next(c for c in all_stereo_cases() if c.name == name)
    return cr.backproject(case)


# ------------------------------------------------------------------------------- the reference's own clouds ---
def test_restatement_gives_the_reference_fusion_golden():
    g, sb = load_golden("g10_fuse_filter"), GoldenScene("scene_b")
    refs = [int(r) for r in g["refs"]]
    case = ci.MapCase("g10", np.stack([sb.gt_depth[r] for r in refs]), g["confidence"], np.stack([sb.colors[r] for r in refs]),
                      np.linalg.inv(sb.K), [(sb.R[r], sb.t[r]) for r in refs], 3)
    pts, rgb, raw = cr.fuse_filter(case, do_filter=False)
    assert raw == len(g["points"]) and same_cloud((pts, rgb), (g["points"], g["colors"]))
    assert same_cloud(cr.filter_points(pts, rgb), (g["f_points"], g["f_colors"]))


def test_restatement_gives_the_reference_stereo_golden():
    g11, g12, sc = load_golden("g11_plane_sweep"), load_golden("g12_stereo_post"), GoldenScene("scene_c")
    ref = int(g11["ref"])
    common = (sc.colors[ref][None], np.linalg.inv(sc.K), [(sc.R[ref], sc.t[ref])], 2.5)
    pts, rgb, per = cr.backproject(ci.MapCase("g12 bp", g11["depth_map"][None], g11["confidence"][None], *common))
    assert per == [len(g12["bp_points"])] and same_cloud((pts, rgb), (g12["bp_points"], g12["bp_colors"]))
    conf4 = np.full((1, sc.H, sc.W), 4.0, np.float32)
    pts, rgb, _ = cr.backproject(ci.MapCase("g12 gt", sc.gt_depth[ref][None], conf4, *common))
    assert same_cloud((pts, rgb), (g12["gt_points"], g12["gt_colors"]))
    assert same_cloud(cr.voxel_downsample(pts, rgb, 0.02), (g12["vox_points"], g12["vox_colors"]))
    # the outlier statistic of the whole cloud (3072 queries), then the reference's threshold and selection
    mean_d = cr.knn_mean(pts, 20)
    keep = mean_d < np.mean(mean_d) + 2.0 * np.std(mean_d)
    assert same_cloud((pts[keep], rgb[keep]), (g12["out_points"], g12["out_colors"]))


# ------------------------------------------------------------------------------------ the package's host path ---
@contextlib.contextmanager
def inverse_is(K_inv):
    """The host path inverts its own intrinsics; the cases give K_inv itself, which is the inverse of no float64
    matrix in general.  For the duration of a host call np.linalg.inv answers with the case's K_inv, and only to the
    one question the host path is known to ask: the inverse of K_scaled, which host_fuse / host_backproject set to
    the identity.  Any other inversion fails the test instead of silently receiving K_inv."""
    real = np.linalg.inv

    def answer(a):
        assert np.array_equal(np.asarray(a), np.eye(3)), "the host path inverted something other than K_scaled"
        return np.array(K_inv, np.float64)
    np.linalg.inv = answer
    try:
        yield
    finally:
        np.linalg.inv = real


def host_fuse(case, do_filter=True):
    pm = PatchMatchMVS.__new__(PatchMatchMVS)
    pm.min_views, pm.K_scaled = case.threshold, np.eye(3)
    n = len(case.poses)
    maps = {j: DepthNormalMap(depth=case.depth[j], normal=None, confidence=case.conf[j]) for j in range(n)}
    poses = {j: amvs.CameraPose(R=np.array(R, np.float64), t=np.array(t, np.float64)) for j, (R, t) in enumerate(case.poses)}
    with inverse_is(case.K_inv):
        pts, rgb = pm._fuse_depth_maps(maps, {j: {"color": case.bgr[j]} for j in range(n)}, poses)
    raw = len(pts)
    if do_filter and raw:
        pts, rgb = pm._filter_points(pts, rgb)
    return pts, rgb, raw


def host_backproject(case):
    rec = DenseStereoReconstructor.__new__(DenseStereoReconstructor)
    rec.K_scaled = np.eye(3)
    clouds, cols, per = [], [], []
    with inverse_is(case.K_inv):
        for j, (R, t) in enumerate(case.poses):
            p, c = rec._backproject(case.depth[j], case.conf[j], case.bgr[j],
                                    amvs.CameraPose(R=np.array(R, np.float64), t=np.array(t, np.float64)), case.threshold)
            clouds.append(p.reshape(-1, 3)), cols.append(np.asarray(c, np.uint8).reshape(-1, 3)), per.append(len(p))
    return np.vstack(clouds), np.vstack(cols), per


def test_host_fusion_equals_restatement_on_the_family():
    n_points = 0
    for case in all_fusion_cases():
        (raw_p, raw_c, raw), want = _fused(case.name)
        got = host_fuse(case, do_filter=False)
        assert got[2] == raw and same_cloud(got, (raw_p, raw_c)), case.name
        got = host_fuse(case)
        assert same_cloud(got, want), case.name
        n_points += raw
    assert n_points > 5000


def test_host_stereo_steps_equal_restatement_on_the_family():
    rec = DenseStereoReconstructor.__new__(DenseStereoReconstructor)
    for case in all_stereo_cases():
        pts, rgb, per = _backprojected(case.name)
        got = host_backproject(case)
        assert got[2] == per and same_cloud(got, (pts, rgb)), case.name
        if len(pts) == 0:
            continue
        for voxel in ci.VOXEL_SIZES:
            assert same_cloud(rec._voxel_down_sample(pts, rgb, voxel), cr.voxel_downsample(pts, rgb, voxel)), (case.name, voxel)
            for mask_name, keep in ci.keep_masks(len(pts)):
                want = cr.voxel_downsample(pts, rgb, voxel, keep)
                assert same_cloud(rec._voxel_down_sample(pts[keep], rgb[keep], voxel), want), (case.name, voxel, mask_name)
        for take_name, idx in ci.take_cases(len(pts)):
            assert same_cloud((pts[idx], rgb[idx]), cr.take(pts, rgb, idx)), (case.name, take_name)
        for bad in (len(pts), -1):
            with pytest.raises(IndexError):
                cr.take(pts, rgb, [0, bad])


def test_knn_restatement_equals_scikit_learn_where_it_uses_its_tree():
    NearestNeighbors = pytest.importorskip("sklearn.neighbors").NearestNeighbors
    checked = 0
    for k in ci.KNN_KS:
        for name, pts in ci.knn_cases(k):
            if len(pts) < 2 * k + 2:
                continue
            dists, _ = NearestNeighbors(n_neighbors=k).fit(pts).kneighbors(pts)
            assert same(np.mean(dists[:, 1:], axis=1), cr.knn_mean(pts, k)), name
            checked += 1
    assert checked == 5 * len(ci.KNN_KS)


def test_fraction_fma_is_the_correctly_rounded_one():
    """Products whose unfused evaluation rounds twice: the exact form differs from it and equals the error-free
    transformation's answer where that is exact."""
    assert cr.fma(1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0) == 2.0 ** -29 + 2.0 ** -60
    assert (1.0 + 2.0 ** -30) * (1.0 + 2.0 ** -30) - 1.0 == 2.0 ** -29
    assert cr.fma(0.1, 10.0, -1.0) == 2.0 ** -54
    assert cr.fma(3.0, 5.0, 7.0) == 22.0


# ------------------------------------------------------------------------- the family tells the near-misses apart ---
def _distinguished_by(variant):
    """Name of the first case whose result the near-miss changes, or None."""
    if variant in ("knn_keep_self", "knn_plain_sum"):
        for k in ci.KNN_KS:
            for name, pts in ci.knn_cases(k):
                if not same(cr.knn_mean(pts, k), cr.knn_mean(pts, k, variant=variant)):
                    return name
        return None
    if variant in ("gt_conf", "ge_depth"):
        for case in all_stereo_cases():
            if cr.select_stereo(case.conf, case.depth, case.threshold) != cr.select_stereo(case.conf, case.depth, case.threshold, variant):
                return case.name
        return None
    if variant in ("unfused_project", "pose_of_map0", "bgr_kept"):
        for case in all_fusion_cases():
            if not same_cloud(cr.fuse_filter(case, False, variant), _fused(case.name)[0]):
                return case.name
        return None
    for case in all_fusion_cases():                          # the filter's near-misses, on the definition's raw cloud
        (pts, rgb, _), want = _fused(case.name)
        if not same_cloud(cr.filter_points(pts, rgb, variant), want):
            return case.name
    return None


def test_every_near_miss_changes_a_result():
    """A condition on the inputs: each variant of cloud_restatement.VARIANTS must change the result of at least one
    case, or no comparison with the device could notice a kernel that computes it.

    single_branch_lerp is the exception, and provably so.  The threshold lies in [a, b], the two neighbours of the
    virtual index among the sorted distances, and no distance lies strictly between them, so the kept set depends only
    on whether the threshold exceeds a.  Either formula returns a only if it adds less than half an ulp to a, and b - a
    is at least one ulp: that needs b - a = 1 ulp and t = 0.5, where both formulas meet the same tie and round it to
    the same even neighbour.  So the two formulas, which do differ in the last bit of the threshold (shown below on
    the family), always keep the same points."""
    survivors = []
    for variant in cr.VARIANTS:
        if variant == "single_branch_lerp":
            continue
        where = _distinguished_by(variant)
        print(f"{variant}: distinguished by {where!r}")
        if where is None:
            survivors.append(variant)
    assert not survivors, f"no case of the family notices {survivors}"
    differs = []
    for case in all_fusion_cases():
        (pts, rgb, raw), want = _fused(case.name)
        if raw == 0:
            continue
        dist = cr.distances(pts)
        if cr.percentile95(dist) != cr.percentile95(dist, "single_branch_lerp"):
            differs.append(case.name)
        assert same_cloud(cr.filter_points(pts, rgb, "single_branch_lerp"), want), case.name
    print(f"single_branch_lerp: threshold differs in the last bits on {differs}, kept set never")
    assert differs
    # a seeded search for a kept set that differs, over the counts whose fraction is at or above 0.5: none, as argued
    rng = np.random.default_rng(5)
    for m in (3, 4, 11, 22, 42) * 40:
        pts = rng.normal(size=(m, 3)) * 10.0 ** rng.integers(-3, 4)
        assert cr.radius_keep(pts)[0] == cr.radius_keep(pts, "single_branch_lerp")[0]


# ------------------------------------------------------------------------------- the family reaches its edges ---
def test_family_reaches_the_edges_it_names():
    fusion = {c.name: _fused(c.name) for c in all_fusion_cases()}
    raw_counts = {name: r[0][2] for name, r in fusion.items()}
    # selected counts, and the two empty results
    for H, W in ci.SIZES:
        got = {raw_counts[c.name] for c in ci.fusion_cases(H, W)}
        assert {0, 1, 2, 3, 4} <= got, (H, W)
    assert set(ci.COUNTS) <= {raw_counts[c.name] for c in ci.fusion_cases(3, 5)}
    cut_away = {raw_counts[n] for n, r in fusion.items() if raw_counts[n] > 0 and len(r[1][0]) == 0}
    assert {1, 2} <= cut_away
    # ties with the threshold on both lattices: the cut is strict
    for name in (n for n in fusion if n.startswith("lattice")):
        keep, thr, dist = cr.radius_keep(fusion[name][0][0])
        assert raw_counts[name] == 343 and sum(d == thr for d in dist) >= 10, name
    # voxel indices that the reciprocal and the truncation get wrong; coordinates on both sides of zero
    for kind, result in (("fuse", fusion["fuse voxel boundaries 17x33"][0]), ("stereo", _backprojected("stereo voxel boundaries 17x33"))):
        pts = result[0]
        assert (pts < 0).any() and (pts > 0).any()
        for variant in ("reciprocal_voxel", "trunc_voxel"):
            n_diff = sum(any(cr.voxel_index(float(v), 0.01) != cr.voxel_index(float(v), 0.01, variant) for v in p) for p in pts)
            print(f"{kind} voxel boundaries: {n_diff} of {len(pts)} points change voxel under {variant}")
            assert n_diff >= 50, (kind, variant)
    # the cross-axis collision: two points of different voxels with one key
    pts = _backprojected("stereo key collision 17x33")[0]
    cells = [tuple(cr.voxel_index(float(v), 1.0) for v in p) for p in pts]
    keys = [cr.voxel_key(p, 1.0) for p in pts]
    assert cells[0] != cells[1] and keys[0] == keys[1] and keys[2] != keys[0] and cells[0][2] < 0
    assert len(cr.voxel_downsample(pts, np.zeros((3, 3), np.uint8), 1.0)[0]) == 2
    # 5 to 50 points per 1 cm voxel, not sorted by voxel
    pts = _backprojected("stereo shuffled voxels 17x33")[0]
    keys = [cr.voxel_key(p, 0.01) for p in pts]
    sizes = np.unique(keys, return_counts=True)[1]
    assert sizes.min() >= 5 and sizes.max() <= 50 and len(sizes) >= 20 and keys != sorted(keys)
    # maps without a selected pixel in every position; one pixel per map
    pers = [tuple(p > 0 for p in _backprojected(c.name)[2]) for c in ci.stereo_cases(3, 5)]
    assert {(False, True, True, True), (True, False, False, True), (True, True, True, False), (False,) * 4} <= set(pers)
    assert _backprojected("stereo key collision 3x5")[2] == [1, 1, 1]
    # the stride cases cross the launch cap in the flat index and in the selected set
    n, H, W = ci.STRIDE_SHAPE
    for kind in ("fuse", "stereo"):
        case = ci.stride_case(kind)
        sel = cr.select_fuse(case.conf, case.threshold)[0] if kind == "fuse" else cr.select_stereo(case.conf, case.depth, case.threshold)[0]
        assert n * H * W > ci.LAUNCH_CAP and 1900 <= len(sel) <= 2100
        assert {0, n * H * W - 1, ci.LAUNCH_CAP - 1, ci.LAUNCH_CAP, H * W - 1, H * W, 2 * H * W - 1, 2 * H * W} <= set(sel)
        assert sum(g >= ci.LAUNCH_CAP for g in sel) >= 100
    # the resident kNN's sample stride is 2 on the fused and filtered sheet (counted on the host path, shown above to
    # equal the restatement): more than 2 * 16384 points are left, fewer than 3 * 16384
    pts, _, raw = host_fuse(ci.big_cloud_case())
    print(f"sheet: {raw} points fused, {len(pts)} left by the filter")
    assert raw == ci.BIG_SHAPE[0] * ci.BIG_SHAPE[1] and 2 * 16384 < len(pts) < 3 * 16384
