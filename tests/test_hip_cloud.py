"""The point-cloud stage on the device (csrc/amvs_fusion.hip, the cloud entry points of csrc/amvs_capi_cloud.hip, the
resident-cloud path of csrc/amvs_knn.hip) against the restatement of tests/cloud_restatement.py on the input family of
tests/cloud_inputs.py; tests/test_cloud_restatement_cpu.py shows on the CPU that the restatement gives the reference's
own clouds and that the family reaches the edges it names.  Every comparison is bit for bit: points as uint64, colours
and counts element for element."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_inputs as ci  # noqa: E402
import cloud_restatement as cr  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = ci.SIZES + (ci.STRIDE_SHAPE[1:],)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint64), b.view(np.uint64)) if a.dtype == np.float64 else np.array_equal(a, b)


def same_cloud(got, want):
    return same(got[0], want[0]) and same(got[1], want[1])


def fusion_family(shape):
    return ci.stride_cases("fuse") if shape == ci.STRIDE_SHAPE[1:] else ci.fusion_cases(*shape)


def stereo_family(shape):
    return ci.stride_cases("stereo") if shape == ci.STRIDE_SHAPE[1:] else ci.stereo_cases(*shape)


_FUSED, _BACKPROJECTED = {}, {}                  # restated once per case, built when a test first asks


def fused(case):
    """((raw points, colours, raw count), (filtered points, colours)) of the restatement."""
    if case.name not in _FUSED:
        raw = cr.fuse_filter(case, do_filter=False)
        _FUSED[case.name] = raw, cr.filter_points(raw[0], raw[1])
    return _FUSED[case.name]


def backprojected(case):
    if case.name not in _BACKPROJECTED:
        _BACKPROJECTED[case.name] = cr.backproject(case)
    return _BACKPROJECTED[case.name]


@pytest.fixture(scope="module")
def amvs_mod():
    import amvs
    return amvs


@pytest.fixture(scope="module")
def engines(amvs_mod):
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = amvs_mod.Engine(shape[0], shape[1], 1, np.eye(3, dtype=np.float32))
        return made[shape]
    yield get
    for eng in made.values():
        eng.close()


def on_device(*arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    torch.cuda.synchronize()
    return out


def device_fuse(eng, case, do_filter, resident):
    if not resident:
        return eng.fuse_filter(case.depth, case.conf, case.bgr, case.K_inv, case.poses, case.threshold, do_filter)
    d_t, c_t = on_device(case.depth, case.conf)
    return eng.fuse_filter(None, None, case.bgr, case.K_inv, case.poses, case.threshold, do_filter,
                           device_ptrs=(d_t.data_ptr(), c_t.data_ptr(), len(case.poses)))


def device_backproject(eng, case, resident=False):
    if not resident:
        return eng.stereo_backproject(case.bgr, case.K_inv, case.poses, case.threshold, depth=case.depth, conf=case.conf, fetch=True)
    d_t, c_t = on_device(case.depth, case.conf)
    return eng.stereo_backproject(case.bgr, case.K_inv, case.poses, case.threshold, fetch=True,
                                  device_ptrs=(d_t.data_ptr(), c_t.data_ptr()))


def assert_no_resident_cloud(eng, what):
    """After an empty result.  Engine.fetch_cloud(0) answers (0, 3) arrays without asking the library, so it shows only
    that the call is harmless; that the library holds no cloud is shown by the voxel grid counting 0 points and by the
    kNN entry refusing both an empty and a non-empty request."""
    from amvs.engine import AmvsError
    pts, rgb = eng.fetch_cloud(0)
    assert pts.shape == (0, 3) and rgb.shape == (0, 3), what
    assert eng.cloud_voxel_downsample(0.02) == 0, what
    with pytest.raises(AmvsError):
        eng.cloud_knn_mean_distance(0, 20)
    with pytest.raises(AmvsError):
        eng.cloud_knn_mean_distance(8, 8)


def check_fusion(eng, case, resident):
    (raw_p, raw_c, m), want = fused(case)
    got = device_fuse(eng, case, False, resident)
    assert got[2] == m and same_cloud(got, (raw_p, raw_c)), f"{case.name}: raw cloud (maps on the device: {resident})"
    if m == 0:
        assert_no_resident_cloud(eng, case.name)
    got = device_fuse(eng, case, True, resident)
    assert got[2] == m and same_cloud(got, want), f"{case.name}: filtered cloud (maps on the device: {resident})"
    if len(want[0]) == 0:
        assert_no_resident_cloud(eng, case.name)
    return m, len(want[0])


def check_backprojection(eng, case, resident):
    pts, rgb, per = backprojected(case)
    counts, total, got_p, got_c = device_backproject(eng, case, resident)
    assert counts == per and total == len(pts), f"{case.name}: counts {counts}, total {total}"
    assert same_cloud((got_p, got_c), (pts, rgb)), f"{case.name} (maps on the device: {resident})"
    return total


# ------------------------------------------------------------------------------------------------ fusion ---
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fusion_raw_and_filtered_equal_restatement(engines, shape):
    eng = engines(shape)
    raws, kept = set(), set()
    for case in fusion_family(shape):
        for resident in (False, True):
            m, m3 = check_fusion(eng, case, resident)
        raws.add(m)
        kept.add((m, m3))
    assert 0 in raws and ({(1, 0), (2, 0)} <= kept or shape == ci.STRIDE_SHAPE[1:])


# ---------------------------------------------------------------------------------------- back-projection ---
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_backprojection_equals_restatement(engines, shape):
    eng = engines(shape)
    totals = set()
    for case in stereo_family(shape):
        for resident in (False, True):
            total = check_backprojection(eng, case, resident)
        if total == 0:
            assert_no_resident_cloud(eng, case.name)
        totals.add(total)
    assert 0 in totals and 1 in totals


# ------------------------------------------------------------------------------- steps on the resident cloud ---
@pytest.mark.parametrize("shape", ci.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resident_voxel_grid_equals_restatement(engines, shape):
    eng = engines(shape)
    for case in stereo_family(shape):
        pts, rgb, _ = backprojected(case)
        n = len(pts)
        for voxel in ci.VOXEL_SIZES:
            # as the reference continues: back-project, mask (the outlier filter's selection) or none, voxel grid ...
            for mask_name, keep in (("no mask", None),) + ci.keep_masks(n):
                device_backproject(eng, case)
                want = cr.voxel_downsample(pts, rgb, voxel, keep)
                m = eng.cloud_voxel_downsample(voxel, keep)
                assert m == len(want[0]) and same_cloud(eng.fetch_cloud(m), want), f"{case.name}: voxel {voxel}, {mask_name}"
                if voxel != 0.02:
                    continue
                # ... and a second, coarser grid on the cloud that stayed resident
                want = cr.voxel_downsample(want[0], want[1], 0.05)
                m = eng.cloud_voxel_downsample(0.05)
                assert m == len(want[0]) and same_cloud(eng.fetch_cloud(m), want), f"{case.name}: {mask_name}, 0.02, then 0.05"


@pytest.mark.parametrize("shape", ci.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cloud_take_equals_restatement_and_a_refusal_changes_nothing(engines, shape):
    from amvs.engine import AmvsError
    eng = engines(shape)
    for case in stereo_family(shape):
        pts, rgb, _ = backprojected(case)
        n = len(pts)
        if n == 0:
            device_backproject(eng, case)
            assert eng.cloud_take(np.zeros(0, np.int64)) == 0
            with pytest.raises(AmvsError):
                eng.cloud_take([0])
            continue
        for take_name, idx in ci.take_cases(n):
            device_backproject(eng, case)
            want = cr.take(pts, rgb, idx)
            assert eng.cloud_take(idx) == len(idx)
            assert same_cloud(eng.fetch_cloud(len(idx)), want), f"{case.name}: {take_name}"
            if len(idx):                                  # the taken cloud is a cloud like any other
                want = cr.voxel_downsample(want[0], want[1], 0.02)
                m = eng.cloud_voxel_downsample(0.02)
                assert m == len(want[0]) and same_cloud(eng.fetch_cloud(m), want), f"{case.name}: {take_name}, then voxel"
        device_backproject(eng, case)
        for bad in (n, -1):
            with pytest.raises(AmvsError):
                eng.cloud_take([0, bad, n - 1])
            assert same_cloud(eng.fetch_cloud(n), (pts, rgb)), f"{case.name}: cloud after the refused index {bad}"
        assert eng.cloud_take([n - 1]) == 1 and same_cloud(eng.fetch_cloud(1), cr.take(pts, rgb, [n - 1]))


# ------------------------------------------------------------------------------- one context, many sizes ---
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_context_through_ascending_and_descending_sizes(amvs_mod, shape):
    """Every call leases its scratch from the context's cache, so a short call after a long one finds the long one's
    bytes behind its own: the whole family on ONE fresh context, by selected count upwards and then downwards (at
    720 x 1024 the 2000-point case comes last, then first)."""
    jobs = [("fuse", c, fused(c)[0][2]) for c in fusion_family(shape)]
    jobs += [("stereo", c, len(backprojected(c)[0])) for c in stereo_family(shape)]
    jobs.sort(key=lambda j: j[2])
    assert jobs[0][2] == 0 and jobs[-1][2] >= 4
    with amvs_mod.Engine(shape[0], shape[1], 1, np.eye(3, dtype=np.float32)) as eng:
        for order in (jobs, jobs[::-1]):
            for kind, case, m in order:
                if kind == "fuse":
                    check_fusion(eng, case, False)
                    continue
                check_backprojection(eng, case, False)
                if m:
                    pts, rgb, _ = backprojected(case)
                    want = cr.voxel_downsample(pts, rgb, 0.02, np.arange(m) % 2 == 0)
                    got_m = eng.cloud_voxel_downsample(0.02, np.arange(m) % 2 == 0)
                    assert got_m == len(want[0]) and same_cloud(eng.fetch_cloud(got_m), want), case.name


# --------------------------------------------------------------------------------------------------- kNN ---
@pytest.mark.parametrize("k", ci.KNN_KS)
def test_knn_mean_distance_equals_brute_force(engines, k):
    eng = engines(ci.SIZES[0])
    for name, pts in ci.knn_cases(k):
        got = eng.knn_mean_distance(pts, k)
        want = cr.knn_mean(pts, k)
        assert same(got, want), f"{name}: {int((got != want).sum())} of {len(want)} means differ"
        if "identical" in name:
            assert not got.any()


@pytest.fixture(scope="module")
def big_cloud(amvs_mod):
    """The fused and filtered cloud of the 160 x 256 sheet, left resident: the cut removes a twentieth of the 40 960
    points and the 1 cm grid next to none (the CPU test counts them on the host path), so the resident kNN samples it
    with stride 2."""
    case = ci.big_cloud_case()
    with amvs_mod.Engine(ci.BIG_SHAPE[0], ci.BIG_SHAPE[1], 1, np.eye(3, dtype=np.float32)) as eng:
        pts, rgb, raw = device_fuse(eng, case, True, False)
        assert raw == ci.BIG_SHAPE[0] * ci.BIG_SHAPE[1] and 2 * 16384 < len(pts) < 3 * 16384
        yield eng, pts


@pytest.mark.parametrize("k", [20, 32])
def test_resident_cloud_knn_equals_host_cloud_knn_and_brute_force(big_cloud, k):
    eng, pts = big_cloud
    n = len(pts)
    resident = eng.cloud_knn_mean_distance(n, k)
    assert same(resident, eng.knn_mean_distance(pts, k))
    assert same(eng.fetch_cloud(n)[0], pts)                       # (the statistic leaves the cloud as it was)
    queries = np.sort(np.random.default_rng(3000).choice(n, 3000, replace=False))
    want = cr.knn_mean(pts, k, queries=queries, chunk=128)
    assert same(resident[queries], want), f"{int((resident[queries] != want).sum())} of 3000 means differ"
