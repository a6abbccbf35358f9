"""Normals from the depth maps on the device (csrc/amvs_cloud_normals.hip and its entry points in
csrc/amvs_capi_cloud.hip) against the restatement of tests/cloud_normals_restatement.py on the input family of
tests/cloud_normals_inputs.py; tests/test_cloud_normals_cpu.py shows on the CPU that the restatement's two forms agree and
that the family reaches every guard and edge.  Every comparison is bit for bit: normals as uint32, counts element for
element."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_normals_inputs as ni  # noqa: E402
import cloud_normals_restatement as nr  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


_RESTATED = {}                                   # restated once per case, built when a test first asks


def restated(case):
    """(camera-frame fit, world-frame fit, cloud step or None).  The small inputs by the loops in the world frame and for
    the cloud, by the twin in the camera frame (the CPU test holds the two to each other in both); the large input by the
    twin."""
    if case.name not in _RESTATED:
        cam = nr.fit_normals_np(*case.fit_args(), False)
        world = (nr.fit_normals_np if case.big else nr.fit_normals)(*case.fit_args(), True)
        cloud = None
        if case.points is not None:
            step = nr.cloud_normals_np if case.big else nr.cloud_normals
            cloud = step(case.points, case.depth, world[0], *case.cloud_args())
        _RESTATED[case.name] = (cam, world, cloud)
    return _RESTATED[case.name]


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


def fit_kwargs(case):
    return dict(min_confidence=case.min_confidence, radius=case.radius, jump=case.jump, min_points=case.min_points)


def device_fit(eng, case, world, resident=False):
    if resident:
        d_t, c_t = on_device(case.depth, case.conf)
        return eng.depth_normals(case.K, case.poses, world=world, device_ptrs=(d_t.data_ptr(), c_t.data_ptr()), **fit_kwargs(case))
    return eng.depth_normals(case.K, case.poses, world=world, depth=case.depth, conf=case.conf, **fit_kwargs(case))


def device_cloud(eng, case, resident=False):
    """((pixels with a normal, points with a normal), normals, seen) of the case's cloud, set with the test hook."""
    n = eng.cloud_set(case.points)
    kw = dict(depth_tolerance=case.depth_tolerance, min_views=case.min_views, **fit_kwargs(case))
    if resident:
        d_t, c_t = on_device(case.depth, case.conf)
        counts = eng.cloud_normals(case.K, case.poses, device_ptrs=(d_t.data_ptr(), c_t.data_ptr()), **kw)
    else:
        counts = eng.cloud_normals(case.K, case.poses, depth=case.depth, conf=case.conf, **kw)
    return (counts,) + eng.fetch_cloud_normals(n)


def check_case(eng, case, resident=False):
    cam, world, cloud = restated(case)
    for is_world, want in ((False, cam), (True, world)):
        got, count = device_fit(eng, case, is_world, resident)
        assert count == want[1], f"{case.name}: {count} pixels with a normal, restatement {want[1]} (world {is_world})"
        assert same(got, want[0]), (f"{case.name}: {int((bits(got) != bits(want[0])).any(-1).sum())} normals differ "
                                    f"(world {is_world}, maps on the device: {resident})")
    if cloud is not None:
        counts, normals, seen = device_cloud(eng, case, resident)
        assert counts == (world[1], cloud[2]), f"{case.name}: counts {counts}"
        assert np.array_equal(seen, cloud[1]), f"{case.name}: {int((seen != cloud[1]).sum())} seen counts differ"
        assert same(normals, cloud[0]), f"{case.name}: {int((bits(normals) != bits(cloud[0])).any(-1).sum())} cloud normals differ"
        # the fit of the cloud call leaves the world-frame maps behind
        held = np.empty(case.depth.shape + (3,), np.float32)
        eng._chk(eng._lib.amvs_fetch_depth_normals(eng._h, 0, case.depth.shape[0], held.ctypes.data_as(C.POINTER(C.c_float))))
        assert same(held, world[0]), case.name


@pytest.mark.parametrize("case", ni.device_family(), ids=lambda c: c.name)
def test_normal_maps_and_cloud_normals_equal_restatement(engines, case):
    """The whole family, except its images of one row, one column and one pixel: a context is 2 x 2 at least (amvs_create),
    so those three are restated on the CPU only, and the device meets their situation -- every used set collinear -- in
    one_valid_row and one_valid_column."""
    check_case(engines(case.shape), case)


def test_a_context_cannot_hold_the_one_row_inputs(amvs_mod):
    from amvs.engine import AmvsError
    left_out = [c.name for c in ni.family() if c not in ni.device_family()]
    assert left_out == ["row_1x9", "col_9x1", "one_pixel"]
    for shape in ((1, 9), (9, 1)):
        with pytest.raises(AmvsError):
            amvs_mod.Engine(shape[0], shape[1], 1, np.eye(3, dtype=np.float32))


@pytest.mark.parametrize("name", ["special_values", "plate_two_views", "scene_4x48x64_r2"])
def test_maps_in_device_memory_give_the_same(engines, name):
    check_case(engines(ni.by_name(name).shape), ni.by_name(name), resident=True)


def test_fetch_of_single_maps_and_its_refusals(engines, amvs_mod):
    case = ni.by_name("borders_r2")
    eng = engines(case.shape)
    want = restated(case)[0][0]
    device_fit(eng, case, False)
    n, H, W = case.depth.shape
    one = np.empty((1, H, W, 3), np.float32)
    for j in range(n):
        eng._chk(eng._lib.amvs_fetch_depth_normals(eng._h, j, 1, one.ctypes.data_as(C.POINTER(C.c_float))))
        assert same(one[0], want[j])
    for first, count in ((n, 1), (0, n + 1), (-1, 1), (0, 0)):
        assert eng._lib.amvs_fetch_depth_normals(eng._h, first, count, one.ctypes.data_as(C.POINTER(C.c_float))) == -1


# -------------------------------------------------------------------------------- the resident sweep maps ---
@pytest.fixture(scope="module")
def swept(amvs_mod):
    """A plane-sweep batch left resident on a context of its own: (engine, host copies of the maps, K, poses)."""
    sc = ni.scene(ni.SCENE_SMALL)
    n, H, W = ni.SCENE_SMALL
    with amvs_mod.Engine(H, W, n, sc.camera.K.astype(np.float32)) as eng:
        for i in range(n):
            eng.set_view(i, sc.grays[i], sc.poses[i].R, sc.poses[i].t)
        refs = [0, 1, 2, 3]
        nbrs = [[1, 2], [0, 2], [1, 3], [2, 1]]
        depths = 1.0 / np.linspace(1 / sc.depth_max, 1 / sc.depth_min, 24)
        eng.plane_sweep_batch(refs, nbrs, depths, 5, 0.6)
        depth, conf = eng.fetch_sweep_maps(0, n)
        poses = [(sc.poses[i].R.astype(np.float64), sc.poses[i].t.astype(np.float64)) for i in refs]
        yield eng, depth.reshape(n, H, W), conf.reshape(n, H, W), sc.camera.K.astype(np.float64), poses


def test_maps_where_0_1_and_2_agree_and_equal_restatement(swept):
    eng, depth, conf, K, poses = swept
    kw = dict(min_confidence=1.5, radius=2, jump=0.05, min_points=3)
    want, count, _ = nr.fit_normals_np(depth, conf, K, poses, 1.5, 2, 0.05, 3, True)
    assert count > 500                                         # (the sweep's maps are rough; enough pixels still fit)
    d_t, c_t = on_device(depth, conf)
    got = {0: eng.depth_normals(K, poses, world=True, depth=depth, conf=conf, **kw),
           1: eng.depth_normals(K, poses, world=True, device_ptrs=(d_t.data_ptr(), c_t.data_ptr()), **kw),
           2: eng.depth_normals(K, poses, world=True, **kw)}
    for where, (normals, n) in got.items():
        assert n == count and same(normals, want), f"maps_where {where}"
    pts = ni.backproject(K, poses[1], *np.meshgrid(np.arange(4.0, 60.0, 3.0), np.arange(4.0, 44.0, 3.0)), 5.0).reshape(-1, 3)
    v, u = np.divmod(np.flatnonzero(conf[1].reshape(-1) >= 1.5)[::5], depth.shape[2])
    pts = np.concatenate([pts, ni.backproject(K, poses[1], u.astype(np.float64), v.astype(np.float64), depth[1][v, u].astype(np.float64))])
    ref = nr.cloud_normals_np(pts, depth, want, K, poses, 0.01, 1)
    assert ref[2] > 100
    for where, maps in ((0, dict(depth=depth, conf=conf)), (1, dict(device_ptrs=(d_t.data_ptr(), c_t.data_ptr()))), (2, {})):
        eng.cloud_set(pts)
        counts = eng.cloud_normals(K, poses, depth_tolerance=0.01, min_views=1, **kw, **maps)
        normals, seen = eng.fetch_cloud_normals(len(pts))
        assert counts == (count, ref[2]) and np.array_equal(seen, ref[1]) and same(normals, ref[0]), f"maps_where {where}"
    from amvs.engine import AmvsError
    with pytest.raises(AmvsError):                             # (three maps asked of a batch of four)
        eng.depth_normals(K, poses[:3], **kw)


# ------------------------------------------------------------------------- one context, large then small ---
def test_small_input_after_a_large_one_on_the_same_context(amvs_mod):
    """The normal maps, the cloud's normals and its counts live in grow-only buffers: a small input after a large one
    finds the large one's values behind its own."""
    big = ni.by_name("scene_4x48x64_r2")
    small = ni.Case("first_map_few_points", big.depth[:1], big.conf[:1], big.K, big.poses[:1], min_confidence=3.0, radius=1,
                    points=big.points[:7], min_views=1)
    with amvs_mod.Engine(big.shape[0], big.shape[1], 1, np.eye(3, dtype=np.float32)) as eng:
        for case in (big, small, big):
            check_case(eng, case)


# --------------------------------------------------------------------------- the normals belong to a cloud ---
def test_steps_that_make_a_cloud_drop_the_normals_and_recomputing_restates_the_new_cloud(engines):
    from amvs.engine import AmvsError
    case = ni.by_name("scene_4x48x64_r2")
    eng = engines(case.shape)
    world = restated(case)[1]
    n = len(case.points)
    kw = dict(depth=case.depth, conf=case.conf, depth_tolerance=case.depth_tolerance, min_views=case.min_views, **fit_kwargs(case))

    def recomputed(m, what):
        pts, _ = eng.fetch_cloud(m)
        with pytest.raises(AmvsError):
            eng.fetch_cloud_normals(m)
        want = nr.cloud_normals_np(pts, case.depth, world[0], *case.cloud_args())
        counts = eng.cloud_normals(case.K, case.poses, **kw)
        normals, seen = eng.fetch_cloud_normals(m)
        assert counts == (world[1], want[2]) and np.array_equal(seen, want[1]) and same(normals, want[0]), what
        assert want[2] > 0

    device_cloud(eng, case)
    idx = np.arange(n - 1, -1, -3)
    assert eng.cloud_take(idx) == len(idx)
    recomputed(len(idx), "after cloud_take")
    m = eng.cloud_voxel_downsample(0.1)
    assert 0 < m < len(idx)
    recomputed(m, "after cloud_voxel_downsample")
    eng.cloud_set(case.points[:5])
    with pytest.raises(AmvsError):
        eng.fetch_cloud_normals(5)
    eng.cloud_set(np.zeros((0, 3)))                            # no resident cloud
    with pytest.raises(AmvsError):
        eng.cloud_normals(case.K, case.poses, **kw)


def test_parameter_errors(engines):
    from amvs.engine import AmvsError
    case = ni.by_name("plate_two_views")
    eng = engines(case.shape)
    eng.cloud_set(case.points)
    good = dict(min_confidence=1.0, radius=2, jump=0.05, min_points=3)
    bad = [dict(radius=0), dict(radius=5), dict(min_points=2), dict(jump=0.0), dict(jump=-0.05), dict(jump=float("nan")),
           dict(jump=float("inf"))]
    for change in bad:
        with pytest.raises(AmvsError):
            eng.depth_normals(case.K, case.poses, depth=case.depth, conf=case.conf, **{**good, **change})
        with pytest.raises(AmvsError):
            eng.cloud_normals(case.K, case.poses, depth=case.depth, conf=case.conf, **{**good, **change})
    for change in (dict(depth_tolerance=0.0), dict(depth_tolerance=float("nan")), dict(depth_tolerance=float("inf")),
                   dict(depth_tolerance=-1.0), dict(min_views=0)):
        with pytest.raises(AmvsError):
            eng.cloud_normals(case.K, case.poses, depth=case.depth, conf=case.conf, **{**good, **change})
    lib, h = eng._lib, eng._h
    n = case.depth.shape[0]
    d, c = case.depth.ctypes.data_as(C.c_void_p), case.conf.ctypes.data_as(C.c_void_p)
    K = np.ascontiguousarray(case.K).ctypes.data_as(C.POINTER(C.c_double))
    P = np.zeros((n, 12)).ctypes.data_as(C.POINTER(C.c_double))
    cnt = (C.c_int64 * 2)()
    for Kp, Pp, dp, where in ((None, P, d, 0), (K, None, d, 0), (K, P, None, 0), (K, P, d, 3), (K, P, d, -1)):
        assert lib.amvs_depth_normals(h, n, dp, c, where, Kp, Pp, 1.0, 2, 0.05, 3, 0, cnt) == -1
        assert lib.amvs_cloud_normals(h, n, dp, c, where, Kp, Pp, 1.0, 2, 0.05, 3, 0.01, 1, cnt) == -1
    assert lib.amvs_depth_normals(h, 0, d, c, 0, K, P, 1.0, 2, 0.05, 3, 0, cnt) == -1
    assert lib.amvs_depth_normals(h, n, d, c, 0, K, P, 1.0, 2, 0.05, 3, 0, None) == -1
    # the refused calls changed nothing: the cloud is still there and the good call still restates
    check_case(eng, case)


# ------------------------------------------------------------------------------------------ the classes ---
def _scene_inputs():
    sc = ni.scene(ni.SCENE_SMALL)
    return sc, sc.images(), dict(sc.poses)


def _spy_on_cloud_normals(obj, patch):
    """Record the arguments of obj._cloud_normals, which still runs."""
    seen = {}
    inner = obj._cloud_normals

    def spy(*args):
        seen["args"] = args
        return inner(*args)
    patch.setattr(obj, "_cloud_normals", spy)
    return seen


def _check_class(obj, make, images, poses, monkeypatch, capsys, held_maps, min_confidence, **fit):
    """reconstruct(with_normals=True) of `obj`: the plain call's points and colours, the restatement's normals for those
    points on the maps the call held (held_maps turns the arguments of _cloud_normals into (depth, conf, cameras)), the
    line it prints, and a plain call afterwards that is the call of a fresh object."""
    plain = obj.reconstruct(images, poses)
    capsys.readouterr()
    with monkeypatch.context() as patch:
        seen = _spy_on_cloud_normals(obj, patch)
        points, colors, normals = obj.reconstruct(images, poses, with_normals=True, **fit)
    said = [ln for ln in capsys.readouterr().out.splitlines() if "Normals:" in ln]
    assert len(plain) == 2 and np.array_equal(points, plain[0]) and np.array_equal(colors, plain[1])
    assert normals.shape == (len(points), 3) and normals.dtype == np.float32 and len(points) > 200
    depth, conf, cams = held_maps(seen["args"])
    maps, _, _ = nr.fit_normals_np(depth, conf, obj.K_scaled, cams, min_confidence, fit.get("normal_radius", 2),
                                   fit.get("normal_jump", 0.05), 3, True)
    want = nr.cloud_normals_np(points, depth, maps, obj.K_scaled, cams, 0.01, 1)
    assert same(normals, want[0]) and want[2] > 100
    assert len(said) == 1 and f"{want[2]:,} of {len(points):,} points" in said[0]
    again, fresh = obj.reconstruct(images, poses), make().reconstruct(images, poses)
    assert len(again) == 2 and np.array_equal(again[0], fresh[0]) and np.array_equal(again[1], fresh[1])
    assert np.array_equal(again[0], plain[0])
    return seen["args"]


@pytest.mark.parametrize("mode, path", [("exact", "resident"), ("fast", "resident"), ("exact", "host maps"), ("exact", "host fusion")])
def test_patchmatch_reconstruct_with_normals(amvs_mod, monkeypatch, capsys, mode, path):
    """The three ways the maps and the cloud reach the normals: device tensors and the cloud of the device fusion; host maps
    (as without PyTorch) and the cloud of the device fusion; host maps and the host fusion's cloud, uploaded first."""
    from amvs import parallel
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    sc, images, poses = _scene_inputs()
    if path == "host maps":
        monkeypatch.setattr(parallel, "_torch_cuda", lambda: None)

    def make():
        return PatchMatchMVS(sc.camera, scale=1.0, patch_size=7, num_iterations=3, num_samples=4, min_views=2, seed=5, device=0,
                             mode=mode, device_fusion=path != "host fusion")

    def held_maps(args):
        kind, data, _ = args[2]
        assert kind == ("resident" if path == "resident" else "host")
        if kind == "resident":
            n, (H, W) = len(data.ref_ids), data.shape
            ids = list(data.ref_ids)
            depth, conf = data.depth.cpu().numpy().reshape(n, H, W), data.confidence.cpu().numpy().reshape(n, H, W)
        else:
            ids = list(data)
            depth, conf = np.stack([data[i].depth for i in ids]), np.stack([data[i].confidence for i in ids])
        return depth, conf, [(poses[i].R, poses[i].t) for i in ids]
    pm = make()
    _check_class(pm, make, images, poses, monkeypatch, capsys, held_maps, 2, normal_radius=2)
    assert pm._cloud_resident == (path != "host fusion")


@pytest.mark.parametrize("path", ["one batch", "two batches", "two batches, host maps", "host filter"])
def test_stereo_reconstruct_with_normals(amvs_mod, monkeypatch, capsys, path):
    """The resident maps of one sweep batch; two batches (one view given a neighbour fewer) collected in device tensors and,
    as without PyTorch, in host arrays; and the outlier filter on the host, whose cloud is uploaded first."""
    from amvs import parallel
    from amvs.core.dense_stereo import DenseStereoReconstructor
    sc, images, poses = _scene_inputs()
    if path == "two batches, host maps":
        monkeypatch.setattr(parallel, "_torch_cuda", lambda: None)

    def make():
        rec = DenseStereoReconstructor(sc.camera, scale=1.0, num_depths=32, min_views=2, device=0,
                                       device_filter=path != "host filter")
        if path.startswith("two batches"):
            inner = rec._find_neighbors
            rec._find_neighbors = lambda ref, *a, **k: inner(ref, *a, **k)[:2 if ref == 1 else None]
        return rec

    def held_maps(args):
        eng, maps = args[0], args[3]
        n = len(maps["poses"])
        assert set(maps) == {"one batch": {"poses"}, "host filter": {"poses"}, "two batches": {"poses", "device_ptrs", "tensors"},
                             "two batches, host maps": {"poses", "depth", "conf"}}[path]
        if "tensors" in maps:
            depth, conf = (t.cpu().numpy() for t in maps["tensors"])
        elif "depth" in maps:
            depth, conf = maps["depth"], maps["conf"]
        else:
            depth, conf = eng.fetch_sweep_maps(0, n)
        return depth.reshape(n, eng.H, eng.W), conf.reshape(n, eng.H, eng.W), maps["poses"]
    rec = make()
    _check_class(rec, make, images, poses, monkeypatch, capsys, held_maps, 1.5, normal_radius=3, normal_jump=0.1)
    assert rec._cloud_resident == (path != "host filter")
    held = [k for k, v in vars(rec).items() if isinstance(v, dict) and ("tensors" in v or "depth" in v)]
    assert not held and not hasattr(rec, "_normal_maps")       # no map outlives the call


def test_with_normals_is_refused_under_a_process_group_of_several_ranks(amvs_mod, monkeypatch):
    from amvs import parallel
    from amvs.core.dense_stereo import DenseStereoReconstructor
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    sc, images, poses = _scene_inputs()
    monkeypatch.setattr(parallel, "rank_world", lambda group: (0, 2))
    for obj in (PatchMatchMVS(sc.camera, scale=1.0, device=0), DenseStereoReconstructor(sc.camera, scale=1.0, device=0)):
        with pytest.raises(NotImplementedError):
            obj.reconstruct(images, poses, with_normals=True)
