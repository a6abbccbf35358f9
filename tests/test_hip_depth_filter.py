"""The cross-view depth-map filter on the device (csrc/amvs_depth_filter.hip and its entry point in
csrc/amvs_capi_cloud.hip) against the restatement of tests/depth_filter_restatement.py on the input family of
tests/depth_filter_inputs.py; tests/test_depth_filter_cpu.py shows on the CPU that the restatement's two forms agree and
that the family reaches every guard and edge.  Every comparison is bit for bit: depths as uint32, counts element for
element, no pixel left out."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_filter_inputs as fi  # noqa: E402
import depth_filter_restatement as fr  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


_RESTATED = {}                                   # restated once per (case, refine), built when a test first asks


def restated(case, refine=True):
    """(depth, count, (valid, kept)).  The small inputs with refine by the loops, the rest by the twin (the CPU test holds
    the two to each other for both)."""
    key = (case.name, refine)
    if key not in _RESTATED:
        form = fr.depth_filter if refine and not case.big else fr.depth_filter_np
        _RESTATED[key] = form(*case.args(refine=refine))[:3]
    return _RESTATED[key]


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


def params(case, refine=True):
    return dict(min_confidence=case.min_confidence, max_px=case.max_px, max_rel=case.max_rel, min_consistent=case.min_consistent,
                refine=refine, neighbours=case.neighbours)


def check(case, got, refine, what):
    want = restated(case, refine)
    depth, count, counts = got
    assert counts == want[2], f"{case.name}: counts {counts}, restatement {want[2]} ({what})"
    assert np.array_equal(count, want[1]), f"{case.name}: {int((count != want[1]).sum())} counts differ ({what})"
    assert same(depth, want[0]), f"{case.name}: {int((bits(depth) != bits(want[0])).sum())} depths differ ({what})"


def run_device(eng, case, refine, maps_on_device, out_on_device):
    """Engine.depth_filter with the maps in host arrays or device tensors and the outputs likewise -> (depth, count, counts)."""
    import torch
    kw = params(case, refine)
    if maps_on_device:
        d_t, c_t = on_device(case.depth, case.conf)
        kw["device_ptrs"] = (d_t.data_ptr(), c_t.data_ptr())
    else:
        kw.update(depth=case.depth, conf=case.conf)
    if not out_on_device:
        return eng.depth_filter(case.K, case.poses, **kw)
    od = torch.full(case.depth.shape, -7.0, dtype=torch.float32, device="cuda")
    oc = torch.full(case.depth.shape, -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    counts = eng.depth_filter(case.K, case.poses, out_ptrs=(od.data_ptr(), oc.data_ptr()), **kw)
    return od.cpu().numpy(), oc.cpu().numpy(), counts


@pytest.mark.parametrize("case", fi.family(), ids=lambda c: c.name)
def test_device_equals_restatement(engines, case):
    eng = engines(case.shape)
    for refine in (True, False):
        check(case, run_device(eng, case, refine, False, False), refine, f"host maps, refine {refine}")


@pytest.mark.parametrize("name", ["special_values", "order_matters", "scene_5_views", "scene_ragged_rows", "big_two_maps"])
def test_maps_and_outputs_in_device_memory_give_the_same(engines, name):
    case = fi.by_name(name)
    eng = engines(case.shape)
    for maps_on_device, out_on_device in ((True, True), (True, False), (False, True)):
        check(case, run_device(eng, case, True, maps_on_device, out_on_device), True,
              f"maps on the device {maps_on_device}, outputs on the device {out_on_device}")


# -------------------------------------------------------------------------------- the resident sweep maps ---
def _scene():
    from amvs.synthetic import make_scene
    return make_scene(5, 48, 64, seed=3)


@pytest.fixture(scope="module")
def swept(amvs_mod):
    """Plane-sweep batches left resident on a context of its own: (engine, sweep, K, poses); sweep() runs the batch again
    and returns host copies of its maps."""
    sc = _scene()
    n, H, W = 5, 48, 64
    with amvs_mod.Engine(H, W, n, sc.camera.K.astype(np.float32)) as eng:
        for i in range(n):
            eng.set_view(i, sc.grays[i], sc.poses[i].R, sc.poses[i].t)
        refs = [0, 1, 2, 3, 4]
        nbrs = [[1, 2], [0, 2], [1, 3], [2, 4], [3, 2]]
        depths = 1.0 / np.linspace(1 / sc.depth_max, 1 / sc.depth_min, 24)

        def sweep():
            eng.plane_sweep_batch(refs, nbrs, depths, 5, 0.6)
            depth, conf = eng.fetch_sweep_maps(0, n)
            return depth.reshape(n, H, W), conf.reshape(n, H, W)
        poses = [(sc.poses[i].R.astype(np.float64), sc.poses[i].t.astype(np.float64)) for i in refs]
        rel = float(np.max(np.abs(np.diff(depths)) / np.minimum(depths[:-1], depths[1:])))
        yield eng, sweep, sc.camera.K.astype(np.float64), poses, rel


@pytest.mark.parametrize("refine", [True, False])
def test_every_maps_where_and_out_where(swept, refine):
    """maps_where 0, 1, 2 times out_where 0, 1, and 2 where it is allowed: one restatement for all of them; in_place leaves
    in the resident maps what the scratch computation returns, and the steps that read resident maps then read it."""
    import torch
    eng, sweep, K, poses, rel = swept
    depth, conf = sweep()
    kw = dict(min_confidence=1.5, max_px=1.5, max_rel=rel, min_consistent=1, refine=refine)
    want = fr.depth_filter_np(depth, conf, K, np.linalg.inv(K), poses, None, 1.5, 1.5, rel, 1, refine)
    print(f"sweep maps: {want[2][1]} of {want[2][0]} valid pixels kept")
    assert want[2][1] > 200                       # (the sweep's maps are rough; enough pixels still agree)
    d_t, c_t = on_device(depth, conf)
    for where, maps in ((0, dict(depth=depth, conf=conf)), (1, dict(device_ptrs=(d_t.data_ptr(), c_t.data_ptr()))), (2, {})):
        got = eng.depth_filter(K, poses, **kw, **maps)
        assert got[2] == want[2] and np.array_equal(got[1], want[1]) and same(got[0], want[0]), f"maps_where {where}, out_where 0"
        od, oc = torch.full(depth.shape, -7.0, device="cuda"), torch.full(depth.shape, -7.0, device="cuda")
        torch.cuda.synchronize()
        counts = eng.depth_filter(K, poses, out_ptrs=(od.data_ptr(), oc.data_ptr()), **kw, **maps)
        assert counts == want[2] and np.array_equal(oc.cpu().numpy(), want[1]) and same(od.cpu().numpy(), want[0]), \
            f"maps_where {where}, out_where 1"
    # the inputs were not written
    assert same(d_t.cpu().numpy(), depth) and same(c_t.cpu().numpy(), conf)
    held = eng.fetch_sweep_maps(0, len(poses))
    assert same(held[0], depth) and same(held[1], conf)
    # in place
    assert eng.depth_filter(K, poses, in_place=True, **kw) == want[2]
    held = eng.fetch_sweep_maps(0, len(poses))
    assert same(held[0], want[0]) and np.array_equal(held[1], want[1])
    # ... and the normals' maps_where = 2 now reads the filtered pair
    normals, n = eng.depth_normals(K, poses, min_confidence=1.0, radius=1, jump=0.2, min_points=3)
    ref, m = eng.depth_normals(K, poses, min_confidence=1.0, radius=1, jump=0.2, min_points=3, depth=want[0], conf=want[1])
    assert n == m and same(normals, ref)


def test_errors_return_einval_and_the_context_stays_usable(swept):
    import torch
    from amvs.engine import AmvsError
    eng, sweep, K, poses, rel = swept
    depth, conf = sweep()
    n = len(poses)
    good = dict(min_confidence=1.5, max_px=1.5, max_rel=rel, min_consistent=1, refine=True, depth=depth, conf=conf)
    bad = [dict(max_px=0.0), dict(max_px=-1.0), dict(max_px=float("nan")), dict(max_px=float("inf")), dict(max_rel=0.0),
           dict(max_rel=float("nan")), dict(max_rel=float("inf")), dict(min_consistent=0), dict(min_consistent=-3),
           dict(neighbours=np.zeros((n, 0), np.int32)),                                   # n_nbr < 1 with a list
           dict(neighbours=np.array([[1], [0], [5], [0], [0]], np.int32)),                # outside -1 .. n - 1
           dict(neighbours=np.array([[1], [0], [-2], [0], [0]], np.int32)),
           dict(neighbours=np.array([[1], [1], [0], [0], [0]], np.int32)),                # its own row
           dict(neighbours=np.array([[1, 2], [0, 2], [3, 3], [0, 1], [0, 1]], np.int32))]  # repeated within a row
    for change in bad:
        with pytest.raises(AmvsError):
            eng.depth_filter(K, poses, **{**good, **change})
    with pytest.raises(AmvsError):                               # a resident batch of five maps, four asked for
        eng.depth_filter(K, poses[:4], min_confidence=1.5, max_rel=rel, min_consistent=1)
    with pytest.raises(AmvsError):                               # in place without resident inputs
        eng._chk(eng._lib.amvs_depth_filter(eng._h, n, depth.ctypes.data_as(C.c_void_p), conf.ctypes.data_as(C.c_void_p), 0,
                                            *_kp(K, poses), None, 0, 1.5, 1.5, rel, 1, 1, None, None, 2, (C.c_int64 * 2)()))
    lib, h = eng._lib, eng._h
    d, c = depth.ctypes.data_as(C.c_void_p), conf.ctypes.data_as(C.c_void_p)
    out = np.empty((2,) + depth.shape, np.float32)
    o0, o1 = out[0].ctypes.data_as(C.c_void_p), out[1].ctypes.data_as(C.c_void_p)
    Kp, Kip, Pp = _kp(K, poses)
    cnt = (C.c_int64 * 2)()
    tail = (None, 0, 1.5, 1.5, rel, 1, 1)
    for args in ((h, n, None, c, 0, Kp, Kip, Pp) + tail + (o0, o1, 0, cnt), (h, n, d, None, 0, Kp, Kip, Pp) + tail + (o0, o1, 0, cnt),
                 (h, n, d, c, 0, None, Kip, Pp) + tail + (o0, o1, 0, cnt), (h, n, d, c, 0, Kp, None, Pp) + tail + (o0, o1, 0, cnt),
                 (h, n, d, c, 0, Kp, Kip, None) + tail + (o0, o1, 0, cnt), (h, n, d, c, 0, Kp, Kip, Pp) + tail + (None, o1, 0, cnt),
                 (h, n, d, c, 0, Kp, Kip, Pp) + tail + (o0, None, 0, cnt), (h, n, d, c, 0, Kp, Kip, Pp) + tail + (o0, o1, 0, None),
                 (h, 0, d, c, 0, Kp, Kip, Pp) + tail + (o0, o1, 0, cnt), (h, n, d, c, 3, Kp, Kip, Pp) + tail + (o0, o1, 0, cnt),
                 (h, n, d, c, 0, Kp, Kip, Pp) + tail + (o0, o1, 3, cnt), (h, n, d, c, -1, Kp, Kip, Pp) + tail + (o0, o1, 0, cnt)):
        assert lib.amvs_depth_filter(*args) == -1
    # device outputs that overlap device inputs
    d_t, c_t = on_device(depth, conf)
    other = torch.empty_like(d_t)
    torch.cuda.synchronize()
    for od, oc in ((d_t, other), (other, c_t), (c_t, d_t), (other, other)):
        with pytest.raises(AmvsError):
            eng.depth_filter(K, poses, min_confidence=1.5, max_px=1.5, max_rel=rel, min_consistent=1,
                             device_ptrs=(d_t.data_ptr(), c_t.data_ptr()), out_ptrs=(od.data_ptr(), oc.data_ptr()))
    # more than 2^31 - 1 pixels: refused before anything is allocated
    import amvs
    with amvs.Engine(4096, 4096, 1, np.eye(3, dtype=np.float32)) as huge:
        big_n = 128
        assert huge._lib.amvs_depth_filter(huge._h, big_n, d, c, 0, Kp, Kip, np.zeros((big_n, 12)).ctypes.data_as(C.POINTER(C.c_double)),
                                           None, 0, 1.5, 1.5, rel, 1, 1, o0, o1, 0, cnt) == -1
    # the refused calls changed nothing: the good call still restates
    want = fr.depth_filter_np(depth, conf, K, np.linalg.inv(K), poses, None, 1.5, 1.5, rel, 1, True)
    got = eng.depth_filter(K, poses, **good)
    assert got[2] == want[2] and np.array_equal(got[1], want[1]) and same(got[0], want[0])
    resident = eng.fetch_sweep_maps(0, n)
    assert same(resident[0], depth) and same(resident[1], conf)


def _kp(K, poses):
    from amvs.engine import _poses64
    Kd = np.ascontiguousarray(K, np.float64).reshape(9)
    Ki = np.ascontiguousarray(np.linalg.inv(np.asarray(K, np.float64))).reshape(9)
    pp = _poses64(poses)
    _kp.keep = (Kd, Ki, pp)                       # (the arrays outlive the call that takes the pointers)
    dp = C.POINTER(C.c_double)
    return Kd.ctypes.data_as(dp), Ki.ctypes.data_as(dp), pp.ctypes.data_as(dp)


# ------------------------------------------------------------------------------------------ the classes ---
FILTER = dict(filter_px=2.0, filter_rel=0.05, filter_min_views=1, filter_refine=True)


def _host_maps(maps, poses):
    """(view ids, depth, conf, cameras, prepared images) of what PatchMatchMVS._reconstruct_maps returned."""
    kind, data, proc = maps
    if kind == "resident":
        ids, (H, W) = list(data.ref_ids), data.shape
        depth, conf = data.depth.cpu().numpy().reshape(len(ids), H, W), data.confidence.cpu().numpy().reshape(len(ids), H, W)
    else:
        ids = list(data)
        depth, conf = np.stack([data[i].depth for i in ids]), np.stack([data[i].confidence for i in ids])
    return ids, depth, conf, [(poses[i].R, poses[i].t) for i in ids], proc


@pytest.mark.parametrize("path, neighbours", [("resident", None), ("resident", 2), ("host maps", None), ("extended", 3)])
def test_patchmatch_reconstruct_with_the_geometric_filter(amvs_mod, monkeypatch, capsys, path, neighbours):
    """reconstruct(geometric_filter=True) -- also with normals, and reconstruct_mesh -- against the chain by hand:
    Engine.depth_filter on the maps the plain call holds (equal to the restatement), then the existing fusion, normals and
    TSDF with filter_min_views as threshold.  Off, the call is what it was."""
    from amvs import parallel
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    from amvs.core.utils import nearest_map_neighbours
    sc = _scene()
    images, poses = sc.images(), dict(sc.poses)
    if path == "host maps":
        monkeypatch.setattr(parallel, "_torch_cuda", lambda: None)

    def make():
        return PatchMatchMVS(sc.camera, scale=1.0, patch_size=7, num_iterations=3, num_samples=4, min_views=2, seed=5, device=0,
                             extended=path == "extended")
    fkw = dict(FILTER, filter_neighbours=neighbours)
    pm = make()
    plain = pm.reconstruct(images, poses)
    off = pm.reconstruct(images, poses, geometric_filter=False, **fkw)
    assert np.array_equal(plain[0], off[0]) and np.array_equal(plain[1], off[1]) and pm._filter_threshold is None
    _, _, maps = pm._reconstruct_maps(images, poses)
    assert maps[0] == ("host" if path == "host maps" else "resident")
    ids, depth, conf, cams, proc = _host_maps(maps, poses)
    assert len(ids) == 5
    # by hand
    eng = pm._engine
    rows = nearest_map_neighbours([poses[i].center for i in ids], neighbours)
    fd, fc, counts = eng.depth_filter(pm.K_scaled, cams, pm.min_views, 2.0, 0.05, 1, True, neighbours=rows, depth=depth, conf=conf)
    want = fr.depth_filter_np(depth, conf, pm.K_scaled, np.linalg.inv(pm.K_scaled), cams, rows, pm.min_views, 2.0, 0.05, 1, True)
    assert counts == want[2] and np.array_equal(fc, want[1]) and same(fd, want[0])
    cols = np.stack([proc[i]["color"] for i in ids])
    pts, rgb, raw = eng.fuse_filter(fd, fc, cols, np.linalg.inv(pm.K_scaled), cams, 1, do_filter=True)
    _, n_normals = eng.cloud_normals(pm.K_scaled, cams, 1, 2, 0.05, 3, 0.01, 1, depth=fd, conf=fc)
    nrm, _ = eng.fetch_cloud_normals(len(pts))
    print(f"{path}: {counts[1]} of {counts[0]} valid pixels kept, {raw} raw points, {len(pts)} points, {n_normals} with a normal; "
          f"plain {len(plain[0])} points")
    assert raw == counts[1] and len(pts) > 0
    origin, voxel, dims, trunc = pm._mesh_grid(pts, None, None, 4.0, 48)
    mesh = eng.tsdf_mesh(pm.K_scaled, cams, 1, origin, voxel, dims, trunc, depth=fd, conf=fc, colors_bgr=cols)
    # the class
    capsys.readouterr()
    got = pm.reconstruct(images, poses, geometric_filter=True, **fkw)
    said = [ln for ln in capsys.readouterr().out.splitlines() if "Geometric filter:" in ln]
    assert len(said) == 1 and f"{counts[1]:,} of {counts[0]:,} valid pixels" in said[0]
    assert len(got) == 2 and np.array_equal(got[0], pts) and np.array_equal(got[1], rgb) and pm._filter_threshold == 1
    got = pm.reconstruct(images, poses, geometric_filter=True, with_normals=True, **fkw)
    assert len(got) == 3 and np.array_equal(got[0], pts) and np.array_equal(got[1], rgb) and same(got[2], nrm)
    # reconstruct_mesh: the maps it fuses are the filtered pair, its threshold filter_min_views, its mesh the one by hand.
    # (The default mode's maps are wrong by multiples at this size, DESIGN.md section 9: the few dozen pixels that agree
    # give no surface, so only the extended mode's mesh is held to having faces.)
    from amvs.engine import Engine
    held = {}
    inner_maps, inner_tsdf = pm._reconstruct_maps, Engine.tsdf_integrate

    def spy_maps(*a, **k):
        out = inner_maps(*a, **k)
        held["maps"] = out[2]
        return out

    def spy_tsdf(self, K, cams_, min_views, *a, **k):
        held["threshold"] = min_views
        return inner_tsdf(self, K, cams_, min_views, *a, **k)
    with monkeypatch.context() as patch:
        patch.setattr(pm, "_reconstruct_maps", spy_maps)
        patch.setattr(Engine, "tsdf_integrate", spy_tsdf)
        got = pm.reconstruct_mesh(images, poses, geometric_filter=True, max_dim=48, **fkw)
    ids2, depth2, conf2, _, _ = _host_maps(held["maps"], poses)
    assert ids2 == ids and same(depth2, fd) and np.array_equal(conf2, fc) and held["threshold"] == 1
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, mesh))
    assert path != "extended" or len(mesh[1]) > 0
    # and a plain call afterwards is the call of a fresh object
    again, fresh = pm.reconstruct(images, poses), make().reconstruct(images, poses)
    assert np.array_equal(again[0], fresh[0]) and np.array_equal(again[1], fresh[1]) and np.array_equal(again[0], plain[0])
    assert pm._filter_threshold is None


@pytest.mark.parametrize("path, neighbours", [("one batch", None), ("one batch", 2), ("two batches", None), ("two batches, host maps", 3)])
def test_stereo_reconstruct_with_the_geometric_filter(amvs_mod, monkeypatch, capsys, path, neighbours):
    """The resident maps of one sweep batch filtered in place; two batches (one view given a neighbour fewer) collected in
    device tensors and, as without PyTorch, in host arrays.  By hand: the maps the plain call held through
    Engine.depth_filter (equal to the restatement), the existing back-projection with filter_min_views, the class's own
    outlier filter and voxel grid, and the normals from the filtered pair."""
    from amvs import parallel
    from amvs.core.dense_stereo import DenseStereoReconstructor
    from amvs.core.utils import nearest_map_neighbours
    sc = _scene()
    images, poses = sc.images(), dict(sc.poses)
    if path == "two batches, host maps":
        monkeypatch.setattr(parallel, "_torch_cuda", lambda: None)

    def make():
        rec = DenseStereoReconstructor(sc.camera, scale=1.0, num_depths=32, min_views=2, device=0)
        if path.startswith("two batches"):
            inner = rec._find_neighbors
            rec._find_neighbors = lambda ref, *a, **k: inner(ref, *a, **k)[:2 if ref == 1 else None]
        return rec
    rec = make()
    seen = {}
    inner = rec._sweep_and_backproject

    def spy(eng, jobs, processed, poses_, depths, H, W, **kw):
        out = inner(eng, jobs, processed, poses_, depths, H, W, **kw)
        maps = out[2]
        if maps is not None and "gfilter" in kw and kw["gfilter"] is None:
            n = len(maps["poses"])
            if "tensors" in maps:
                depth, conf = (t.cpu().numpy() for t in maps["tensors"])
            elif "depth" in maps:
                depth, conf = maps["depth"], maps["conf"]
            else:
                depth, conf = eng.fetch_sweep_maps(0, n)
            seen.update(depth=depth.reshape(n, H, W).copy(), conf=conf.reshape(n, H, W).copy(), cams=maps["poses"], planes=depths,
                        cols=np.stack([processed[j[0]]["color"] for j in jobs]), kind=set(maps))
        return out
    monkeypatch.setattr(rec, "_sweep_and_backproject", spy)
    plain = rec.reconstruct(images, poses, with_normals=True)
    assert seen["kind"] == {"one batch": {"poses"}, "two batches": {"poses", "device_ptrs", "tensors"},
                            "two batches, host maps": {"poses", "depth", "conf"}}[path]
    off = rec.reconstruct(images, poses, geometric_filter=False, filter_min_views=1, filter_neighbours=neighbours)
    assert np.array_equal(plain[0], off[0]) and np.array_equal(plain[1], off[1]) and rec._filter_threshold is None
    depth, conf, cams = seen["depth"], seen["conf"], seen["cams"]
    # by hand; filter_rel is left to its default, the largest relative plane spacing
    eng = rec._engine
    rel = rec.plane_spacing(seen["planes"])
    centers = [-np.asarray(R).T @ np.asarray(t) for R, t in cams]
    rows = nearest_map_neighbours(centers, neighbours)
    fd, fc, counts = eng.depth_filter(rec.K_scaled, cams, 1.5, 1.0, rel, 1, True, neighbours=rows, depth=depth, conf=conf)
    want = fr.depth_filter_np(depth, conf, rec.K_scaled, np.linalg.inv(rec.K_scaled), cams, rows, 1.5, 1.0, rel, 1, True)
    assert counts == want[2] and np.array_equal(fc, want[1]) and same(fd, want[0])
    _, total = eng.stereo_backproject(seen["cols"], np.linalg.inv(rec.K_scaled), cams, 1, depth=fd, conf=fc)
    assert total == counts[1] and total > 0
    pts, rgb = rec._filter_and_downsample_device(eng, total, voxel_size=0.02)
    if not rec._cloud_resident:                                  # (the outlier filter took the host path)
        eng.cloud_set(pts, rgb)
    _, n_normals = eng.cloud_normals(rec.K_scaled, cams, 1, 2, 0.05, 3, 0.01, 1, depth=fd, conf=fc)
    nrm, _ = eng.fetch_cloud_normals(len(pts))
    print(f"{path}: {counts[1]} of {counts[0]} valid pixels kept at relative depth {rel:.4f}, {len(pts)} points, {n_normals} with a "
          f"normal; plain {len(plain[0])} points")
    # the class
    capsys.readouterr()
    got = rec.reconstruct(images, poses, geometric_filter=True, filter_min_views=1, filter_neighbours=neighbours)
    said = [ln for ln in capsys.readouterr().out.splitlines() if "Geometric filter:" in ln]
    assert len(said) == 1 and f"{counts[1]:,} of {counts[0]:,} valid pixels" in said[0]
    assert len(got) == 2 and np.array_equal(got[0], pts) and np.array_equal(got[1], rgb) and rec._filter_threshold == 1
    got = rec.reconstruct(images, poses, geometric_filter=True, filter_min_views=1, filter_neighbours=neighbours, with_normals=True)
    assert len(got) == 3 and np.array_equal(got[0], pts) and np.array_equal(got[1], rgb) and same(got[2], nrm)
    again, fresh = rec.reconstruct(images, poses), make().reconstruct(images, poses)
    assert np.array_equal(again[0], fresh[0]) and np.array_equal(again[1], fresh[1]) and np.array_equal(again[0], plain[0])
    assert rec._filter_threshold is None


def test_the_geometric_filter_is_refused_under_a_process_group_of_several_ranks(amvs_mod, monkeypatch):
    from amvs import parallel
    from amvs.core.dense_stereo import DenseStereoReconstructor
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    sc = _scene()
    images, poses = sc.images(), dict(sc.poses)
    monkeypatch.setattr(parallel, "rank_world", lambda group: (0, 2))
    pm = PatchMatchMVS(sc.camera, scale=1.0, device=0)
    with pytest.raises(NotImplementedError):
        pm.reconstruct(images, poses, geometric_filter=True)
    with pytest.raises(NotImplementedError):
        pm.reconstruct_mesh(images, poses, geometric_filter=True)
    with pytest.raises(NotImplementedError):
        DenseStereoReconstructor(sc.camera, scale=1.0, device=0).reconstruct(images, poses, geometric_filter=True)
