"""PatchMatch and plane sweep on images where the NCC degenerates (tests/degenerate_images.py): flat areas, saturation,
black borders, a constant source view, a checkerboard against flat sources and non-8-bit flat areas.

On a flat window the reference's variance is rounding noise, often negative, so the PatchMatch cost is NaN and the
plane sweep's NCC is NaN or follows the sign of a rounded covariance.  The kernels have their own code for these
values (the lean square root / reciprocal and their fall-backs, the NaN-aware selection, the confidence test, the
plane sweep's squared vote gates); the parity suites elsewhere never reach it because make_scene's texture keeps
every window well conditioned.

Bar: BIT-EXACT against the CPU oracle (NaN equal to NaN) in both arithmetic modes; every degenerate test also
asserts that the oracle side shows the degeneracy the test is for.
"""
import numpy as np
import pytest

import degenerate_images as di

pytestmark = pytest.mark.gpu

PM_CASES = 24
SWEEP_CASES = 24


@pytest.fixture(scope="module", autouse=True)
def _oracle_threads():
    from oracle import oracle
    oracle.set_threads(16)


def _eq(a, b, what):
    a = np.asarray(a)
    b = np.asarray(b)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} elements differ " \
                       f"(first at {np.argwhere(~same)[0]}: {a[~same][0]!r} vs {b[~same][0]!r})"


def _mixed_depth(case, ref, seed):
    """Random depths over the left half, the ground truth over the right half."""
    sc = case.scene
    rng = np.random.default_rng(seed)
    d = np.exp(rng.uniform(np.log(sc.depth_min), np.log(sc.depth_max), (case.H, case.W))).astype(np.float32)
    d[:, case.W // 2:] = sc.depths[ref][:, case.W // 2:]
    return d


# ------------------------------------------------------------------ primitives ----
# (content, code): the classes of degenerate_images.py; the flat codes are those with the most NaN costs (26, 230)
# and the exact zeros of black (0)
PRIM_CONTENT = [("flat", 26), ("flat", 230), ("flat", 0), ("saturated", None), ("border", None),
                ("const_source", 128), ("checker", 230)]
# exact mode on its packed 8-bit maps, the same with the f32 sampling forced, the fast mode; float images (exact)
PRIM_VARIANTS = ["exact", "exact-f32", "fast"]
PRIM_K = (3, 5, 7, 11, 13, 21, 31)      # compiled, compiled (13, 21) and run-time k (31)


def _primitives(case, mode, force_f32, what):
    """box_stats, eval_cost, confidence, propagate_step (4 offsets) and refine_step against the oracle, for every k of
    PRIM_K with S cycling through 2, 4, 6.  Returns the oracle's reach: (NaN cost on the flat area seen,
    exact-zero reference variance seen)."""
    from oracle import oracle
    sc = case.scene
    ref = case.ref
    others = [i for i in range(case.n) if i != ref]
    nan_flat = zero_var = False
    with case.engine(mode) as eng:
        if force_f32:
            eng.set_sampling(True)
        for j, k in enumerate(PRIM_K):
            S = (2, 4, 6)[j % 3]
            srcs = others[:S] if j % 2 == 0 else others[::-1][:S]
            tag = f"{what} k{k} S{S} srcs {srcs}"
            m, v = eng.box_stats(ref, k)
            om, ov = oracle.box_stats(case.grays[ref], k)
            _eq(m, om, f"{tag}: box mean")
            _eq(v, ov, f"{tag}: box var")
            zero_var |= bool((ov == 0).any())
            ctx = case.oracle_ctx(ref, srcs, k, mode)
            depth = _mixed_depth(case, ref, k)
            cost = eng.eval_cost(ref, srcs, k, depth)
            ocost = ctx.patch_cost(depth)
            _eq(cost, ocost, f"{tag}: eval_cost")
            nan_flat |= bool(np.isnan(ocost[case.flat[ref]]).any()) if case.flat[ref].any() else False
            _eq(eng.confidence(ref, srcs, k, depth), ctx.confidence(depth), f"{tag}: confidence")
            # the steps start from a state with NaN costs where the oracle has them
            rng = np.random.default_rng(k)
            normal = rng.normal(size=(case.H, case.W, 3)).astype(np.float32)
            normal[..., 2] = -np.abs(normal[..., 2]) - 0.5
            normal /= np.linalg.norm(normal, axis=-1, keepdims=True)
            normal = normal.astype(np.float32)
            c0 = ctx.patch_cost(depth)
            for oy, ox in ((1, 0), (0, 1), (-1, 0), (0, -1)):
                got = eng.propagate_step(ref, srcs, k, depth, normal, c0, oy, ox, sc.depth_min)
                want = ctx.propagate_step(depth, normal, c0, oy, ox, sc.depth_min)
                for a, b, name in zip(got, want, ("depth", "normal", "cost")):
                    _eq(a, b, f"{tag}: propagate ({oy},{ox}) {name}")
            d, n, c = depth, normal, c0
            od, on, oc = d, n, c
            for draw in (1, 2):
                d, n, c = eng.refine_step(ref, srcs, k, d, n, c, 11, ref, draw, np.float32(2.0), np.float32(0.5),
                                          sc.depth_min, sc.depth_max)
                u, nz = oracle.rng_fill(11, ref, draw, case.H * case.W)
                od, on, oc = ctx.refine_step(od, on, oc, u, nz, 2.0, 0.5, sc.depth_min, sc.depth_max)
                for a, b, name in zip((d, n, c), (od, on, oc), ("depth", "normal", "cost")):
                    _eq(a, b, f"{tag}: refine draw {draw} {name}")
            ctx.close()
    return nan_flat, zero_var


@pytest.mark.timeout(120)
@pytest.mark.parametrize("variant", PRIM_VARIANTS)
@pytest.mark.parametrize("content,code", PRIM_CONTENT)
def test_primitives_on_degenerate_content(content, code, variant):
    case = di.make_case(content, 7, 72, 96, seed=3, ref=2, code=code, rect_frac=0.6)
    mode = "fast" if variant == "fast" else "exact"
    nan_flat, zero_var = _primitives(case, mode, variant == "exact-f32", f"{variant} {case.desc}")
    # reach: the flat rectangle's windows give NaN costs; black and clipped areas give exactly zero variance
    if content == "flat" and code != 0:
        assert nan_flat, f"{variant} {case.desc}: the oracle shows no NaN cost on the flat rectangle"
    if content in ("border", "saturated") or code == 0:
        assert zero_var, f"{variant} {case.desc}: the oracle shows no exactly-zero reference variance"


@pytest.mark.timeout(120)
@pytest.mark.parametrize("seed", [4, 9])
def test_primitives_on_float_images(seed):
    """Non-8-bit images: the exact mode samples the f32 images (the float content's flat area is off the code grid)."""
    case = di.make_case("float", 7, 72, 96, seed=seed, ref=2, rect_frac=0.6)
    with case.engine() as eng:
        assert eng.sampling_mode() == "f32"
    nan_flat, _ = _primitives(case, "exact", False, f"float {case.desc}")
    assert nan_flat, f"{case.desc}: the oracle shows no NaN cost on the flat rectangle"


# ------------------------------------------------------------------ PatchMatch ----
def _run_pm(case, c, refs, srcs):
    from amvs.engine import make_pm_params
    sc = case.scene
    with case.engine(c["mode"]) as eng:
        if c.get("split"):
            eng.set_split_tuning(*c["split"])
        kw = dict(tile_rows=c["rows"], views_per_launch=c["vpl"], schedule=c["schedule"])
        if c.get("one_per_call"):
            for it in range(c["iters"]):
                p = make_pm_params(c["k"], 1, c["samples"], sc.depth_min, sc.depth_max, first_iteration=it,
                                   confidence=it == c["iters"] - 1, **kw)
                out = eng.patchmatch(refs, srcs, p, c["pm_seed"])
            return out
        p = make_pm_params(c["k"], c["iters"], c["samples"], sc.depth_min, sc.depth_max, **kw)
        return eng.patchmatch(refs, srcs, p, c["pm_seed"])


def _pm_case(case, c, refs, srcs):
    """Every reference view against the oracle; returns the oracle's NaN fraction of the cost at its final depth, per
    reference view."""
    sc = case.scene
    what = f"{case.desc}: " + ", ".join(f"{k}={c[k]}" for k in ("mode", "k", "S", "iters", "samples", "schedule", "split",
                                                             "rows", "vpl", "one_per_call", "pm_seed") if k in c)
    d, nrm, cf = _run_pm(case, c, refs, srcs)
    nan = []
    for i, r in enumerate(refs):
        ctx = case.oracle_ctx(r, srcs[i], c["k"], c["mode"])
        od, on, oc = ctx.patchmatch(c["iters"], c["samples"], sc.depth_min, sc.depth_max, c["pm_seed"], r)
        _eq(d[i], od, f"{what} view {r} depth")
        _eq(nrm[i], on, f"{what} view {r} normal")
        _eq(cf[i], oc, f"{what} view {r} confidence")
        nan.append(np.isnan(ctx.patch_cost(od)).mean())
        ctx.close()
    return nan


@pytest.mark.timeout(120)
@pytest.mark.parametrize("content,code,mode,k,S,schedule,one_per_call", di.PM_FIXED)
def test_patchmatch_fixed_degenerate_cases(content, code, mode, k, S, schedule, one_per_call):
    case = di.make_case(content, 5, 96, 128, seed=3, ref=2, code=code)
    c = dict(mode=mode, k=k, S=S, iters=3, samples=3, schedule=schedule, split=(2, 4, 0) if schedule == "split" else None,
             rows=0, vpl=0, one_per_call=one_per_call, pm_seed=7)
    refs = [2, 0]
    srcs = [[1, 3, 0, 4][:S], [1, 2, 3, 4][:S]]
    nan = _pm_case(case, c, refs, srcs)[0]
    # reach: the final depths of view 2 leave NaN costs (the state the NaN-aware selection keeps)
    assert nan >= 0.05, f"{case.desc} {mode} k{k}: only {nan:.1%} NaN cost at the oracle's final depth"


@pytest.mark.timeout(300)
def test_patchmatch_random_degenerate_cases():
    """PM_CASES seeded draws of draw_pm_case; every view of every case against the oracle.  Reach: a quarter of the
    cases end with NaN costs at the oracle's final depth."""
    nans = []
    for i in range(PM_CASES):
        rng = np.random.default_rng([20261016, i])
        c = di.draw_pm_case(rng)
        case = di.case_from_draw(c)
        refs = list(range(c["n"]))
        srcs = [[int(j) for j in rng.permutation([j for j in refs if j != r])[:c["S"]]] for r in refs]
        nans.append(max(_pm_case(case, c, refs, srcs)))
    assert np.mean(np.array(nans) > 0) >= 0.25, f"NaN cost fractions at the oracle's final depths: {nans}"


# ------------------------------------------------------------------ plane sweep ----
def _sweep_case(case, c, refs, nbrs, depths):
    """Plane sweep of `refs` (one call per view, or plane_sweep_batch) against the oracle; returns the oracle's
    confidence maps."""
    what = f"{case.desc}: " + ", ".join(f"{k}={c[k]}" for k in ("mode", "k", "S", "D", "thresh", "rows", "ppw", "batch"))
    with case.engine(c["mode"]) as eng:
        eng.set_sweep_tuning(c["rows"], c["ppw"])
        if c["batch"]:
            eng.plane_sweep_batch(refs, nbrs, depths, c["k"], c["thresh"])
            dm, cf = eng.fetch_sweep_maps(0, len(refs))
        else:
            out = [eng.plane_sweep(r, nb, depths, c["k"], c["thresh"]) for r, nb in zip(refs, nbrs)]
            dm, cf = [o[0] for o in out], [o[1] for o in out]
    confs = []
    for i, (r, nb) in enumerate(zip(refs, nbrs)):
        ctx = case.oracle_ctx(r, nb, c["k"], c["mode"])
        od, oc = ctx.plane_sweep(depths, c["thresh"])
        ctx.close()
        _eq(dm[i], od, f"{what} view {r} depth")
        _eq(cf[i], oc, f"{what} view {r} confidence")
        confs.append(oc)
    return confs


def _sweep_ncc_nan(case, ref, nbrs, k, depths):
    """Whether the reference's NCC (dense_stereo.py:333-345) is NaN somewhere for some plane and source."""
    from oracle import oracle
    ctx = case.oracle_ctx(ref, nbrs, k)
    try:
        for z in depths:
            for s in range(len(nbrs)):
                sampled, _ = ctx.sample(s, np.full((case.H, case.W), z, np.float32))
                if np.isnan(oracle.ncc(case.grays[ref], sampled, k, 1)).any():
                    return True
    finally:
        ctx.close()
    return False


@pytest.mark.timeout(120)
@pytest.mark.parametrize("content,code,mode,k,thresh", di.SWEEP_FIXED)
def test_plane_sweep_fixed_degenerate_cases(content, code, mode, k, thresh):
    case = di.make_case(content, 5, 96, 128, seed=3, ref=2, code=code)
    depths = di.sweep_depths(case.scene, 24)
    c = dict(mode=mode, k=k, S=4, D=24, thresh=thresh, rows=0, ppw=0, batch=False)
    confs = _sweep_case(case, c, [2], [[1, 3, 0, 4]], depths)
    if content == "checker":
        # reach: the checkerboard against a flat source makes x = var1 var2 + 1e-8 negative: NaN NCC
        assert _sweep_ncc_nan(case, 2, [1, 3, 0, 4], k, depths), f"{case.desc} k{k}: no NaN NCC in the oracle"
    elif content in ("flat", "float") and thresh == 0:
        # reach: at threshold 0 a flat window's vote follows the sign of the rounded covariance
        votes = confs[0][case.flat[2]].mean()
        assert 0.0 < votes < 4.0, f"{case.desc} {mode} k{k} thr {thresh}: flat-area votes {votes}"


@pytest.mark.timeout(300)
def test_plane_sweep_random_degenerate_cases():
    """SWEEP_CASES seeded draws of draw_sweep_case, one or two reference views each, against the oracle."""
    for i in range(SWEEP_CASES):
        rng = np.random.default_rng([20261017, i])
        c = di.draw_sweep_case(rng)
        case = di.case_from_draw(c)
        refs = [0, 1] if c["n"] > 3 else [0]
        nbrs = [[int(j) for j in rng.permutation([j for j in range(c["n"]) if j != r])[:c["S"]]] for r in refs]
        _sweep_case(case, c, refs, nbrs, di.sweep_depths(case.scene, c["D"]))


# ------------------------------------------------------------------ end to end ----
@pytest.mark.timeout(240)
@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_patchmatch_reconstruct_on_degenerate_images_equals_an_oracle_backed_run(mode, capsys):
    """PatchMatchMVS.reconstruct on BGR images with flat areas, a constant view and black borders, against the same
    pipeline with every device step replaced (as test_hip_workload_parity.py::
    test_cli_default_reconstruct_equals_an_oracle_backed_run): point for point."""
    import amvs
    from amvs.core.imageprep import prepare_views
    from oracle import oracle
    n, h, w = 6, 288, 384                                    # processed at 72 x 96
    case = di.make_case("flat", n, h, w, seed=77, code=230)
    rng = np.random.default_rng(5)
    codes = np.stack([np.round(g * 255.0).astype(np.uint8) for g in case.grays])
    codes, _ = di.apply_border(codes, rng)
    codes[4] = 26
    colors = di.colors_of(codes)
    poses = case.poses()
    cam = amvs.Camera(K=case.scene.camera.K.copy(), dist=np.zeros(5))
    pm = amvs.PatchMatchMVS(cam, scale=0.25, num_iterations=2, num_samples=3, min_views=2, seed=5, mode=mode)
    pts, cols = pm.reconstruct([{"image": c} for c in colors], poses)
    capsys.readouterr()
    ids = sorted(poses)
    proc = dict(zip(ids, prepare_views([colors[i] for i in ids], 0.25)))
    K32 = pm.K_scaled.astype(np.float32)
    maps, nan = {}, []
    for slot, r in enumerate(ids):
        srcs = pm._select_source_views(r, ids, poses, k=4)
        ctx = oracle.ViewContext(K32, proc[r]["gray"], poses[r].R, poses[r].t, [proc[i]["gray"] for i in srcs],
                                 [poses[i].R for i in srcs], [poses[i].t for i in srcs], pm.patch_size, mode=mode)
        d, nr, cf = ctx.patchmatch(2, 3, pm.depth_min, pm.depth_max, 5, slot)
        nan.append(np.isnan(ctx.patch_cost(d)).mean())
        maps[r] = amvs.DepthNormalMap(depth=d, normal=nr, confidence=cf)
        ctx.close()
    want_p, want_c = pm._fuse_depth_maps(maps, proc, poses)
    assert len(want_p) > 0, "the scene must fuse some points for the comparison to mean anything"
    want_p, want_c = pm._filter_points(want_p, want_c)
    assert max(nan) > 0.0, f"{mode}: the oracle's final costs have no NaN ({nan})"
    assert pts.shape == want_p.shape and np.array_equal(pts, want_p), \
        f"{mode} {case.desc}: clouds differ ({len(pts)} vs {len(want_p)} points)"
    assert np.array_equal(cols, want_c)


@pytest.mark.timeout(240)
@pytest.mark.parametrize("content,code", [("flat", 230), ("saturated", None)])
def test_stereo_reconstruct_on_degenerate_images_device_filter_equals_sklearn(content, code):
    """DenseStereoReconstructor.reconstruct: the device filter equals the scikit-learn one on degenerate images, whose
    flat areas give many coincident points (kNN ties, long voxel runs)."""
    pytest.importorskip("sklearn.neighbors")
    from amvs.core.dense_stereo import DenseStereoReconstructor
    case = di.make_case(content, 5, 120, 160, seed=21, code=code)
    images = case.images()
    clouds = []
    for device_filter in (True, False):
        rec = DenseStereoReconstructor(case.scene.camera, scale=1.0, device_filter=device_filter)
        clouds.append(rec.reconstruct(images, case.poses(), max_pairs=30))
    (p_dev, c_dev), (p_host, c_host) = clouds
    assert len(p_host) > 100, f"{case.desc}: only {len(p_host)} points"
    assert np.array_equal(p_dev, p_host) and np.array_equal(c_dev, c_host), f"{case.desc}: clouds differ"
