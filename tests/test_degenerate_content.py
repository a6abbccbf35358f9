"""CPU side of tests/test_hip_degenerate.py (no GPU needed).

The helper tests/degenerate_images.py makes what it claims; the oracle still shows, on the GPU file's standard cases,
the degeneracy those cases are there for (so a later change to the helper cannot silently lose it); and the oracle
obeys the reference's NaN rules in its steps (mvs_patchmatch.py:452-455, :486-489: better = new < cost).
"""
import numpy as np
import pytest

import degenerate_images as di


@pytest.fixture(scope="module", autouse=True)
def _oracle_threads():
    from oracle import oracle
    oracle.set_threads(16)


# ------------------------------------------------------------------ the helper ----
@pytest.mark.timeout(60)
@pytest.mark.parametrize("content", di.CLASSES)
def test_helper_makes_what_it_claims(content):
    a = di.make_case(content, 5, 40, 56, seed=11, ref=1, code=230)
    b = di.make_case(content, 5, 40, 56, seed=11, ref=1, code=230)
    for ga, gb in zip(a.grays, b.grays):
        assert ga.dtype == np.float32 and np.array_equal(ga, gb), f"{a.desc}: not deterministic per seed"
    for ca, cb in zip(a.colors, b.colors):
        assert ca.dtype == np.uint8 and ca.shape == (40, 56, 3) and np.array_equal(ca, cb)
    assert a.is_u8() == (content != "float"), f"{a.desc}: 8-bit exactness"
    g = np.stack(a.grays)
    if content != "texture":
        assert a.flat.any(), a.desc
    if content == "flat":
        assert np.all(g[a.flat] == np.float32(230) / np.float32(255)), a.desc
        assert np.array_equal(a.flat[0], a.flat[3]), "the rectangle is at the same place in every view"
    elif content == "saturated":
        codes = np.round(g * 255)
        assert (codes == 0).any() and (codes == 255).any() and np.array_equal(a.flat, (codes == 0) | (codes == 255))
    elif content == "border":
        assert np.all(g[a.flat] == 0.0)
        for v in range(a.n):                                     # every view has a full black row or column
            f = a.flat[v]
            assert f[0].all() or f[-1].all() or f[:, 0].all() or f[:, -1].all(), f"view {v}"
    elif content == "const_source":
        views = [v for v in range(a.n) if a.flat[v].all()]
        assert len(views) == 1 and views[0] != a.ref and np.all(g[views[0]] == np.float32(230) / np.float32(255))
    elif content == "checker":
        rect = np.any(a.flat, axis=0)
        assert set(np.unique(np.round(g[a.ref][rect] * 255))) == {0.0, 255.0}
        assert np.all(g[[v for v in range(a.n) if v != a.ref]][:, rect] == np.float32(230) / np.float32(255))
    elif content == "float":
        vals = g[a.flat]
        assert np.all(vals == vals[0]) and np.round(vals[0] * 255) / np.float32(255) != vals[0]
    # another seed gives other images
    c = di.make_case(content, 5, 40, 56, seed=12, ref=1, code=230)
    assert not all(np.array_equal(x, y) for x, y in zip(a.grays, c.grays))


@pytest.mark.timeout(30)
def test_draws_are_deterministic_and_cover_the_space():
    pm = [di.draw_pm_case(np.random.default_rng([20261016, i])) for i in range(200)]
    assert pm[:5] == [di.draw_pm_case(np.random.default_rng([20261016, i])) for i in range(5)]
    assert {c["k"] for c in pm} >= {3, 13, 21, 31} and max(c["k"] for c in pm) == 31
    assert {c["schedule"] for c in pm} == {"auto", "paired", "view-major", "split"}
    assert all(c["mode"] == "fast" for c in pm if c["schedule"] == "split")
    assert not any(c["one_per_call"] for c in pm if c["schedule"] == "split") and any(c["one_per_call"] for c in pm)
    assert {c["content"] for c in pm} == set(di.DEGENERATE)
    sw = [di.draw_sweep_case(np.random.default_rng([20261017, i])) for i in range(200)]
    assert min(c["D"] for c in sw) < 32 < max(c["D"] for c in sw)
    assert {c["thresh"] for c in sw} == {0.8, 0.3, 2.0 ** -10, 0.0005, 0.0, -0.3, 1.5}
    assert any(c["batch"] for c in sw) and {c["rows"] for c in sw} == {0, 5, 13, 32, 47, 64}


# ------------------------------------------------------------------ reach of the standard cases ----
@pytest.mark.timeout(60)
def test_oracle_reach_of_the_fixed_patchmatch_cases():
    """Every fixed PatchMatch case of the GPU file leaves >= 5 % NaN costs at the oracle's final depth of view 2 (the
    texture of make_scene alone: none)."""
    for content, code, mode, k, S, _, _ in di.PM_FIXED:
        case = di.make_case(content, 5, 96, 128, seed=3, ref=2, code=code)
        sc = case.scene
        ctx = case.oracle_ctx(2, [1, 3, 0, 4][:S], k, mode)
        d, _, _ = ctx.patchmatch(3, 3, sc.depth_min, sc.depth_max, 7, 2)
        nan = np.isnan(ctx.patch_cost(d)).mean()
        ctx.close()
        assert nan >= 0.05, f"{case.desc} {mode} k{k}: {nan:.1%} NaN cost"
    case = di.make_case("texture", 5, 96, 128, seed=3, ref=2)
    ctx = case.oracle_ctx(2, [1, 3, 0, 4], 5, "fast")
    d, _, _ = ctx.patchmatch(3, 3, case.scene.depth_min, case.scene.depth_max, 7, 2)
    assert not np.isnan(ctx.patch_cost(d)).any()


@pytest.mark.timeout(60)
def test_oracle_reach_of_the_fixed_sweep_cases():
    """Checkerboard cases: NaN NCC (x = var1 var2 + 1e-8 < 0).  Flat cases at threshold 0: flat-area votes strictly
    between none and all -- and in both modes, so neither an always-voting nor a never-voting kernel passes."""
    from oracle import oracle
    modes = set()
    for content, code, mode, k, thresh in di.SWEEP_FIXED:
        case = di.make_case(content, 5, 96, 128, seed=3, ref=2, code=code)
        depths = di.sweep_depths(case.scene, 24)
        if content == "checker":
            ctx = case.oracle_ctx(2, [1, 3, 0, 4], k)
            nan = 0
            for z in depths:
                for s in range(4):
                    sampled, _ = ctx.sample(s, np.full((case.H, case.W), z, np.float32))
                    nan += int(np.isnan(oracle.ncc(case.grays[2], sampled, k, 1)).sum())
            ctx.close()
            assert nan > 0, f"{case.desc} k{k}: no NaN NCC"
        elif content in ("flat", "float") and thresh == 0:
            ctx = case.oracle_ctx(2, [1, 3, 0, 4], k, mode)
            _, conf = ctx.plane_sweep(depths, thresh)
            ctx.close()
            votes = float(conf[case.flat[2]].mean())
            assert 0.0 < votes < 4.0, f"{case.desc} {mode} k{k}: flat-area votes {votes}"
            modes.add(mode)
    assert modes == {"exact", "fast"}


# ------------------------------------------------------------------ the oracle's NaN rules ----
@pytest.mark.timeout(60)
@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_oracle_steps_keep_nan_hypotheses_and_never_make_nan(mode):
    """better = new_cost < best_cost (mvs_patchmatch.py:452, :486) is false for a NaN on either side: a pixel whose
    cost is NaN keeps its depth, normal and cost through propagate_step and refine_step, and a finite cost never
    becomes NaN."""
    from oracle import oracle
    case = di.make_case("flat", 5, 64, 80, seed=3, ref=2, code=230)
    sc = case.scene
    ctx = case.oracle_ctx(2, [1, 3, 0, 4], 5, mode)
    rng = np.random.default_rng(1)
    depth = np.exp(rng.uniform(np.log(sc.depth_min), np.log(sc.depth_max), (case.H, case.W))).astype(np.float32)
    depth[:, case.W // 2:] = sc.depths[2][:, case.W // 2:]
    normal = np.zeros((case.H, case.W, 3), np.float32)
    normal[..., 2] = -1.0
    cost = ctx.patch_cost(depth)
    nan = np.isnan(cost)
    assert nan.mean() > 0.05, f"{case.desc} {mode}: {nan.mean():.1%} NaN cost"
    steps = [("propagate", o) for o in ((1, 0), (0, 1), (-1, 0), (0, -1))] + [("refine", draw) for draw in (1, 2, 3)]
    for kind, arg in steps:
        if kind == "propagate":
            d, n, c = ctx.propagate_step(depth, normal, cost, arg[0], arg[1], sc.depth_min)
        else:
            u, nz = oracle.rng_fill(5, 2, arg, case.H * case.W)
            d, n, c = ctx.refine_step(depth, normal, cost, u, nz, 2.0, 0.5, sc.depth_min, sc.depth_max)
        what = f"{mode} {kind} {arg}"
        assert np.array_equal(d[nan], depth[nan]) and np.array_equal(n[nan], normal[nan]), f"{what}: NaN pixel moved"
        assert np.isnan(c[nan]).all(), f"{what}: a NaN cost was replaced"
        assert not np.isnan(c[~nan]).any(), f"{what}: a finite cost became NaN"
        moved = ~nan & (c != cost)
        assert np.all(c[moved] < cost[moved]), f"{what}: a cost grew"
        assert moved.any(), f"{what}: no pixel improved"
