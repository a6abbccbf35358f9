"""Every code path of the extended mode's kernels (csrc/amvs_extended.hip) against the float64 reference
(oracle/xpm_oracle.py, Ref64), with every reference view of each call compared.

Paths: the window cost for N = 3..7 taps per axis in 8-bit and float sampling (the float sampling both
forced with set_sampling(True) on 8-bit views and taken because the views are not 8-bit exact) and the
generic loop (patch 15, 31 and the window (9, 3) that does not fit); 2, 3, 5 and 6 sources; a ragged
image size and images smaller than the window; a subset of reference views in another order than their
slots; iterations 0, 1, 2, 3 and 6, num_refine 0 and 6, view propagation off.  Phases: xpm_init, the
eval hook, the view candidates, the red and the black half sweep (each from the GPU's own state before
it) and xpm_consistency.

TOLERANCE RULE.  The reference returns a decision margin per pixel (see oracle/xpm_oracle.py): the distance
of the closest validity decision from its threshold (pixels / relative) and, for a half sweep, the gap of
the closest comparison between two different planes, in units of the sum of their cost error bounds.  On
every pixel whose margin exceeds EPS_GEOM = 1e-3 (EPS_CONS = 1e-4 for the consistency count, whose
projections the kernel forms without an incremental chain) and whose sweep gaps exceed 1:
  * the same validity, i.e. the same +inf pattern;
  * |cost - reference| <= COST_ABS + COST_KAPPA * kappa * 2^-24, kappa the conditioning of the pixel's
    per-source NCCs (sum r^2 / var r + sum v^2 / var v): the kernels accumulate the window sums in float32
    (v_rcp_f32 / v_rsq_f32, FMAs), so their error grows with kappa.  Measured on the MI355X over every case
    below: at most 7.0 kappa 2^-24 (the float32 CPU restatement: 3.6), so COST_KAPPA = 32 leaves a factor
    of 4.5; the sweep gaps use the measured level GAP_KAPPA = 8;
  * a half sweep picks the same plane: depth within 1e-5 relative, normal within 1e-5, and a winner cost
    within twice the bound (planes that agree to 5e-6 are not told apart);
  * consistency: the same count.
The pixels excluded by the margins must stay below MAX_EXCLUDED = 2 % for the window costs and the
consistency (measured: at most 0.13 % and 0.6 %).  A half sweep compares ~10 hypotheses per pixel, and
once the maps have converged its refinements are near-ties that float32 cannot order: measured exclusions
of 1.2-5 % (iterations 0-2) and up to 16 % (iterations 3-6), hence MAX_EXCLUDED_SWEEP = 12 % / 35 %; the
fraction rule below bounds the mismatches over all swept pixels regardless.  The fraction rules of
tests/test_extended_oracle.py (>= 99.5 % of the costs within 2e-4, >= 99.8 % with the same +inf pattern,
>= 99 % of the swept planes equal -- 98 % after iteration 2) apply to every case as well.

Each of these one-line kernel faults makes at least one case fail: keep = n_valid / 2 in xbetter_half
(nsrc5, nsrc6), Rs transposed in the consistency kernel (every consistency count), u >= 1 in the corner test
of xcost_t (p3s1-u8, p5s1-u8, p7s2-u8), rintf for floorf in the N = 6 path (p11s2-*), and the float sampler's
weights taken from the unclamped origin (test_float_sampler_reads_the_edge_columns).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 11
EPS_GEOM = 1e-3
EPS_CONS = 1e-4
COST_ABS = 2e-6
COST_KAPPA = 32.0
GAP_KAPPA = 8.0
MAX_EXCLUDED = 0.02
MAX_EXCLUDED_SWEEP = (0.12, 0.35)      # iterations <= 2, later


def cost_tol(kappa):
    return COST_ABS + COST_KAPPA * np.asarray(kappa) * 2.0 ** -24


def gap_tol(kappa):
    return COST_ABS + GAP_KAPPA * np.asarray(kappa) * 2.0 ** -24


def case(name, **kw):
    c = dict(name=name, NV=5, H=40, W=56, patch=7, stride=2, sampling="u8", n_src=4, refs=None, iters=(0, 2),
             num_refine=2, vp=True, scene_seed=17)
    c.update(kw)
    return c


CASES = []
for _p, _s, _hw in ((3, 1, (32, 48)), (5, 1, (32, 48)), (7, 2, (32, 48)), (11, 2, (32, 48)), (13, 2, (32, 48)),
                    (15, 2, (32, 48)), (9, 3, (32, 48)), (31, 2, (40, 48))):
    for _it, _smp in enumerate(("u8", "force", "float")):
        CASES.append(case(f"p{_p}s{_s}-{_smp}", patch=_p, stride=_s, sampling=_smp, H=_hw[0], W=_hw[1], iters=(_it,)))
CASES += [
    case("nsrc2", NV=7, n_src=2, iters=(1,)),
    case("nsrc3", NV=7, n_src=3, iters=(1,)),
    case("nsrc5", NV=7, n_src=5, iters=(1,)),
    case("nsrc6", NV=7, n_src=6, iters=(1,)),
    case("nsrc6-float", NV=7, n_src=6, sampling="float", iters=(1,)),
    case("ragged-37x61", H=37, W=61, iters=(0, 1)),
    case("ragged-37x61-p15-float", H=37, W=61, patch=15, sampling="float", iters=(1,)),
    case("tiny-p11", H=9, W=40, patch=11, iters=(0,)),
    case("tiny-p15-generic", H=40, W=13, patch=15, sampling="float", iters=(0,)),
    case("subset-3-0", refs=(3, 0), iters=(0, 1)),
    case("iters-nr0", iters=(1, 3, 6), num_refine=0),
    case("iters-nr6", iters=(3,), num_refine=6),
    case("no-viewprop", iters=(0, 3), vp=False),
]


def _sources(NV, n_src):
    return [[j for j in sorted(range(NV), key=lambda j: (abs(j - r), j)) if j != r][:n_src] for r in range(NV)]


def _scene(c):
    from amvs.synthetic import make_scene
    sc = make_scene(c["NV"], c["H"], c["W"], seed=c["scene_seed"])
    codes = [np.round(g * 255.0).clip(0, 255).astype(np.uint8) for g in sc.grays]
    if c["sampling"] == "float":
        grays = [g.astype(np.float32) for g in sc.grays]           # not 8-bit exact
    else:
        grays = [cc.astype(np.float32) / np.float32(255.0) for cc in codes]
    return sc, codes, grays


def collect(c):
    """Run the case on the GPU; every map the phases produced, on the host."""
    import torch
    import amvs
    from amvs.engine import make_xpm_params
    sc, codes, grays = _scene(c)
    NV, H, W = c["NV"], c["H"], c["W"]
    refs = list(c["refs"] if c["refs"] is not None else range(NV))
    srcs = [_sources(NV, c["n_src"])[r] for r in refs]
    eng = amvs.Engine(H, W, NV, sc.camera.K.astype(np.float32), mode="exact")
    for i in range(NV):
        eng.set_view(i, grays[i], sc.poses[i].R, sc.poses[i].t)
    if c["sampling"] == "force":
        eng.set_sampling(True)
    out = {"sampling_mode": np.array(eng.sampling_mode())}
    dev = torch.device("cuda", 0)
    # every view starts from its true depth, fronto-parallel (views that are not references keep it)
    depth = torch.tensor(np.stack(sc.depths).reshape(NV, H * W), dtype=torch.float32, device=dev)
    nrm = np.zeros((NV, H * W, 3), np.float32)
    nrm[..., 2] = -1.0
    normal = torch.tensor(nrm.reshape(NV, 3 * H * W), device=dev)
    cost = torch.full((NV, H * W), 0.5, dtype=torch.float32, device=dev)
    ptrs = (depth.data_ptr(), normal.data_ptr(), cost.data_ptr())

    def host(tag):
        torch.cuda.synchronize()
        out[tag + "_d"] = depth.cpu().numpy().reshape(NV, H, W)
        out[tag + "_n"] = normal.cpu().numpy().reshape(NV, H, W, 3)
        out[tag + "_c"] = cost.cpu().numpy().reshape(NV, H, W)

    host("start")
    p = make_xpm_params(c["patch"], sc.depth_min, sc.depth_max, window_stride=c["stride"], num_refine=c["num_refine"],
                        view_propagation=c["vp"])
    eng.xpm_init(refs, srcs, p, SEED, *ptrs)
    eng.sync()
    host("init")
    done = 0
    for it in c["iters"]:
        while done < it:
            eng.xpm_iterate(refs, srcs, p, done, SEED, *ptrs)
            done += 1
        eng.sync()
        host(f"it{it}_pre")
        ev = torch.full((len(refs), H * W), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        eng.xpm_step(refs, srcs, p, it, SEED, "eval", *ptrs, cost_out_ptr=ev.data_ptr())
        eng.sync()
        out[f"it{it}_eval"] = ev.cpu().numpy().reshape(len(refs), H, W)
        eng.xpm_step(refs, srcs, p, it, SEED, "candidates", *ptrs)
        eng.sync()
        if c["vp"]:
            out[f"it{it}_cd"], out[f"it{it}_cn"] = eng.xpm_fetch_candidates(len(refs))
        for phase in ("red", "black"):
            eng.xpm_step(refs, srcs, p, it, SEED, phase, *ptrs)
            eng.sync()
            host(f"it{it}_{phase}")
        done = it + 1
    conf = torch.full((len(refs), H * W), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    eng.xpm_consistency(refs, srcs, p, *ptrs, conf.data_ptr())
    eng.sync()
    host("final")
    out["conf"] = conf.cpu().numpy().reshape(len(refs), H, W)
    eng.close()
    return out


def _excluded_ok(excl, n, what, limit=None):
    limit = MAX_EXCLUDED if limit is None else limit
    frac = excl / max(n, 1)
    assert frac <= limit, f"{what}: {frac:.4f} of the pixels excluded by the margins (> {limit})"
    return frac


def check(c, data):
    """Compare one collected case with the reference; returns a dict of measured figures."""
    from oracle import oracle, xpm_oracle
    sc, codes, grays = _scene(c)
    NV, H, W = c["NV"], c["H"], c["W"]
    refs = list(c["refs"] if c["refs"] is not None else range(NV))
    srcs_all = _sources(NV, c["n_src"])
    want_mode = "u8-pairs" if c["sampling"] == "u8" else "f32"
    assert str(data["sampling_mode"]) == want_mode, (c["name"], str(data["sampling_mode"]))
    K = sc.camera.K.astype(np.float32)
    Ki = np.linalg.inv(K).astype(np.float32)
    poses = [(sc.poses[i].R, sc.poses[i].t) for i in range(NV)]
    R64 = {r: xpm_oracle.Ref64(K, Ki, grays, poses, r, srcs_all[r], c["patch"], c["stride"]) for r in refs}
    rng = lambda seed, view, draw, n: oracle.rng_fill(seed, view, draw, n)      # noqa: E731
    others = [v for v in range(NV) if v not in refs]
    name = c["name"]
    stats = dict(cost_err=0.0, cost_err_kappa=0.0, excluded=0.0)
    yy, xx = np.mgrid[0:H, 0:W]

    def untouched(tag):
        for key in ("_d", "_n", "_c"):
            assert np.array_equal(data[tag + key][others], data["start" + key][others]), \
                f"{name} {tag}: a view that is not a reference was written"

    # ---- xpm_init: log-uniform depth and normals around the viewing direction from draw 0 ----
    p_log_min, p_log_max = np.log(float(sc.depth_min)), np.log(float(sc.depth_max))
    for r in refs:
        wd, wn = xpm_oracle.init_state(SEED, r, H, W, np.float32(p_log_max - p_log_min), np.float32(p_log_min), rng)
        assert (np.abs(data["init_d"][r] - wd) <= 1e-5 * wd).all(), f"{name} init depth view {r}"
        assert (np.abs(data["init_n"][r] - wn) <= 1e-5).all(), f"{name} init normal view {r}"
        assert np.isinf(data["init_c"][r]).all()
    untouched("init")

    def cost_rule(got, want, m, k, what):
        """the fraction rules and the margin rule for one map of window costs"""
        same_inf = np.isinf(got) == np.isinf(want)
        fin = np.isfinite(got) & np.isfinite(want)
        assert same_inf.mean() >= 0.998, f"{what}: +inf pattern differs on {(~same_inf).sum()} pixels"
        if fin.any():
            assert (np.abs(got[fin] - want[fin]) <= 2e-4).mean() >= 0.995, f"{what}: cost differs"
        sel = m > EPS_GEOM
        frac = _excluded_ok((~sel).sum(), sel.size, what)
        stats["excluded"] = max(stats["excluded"], frac)
        bad_inf = sel & ~same_inf
        assert not bad_inf.any(), f"{what}: validity differs on {bad_inf.sum()} decided pixels (excluded {frac:.4f})"
        fs = sel & fin
        with np.errstate(invalid="ignore"):
            err = np.abs(got - want)
        bad = fs & (err > cost_tol(k))
        assert not bad.any(), (f"{what}: {bad.sum()} costs outside the bound, max err {err[bad].max():.3e} "
                               f"at kappa {k[bad][np.argmax(err[bad])]:.1f} (excluded {frac:.4f})")
        if fs.any():
            stats["cost_err"] = max(stats["cost_err"], float(err[fs].max()))
            stats["cost_err_kappa"] = max(stats["cost_err_kappa"], float((err[fs] / (np.maximum(k[fs], 1.0) * 2.0 ** -24)).max()))

    for it in c["iters"]:
        d0, n0, c0 = data[f"it{it}_pre_d"], data[f"it{it}_pre_n"], data[f"it{it}_pre_c"]
        untouched(f"it{it}_pre")
        # ---- window cost of the current planes ----
        for slot, r in enumerate(refs):
            want, m, k = R64[r].cost_map(d0[r], n0[r])
            cost_rule(data[f"it{it}_eval"][slot], want, m, k, f"{name} it {it} eval view {r}")
        # ---- view candidates (float32 restatement) ----
        if c["vp"]:
            cd, cn = data[f"it{it}_cd"], data[f"it{it}_cn"]
            for slot, r in enumerate(refs):
                v32 = xpm_oracle.View(K, Ki, codes, poses, r, srcs_all[r], 3, 1)
                wd, wn = v32.view_candidates(d0, n0, it % c["n_src"], sc.depth_min, sc.depth_max)
                same = (cd[slot] > 0) == (wd > 0)
                both = (cd[slot] > 0) & (wd > 0)
                assert same.mean() >= 0.998, f"{name} it {it} candidates view {r}: {same.mean():.4f}"
                close = np.abs(cd[slot][both] - wd[both]) <= 1e-5 * wd[both]
                assert close.mean() >= 0.998, f"{name} it {it} candidates view {r}"
                assert (np.abs(cn[slot][both] - wn[both]).max(axis=-1) <= 1e-4).mean() >= 0.998
        else:
            cd = np.zeros((len(refs), H, W), np.float32)
            cn = np.zeros((len(refs), H, W, 3), np.float32)
        # ---- red, then black half sweep, each from the GPU's state before it ----
        before = f"it{it}_pre"
        for colour, phase in ((0, "red"), (1, "black")):
            tag = f"it{it}_{phase}"
            untouched(tag)
            swept = ((xx + yy + colour) & 1) == 0
            for slot, r in enumerate(refs):
                db, nb, cb = data[before + "_d"][r], data[before + "_n"][r], data[before + "_c"][r]
                da, na, ca = data[tag + "_d"][r], data[tag + "_n"][r], data[tag + "_c"][r]
                what = f"{name} it {it} {phase} view {r}"
                assert np.array_equal(da[~swept], db[~swept]) and np.array_equal(na[~swept], nb[~swept]), \
                    f"{what}: the other colour was written"
                wd, wn, wc, wk, wm, wg = R64[r].half_sweep(db, nb, cb, cd[slot], cn[slot], colour, it, SEED, rng,
                                                           sc.depth_min, sc.depth_max, num_refine=c["num_refine"],
                                                           view_propagation=c["vp"], cost_tol=gap_tol)
                same_d = np.abs(da - wd) <= 1e-5 * np.abs(wd)
                min_same = 0.99 if it <= 2 else 0.98
                assert same_d[swept].mean() >= min_same, f"{what}: {same_d[swept].mean():.4f} of the planes agree"
                sel = swept & (wm > EPS_GEOM) & (wg > 1.0)
                frac = _excluded_ok((swept & ~sel).sum(), swept.sum(), what, MAX_EXCLUDED_SWEEP[it > 2])
                stats["excluded"] = max(stats["excluded"], frac)
                same_n = (np.abs(na - wn) <= 1e-5).all(axis=-1)
                bad = sel & ~(same_d & same_n)
                assert not bad.any(), f"{what}: {bad.sum()} decided pixels picked another plane (excluded {frac:.4f})"
                same_inf = np.isinf(ca) == np.isinf(wc)
                assert not (sel & ~same_inf).any(), f"{what}: +inf pattern of the winners differs"
                fin = sel & np.isfinite(ca) & np.isfinite(wc)
                with np.errstate(invalid="ignore"):
                    err = np.abs(ca - wc)
                # planes that agree to 5e-6 are not told apart: either may win, each with its own error
                assert not (fin & (err > 2.0 * cost_tol(wk))).any(), f"{what}: winner cost outside the bound"
            before = tag
    # ---- geometric consistency of the final state ----
    untouched("final")
    for slot, r in enumerate(refs):
        want, m = R64[r].consistency(data["final_d"], data["final_c"][r])
        got = data["conf"][slot]
        what = f"{name} consistency view {r}"
        sel = m > EPS_CONS
        frac = _excluded_ok((~sel).sum(), sel.size, what)
        stats["excluded"] = max(stats["excluded"], frac)
        bad = sel & (got != want)
        assert not bad.any(), f"{what}: {bad.sum()} counts differ (excluded {frac:.4f})"
        assert (got == want).mean() >= 0.995
    return stats


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_extended_path_matches_the_reference(c):
    stats = check(c, collect(c))
    print(c["name"], {k: round(v, 6) for k, v in stats.items()})


def test_consistency_counts_sources_on_consistent_maps():
    """Counts that are not all zero: on a converged state xpm_consistency agrees with the reference on
    pixels that most sources confirm (the case matrix above starts from a few iterations only).  Measured:
    19 % of the pixels of 5 views of 40x56 confirmed by 3 or more of their 4 sources (the image margins
    are seen by fewer)."""
    c = case("converged", iters=(5,))
    data = collect(c)
    check(c, data)
    assert (data["conf"] >= 3).mean() > 0.15, (data["conf"] >= 3).mean()


# ------------------------------------------------------------------------------------------------------
# the float sampler at the image edge
def test_float_sampler_reads_the_edge_columns():
    """A source that is the reference shifted by an integer number of pixels, fronto-parallel planes at
    depths a few ulp around the shift's depth: the right-most taps land on u = W - 1 and the bottom taps
    on v = H - 1, where the kernel's float32 chain may round them past the edge although the corner test
    passed.  The float sampler must still read column W - 1 / row H - 1 (it read column W - 2 / row H - 2
    with a weight of ~0 before the clamp of its weights)."""
    import torch
    import amvs
    from amvs.engine import make_xpm_params
    from oracle import xpm_oracle
    H, W, shift = 30, 48, 3
    rng = np.random.default_rng(5)
    f = 0.8 * W
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)
    d_int = np.float32(4.0)
    tx = float(shift) * float(d_int) / f
    poses = [(np.eye(3), np.zeros(3)), (np.eye(3), np.array([tx, 0.0, 0.0])), (np.eye(3), np.array([-tx, 0.0, 0.0]))]
    grays = [rng.random((H, W)).astype(np.float32) * np.float32(0.9) + np.float32(0.05) for _ in range(3)]
    eng = amvs.Engine(H, W, 3, K, mode="exact")
    for i in range(3):
        eng.set_view(i, grays[i], *poses[i])
    assert eng.sampling_mode() == "f32"
    dev = torch.device("cuda", 0)
    jit = rng.integers(-24, 25, (H, W)).astype(np.float64)
    dmap = (float(d_int) * (1.0 + jit * 2.0 ** -24)).astype(np.float32)
    depth = torch.tensor(np.stack([dmap] * 3).reshape(3, -1), device=dev)
    nrm = np.zeros((3, H * W, 3), np.float32)
    nrm[..., 2] = -1
    normal = torch.tensor(nrm.reshape(3, -1), device=dev)
    cost = torch.zeros((3, H * W), dtype=torch.float32, device=dev)
    Ki = np.linalg.inv(K).astype(np.float32)
    checked = 0
    for patch, stride in ((7, 2), (5, 1), (11, 2)):
        p = make_xpm_params(patch, 1.0, 10.0, window_stride=stride)
        ev = torch.full((1, H * W), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        eng.xpm_step([0], [[1, 2]], p, 2, SEED, "eval", depth.data_ptr(), normal.data_ptr(), cost.data_ptr(),
                     cost_out_ptr=ev.data_ptr())
        eng.sync()
        got = ev.cpu().numpy().reshape(H, W)
        ref = xpm_oracle.Ref64(K, Ki, grays, poses, 0, [1, 2], patch, stride)
        want, m, k = ref.cost_map(dmap, nrm[0].reshape(H, W, 3), edge_tol=1e-3)
        both = np.isfinite(got) & np.isfinite(want)
        with np.errstate(invalid="ignore"):
            err = np.abs(got - want)
        bad = both & (err > cost_tol(k))
        assert not bad.any(), f"patch {patch}: {bad.sum()} costs wrong at the edge, max err {err[bad].max():.3e}"
        edge = both & (m < 1e-3)                 # a footprint on the last column / row (or the first)
        checked += int(edge.sum())
        # the pixels whose window is not on an edge are decided: same validity everywhere else
        assert not ((m > EPS_GEOM) & (np.isinf(got) != np.isinf(want))).any()
    eng.close()
    assert checked >= 20, f"only {checked} windows on the edge were compared"


# ------------------------------------------------------------------------------------------------------
# invariances the host code relies on (bit-exact)
def _inv_setup(NV=5, H=40, W=56):
    import torch
    import amvs
    from amvs.engine import make_xpm_params
    from amvs.synthetic import make_scene
    sc = make_scene(NV, H, W, seed=17)
    eng = amvs.Engine(H, W, NV, sc.camera.K.astype(np.float32), mode="fast")
    for i in range(NV):
        eng.set_view(i, np.round(sc.grays[i] * 255).clip(0, 255).astype(np.float32) / np.float32(255), sc.poses[i].R, sc.poses[i].t)
    p = make_xpm_params(7, sc.depth_min, sc.depth_max, window_stride=2)
    dev = torch.device("cuda", 0)
    st = [torch.zeros((NV, H * W), dtype=torch.float32, device=dev), torch.zeros((NV, 3 * H * W), dtype=torch.float32, device=dev),
          torch.zeros((NV, H * W), dtype=torch.float32, device=dev)]
    return eng, p, st, _sources(NV, 4)


def test_split_calls_with_a_snapshot_equal_one_call():
    """_sweep_extended splits the views of an iteration over several calls that read one snapshot; the
    maps must be those of a single call over all views."""
    import torch
    eng, p, st, srcs = _inv_setup()
    maps = []
    for split in (False, True):
        eng.xpm_init(list(range(5)), srcs, p, SEED, *[t.data_ptr() for t in st])
        for it in range(3):
            ptrs = [t.data_ptr() for t in st]
            if not split:
                eng.xpm_iterate(list(range(5)), srcs, p, it, SEED, *ptrs)
            else:
                torch.cuda.synchronize()
                snap_d, snap_n = st[0].clone(), st[1].clone()
                torch.cuda.synchronize()
                for part in ((4, 1), (0, 3, 2)):
                    eng.xpm_iterate(list(part), [srcs[r] for r in part], p, it, SEED, *ptrs, snap_d.data_ptr(), snap_n.data_ptr())
                eng.sync()
                del snap_d, snap_n
        eng.sync()
        maps.append([t.cpu().numpy().copy() for t in st])
    eng.close()
    for a, b in zip(*maps):
        assert np.array_equal(a, b)


def test_step_phases_equal_iterate():
    """xpm_step run phase by phase (candidates, red, black) is xpm_iterate, bit for bit."""
    eng, p, st, srcs = _inv_setup()
    maps = []
    for by_phase in (False, True):
        ptrs = [t.data_ptr() for t in st]
        eng.xpm_init(list(range(5)), srcs, p, SEED, *ptrs)
        for it in range(3):
            if by_phase:
                for phase in ("candidates", "red", "black"):
                    eng.xpm_step(list(range(5)), srcs, p, it, SEED, phase, *ptrs)
            else:
                eng.xpm_iterate(list(range(5)), srcs, p, it, SEED, *ptrs)
        eng.sync()
        maps.append([t.cpu().numpy().copy() for t in st])
    eng.close()
    for a, b in zip(*maps):
        assert np.array_equal(a, b)
