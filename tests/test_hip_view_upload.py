"""The view-upload stage on the device -- amvs_set_view_bgr8 (csrc/amvs_prep.hip), the 8-bit pack and its losslessness
flag (pack_pairs_kernel), amvs_set_view and amvs_set_view_device (csrc/amvs_capi.hip) -- against the independent
restatement of tests/view_upload_restatement.py on the input family of tests/view_upload_inputs.py;
tests/test_view_upload_cpu.py shows on the CPU that the restatement stays within a derived bound of true bilinear
interpolation and that the family reaches every edge.  Every comparison is bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import view_upload_inputs as vi  # noqa: E402
import view_upload_restatement as vr  # noqa: E402

pytestmark = pytest.mark.gpu

EYE = np.eye(3)


@pytest.fixture(scope="module")
def amvs_mod():
    import amvs
    return amvs


def _eq(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} elements differ " \
                       f"(first at {np.argwhere(~same)[0]}: {a[~same][0]!r} vs {b[~same][0]!r})"


def _bits_eq(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    diff = a.view(np.uint32) != b.view(np.uint32)
    assert a.shape == b.shape and not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} elements differ in their bits"


def pinhole(H, W):
    f = 0.8 * max(H, W)
    return np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]], np.float32)


def shift(i):
    return np.array([0.05 * i, 0.0, 0.0])


_RESTATED = {}


def restated(case, kind):
    """The small pairs by the loops, the large one by the vectorised form (the CPU test holds it to the loops)."""
    key = (case.name, kind)
    if key not in _RESTATED:
        form = vr.prepare_np if case.big else vr.prepare
        _RESTATED[key] = form(vi.source(case, kind), *case.dst)
    return _RESTATED[key]


# --------------------------------------------------------------------------------------------- amvs_set_view_bgr8 ---
@pytest.mark.parametrize("case", vi.RESIZE_CASES, ids=lambda c: c.name)
def test_bgr8_preparation_equals_the_restatement(amvs_mod, case):
    """Every content of the pair is one view of three contexts: prepared on the device with the colour image returned,
    prepared on the device without it (scaled_bgr_out omitted), and uploaded with set_view from the restatement's gray.
    The returned colour image is the restatement's byte for byte; the gray map is checked through what the kernels read:
    the 3 x 3 window statistics of every view and, from 16 x 16 on, a cost map at patch 5."""
    H, W = case.dst
    kinds = case.contents
    n = len(kinds)
    K = pinhole(H, W)
    with amvs_mod.Engine(H, W, n, K) as dev, amvs_mod.Engine(H, W, n, K) as bare, amvs_mod.Engine(H, W, n, K) as host:
        for i, kind in enumerate(kinds):
            want = restated(case, kind)
            src = vi.source(case, kind)
            color = dev.set_view_bgr8(i, src, EYE, shift(i))
            assert color.shape == (H, W, 3) and color.dtype == np.uint8
            bad = np.argwhere(color != want["color"])
            assert len(bad) == 0, f"{case.name} {kind}: {len(bad)} colour bytes differ, first at {bad[0]}"
            assert bare.set_view_bgr8(i, src, EYE, shift(i), want_color=False) is None
            host.set_view(i, want["gray"], EYE, shift(i))
        assert dev.sampling_mode() == bare.sampling_mode() == host.sampling_mode() == "u8-pairs"
        for i, kind in enumerate(kinds):
            mh, vh = host.box_stats(i, 3)
            for eng, name in ((dev, "prepared"), (bare, "prepared without the colour image")):
                m, v = eng.box_stats(i, 3)
                _bits_eq(m, mh, f"{case.name} {kind} {name}: mean")
                _bits_eq(v, vh, f"{case.name} {kind} {name}: variance")
        if H >= 16 and W >= 16:
            d = np.full((H, W), 5.0, np.float32)
            srcs = list(range(1, min(n, 4)))
            ch = host.eval_cost(0, srcs, 5, d)
            assert np.isfinite(ch).any()
            _eq(dev.eval_cost(0, srcs, 5, d), ch, f"{case.name}: cost")
            _eq(bare.eval_cost(0, srcs, 5, d), ch, f"{case.name}: cost without the colour image")


def test_one_context_reused_across_source_sizes(amvs_mod):
    """Sources of ascending and then descending size into one view of one context (the staging buffer is regrown between
    them, the tables rewritten): each result equals that of a fresh context and the restatement."""
    H, W = 20, 47
    K = pinhole(H, W)
    sizes = [(1, 7), (3, 5), (300, 5), (5, 300), (64, 48), (90, 130)]
    order = sizes + sizes[-2::-1]
    assert [h * w for h, w in sizes] == sorted(h * w for h, w in sizes)
    fresh = {}
    for h, w in sizes:
        src = vi.content("random", h, w)
        with amvs_mod.Engine(H, W, 1, K) as eng:
            color = eng.set_view_bgr8(0, src, EYE, shift(0))
            assert np.array_equal(color, vr.prepare(src, H, W)["color"]), f"fresh context, source {h} x {w}"
            fresh[(h, w)] = (color, eng.box_stats(0, 3), eng.sampling_mode())
    with amvs_mod.Engine(H, W, 1, K) as eng:
        for h, w in order:
            color = eng.set_view_bgr8(0, vi.content("random", h, w), EYE, shift(0))
            want = fresh[(h, w)]
            assert np.array_equal(color, want[0]), f"reused context, source {h} x {w}: colour image"
            m, v = eng.box_stats(0, 3)
            _bits_eq(m, want[1][0], f"reused context, source {h} x {w}: mean")
            _bits_eq(v, want[1][1], f"reused context, source {h} x {w}: variance")
            assert eng.sampling_mode() == want[2] == "u8-pairs"


# ------------------------------------------------------------------------------------------------------ the switch ---
PATCH = 5
PM = dict(iters=2, samples=2, seed=7)
REF, SRCS = 1, [0, 2]


class Rig:
    """Cameras of the 9 x 11 gray cases and the runs every switch test repeats."""

    def __init__(self, amvs_mod):
        from amvs.synthetic import arc_poses
        self.amvs = amvs_mod
        self.H, self.W = vi.GRAY_SHAPE
        self.K = pinhole(self.H, self.W)
        self.poses = arc_poses(vi.GRAY_VIEWS + 1)
        self.dmin, self.dmax = 3.0, 8.0
        self.planes = (1.0 / np.linspace(1 / 9.0, 1 / 2.5, 12)).astype(np.float32)
        self.flat = np.full((self.H, self.W), 5.0, np.float32)
        self._clean = {}

    def engine(self, grays, mode="exact", n_views=None, views=None):
        eng = self.amvs.Engine(self.H, self.W, n_views or len(grays), self.K, mode=mode)
        for i in (range(len(grays)) if views is None else views):
            eng.set_view(i, grays[i], self.poses[i].R, self.poses[i].t)
        return eng

    def patchmatch(self, eng):
        from amvs.engine import make_pm_params
        p = make_pm_params(PATCH, PM["iters"], PM["samples"], self.dmin, self.dmax)
        d, n, c = eng.patchmatch([REF], [SRCS], p, seed=PM["seed"])
        return d[0], n[0], c[0]

    def sweep(self, eng):
        return eng.plane_sweep(REF, SRCS, self.planes, PATCH, 0.8)

    def oracle(self, grays, mode="exact"):
        from oracle import oracle
        ctx = oracle.ViewContext(self.K, grays[REF], self.poses[REF].R, self.poses[REF].t, [grays[i] for i in SRCS],
                                 [self.poses[i].R for i in SRCS], [self.poses[i].t for i in SRCS], PATCH, mode=mode)
        return (ctx.patchmatch(PM["iters"], PM["samples"], self.dmin, self.dmax, PM["seed"], REF), ctx.plane_sweep(self.planes, 0.8),
                ctx.patch_cost(self.flat))

    def cost(self, eng):
        return eng.eval_cost(REF, SRCS, PATCH, self.flat)

    def clean(self, mode):
        """(patchmatch, sweep, cost map) of a context that only ever saw the exact views."""
        if mode not in self._clean:
            with self.engine(vi.exact_views(), mode) as eng:
                assert eng.sampling_mode() == "u8-pairs"
                self._clean[mode] = (self.patchmatch(eng), self.sweep(eng), self.cost(eng))
        return self._clean[mode]


@pytest.fixture(scope="module")
def rig(amvs_mod):
    return Rig(amvs_mod)


def _same_maps(got, want, what):
    for g, w, name in zip(got, want, ("depth", "normal / confidence", "confidence")):
        _eq(g, w, f"{what}: {name}")


def test_clean_context_equals_the_oracle(rig):
    """The control the other switch tests compare with: exact views, packed sampling, both arithmetic modes."""
    for mode in ("exact", "fast"):
        pm, sweep, cost = rig.clean(mode)
        opm, osweep, ocost = rig.oracle(vi.exact_views(), mode)
        _same_maps(pm, opm, f"clean {mode} patchmatch")
        _same_maps(sweep, osweep, f"clean {mode} sweep")
        _eq(cost, ocost, f"clean {mode} cost")
        assert np.isfinite(pm[0]).all() and sweep[1].max() > 0


@pytest.mark.parametrize("case", vi.gray_cases(), ids=lambda c: c.name)
def test_losslessness_switch(rig, case):
    """One pixel of one view off its code (or not): the sampling mode follows the flag the restatement states, fast mode
    refuses to sweep exactly when a view is inexact, the exact sweeps and a cost map equal the oracle on the images as
    given (which is what tells a false "lossless": the packed map would hold the rounded pixel), and uploading the exact image over the
    changed view brings back the packed path, fast mode and the maps of a context that never saw anything else."""
    expect = "u8-pairs" if case.all_lossless else "f32"
    assert vr.pack_views(case.grays) == case.lossless
    with rig.engine(case.grays) as eng:
        assert eng.sampling_mode() == expect
        for v in range(vi.GRAY_VIEWS):
            eng.box_stats(v, PATCH)                         # the window statistics of the changed view are now cached
        if case.finite:
            opm, osweep, ocost = rig.oracle(case.grays)
            _same_maps(rig.patchmatch(eng), opm, f"{case.name} patchmatch against the oracle")
            _same_maps(rig.sweep(eng), osweep, f"{case.name} sweep against the oracle")
            _eq(rig.cost(eng), ocost, f"{case.name} cost against the oracle")
            if case.name.startswith("code_plus_0p49"):                   # a quantised pixel would show: the cost of the
                changed = ocost != rig.oracle(case.exact)[2]            # exact views differs where a window holds the pixel
                assert changed.any(), "the oracle cannot tell the changed pixel from its code"
        if case.view >= 0:
            v = case.view
            eng.set_view(v, case.exact[v], rig.poses[v].R, rig.poses[v].t)
            assert eng.sampling_mode() == "u8-pairs"
            _same_maps(rig.patchmatch(eng), rig.clean("exact")[0], f"{case.name} patchmatch after the exact re-upload")
            _same_maps(rig.sweep(eng), rig.clean("exact")[1], f"{case.name} sweep after the exact re-upload")
            _eq(rig.cost(eng), rig.clean("exact")[2], f"{case.name} cost after the exact re-upload")
    with rig.engine(case.grays, mode="fast") as eng:
        assert eng.sampling_mode() == expect
        if case.all_lossless:
            if case.finite:
                opm, osweep, _ = rig.oracle(case.grays, "fast")
                _same_maps(rig.patchmatch(eng), opm, f"{case.name} fast patchmatch against the oracle")
                _same_maps(rig.sweep(eng), osweep, f"{case.name} fast sweep against the oracle")
        else:
            with pytest.raises(rig.amvs.AmvsError, match="8-bit"):
                rig.patchmatch(eng)
            with pytest.raises(rig.amvs.AmvsError, match="8-bit"):
                rig.sweep(eng)
        if case.view >= 0:
            v = case.view
            eng.set_view(v, case.exact[v], rig.poses[v].R, rig.poses[v].t)
            assert eng.sampling_mode() == "u8-pairs"
            _same_maps(rig.patchmatch(eng), rig.clean("fast")[0], f"{case.name} fast patchmatch after the exact re-upload")
            _same_maps(rig.sweep(eng), rig.clean("fast")[1], f"{case.name} fast sweep after the exact re-upload")


def test_inexact_reupload_over_an_exact_view_sets_the_flag(rig):
    """The other direction, on a context whose flags were already read back: exact, then one pixel half a code off."""
    case = vi.gray_case("code_plus_0p49_v2_y4x6")
    with rig.engine(case.exact) as eng:
        assert eng.sampling_mode() == "u8-pairs"
        _same_maps(rig.patchmatch(eng), rig.clean("exact")[0], "before")
        v = case.view
        eng.set_view(v, case.grays[v], rig.poses[v].R, rig.poses[v].t)
        assert eng.sampling_mode() == "f32"
        _same_maps(rig.patchmatch(eng), rig.oracle(case.grays)[0], "after the inexact re-upload")


def test_views_never_uploaded_do_not_influence_the_flag(rig):
    """A context of four views with three uploaded, and one of three with only the two exact views of an inexact case."""
    exact = vi.exact_views()
    with rig.engine(exact, mode="fast", n_views=4) as eng:
        assert eng.sampling_mode() == "u8-pairs"
        _same_maps(rig.patchmatch(eng), rig.clean("fast")[0], "three of four views uploaded")
    case = vi.gray_case("ulp_up_v2_y4x6")
    with rig.engine(case.grays, views=(0, 1)) as eng:
        assert eng.sampling_mode() == "u8-pairs"
    with rig.engine(case.grays, views=(1, 2)) as eng:
        assert eng.sampling_mode() == "f32"


# --------------------------------------------------------------------------------------------- amvs_set_view_device ---
def _outcome(rig, fn):
    try:
        return fn()
    except rig.amvs.AmvsError as e:
        return "refused: " + str(e).split(":")[-1].strip()


@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("name", ["control", "code_plus_0p49_v1_y8x10"])
def test_set_view_device_equals_set_view(rig, name, mode):
    """The same images from torch device tensors (torch synchronised before the call, as include/amvs.h requires): the
    sampling mode, the window statistics and a PatchMatch result of the set_view context, or its refusal."""
    import torch
    case = vi.gray_case(name)
    tensors = [torch.from_numpy(g.copy()).cuda() for g in case.grays]
    torch.cuda.synchronize()
    with rig.engine(case.grays, mode) as host, rig.amvs.Engine(rig.H, rig.W, vi.GRAY_VIEWS, rig.K, mode=mode) as dev:
        for i, t in enumerate(tensors):
            assert t.is_contiguous() and t.dtype == torch.float32
            dev.set_view_device(i, t.data_ptr(), rig.poses[i].R, rig.poses[i].t)
        dev.sync()
        assert dev.sampling_mode() == host.sampling_mode() == ("u8-pairs" if case.all_lossless else "f32")
        for v in range(vi.GRAY_VIEWS):
            a, b = _outcome(rig, lambda: dev.box_stats(v, PATCH)), _outcome(rig, lambda: host.box_stats(v, PATCH))
            assert isinstance(a, str) == isinstance(b, str), f"{name} {mode} view {v}: {a if isinstance(a, str) else b}"
            if isinstance(a, str):
                assert a == b
            else:
                _bits_eq(a[0], b[0], f"{name} {mode} view {v}: mean")
                _bits_eq(a[1], b[1], f"{name} {mode} view {v}: variance")
        a, b = _outcome(rig, lambda: rig.patchmatch(dev)), _outcome(rig, lambda: rig.patchmatch(host))
        if mode == "fast" and not case.all_lossless:
            assert isinstance(a, str) and a == b and "8-bit" in a
        else:
            _same_maps(a, b, f"{name} {mode}: patchmatch")
            _same_maps(a, rig.oracle(case.grays, mode)[0], f"{name} {mode}: patchmatch against the oracle")
    del tensors
