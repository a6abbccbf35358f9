"""Where the fast sweep step takes the reference window's (mean1, var1) and the centre depth from is performance only
(include/amvs_step.h amvs_set_step_sources): with the statistics loaded from the per-view maps or formed in the kernel from
the packed reference codes, and with the centre depth loaded again or kept from the sampling load, every combination
gives IDENTICAL depth / normal / confidence maps (the cost drives every selection, so a cost that differed in one bit
would move them), and they are the CPU oracle's fast mode.

Each case is one PatchMatch call of two iterations with one refinement sample: the propagation launches of both
parities (neighbours below / right, then above / left), a refinement launch of each parity and the confidence launch,
on the paired-band and on the classic schedule.  The shapes are the smallest at which the new code takes another path:
    W   7 narrower than a strip, 58 exactly one 7x7 strip, 59 a second strip of one column, 64 and 117 two and three
        strips of the other patch sizes; with 11x11 and W = 7 the window is clipped at both image edges at once
    H   7 / 19 / 37 with band heights that leave an odd, unpaired last band (19 = 8 + 8 + 3, 37 = 4 x 8 + 5) or a lower
        band shorter than its partner (19 = 12 + 7, 37 = 3 x 10 + 7)
    K   3 .. 11 (one and two packed registers of codes with 1, 3, 1, 3 and 1 stale bytes below the window), S 2 .. 4
    images of random codes, all 0, all 255 (the largest window sums) and random 254 / 255
"""
import numpy as np
import pytest

from degenerate_images import Case, colors_of, grays_of
from test_hip_fullsize_parity import _eq

pytestmark = pytest.mark.gpu

SEED = 11
SOURCES = [(False, False), (True, False), (False, True), (True, True)]        # (ref_stats in kernel, centre depth kept)
NAMES = ("depth", "normal", "confidence")

#        W    H   K  S  band rows  content
CASES = [(7, 7, 3, 2, 8, "random"),
         (7, 19, 11, 4, 8, "random"),
         (58, 19, 7, 4, 12, "random"),
         (59, 37, 7, 4, 8, "random"),
         (59, 37, 7, 3, 10, "255"),
         (64, 19, 5, 2, 8, "random"),
         (64, 37, 9, 3, 10, "random"),
         (117, 37, 11, 4, 8, "random"),
         (117, 19, 7, 4, 12, "0"),
         (117, 7, 5, 3, 8, "255"),
         (58, 7, 9, 2, 8, "0"),
         (117, 37, 3, 4, 10, "random"),
         (64, 37, 11, 2, 8, "bright"),
         (59, 19, 3, 3, 12, "random"),
         (7, 37, 5, 4, 10, "random"),
         (58, 37, 9, 4, 8, "bright")]


def _case(W, H, S, content):
    from amvs.synthetic import make_scene
    n = S + 1
    sc = make_scene(n, H, W, seed=5)
    rng = np.random.default_rng([W, H, S])
    codes = {"random": lambda: rng.integers(0, 256, (n, H, W)), "0": lambda: np.zeros((n, H, W)),
             "255": lambda: np.full((n, H, W), 255), "bright": lambda: rng.integers(254, 256, (n, H, W))}[content]()
    codes = codes.astype(np.uint8)
    return Case(sc, content, grays_of(codes), colors_of(codes), np.zeros((n, H, W), bool), 0, f"{content} {n}x{H}x{W}")


_ORACLE = {}


def _oracle_maps(case, W, H, K, S, content):
    """The oracle's maps of a case, computed once and shared by both schedules."""
    key = (W, H, K, S, content)
    if key not in _ORACLE:
        sc = case.scene
        _ORACLE[key] = case.oracle_ctx(0, list(range(1, S + 1)), K, mode="fast").patchmatch(2, 1, sc.depth_min, sc.depth_max,
                                                                                            SEED, 0)
    return _ORACLE[key]


@pytest.mark.parametrize("schedule", ["paired", "view-major"])
@pytest.mark.parametrize("W,H,K,S,rows,content", CASES)
def test_step_sources_give_identical_maps(W, H, K, S, rows, content, schedule):
    from amvs.engine import make_pm_params
    case = _case(W, H, S, content)
    sc = case.scene
    p = make_pm_params(K, 2, 1, sc.depth_min, sc.depth_max, mode="fast", schedule=schedule, tile_rows=rows)
    maps = {}
    with case.engine("fast") as eng:
        for src in SOURCES:
            eng.set_step_sources(*src)
            assert eng.step_sources(K) == src              # the launches of this call take this path
            maps[src] = eng.patchmatch([0], [list(range(1, S + 1))], p, SEED)
            assert eng.last_tile_rows() == rows
    what = f"{W}x{H} k={K} S={S} rows={rows} {content} {schedule}"
    for src in SOURCES[1:]:
        for a, b, name in zip(maps[src], maps[SOURCES[0]], NAMES):
            _eq(a, b, f"{what} {name}: (ref_stats, centre_depth) in registers = {src} vs maps and loads")
    od, on, oc = _oracle_maps(case, W, H, K, S, content)
    for src in (SOURCES[0], SOURCES[-1]):
        _eq(maps[src][0][0], od, f"{what} {src} depth vs oracle")
        _eq(maps[src][2][0], oc, f"{what} {src} confidence vs oracle")
        _eq(maps[src][1][0], on, f"{what} {src} normal vs oracle")


def test_single_steps_and_split_schedule_take_the_switch():
    """The single-step entry points (cost evaluation and confidence: the run-time-mode kernel; one propagation and one
    refinement step with their costs) and the split schedule's window kernel with the statistics from the registers
    against the maps; and a patch size beyond the in-kernel form (17 x 17) keeps working with the switch on."""
    from amvs import _lib
    from amvs.engine import make_pm_params
    W, H, K, S = 59, 19, 7, 3
    case = _case(W, H, S, "random")
    sc = case.scene
    srcs = list(range(1, S + 1))
    rng = np.random.default_rng(3)
    depth = rng.uniform(sc.depth_min, sc.depth_max, (H, W)).astype(np.float32)
    normal = rng.normal(size=(H, W, 3)).astype(np.float32)
    assert _lib.load().amvs_step_sources_max_patch() == 15
    got = {}
    with case.engine("fast") as eng:
        for src in (SOURCES[0], SOURCES[-1]):
            eng.set_step_sources(*src)
            cost = eng.eval_cost(0, srcs, K, depth)
            out = [cost, eng.confidence(0, srcs, K, depth)]
            out += list(eng.propagate_step(0, srcs, K, depth, normal, cost, -1, 0, sc.depth_min))
            out += list(eng.refine_step(0, srcs, K, depth, normal, cost, SEED, 0, 3, 0.5 * (sc.depth_max - sc.depth_min), 0.25,
                                        sc.depth_min, sc.depth_max))
            out += list(eng.patchmatch([0], [srcs], make_pm_params(K, 2, 1, sc.depth_min, sc.depth_max, mode="fast",
                                                                   schedule="split"), SEED))
            out += list(eng.patchmatch([0], [srcs], make_pm_params(17, 1, 1, sc.depth_min, sc.depth_max, mode="fast"), SEED))
            got[src] = out
    assert len(got[SOURCES[0]]) == len(got[SOURCES[-1]]) >= 12
    for i, (a, b) in enumerate(zip(got[SOURCES[-1]], got[SOURCES[0]])):
        _eq(a, b, f"single steps / split / 17x17, output {i}: registers vs maps and loads")


#              W    H   K  S  content
COST_CASES = [(7, 19, 11, 4, "random"), (58, 7, 3, 2, "255"), (59, 37, 7, 4, "random"), (64, 19, 5, 2, "bright"),
              (117, 37, 9, 3, "random"), (117, 19, 11, 4, "random")]


@pytest.mark.parametrize("W,H,K,S,content", COST_CASES)
def test_costs_are_identical_and_the_oracles(W, H, K, S, content):
    """The COST maps themselves, through the single-step entry points, for all four settings: the evaluated cost and
    the confidence of a depth map (equal to the oracle's), and the depth / normal / cost after a propagation step of
    each parity (neighbour below, neighbour to the left) and after a refinement step."""
    case = _case(W, H, S, content)
    sc = case.scene
    srcs = list(range(1, S + 1))
    rng = np.random.default_rng([W, H, K])
    depth = rng.uniform(sc.depth_min, sc.depth_max, (H, W)).astype(np.float32)
    normal = rng.normal(size=(H, W, 3)).astype(np.float32)
    got = {}
    with case.engine("fast") as eng:
        for src in SOURCES:
            eng.set_step_sources(*src)
            assert eng.step_sources(K) == src
            cost = eng.eval_cost(0, srcs, K, depth)
            out = [cost, eng.confidence(0, srcs, K, depth)]
            out += list(eng.propagate_step(0, srcs, K, depth, normal, cost, 1, 0, sc.depth_min))
            out += list(eng.propagate_step(0, srcs, K, depth, normal, cost, 0, -1, sc.depth_min))
            out += list(eng.refine_step(0, srcs, K, depth, normal, cost, SEED, 0, 3, 0.5 * (sc.depth_max - sc.depth_min), 0.25,
                                        sc.depth_min, sc.depth_max))
            got[src] = out
    names = ["evaluated cost", "confidence"] + [f"{step} {m}" for step in ("propagation (+1, 0)", "propagation (0, -1)", "refinement")
                                                for m in ("depth", "normal", "cost")]
    for src in SOURCES[1:]:
        for a, b, name in zip(got[src], got[SOURCES[0]], names):
            _eq(a, b, f"{W}x{H} k={K} S={S} {content} {name}: registers = {src} vs maps and loads")
    ctx = case.oracle_ctx(0, srcs, K, mode="fast")
    _eq(got[SOURCES[-1]][0], ctx.patch_cost(depth), f"{W}x{H} k={K} evaluated cost vs oracle")
    _eq(got[SOURCES[-1]][1], ctx.confidence(depth), f"{W}x{H} k={K} confidence vs oracle")
    od, on, oc = ctx.propagate_step(depth, normal, got[SOURCES[0]][0], 1, 0, sc.depth_min)
    for a, b, name in zip(got[SOURCES[-1]][2:5], (od, on, oc), ("depth", "normal", "cost")):
        _eq(a, b, f"{W}x{H} k={K} propagation (+1, 0) {name} vs oracle")


def test_the_switch_resolves_as_documented():
    """amvs_get_step_sources: the automatic table takes both parts up to 11 x 11 and neither from 13 x 13; a forced
    setting holds up to 15 x 15 and is ignored (reported as the maps and loads) beyond, where nothing else is compiled;
    values outside -1 .. 1 are refused."""
    import amvs
    case = _case(59, 19, 2, "random")
    with case.engine("fast") as eng:
        for k in (3, 5, 7, 9, 11):
            assert eng.step_sources(k) == (True, True), k
        for k in (13, 15, 17, 29, 31):
            assert eng.step_sources(k) == (False, False), k
        eng.set_step_sources(True, False)
        assert eng.step_sources(7) == (True, False) and eng.step_sources(15) == (True, False)
        assert eng.step_sources(17) == (False, False) and eng.step_sources(31) == (False, False)
        eng.set_step_sources(False, True)
        assert eng.step_sources(5) == (False, True)
        eng.set_step_sources(None, None)
        assert eng.step_sources(5) == (True, True) and eng.step_sources(13) == (False, False)
        with pytest.raises(amvs.engine.AmvsError):
            eng._chk(eng._lib.amvs_set_step_sources(eng._h, 2, 0))
