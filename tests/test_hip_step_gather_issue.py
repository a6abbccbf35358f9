"""The fast sweep step requests the gathers of a row together and a row's candidate depth one own row ahead
(csrc/amvs_fast_common.h fast_sample_sources, csrc/amvs_kernels_fast.hip request_depth): scheduling only, so depth, normal,
confidence and cost maps stay the CPU oracle's fast mode bit for bit.

What can go wrong is an index or a row, not a rounding: the depth requested ahead is d_in[pix + noff] of the NEXT row the
wave samples itself -- below for a wave walking down, above for the lower band of a pair, none after a wave's last own row
(a paired wave takes its last K/2 rows from the partner), none for a step outside the wave's rows -- with the in-image rule
of the load it replaces, at every image edge for all four propagation offsets; and the two-lane row coordinate and depth
hand .x to even and .y to odd sources, so S = 3 ends on a source without a partner.  The shapes are the smallest with
those edges, bands forced to 6 rows:
    W   7 one strip narrower than a wave; 58 and 59 one column into a second 7x7 strip; 117 three strips
    H   7 = 6 + 1 a one-row lower band (classic: a one-row strip); 11 = 6 + 5 a lower band shorter than its partner;
        12 exactly one pair; 13 a pair and an odd one-row band that runs unpaired; 17 = 6 + 6 + 5 a pair and an odd
        short band; 37 three pairs and a one-row band
    K   3, 9, 11 classic; 5 and 7 paired and classic;  S 2, 3, 4
Every PatchMatch case runs two iterations (both parities: all four offsets) with one refinement sample for the four
settings of amvs_set_step_sources (the depth history of DHIST takes the value requested ahead).
"""
import numpy as np
import pytest

from test_hip_fullsize_parity import _eq
from test_hip_step_ref_stats import NAMES, SEED, SOURCES, _case

pytestmark = pytest.mark.gpu

ROWS = 6

#        W    H   K  S  schedule
CASES = [(7, 7, 5, 2, "paired"),
         (58, 12, 5, 3, "paired"),
         (59, 13, 5, 4, "paired"),
         (117, 17, 5, 3, "paired"),
         (58, 37, 5, 2, "paired"),
         (59, 11, 5, 3, "paired"),
         (59, 7, 7, 3, "paired"),
         (117, 12, 7, 4, "paired"),
         (7, 13, 7, 4, "paired"),
         (58, 17, 7, 4, "paired"),
         (59, 37, 7, 3, "paired"),
         (117, 37, 7, 4, "paired"),
         (58, 11, 7, 4, "paired"),
         (7, 12, 7, 2, "paired"),
         (117, 7, 3, 2, "view-major"),
         (7, 12, 3, 3, "view-major"),
         (58, 13, 3, 4, "view-major"),
         (59, 37, 3, 3, "view-major"),
         (59, 17, 5, 3, "view-major"),
         (117, 37, 5, 4, "view-major"),
         (58, 7, 7, 2, "view-major"),
         (59, 12, 7, 3, "view-major"),
         (117, 13, 7, 4, "view-major"),
         (7, 37, 7, 4, "view-major"),
         (7, 17, 9, 3, "view-major"),
         (58, 37, 9, 4, "view-major"),
         (59, 13, 9, 2, "view-major"),
         (117, 17, 11, 4, "view-major"),
         (7, 37, 11, 3, "view-major"),
         (59, 12, 11, 2, "view-major"),
         (58, 7, 11, 3, "view-major")]


def test_the_cases_cover_what_the_docstring_says():
    """(no GPU work: the list above against the axes it claims)"""
    assert {c[0] for c in CASES} == {7, 58, 59, 117} and {c[1] for c in CASES} >= {7, 12, 13, 17, 37}
    assert {(c[2], c[4]) for c in CASES} == {(5, "paired"), (7, "paired")} | {(k, "view-major") for k in (3, 5, 7, 9, 11)}
    for k, sched in {(c[2], c[4]) for c in CASES}:
        assert {c[3] for c in CASES if (c[2], c[4]) == (k, sched)} >= {3} | ({2, 4} if sched == "paired" else set()), (k, sched)
    for k in (5, 7):
        assert {c[1] for c in CASES if (c[2], c[4]) == (k, "paired")} >= {7, 12, 13, 17, 37}, k
    assert {c[3] for c in CASES} == {2, 3, 4}


@pytest.mark.parametrize("W,H,K,S,schedule", CASES)
def test_patchmatch_is_the_oracles(W, H, K, S, schedule):
    from amvs.engine import make_pm_params
    case = _case(W, H, S, "random")
    sc = case.scene
    srcs = list(range(1, S + 1))
    p = make_pm_params(K, 2, 1, sc.depth_min, sc.depth_max, mode="fast", schedule=schedule, tile_rows=ROWS)
    want = case.oracle_ctx(0, srcs, K, mode="fast").patchmatch(2, 1, sc.depth_min, sc.depth_max, SEED, 0)
    with case.engine("fast") as eng:
        for src in SOURCES:
            eng.set_step_sources(*src)
            assert eng.step_sources(K) == src
            got = eng.patchmatch([0], [srcs], p, SEED)
            assert eng.last_tile_rows() == ROWS
            for g, w, name in zip(got, want, NAMES):
                _eq(g[0], w, f"{W}x{H} k={K} S={S} rows={ROWS} {schedule} (ref_stats, centre_depth) = {src}: {name} vs oracle")


#               W    H   K  S
STEP_CASES = [(7, 7, 3, 2), (58, 12, 5, 3), (59, 13, 7, 4), (117, 17, 9, 3), (59, 37, 11, 4), (117, 37, 7, 3), (7, 17, 7, 4),
              (58, 37, 5, 2)]
OFFSETS = [(1, 0), (0, 1), (-1, 0), (0, -1)]


@pytest.mark.parametrize("W,H,K,S", STEP_CASES)
def test_single_steps_and_their_costs_are_the_oracles(W, H, K, S):
    """One propagation step of each of the four offsets and one refinement step through the single-step entry points:
    depth, normal AND cost against the oracle's, for the four settings of the switch; and the evaluated cost and the
    confidence of the depth map (the run-time-mode instantiation of the same kernel)."""
    from oracle import oracle
    case = _case(W, H, S, "random")
    sc = case.scene
    srcs = list(range(1, S + 1))
    rng = np.random.default_rng([W, H, K, S])
    depth = rng.uniform(sc.depth_min, sc.depth_max, (H, W)).astype(np.float32)
    normal = rng.normal(size=(H, W, 3)).astype(np.float32)
    ctx = case.oracle_ctx(0, srcs, K, mode="fast")
    cost = ctx.patch_cost(depth)
    conf = ctx.confidence(depth)
    dr, nr, draw = np.float32(0.5 * (sc.depth_max - sc.depth_min)), np.float32(0.25), 3
    want = [ctx.propagate_step(depth, normal, cost, oy, ox, sc.depth_min) for oy, ox in OFFSETS]
    u, nz = oracle.rng_fill(SEED, 0, draw, H * W)
    want.append(ctx.refine_step(depth, normal, cost, u, nz, dr, nr, sc.depth_min, sc.depth_max))
    steps = [f"propagation {o}" for o in OFFSETS] + ["refinement"]
    with case.engine("fast") as eng:
        for src in SOURCES:
            eng.set_step_sources(*src)
            assert eng.step_sources(K) == src
            what = f"{W}x{H} k={K} S={S} (ref_stats, centre_depth) = {src}"
            _eq(eng.eval_cost(0, srcs, K, depth), cost, f"{what}: evaluated cost vs oracle")
            _eq(eng.confidence(0, srcs, K, depth), conf, f"{what}: confidence vs oracle")
            got = [eng.propagate_step(0, srcs, K, depth, normal, cost, oy, ox, sc.depth_min) for oy, ox in OFFSETS]
            got.append(eng.refine_step(0, srcs, K, depth, normal, cost, SEED, 0, draw, dr, nr, sc.depth_min, sc.depth_max))
            for g, w, step in zip(got, want, steps):
                for a, b, name in zip(g, w, ("depth", "normal", "cost")):
                    _eq(a, b, f"{what}: {step} {name} vs oracle")


def test_split_schedule_and_17x17_are_the_oracles():
    """The split schedule (its window half requests no depth: it samples nothing) and a 17 x 17 call (beyond the paired
    schedule and the register sources) against the oracle."""
    from amvs.engine import make_pm_params
    W, H, S = 59, 19, 3
    case = _case(W, H, S, "random")
    sc = case.scene
    srcs = list(range(1, S + 1))
    with case.engine("fast") as eng:
        for K, kw in ((7, dict(schedule="split")), (17, dict(tile_rows=ROWS))):
            want = case.oracle_ctx(0, srcs, K, mode="fast").patchmatch(2, 1, sc.depth_min, sc.depth_max, SEED, 0)
            got = eng.patchmatch([0], [srcs], make_pm_params(K, 2, 1, sc.depth_min, sc.depth_max, mode="fast", **kw), SEED)
            for g, w, name in zip(got, want, NAMES):
                _eq(g[0], w, f"{W}x{H} k={K} {kw}: {name} vs oracle")
