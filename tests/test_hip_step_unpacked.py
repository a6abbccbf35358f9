"""The fast sweep step's register-source variants are compiled in two translation units, split by source count
(csrc/amvs_dispatch.h UnpackedRegsSourceCounts / PackedRegsSourceCounts): amvs_kernels_fast_regs.hip, built without the
compiler's packing of f32 pairs, holds S = 2 .. 5 and amvs_kernels_fast_regs_packed.hip, built as before, S = 6; every
other launch of the step stays in amvs_kernels_fast.hip.  A packed operation is the two IEEE operations it holds, so the
arithmetic cannot move; what can go wrong is a launch that reaches a kernel its unit no longer holds, or holds twice.
So every route is walked once and compared bit for bit with the CPU oracle's fast mode (depth / normal / confidence):
    S   2, 3, 4 (the unit without packing) and 6 (the unit built as before); 5, the last of the first unit's list, twice
    K   3, 7, 11 (both register sources by default), 13 (register sources only when forced), 17 (none compiled: the
        launch must stay in amvs_kernels_fast.hip whatever the switch says)
    the paired schedule (compiled up to 11 x 11 and four sources) and the classic one
    the four settings of amvs_set_step_sources, with amvs_get_step_sources asserting which path ran
    one split-schedule call per unit, and single steps of every mode: propagation with all four offsets (both parities),
    refinement, cost evaluation and confidence (the last two: the run-time-mode instantiations)
on images of W 7 / 59 / 117 (narrower than a strip; one column into a second 7x7 strip; three strips) and H 7 / 13 / 37
in bands of 6 rows (a one-row lower band; a pair and an odd one-row band; three pairs and a one-row band whose partner
band is short) -- the shape families of tests/test_hip_step_gather_issue.py.
"""
import numpy as np
import pytest

from test_hip_fullsize_parity import _eq
from test_hip_step_ref_stats import NAMES, SEED, SOURCES, _case

pytestmark = pytest.mark.gpu

ROWS = 6
REGS_MAX_PATCH = 15          # a forced setting of the switch holds up to here (amvs_step_sources_max_patch)

#        W    H   K  S  schedule
CASES = [(7, 7, 7, 4, "paired"),
         (59, 13, 7, 2, "paired"),
         (117, 37, 7, 3, "paired"),
         (59, 37, 3, 4, "paired"),
         (117, 7, 3, 3, "paired"),
         (117, 13, 11, 4, "paired"),
         (7, 37, 11, 2, "paired"),
         (59, 13, 7, 6, "view-major"),
         (117, 37, 7, 4, "view-major"),
         (7, 13, 3, 6, "view-major"),
         (59, 37, 3, 2, "view-major"),
         (117, 7, 11, 6, "view-major"),
         (59, 37, 11, 3, "view-major"),
         (59, 7, 13, 6, "view-major"),
         (117, 13, 13, 4, "view-major"),
         (7, 37, 13, 2, "view-major"),
         (59, 37, 17, 6, "view-major"),
         (117, 13, 17, 3, "view-major"),
         (7, 7, 17, 4, "view-major"),
         (59, 13, 7, 5, "view-major"),
         (117, 37, 11, 5, "view-major")]

#               W    H   K  S
STEP_CASES = [(7, 7, 3, 6), (59, 13, 7, 4), (59, 7, 7, 6), (117, 37, 11, 6), (59, 37, 13, 3), (117, 13, 17, 2), (7, 37, 11, 2)]
OFFSETS = [(1, 0), (0, 1), (-1, 0), (0, -1)]


def _expected_sources(K, src):
    """What amvs_get_step_sources reports for a forced setting: held where the variants are compiled, none beyond."""
    return src if K <= REGS_MAX_PATCH else (False, False)


def test_the_cases_cover_what_the_docstring_says():
    """(no GPU work: the lists above against the axes they claim)"""
    for cases in (CASES, STEP_CASES):
        assert {c[0] for c in cases} == {7, 59, 117} and {c[1] for c in cases} == {7, 13, 37}
        assert {c[2] for c in cases} == {3, 7, 11, 13, 17} and {c[3] for c in cases} >= {2, 3, 4, 6}
    assert {(c[2], c[3]) for c in CASES if c[4] == "paired"} >= {(3, 4), (7, 2), (7, 3), (7, 4), (11, 4)}
    assert all(c[2] <= 11 and c[3] <= 4 for c in CASES if c[4] == "paired")          # (beyond, the call runs classic)
    for k in (3, 7, 11, 13, 17):
        classic = {c[3] for c in CASES if c[2] == k and c[4] == "view-major"}          # both units at every patch size
        assert 6 in classic and classic & {2, 3, 4}, k


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
            assert eng.step_sources(K) == _expected_sources(K, src)
            got = eng.patchmatch([0], [srcs], p, SEED)
            assert eng.last_tile_rows() == ROWS
            for g, w, name in zip(got, want, NAMES):
                _eq(g[0], w, f"{W}x{H} k={K} S={S} rows={ROWS} {schedule} (ref_stats, centre_depth) = {src}: {name} vs oracle")


@pytest.mark.parametrize("W,H,K,S", STEP_CASES)
def test_single_steps_of_every_mode_are_the_oracles(W, H, K, S):
    """One propagation step of each of the four offsets (both parities) and one refinement step through the single-step
    entry points -- depth, normal and cost -- and the evaluated cost and the confidence of the depth map, for the four
    settings of the switch."""
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
        eng.set_step_tuning(tile_rows=[(ROWS, ROWS)])
        for src in SOURCES:
            eng.set_step_sources(*src)
            assert eng.step_sources(K) == _expected_sources(K, src)
            what = f"{W}x{H} k={K} S={S} (ref_stats, centre_depth) = {src}"
            _eq(eng.eval_cost(0, srcs, K, depth), cost, f"{what}: evaluated cost vs oracle")
            _eq(eng.confidence(0, srcs, K, depth), conf, f"{what}: confidence vs oracle")
            got = [eng.propagate_step(0, srcs, K, depth, normal, cost, oy, ox, sc.depth_min) for oy, ox in OFFSETS]
            got.append(eng.refine_step(0, srcs, K, depth, normal, cost, SEED, 0, draw, dr, nr, sc.depth_min, sc.depth_max))
            for g, w, step in zip(got, want, steps):
                for a, b, name in zip(g, w, ("depth", "normal", "cost")):
                    _eq(a, b, f"{what}: {step} {name} vs oracle")


@pytest.mark.parametrize("S", [4, 6])
def test_split_schedule_is_the_oracles(S):
    """The split schedule with the statistics from the registers: its window half is the PRE instantiation of the
    register-source units, one call per unit."""
    from amvs.engine import make_pm_params
    W, H, K = 59, 13, 7
    case = _case(W, H, S, "random")
    sc = case.scene
    srcs = list(range(1, S + 1))
    want = case.oracle_ctx(0, srcs, K, mode="fast").patchmatch(2, 1, sc.depth_min, sc.depth_max, SEED, 0)
    with case.engine("fast") as eng:
        eng.set_step_sources(True, True)
        assert eng.step_sources(K) == (True, True)
        got = eng.patchmatch([0], [srcs], make_pm_params(K, 2, 1, sc.depth_min, sc.depth_max, mode="fast", schedule="split"), SEED)
        for g, w, name in zip(got, want, NAMES):
            _eq(g[0], w, f"{W}x{H} k={K} S={S} split schedule: {name} vs oracle")
