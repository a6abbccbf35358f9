"""The dispatch order of the sweep steps is performance only (include/amvs.h amvs_set_launch_order): at a ragged
shape -- an odd number of bands, a narrow last strip column, 5 views in groups of 2 so that the last group is
short -- the maps of
    * the edge-first order on one stream,
    * the edge-first order with the view groups on two streams, equal priorities and a high / low pair,
    * the top-to-bottom order on one stream (the order before edge-first existed)
are identical BIT FOR BIT in both arithmetic modes and for every strip schedule, and they are the CPU oracle's.
A second context sweeping at the same time on the same device (its own two streams) gets its own results too.
"""
import threading

import numpy as np
import pytest

from test_hip_fullsize_parity import _eq, _u8_scene, _oracle_ctx

pytestmark = pytest.mark.gpu

H, W, N_VIEWS, K, S = 97, 131, 5, 7, 4          # 131 = 2 x 58 + 15 columns; 97 rows in bands of 11 -> 9 bands
ORDERS = [(1, 0), (1, 1), (1, 2), (0, 0)]       # (edge_first, group_overlap)


def _engine(sc, mode):
    import amvs
    ids = sorted(sc.poses)
    eng = amvs.Engine(H, W, len(ids), sc.camera.K.astype(np.float32), mode=mode)
    for i in ids:
        eng.set_view(i, sc.grays[i], sc.poses[i].R, sc.poses[i].t)
    return eng


def _batch(sc):
    ids = sorted(sc.poses)
    return ids, [[j for j in ids if j != r][:S] for r in ids]


def _params(sc, mode, schedule, tile_rows=11, vpl=2):
    from amvs.engine import make_pm_params
    return make_pm_params(K, 2, 2, sc.depth_min, sc.depth_max, mode=mode, schedule=schedule, views_per_launch=vpl,
                          tile_rows=tile_rows)


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("schedule", ["auto", "view-major", "band-major", "paired"])
def test_orders_and_overlap_give_identical_maps(mode, schedule):
    sc = _u8_scene(N_VIEWS, H, W, 77)
    refs, srcs = _batch(sc)
    p = _params(sc, mode, schedule)
    maps = {}
    with _engine(sc, mode) as eng:
        for order in ORDERS:
            eng.set_launch_order(*order)
            maps[order] = eng.patchmatch(refs, srcs, p, 11)
            assert eng.last_views_per_launch() == 2 and eng.last_tile_rows() == 11
            t = eng.timing()
            assert t["sweep_launches"] == 3 * 2 * (2 + 2)
            assert t["sweep_ms"] > 0.0
    base = maps[(0, 0)]
    for order in ORDERS[:-1]:
        for a, b, what in zip(maps[order], base, ("depth", "normal", "confidence")):
            _eq(a, b, f"{mode} {schedule} {what}: edge_first, overlap = {order} vs top-to-bottom on one stream")
    for r in (0, 4):                                   # a view of a full group and the short last group
        od, on, oc = _oracle_ctx(sc, r, srcs[r], K, mode).patchmatch(2, 2, sc.depth_min, sc.depth_max, 11, r)
        _eq(base[0][r], od, f"{mode} {schedule} view {r} depth vs oracle")
        _eq(base[2][r], oc, f"{mode} {schedule} view {r} confidence vs oracle")
        _eq(base[1][r], on, f"{mode} {schedule} view {r} normal vs oracle")


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_overlapped_union_timing_is_chip_time(mode):
    """With the groups on two streams sweep_ms is the union of the groups' intervals: it cannot exceed the time
    between the call's first and last event, which the sum of two overlapping streams could."""
    sc = _u8_scene(N_VIEWS, H, W, 77)
    refs, srcs = _batch(sc)
    p = _params(sc, mode, "auto")
    with _engine(sc, mode) as eng:
        for overlap in (0, 1, 2):
            eng.set_launch_order(1, overlap)
            eng.patchmatch(refs, srcs, p, 11)
            t = eng.timing()
            eng.set_step_timing(True)
            eng.patchmatch(refs, srcs, p, 11)
            steps = eng.step_times()
            eng.set_step_timing(False)
            assert len(steps) == t["sweep_launches"] and (steps > 0).all()
            assert t["init_ms"] >= 0 and t["confidence_ms"] > 0 and t["sweep_ms"] > 0
            if overlap:
                # a group's launches lie inside the union, so they cannot add up to more than it
                assert steps[:8].sum() <= eng.timing()["sweep_ms"] * 1.05 + 0.05


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_second_context_sweeping_at_the_same_time(mode):
    """Two contexts on one device, each with its groups on two streams of its own, driven from two threads at once
    on different scenes: each gets the maps it gets alone."""
    scenes = [_u8_scene(N_VIEWS, H, W, 77), _u8_scene(N_VIEWS, H, W, 78)]
    alone = []
    for sc in scenes:
        refs, srcs = _batch(sc)
        with _engine(sc, mode) as eng:
            eng.set_launch_order(0, 0)
            alone.append(eng.patchmatch(refs, srcs, _params(sc, mode, "auto"), 5))
    engines = [_engine(sc, mode) for sc in scenes]
    results = [[None] * 4 for _ in scenes]
    errors = []

    def work(i):
        try:
            sc, eng = scenes[i], engines[i]
            refs, srcs = _batch(sc)
            for rep in range(4):
                eng.set_launch_order(1, 1 + (rep + i) % 2)
                results[i][rep] = eng.patchmatch(refs, srcs, _params(sc, mode, "auto"), 5)
        except Exception as e:  # noqa: BLE001  (reported below, in the main thread)
            errors.append(e)

    try:
        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        for eng in engines:
            eng.close()
    assert not errors, errors
    for i in range(2):
        for rep in range(4):
            for a, b, what in zip(results[i][rep], alone[i], ("depth", "normal", "confidence")):
                _eq(a, b, f"{mode} context {i} run {rep} {what}: concurrent vs alone")


def test_handles_survive_three_context_lifetimes():
    """Every stream and event a context owns is created, reused and destroyed: one PatchMatch call each with the
    groups on one stream, on two equal streams and on a high / low pair, with the split schedule and with step
    timing on, then the engine is destroyed -- three times over in one process.  Every configuration gives the same
    maps bit for bit in every round, and within a round the three group_overlap settings agree bit for bit."""
    sc = _u8_scene(N_VIEWS, H, W, 77)
    refs, srcs = _batch(sc)
    rounds = []
    for _ in range(3):
        maps = {}
        with _engine(sc, "fast") as eng:
            for overlap in (0, 1, 2):
                eng.set_launch_order(1, overlap)
                maps[f"overlap {overlap}"] = eng.patchmatch(refs, srcs, _params(sc, "fast", "auto"), 11)
            maps["split"] = eng.patchmatch(refs, srcs, _params(sc, "fast", "split"), 11)
            eng.set_step_timing(True)
            maps["step timing"] = eng.patchmatch(refs, srcs, _params(sc, "fast", "auto"), 11)
            assert len(eng.step_times()) == eng.timing()["sweep_launches"]
        rounds.append(maps)
    for n, maps in enumerate(rounds):
        for config in maps:
            for a, b, what in zip(maps[config], rounds[0][config], ("depth", "normal", "confidence")):
                _eq(a, b, f"{config} {what}: round {n} vs round 0")
        for overlap in (1, 2):
            for a, b, what in zip(maps[f"overlap {overlap}"], maps["overlap 0"], ("depth", "normal", "confidence")):
                _eq(a, b, f"round {n} {what}: overlap {overlap} vs one stream")
