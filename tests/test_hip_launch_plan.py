"""The automatic launch plan against REAL occupancy (csrc/amvs_launch_plan.h; its arithmetic alone is pinned on the
host by tests/test_launch_plan_cpu.py, where the resident waves per CU are an input).  Every case is one call at the
smallest shape that reaches a branch of the policy -- one iteration of one sample, or a plane sweep of a few planes --
and asserts (views per launch, strip rows, sweep launches).  The expected values are literals recorded from the
library as it stood BEFORE the policy moved into that header: they pin the plan, they are not a new behaviour.
A plane sweep does not touch the views per launch: a fresh context reports 0.
"""
import numpy as np
import pytest

from test_hip_fullsize_parity import _u8_scene

pytestmark = pytest.mark.gpu

N_VIEWS, S = 9, 4
SIZES = {"small": (97, 131), "wide": (40, 2100), "wider": (40, 3100)}     # beyond 2048 and beyond 3072 columns
PLANES = 6

# name -> (size, mode, what runs)
CASES = {
    "fast_k7_8refs": ("small", "fast", dict(k=7, n_ref=8)),                       # groups of four
    "exact_k7_8refs": ("small", "exact", dict(k=7, n_ref=8)),                     # the whole batch
    "fast_k7_6refs": ("small", "fast", dict(k=7, n_ref=6)),                       # 6 % 4 != 0: the whole batch
    "fast_k3": ("small", "fast", dict(k=3, n_ref=8)),                             # classic
    "fast_k5": ("small", "fast", dict(k=5, n_ref=8)),                             # paired
    "fast_k9": ("small", "fast", dict(k=9, n_ref=8)),                             # classic, the whole batch
    "fast_k7_band_major": ("small", "fast", dict(k=7, n_ref=8, schedule="band-major")),
    "fast_k7_caps_only": ("small", "fast", dict(k=7, n_ref=8, caps=[(2, 1)])),
    "exact_k7_caps_only": ("small", "exact", dict(k=7, n_ref=8, caps=[(2, 1)])),
    "fast_k31": ("small", "fast", dict(k=31, n_ref=8)),                           # the run-time-k kernels
    "exact_k31": ("small", "exact", dict(k=31, n_ref=8)),
    "fast_k7_2100_columns": ("wide", "fast", dict(k=7, n_ref=8)),
    "fast_k7_3100_columns": ("wider", "fast", dict(k=7, n_ref=8)),
    "fast_k7_split": ("small", "fast", dict(k=7, n_ref=8, schedule="split")),
    "sweep_k7": ("small", "exact", dict(k=7, sweep=True)),                        # 8-bit keys
    "sweep_k31": ("small", "exact", dict(k=31, sweep=True)),
    "sweep_k7_rows20": ("small", "exact", dict(k=7, sweep=True, sweep_rows=20)),
}

# (last_views_per_launch, last_tile_rows, timing()["sweep_launches"])
EXPECTED = {
    "fast_k7_8refs": (4, 8, 6),
    "exact_k7_8refs": (8, 8, 3),
    "fast_k7_6refs": (6, 8, 3),
    "fast_k3": (4, 8, 6),
    "fast_k5": (4, 8, 6),
    "fast_k9": (8, 8, 3),
    "fast_k7_band_major": (4, 14, 6),
    "fast_k7_caps_only": (4, 8, 6),
    "exact_k7_caps_only": (8, 8, 3),
    "fast_k31": (8, 8, 3),
    "exact_k31": (8, 8, 3),
    "fast_k7_2100_columns": (8, 8, 3),
    "fast_k7_3100_columns": (8, 8, 3),
    "fast_k7_split": (8, 64, 3),
    "sweep_k7": (0, 49, 1),
    "sweep_k31": (0, 25, 1),
    "sweep_k7_rows20": (0, 20, 1),
}


@pytest.fixture(scope="module")
def scenes():
    return {name: _u8_scene(N_VIEWS, h, w, 41) for name, (h, w) in SIZES.items()}


def run_case(sc, size, mode, k, n_ref=1, schedule="auto", caps=None, sweep=False, sweep_rows=0):
    import amvs
    from amvs.engine import make_pm_params
    h, w = SIZES[size]
    ids = sorted(sc.poses)
    with amvs.Engine(h, w, len(ids), sc.camera.K.astype(np.float32), mode=mode) as eng:
        for i in ids:
            eng.set_view(i, sc.grays[i], sc.poses[i].R, sc.poses[i].t)
        if sweep:
            eng.set_sweep_tuning(sweep_rows, 0)
            eng.plane_sweep(0, ids[1:1 + S], np.linspace(sc.depth_min, sc.depth_max, PLANES), k, 0.5)
        else:
            if caps:
                eng.set_step_tuning(wgs_per_cu=caps)
            refs = ids[:n_ref]
            srcs = [[j for j in ids if j != r][:S] for r in refs]
            eng.patchmatch(refs, srcs, make_pm_params(k, 1, 1, sc.depth_min, sc.depth_max, mode=mode, schedule=schedule), 5)
        return eng.last_views_per_launch(), eng.last_tile_rows(), int(eng.timing()["sweep_launches"])


@pytest.mark.parametrize("name", list(CASES))
def test_automatic_plan_is_the_recorded_one(scenes, name):
    size, mode, what = CASES[name]
    got = run_case(scenes[size], size, mode, **what)
    print(name, got)
    assert got == EXPECTED[name], name
