"""The launch policy (csrc/amvs_launch_plan.h) on the host: the plan the entry points compute -- the same functions, through
amvs_plan_patchmatch / amvs_plan_plane_sweep, with the resident waves per CU and the kernel facts as inputs -- equals an
independent restatement (tests/launch_plan_restatement.py) field for field, exactly, on a seeded sample of a grid that
crosses every branch of the policy; depth_range / normal_range are compared as float32 bits.  No GPU involved."""
import itertools
import random

import numpy as np
import pytest

import launch_plan_restatement as R

H_ = [40, 97, 1080, 2160]
W_ = [100, 131, 1920, 2100, 3100, 3840]           # both wide-image thresholds, 2048 and 3072
N_CU = [4, 8, 256]
N_REF = [1, 2, 5, 8, 12, 16, 32, 40]
N_SRC = [2, 4, 6]
PATCH = [3, 5, 7, 9, 11, 13, 29, 31]
WAVES = [4, 8, 16, 20]
TABLES = ["absent", "rows", "caps", "both", "short"]
LIMITS = dict(sweep_max_th=32, sweep_max_th8=64, sweep_max_chunk=4096, sweep_max_chunk8=32)
DEPTH_MIN, DEPTH_MAX = 0.7, 13.1


def test_header_matches_its_table_and_every_symbol_is_exported():
    """include/amvs_plan.h declares exactly what _lib.PLAN_SIGNATURES binds, the library exports it, and include/amvs.h
    keeps its own symbols."""
    import ctypes
    import os
    import re
    from amvs import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "amvs_plan.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(amvs_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.PLAN_SIGNATURES) == {"amvs_plan_patchmatch", "amvs_plan_plane_sweep"}
    assert not declared & set(_lib.SIGNATURES)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} not exported"


def _device(rng):
    return dict(H=rng.choice(H_), W=rng.choice(W_), n_cu=rng.choice(N_CU), packed_maps=rng.choice([0, 1]))


def _facts(rng, patch):
    base = rng.choice(WAVES)
    # entry w: the residency under a cap of w workgroups of four waves
    return dict(out_width=64 - 2 * (patch // 2), waves_per_cu=[base] + [min(base, 4 * w) for w in range(1, 9)],
                patch_compiled=int(patch <= 29), pair_supported=rng.choice([0, 1]), fast_pair_supported=rng.choice([0, 1]),
                fast_regs_supported=rng.choice([0, 1]), **LIMITS)


def _tuning(rng, n_iterations):
    kind = rng.choice(TABLES)
    n = 1 if kind == "short" else rng.choice([1, n_iterations, n_iterations + 1])
    rows = [rng.choice([0, 6, 10, 14]) for _ in range(2 * n)] if kind in ("rows", "both", "short") else None
    caps = [rng.choice([0, 1, 2, 3, 8]) for _ in range(2 * n)] if kind in ("caps", "both", "short") else None
    split = rng.choice([(0, 0, 0), (3, 8, 1024)])
    t = dict(default_band_major=rng.choice([0, 0, 1]), split_groups=split[0], split_sample_rows=split[1], split_sample_lds=split[2],
             edge_first=rng.choice([-1, 0, 1]), group_overlap=rng.choice([0, 1, 2]), sweep_tile_rows=rng.choice([0, 20, 48]),
             sweep_chunk=rng.choice([0, 5]), sweep_key8=rng.choice([0, 1]), ref_stats_source=rng.choice([-1, 0, 1]),
             depth_source=rng.choice([-1, 0, 1]))
    if rows:
        t["tune_rows"] = rows
    if caps:
        t["tune_cap"] = caps
    return kind, t


def _call(rng):
    return dict(n_ref=rng.choice(N_REF), n_src=rng.choice(N_SRC), fast=rng.choice([0, 1]), patch_size=rng.choice(PATCH),
                num_iterations=rng.choice([1, 3]), num_samples=rng.choice([0, 3]), tile_rows=rng.choice([0, 0, 11]),
                views_per_launch=rng.choice([0, 0, 2, 3]), schedule=rng.choice([0, 1, 2, 3, 4]), first_iteration=rng.choice([0, 2]),
                depth_min=DEPTH_MIN, depth_max=DEPTH_MAX)


def _native_patchmatch(dev, call, tun, facts):
    from amvs import _lib
    c = dict(call)
    p = _lib.PmParams(patch_size=c.pop("patch_size"), num_iterations=c.pop("num_iterations"), num_samples=c.pop("num_samples"),
                      tile_rows=c.pop("tile_rows"), views_per_launch=c.pop("views_per_launch"), depth_min=c.pop("depth_min"),
                      depth_max=c.pop("depth_max"), schedule=c.pop("schedule"), first_iteration=c.pop("first_iteration"))
    return _lib.plan_patchmatch(dev, dict(p=p, **c), tun, facts)


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def test_patchmatch_plan_equals_the_restatement():
    rng = random.Random(20240521)
    seen = {k: set() for k in ("H", "W", "n_cu", "n_ref", "n_src", "patch", "fast", "packed", "schedule", "waves", "tile_rows",
                               "vpl_asked", "first", "samples", "table", "overlap_asked", "edge_asked", "split_set",
                               "paired", "band_major", "vpl", "overlap", "edge_first", "wg_cap", "regs")}
    for _ in range(4000):
        dev, call = _device(rng), _call(rng)
        facts = _facts(rng, call["patch_size"])
        kind, tun = _tuning(rng, call["num_iterations"])
        plan, steps = _native_patchmatch(dev, call, tun, facts)
        want_plan, want_steps = R.plan_patchmatch(dev, call, tun, facts)
        tag = f"dev={dev} call={call} tuning={tun} facts={facts}"
        assert plan == want_plan, f"{tag}: {[(k, plan[k], want_plan[k]) for k in plan if plan[k] != want_plan[k]]}"
        assert len(steps) == len(want_steps), tag
        for got, want in zip(steps, want_steps):
            for k in ("depth_range", "normal_range"):
                assert _bits(got.pop(k)) == _bits(want.pop(k)), f"{tag}: {k} of iteration {got['iter']}"
            assert got == want, tag
        # properties that need no restatement
        vpl, n_groups, n_ref = plan["views_per_launch"], plan["n_groups"], call["n_ref"]
        assert vpl * n_groups >= n_ref > vpl * (n_groups - 1), tag
        assert all(s["rows"] >= 1 and s["tiles_y"] * s["rows"] >= dev["H"] > (s["tiles_y"] - 1) * s["rows"] for s in steps), tag
        assert plan["launches"] == n_groups * len(steps), tag
        assert len(steps) == call["num_iterations"] * (2 + call["num_samples"]), tag
        assert plan["overlap"] == 0 or n_groups > 1, tag
        assert plan["last_tile_rows"] == (steps[-1]["rows"] if steps else plan["tile_rows"]), tag
        for k, v in (("H", dev["H"]), ("W", dev["W"]), ("n_cu", dev["n_cu"]), ("n_ref", n_ref), ("n_src", call["n_src"]),
                     ("patch", call["patch_size"]), ("fast", call["fast"]), ("packed", dev["packed_maps"]),
                     ("schedule", call["schedule"]), ("waves", facts["waves_per_cu"][0]), ("tile_rows", call["tile_rows"]),
                     ("vpl_asked", call["views_per_launch"]), ("first", call["first_iteration"]), ("samples", call["num_samples"]),
                     ("table", kind), ("overlap_asked", tun["group_overlap"]), ("edge_asked", tun["edge_first"]),
                     ("split_set", tun["split_groups"]), ("paired", plan["paired"]), ("band_major", plan["band_major"]),
                     ("vpl", vpl), ("overlap", plan["overlap"]), ("edge_first", plan["edge_first"]),
                     ("regs", (plan["ref_in_kernel"], plan["depth_hist"]))):
            seen[k].add(v)
        seen["wg_cap"].update(s["wg_cap"] for s in steps)
    # the sample reached every value of the grid and both outcomes of every decision
    assert seen["H"] == set(H_) and seen["W"] == set(W_) and seen["n_cu"] == set(N_CU) and seen["n_ref"] == set(N_REF)
    assert seen["n_src"] == set(N_SRC) and seen["patch"] == set(PATCH) and seen["waves"] == set(WAVES) and seen["table"] == set(TABLES)
    assert seen["schedule"] == {0, 1, 2, 3, 4} and seen["tile_rows"] == {0, 11} and seen["vpl_asked"] == {0, 2, 3}
    assert seen["first"] == {0, 2} and seen["samples"] == {0, 3} and seen["split_set"] == {0, 3}
    assert seen["overlap_asked"] == {0, 1, 2} and seen["edge_asked"] == {-1, 0, 1}
    for k in ("fast", "packed", "paired", "band_major", "edge_first"):
        assert seen[k] == {0, 1}, k
    assert seen["overlap"] == {0, 1, 2} and {4, 32, 40} <= seen["vpl"] and seen["wg_cap"] == {0, 1, 2, 3, 8}
    assert seen["regs"] == set(itertools.product((0, 1), repeat=2))


def test_plane_sweep_plan_equals_the_restatement():
    from amvs import _lib
    rng = random.Random(77)
    key8, rows = set(), set()
    for _ in range(3000):
        dev, patch = _device(rng), rng.choice(PATCH)
        facts = _facts(rng, patch)
        _, tun = _tuning(rng, 1)
        n_ref, D = rng.choice(N_REF), rng.choice([1, 2, 7, 64, 300])
        plan = _lib.plan_plane_sweep(dev, tun, facts, n_ref, D)
        tag = f"dev={dev} patch={patch} tuning={tun} n_ref={n_ref} D={D}"
        assert plan == R.plan_plane_sweep(dev, tun, facts, n_ref, D), tag
        assert plan["n_chunks"] * plan["chunk"] >= D > (plan["n_chunks"] - 1) * plan["chunk"], tag
        assert 1 <= plan["tile_rows"] <= (LIMITS["sweep_max_th8"] if plan["key8"] else LIMITS["sweep_max_th"]), tag
        assert plan["tiles_y"] * plan["tile_rows"] >= dev["H"] > (plan["tiles_y"] - 1) * plan["tile_rows"], tag
        if plan["key8"]:
            assert facts["patch_compiled"] and tun["sweep_key8"] and plan["chunk"] <= LIMITS["sweep_max_chunk8"], tag
        key8.add(plan["key8"])
        rows.add(plan["tile_rows"])
    assert key8 == {0, 1} and {20, 48} <= rows


def test_plans_refuse_what_they_cannot_read():
    """A workgroup cap's residency the plan would read but the caller left unfilled is an error, not a division by zero."""
    from amvs import _lib
    rng = random.Random(5)
    dev, call = _device(rng), dict(_call(rng), tile_rows=0, schedule=1, num_iterations=1)
    facts = _facts(rng, call["patch_size"])
    _, tun = _tuning(rng, 1)
    tun = dict(tun, tune_cap=[3, 3])
    tun.pop("tune_rows", None)
    _native_patchmatch(dev, call, tun, facts)
    for w in (0, 3):
        bad = dict(facts, waves_per_cu=[0 if i == w else v for i, v in enumerate(facts["waves_per_cu"])])
        with pytest.raises(_lib.AmvsError):
            _native_patchmatch(dev, call, tun, bad)
    _native_patchmatch(dev, call, tun, dict(facts, waves_per_cu=[v if i in (0, 3) else 0 for i, v in enumerate(facts["waves_per_cu"])]))
