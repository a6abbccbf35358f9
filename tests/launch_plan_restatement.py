"""An independent statement of the launch policy of the PatchMatch sweep steps and the plane sweep, in plain Python,
written from the text of the policy as it stood when it still lived inside the entry points (the head of
csrc/amvs_capi.hip, the plane-sweep entry point, step_regs of csrc/amvs_context.hip).  tests/test_launch_plan_cpu.py
compares it field for field with what csrc/amvs_launch_plan.h computes (amvs_plan_patchmatch / amvs_plan_plane_sweep).

Inputs are dicts keyed as include/amvs_plan.h names them: dev (H, W, n_cu, packed_maps), call (n_ref, n_src, fast and the
amvs_pm_params fields), tun (the setters' knobs; tune_rows / tune_cap flat lists), facts (out_width, waves_per_cu[9],
patch_compiled, pair_supported, fast_pair_supported, fast_regs_supported, the sweep_max_* limits).  All integers are
Python integers (the C side stays far from 2^31 on the test's grid); the policy's floating point is double, as Python's.
"""
import math

import numpy as np

SCHED_AUTO, SCHED_VIEW_MAJOR, SCHED_BAND_MAJOR, SCHED_SPLIT, SCHED_PAIRED = range(5)
PROP, REFINE = 1, 2


def cdiv(a, b):
    return -(-a // b)


def views_per_launch_auto(W, n_ref, patch, fast):
    if fast and patch <= 7 and W <= 2048 and n_ref >= 8 and n_ref % 4 == 0:
        return 4
    return min(n_ref, 32)


def tile_rows(dev, facts, patch, n_jobs, requested, cap, wg_cap=0, paired=False):
    """Rows per wave strip: the height up to the locality cap with the best (fill of the last generation of resident
    waves) x (useful fraction of the sampled rows); ties go to the taller strip."""
    if requested > 0:
        return min(requested, cap)
    H, W = dev["H"], dev["W"]
    cols = cdiv(W, facts["out_width"])
    slots = dev["n_cu"] * facts["waves_per_cu"][wg_cap]
    if paired:
        tall = max(3 * patch - 3, 8)
        wide = W > 3072
    else:
        tall = max(4 * patch - 4, 12)
        wide = W > 2048
    if wide:
        tall = max(tall * 2 // 3, 8)
    tall = min(tall, cap)
    lowest = min(tall, 8)
    best, best_score = lowest, -1.0
    th = tall
    while th >= lowest:
        bands = cdiv(H, th)
        g = float(n_jobs * cols * bands) / float(slots)
        if g > 1.0:
            fill = g / math.ceil(g)
        elif g >= 0.75:
            fill = 1.0
        else:
            fill = g / 0.75
        if paired:
            sampled = float(bands // 2) * (2 * th + patch - 1) + float(bands % 2) * (th + patch - 1)
            useful = float(H) / sampled
        else:
            useful = float(th) / float(th + patch - 1)
        score = fill * useful
        if score > best_score + 1e-9:
            best, best_score = th, score
        th -= 2
    return best


def band_rows(dev, facts, patch, n_jobs):
    """Band-major: one band of all views of the launch about fills an XCD's wave slots."""
    cols = cdiv(dev["W"], facts["out_width"])
    slots_xcd = max(dev["n_cu"] // 8, 1) * facts["waves_per_cu"][0]
    together = max(slots_xcd // (n_jobs * cols), 1)
    return max(cdiv(dev["H"], 8 * together), 2 * patch, 8)


def table_entry(table, it, refine):
    """amvs_set_step_tuning: [iteration][0 = propagation, 1 = refinement]; beyond the table its last row; 0 = automatic."""
    if not table:
        return 0
    idx = 2 * it + (1 if refine else 0)
    if idx < len(table):
        return table[idx]
    return table[len(table) - 2 + (1 if refine else 0) if len(table) >= 2 else 0]


def schedule(call):
    """The launches of one view group: per iteration two propagations then num_samples refinements."""
    steps = []
    first, n, samples = call["first_iteration"], call["num_iterations"], call["num_samples"]
    for it in range(first, first + n):
        sgn = 1 if it % 2 == 0 else -1
        steps.append(dict(mode=PROP, oy=sgn, ox=0, depth_range=np.float32(0), normal_range=np.float32(0), draw=0, flip_d=1, iter=it))
        steps.append(dict(mode=PROP, oy=0, ox=sgn, depth_range=np.float32(0), normal_range=np.float32(0), draw=0, flip_d=1, iter=it))
        # ranges formed in double from the float32 depth limits, cast once
        span = float(np.float32(call["depth_max"])) - float(np.float32(call["depth_min"]))
        dr = np.float32(span * 0.5 ** it)
        nr = np.float32(0.5 * 0.5 ** it)
        for s in range(samples):
            steps.append(dict(mode=REFINE, oy=0, ox=0, depth_range=dr, normal_range=nr, draw=1 + it * samples + s, flip_d=1, iter=it))
    return steps


def step_sources(tun, facts, patch):
    if not facts["fast_regs_supported"]:
        return 0, 0
    auto = 1 if patch <= 11 else 0
    stats = auto if tun["ref_stats_source"] < 0 else int(tun["ref_stats_source"] != 0)
    hist = auto if tun["depth_source"] < 0 else int(tun["depth_source"] != 0)
    return stats, hist


def plan_patchmatch(dev, call, tun, facts):
    """(plan, steps) with the fields of amvs_pm_plan / amvs_plan_step."""
    H, W = dev["H"], dev["W"]
    n_ref, patch, fast = call["n_ref"], call["patch_size"], bool(call["fast"])
    steps = schedule(call)
    parity = len(steps) % 2
    cols = cdiv(W, facts["out_width"])
    stats, hist = step_sources(tun, facts, patch)
    plan = dict(band_major=0, paired=0, overlap=0, edge_first=0, tiles_x=cols, n_steps=len(steps), final_parity=parity,
                split_groups=0, split_vpl=0, split_tile_rows=0, s_tile_rows=0, s_lds=0, s_tiles_x=0, s_tiles_y=0,
                ref_in_kernel=stats, depth_hist=hist,
                single_step_rows=tile_rows(dev, facts, patch, 1, 0, 64) if facts["waves_per_cu"][0] >= 1 else 0)
    if call["schedule"] == SCHED_SPLIT:
        if call["views_per_launch"] > 0:
            G = cdiv(n_ref, call["views_per_launch"])
        else:
            G = tun["split_groups"] if tun["split_groups"] > 0 else 2
        G = min(G, n_ref, 8)
        vpl = cdiv(n_ref, G)
        G = cdiv(n_ref, vpl)
        TH = call["tile_rows"] if call["tile_rows"] > 0 else min(H, 64)
        s_TH = tun["split_sample_rows"] if tun["split_sample_rows"] > 0 else 4
        for st in steps:
            st.update(rows=TH, wg_cap=0, tiles_y=cdiv(H, TH))
        plan.update(views_per_launch=n_ref, n_groups=1, tile_rows=TH, tiles_y=cdiv(H, TH), last_tile_rows=TH, launches=len(steps),
                    split_groups=G, split_vpl=vpl, split_tile_rows=TH, s_tile_rows=s_TH, s_lds=tun["split_sample_lds"],
                    s_tiles_x=cdiv(W, 64), s_tiles_y=cdiv(H, s_TH))
        return plan, steps
    sched = call["schedule"]
    band_major = bool(tun["default_band_major"]) if sched == SCHED_AUTO else sched == SCHED_BAND_MAJOR
    wanted = sched == SCHED_PAIRED or (sched == SCHED_AUTO and not band_major and 5 <= patch <= 7)
    compiled = facts["fast_pair_supported"] if fast else (dev["packed_maps"] and facts["pair_supported"])
    paired = bool(wanted and compiled)
    vpl = call["views_per_launch"] if call["views_per_launch"] > 0 else views_per_launch_auto(W, n_ref, patch, fast)
    vpl = min(vpl, n_ref)
    n_groups = cdiv(n_ref, vpl)
    if call["tile_rows"] > 0 or not band_major:
        TH = tile_rows(dev, facts, patch, vpl, call["tile_rows"], 1 << 20, 0, paired)
    else:
        TH = band_rows(dev, facts, patch, vpl)
    last = TH
    for st in steps:
        rows, cap = TH, 0
        if not band_major:
            refine = st["mode"] == REFINE
            t_rows, t_cap = table_entry(tun.get("tune_rows"), st["iter"], refine), table_entry(tun.get("tune_cap"), st["iter"], refine)
            cap = t_cap if t_cap > 0 else 0
            if call["tile_rows"] > 0:
                pass                                            # the caller fixed the strip height
            elif t_rows > 0:
                rows = t_rows
            elif t_cap > 0:
                rows = tile_rows(dev, facts, patch, vpl, 0, 1 << 20, t_cap)
        st.update(rows=rows, wg_cap=cap, tiles_y=cdiv(H, rows))
        last = rows
    overlap = tun["group_overlap"] if n_groups > 1 else 0
    edge_first = (1 if overlap else 0) if tun["edge_first"] < 0 else tun["edge_first"]
    plan.update(band_major=int(band_major), paired=int(paired), views_per_launch=vpl, n_groups=n_groups, tile_rows=TH,
                tiles_y=cdiv(H, TH), overlap=overlap, edge_first=edge_first, last_tile_rows=last, launches=n_groups * len(steps))
    return plan, steps


def plan_plane_sweep(dev, tun, facts, n_ref, D):
    """The fields of amvs_sweep_plan: the fewest evenly high bands of at most 64 rows with 8-bit keys (compiled patches,
    chunks of at most sweep_max_chunk8 planes) or 32 rows with 16-bit keys; even chunks for ~8 waves per slot."""
    H, W = dev["H"], dev["W"]
    cols = cdiv(W, facts["out_width"])
    forced = tun["sweep_tile_rows"]

    def shape(max_rows):
        TH = cdiv(H, cdiv(H, max_rows))
        if 1 <= forced <= max_rows and forced < H:
            TH = forced
        tiles_y = cdiv(H, TH)
        strips = n_ref * cols * tiles_y
        slots = dev["n_cu"] * 16
        want = min(max(cdiv(8 * slots, strips), 1), (D + 1) // 2)
        chunk = cdiv(D, want)
        chunk = cdiv(D, cdiv(D, chunk))
        if tun["sweep_chunk"] >= 1:
            chunk = min(tun["sweep_chunk"], D)
        chunk = min(chunk, facts["sweep_max_chunk"])
        return dict(tile_rows=TH, tiles_x=cols, tiles_y=tiles_y, chunk=chunk, n_chunks=cdiv(D, chunk), key8=0)

    if facts["patch_compiled"] and tun["sweep_key8"] != 0 and (forced == 0 or forced > facts["sweep_max_th"]):
        s = shape(facts["sweep_max_th8"])
        if s["chunk"] <= facts["sweep_max_chunk8"]:
            s["key8"] = 1
            return s
    return shape(facts["sweep_max_th"])
