#!/usr/bin/env python
"""Per-workgroup timeline of the sweep launches of one PatchMatch step (needs a library built with
-DAMVS_STEP_TRACE -- ALL=1 tools/build_variant.sh trace -DAMVS_STEP_TRACE -- and selected with AMVS_LIB).

    AMVS_LIB=$PWD/build/variants/libamvs_trace.so python tools/step_timeline.py tools/plans/timeline.txt

Plan line:  tag | views height width mode edge_first group_overlap      ('#' starts a comment)

One step of the bench configuration (8 iterations x (2 propagation + 8 refinement) launches per view group) is run
once to warm up and once traced.  Wave 0 of every workgroup recorded the 100 MHz wall clock at entry and before
exit and the XCC it ran on (include/amvs.h amvs_fetch_step_trace).  Per launch kind and iteration (mean over the
launches of that kind and over the view groups) the script prints
    span      first entry to last exit of the launch, us
    wg        mean workgroup duration, us
    slots     the largest number of workgroups resident at once (the launch's slot capacity as it ran)
    used      sum of workgroup durations / (slots x span): the slot-time that held a workgroup
    ramp      empty slot-time before the slots first fill (share of slots x span)
    turnover  empty slot-time between the first fill and the moment the last workgroup has started
    tail      empty slot-time after the last workgroup has started
and, for the last iteration, resident workgroups per XCC over time and the mean workgroup duration by band row.
With overlapping view groups the launches of two groups share the chip: the per-launch figures then describe one
group's launches, and the line "step" gives first entry to last exit over the whole call.
"""
import sys

import numpy as np

sys.path.insert(0, ".")


def launch_stats(rec):
    """rec: (blocks, 4) records of one launch -> dict, or None for an empty launch."""
    rec = rec[rec[:, 0] > 0]
    if len(rec) == 0:
        return None
    t0 = rec[:, 0].astype(np.int64)
    t1 = rec[:, 1].astype(np.int64)
    ok = t1 >= t0
    t0, t1, rec = t0[ok], t1[ok], rec[ok]
    start, end = t0.min(), t1.max()
    span = float(end - start)
    # resident workgroups over time
    ev = np.concatenate([np.stack([t0, np.ones_like(t0)], 1), np.stack([t1, -np.ones_like(t1)], 1)])
    ev = ev[np.lexsort((-ev[:, 1], ev[:, 0]))]
    res = np.cumsum(ev[:, 1])
    slots = int(res.max())
    tt = ev[:, 0]
    dt = np.diff(np.concatenate([tt, [end]])).astype(np.float64)
    empty = (slots - res) * dt                       # empty slot-time after each event
    t_full = tt[np.argmax(res >= slots)]             # slots first full
    t_last = t0.max()                                # last workgroup has started
    ramp = empty[tt < t_full].sum()
    tail = empty[tt >= t_last].sum()
    turnover = empty.sum() - ramp - tail
    cap = slots * span if span > 0 else 1.0
    return {"span_us": span / 100.0, "wg_us": float((t1 - t0).mean()) / 100.0, "slots": slots, "n": len(rec),
            "used": float((t1 - t0).sum()) / cap, "ramp": ramp / cap, "turnover": turnover / cap, "tail": tail / cap,
            "start": start, "end": end, "t0": t0, "t1": t1, "xcc": (rec[:, 2] & 0xF).astype(np.int64),
            "row": ((rec[:, 3] >> 20) & 0xFFFFF).astype(np.int64)}


def run_cell(tag, views, H, W, mode, edge_first, overlap, iters=8, samples=8):
    import amvs
    from amvs.engine import make_pm_params
    from amvs.synthetic import make_scene

    sc = make_scene(views, H, W, seed=1234, device="cuda")
    ids = sorted(sc.poses)
    pm = amvs.PatchMatchMVS.__new__(amvs.PatchMatchMVS)
    sources = [pm._select_source_views(r, ids, sc.poses, k=4) for r in ids]
    with amvs.Engine(H, W, views, sc.camera.K.astype(np.float32), mode=mode) as eng:
        for i in ids:
            g = (np.round(sc.grays[i] * 255.0).clip(0, 255).astype(np.uint8)).astype(np.float32) / np.float32(255.0)
            eng.set_view(i, g, sc.poses[i].R, sc.poses[i].t)
        eng.set_launch_order(edge_first, overlap)
        p = make_pm_params(7, iters, samples, sc.depth_min, sc.depth_max)
        import torch
        outs = [torch.empty(views * H * W * c, dtype=torch.float32, device="cuda") for c in (1, 3, 1)]
        for _ in range(2):
            eng.patchmatch_device(ids, sources, p, 42, *[o.data_ptr() for o in outs])
            eng.sync()
        t = eng.timing()
        trace = eng.step_trace()
        vpl, rows = eng.last_views_per_launch(), eng.last_tile_rows()
    if trace is None:
        sys.exit("this library records no trace: build it with -DAMVS_STEP_TRACE and select it with AMVS_LIB")
    per_group = iters * (2 + samples)
    groups = trace.shape[0] // per_group
    print(f"== {tag}: {views} x {W}x{H} {mode}, edge_first={edge_first} group_overlap={overlap}; {groups} groups of {vpl} views, "
          f"{rows} rows per strip; sweep {t['sweep_ms']:.3f} ms over {t['sweep_launches']} launches "
          f"({t['sweep_ms'] / max(t['sweep_launches'], 1) * 1e3:.1f} us per launch)")
    stats = [launch_stats(trace[i]) for i in range(trace.shape[0])]
    live = [s for s in stats if s]
    print(f"step: first entry to last exit {(max(s['end'] for s in live) - min(s['start'] for s in live)) / 1e5:.3f} ms")
    print("kind   iter   span_us   wg_us  slots  blocks   used    ramp  turnover   tail   (empty = ramp + turnover + tail)")
    tot = {k: 0.0 for k in ("used", "ramp", "turnover", "tail")}
    n_tot = 0
    for it in range(iters):
        for kind, sl in (("PROP", range(0, 2)), ("REFINE", range(2, 2 + samples))):
            sel = [stats[g * per_group + it * (2 + samples) + j] for g in range(groups) for j in sl]
            sel = [s for s in sel if s]
            m = {k: float(np.mean([s[k] for s in sel])) for k in ("span_us", "wg_us", "slots", "n", "used", "ramp", "turnover", "tail")}
            print(f"{kind:6s} {it:4d} {m['span_us']:9.1f} {m['wg_us']:7.1f} {m['slots']:6.0f} {m['n']:7.0f} {m['used']:6.3f} "
                  f"{m['ramp']:7.3f} {m['turnover']:8.3f} {m['tail']:7.3f}")
            for s in sel:
                for k in tot:
                    tot[k] += s[k] * s["span_us"]
                n_tot += s["span_us"]
    print("all launches, weighted by span: " + "  ".join(f"{k} {v / n_tot:.3f}" for k, v in tot.items()))
    # gaps between consecutive launches of one group (kernel boundaries)
    gaps = []
    for g in range(groups):
        ss = [s for s in stats[g * per_group:(g + 1) * per_group] if s]
        gaps += [(b["start"] - a["end"]) / 100.0 for a, b in zip(ss, ss[1:])]
    print(f"kernel boundary (last exit of a launch to first entry of the group's next): mean {np.mean(gaps):.2f} us, "
          f"max {np.max(gaps):.2f} us; {len(gaps)} boundaries = {np.sum(gaps) / 1e3:.3f} ms of the step")
    # last refinement launch of group 0: per-XCC residency over time, duration by band row
    s = stats[per_group - 1]
    nb = 10
    edges = np.linspace(s["start"], s["end"], nb + 1)
    print(f"last REFINE launch of group 0 ({s['span_us']:.1f} us): resident workgroups per XCC in {nb} equal time slices")
    for x in sorted(set(s["xcc"].tolist())):
        m = s["xcc"] == x
        occ = [float(np.clip(np.minimum(s["t1"][m], edges[i + 1]) - np.maximum(s["t0"][m], edges[i]), 0, None).sum()
                     / max(edges[i + 1] - edges[i], 1)) for i in range(nb)]
        print(f"  xcc {x}: " + " ".join(f"{o:6.1f}" for o in occ) + f"   blocks {int(m.sum())}")
    print("mean workgroup duration by band row of the workgroup's first wave (us; all REFINE launches of the last iteration):")
    sel = [stats[g * per_group + (iters - 1) * (2 + samples) + j] for g in range(groups) for j in range(2, 2 + samples)]
    rows_all = np.concatenate([x["row"] for x in sel if x])
    dur_all = np.concatenate([(x["t1"] - x["t0"]) / 100.0 for x in sel if x])
    print("  " + " ".join(f"{r}:{dur_all[rows_all == r].mean():.0f}" for r in sorted(set(rows_all.tolist()))))
    sys.stdout.flush()


def main():
    plan = sys.argv[1]
    for line in open(plan):
        line = line.split("#")[0].strip()
        if "|" not in line:
            continue
        tag, args = [x.strip() for x in line.split("|", 1)]
        views, H, W, mode, edge_first, overlap = args.split()
        run_cell(tag, int(views), int(H), int(W), mode, int(edge_first), int(overlap))


if __name__ == "__main__":
    main()
