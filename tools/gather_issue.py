#!/usr/bin/env python3
"""How the fast sweep step requests the gathers of a row: the loads and the vmcnt waits of the compiled code inside
the priority window of fast_sample_sources (between `s_setprio 1` and `s_setprio 0`), per instantiation of
pm_step_fast_kernel.

    tools/gather_issue.py [--root DIR] [--asm FILE ...] [--table] [K,S,MODE,PRE,PAIR,STATS,DHIST ...]

Compiles the device assembly of the step translation units (csrc/amvs_kernels_fast.hip, csrc/amvs_kernels_fast_regs.hip
and, where the tree at DIR has it, csrc/amvs_kernels_fast_regs_packed.hip; DIR defaults to this tree; a few minutes, all at
once) with the flags of csrc/Makefile, each unit's own included (`make print-sched-flags-<unit>`), or reads assembly files
given with --asm.  An instantiation is named by its template arguments as
numbers: 7,4,2,0,1,1,1 is <7, 4, MODE_REFINE, PRE false, PAIR, STATS, DHIST> (MODE: 1 propagation, 2 refinement,
-1 the run-time mode); without any, every instantiation found is listed.  For each it prints
  * the `global_load_*` and `s_waitcnt vmcnt` instructions of the FIRST priority window, in order,
  * the number of vmcnt waits inside that window (a wait between two gathers is a round trip the row stands still for),
  * VGPRs, SGPRs, scratch bytes and the number of v_writelane / v_readlane instructions (SGPR spills into lanes),
  * in the whole kernel: packed f32 operations (v_pk_fma_f32, v_pk_add_f32, v_pk_mul_f32), v_mov_b32_e32 and s_nop.
--table prints one line per instantiation instead.  It reads wait counts and loads only; it judges nothing.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ("amvs_kernels_fast.hip", "amvs_kernels_fast_regs.hip", "amvs_kernels_fast_regs_packed.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "--cuda-device-only", "-S"]
BEGIN = re.compile(r"; -- Begin function (\S+)")
STEP = re.compile(r"pm_step_fast_kernelIL(i\d+|in\d+)EL(i\d+|in\d+)EL(i\d+|in\d+)ELb([01])ELb([01])ELb([01])ELb([01])EE")
MODES = {1: "PROP", 2: "REFINE", -1: "RUNTIME"}


def compile_units(root, extra):
    csrc = os.path.join(root, "3d-reconstruction-tool_amd", "csrc")
    tmp = tempfile.mkdtemp(prefix="gather_issue_")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    jobs = []
    for u in UNITS:
        if not os.path.exists(os.path.join(csrc, u)):
            continue
        # (a tree from before the Makefile stated them per unit has none for these units: the empty answer of a failed make)
        own = subprocess.run(["make", "-s", "-C", csrc, "print-sched-flags-" + u[:-4]], capture_output=True, text=True)
        own = own.stdout.split() if own.returncode == 0 else []
        out = os.path.join(tmp, u.replace(".hip", ".s"))
        jobs.append((out, subprocess.Popen([hipcc] + FLAGS + own + extra + [os.path.join(csrc, u), "-o", out])))
    for out, p in jobs:
        if p.wait() != 0:
            raise SystemExit(f"compiling {out} failed")
    return [out for out, _ in jobs]


def number(tok):
    return -int(tok[2:]) if tok.startswith("in") else int(tok[1:])


def step_kernels(path):
    """{(K, S, MODE, PRE, PAIR, STATS, DHIST): lines of the function} of one assembly file"""
    out, key = {}, None
    for line in open(path):
        m = BEGIN.search(line)
        if m:
            # (up to the next function: the resource comments -- NumVgprs, ScratchSize -- follow `-- End function`)
            s = STEP.search(m.group(1))
            key = tuple(number(g) if i < 3 else int(g) for i, g in enumerate(s.groups())) if s else None
            if key is not None:
                out[key] = []
        if key is not None:
            out[key].append(line.rstrip("\n"))
    return out


def describe(body):
    window, inside, done = [], False, False
    for line in body:
        code = line.split(";", 1)[0].strip()
        if not code:
            continue
        if not done and code.startswith("s_setprio"):
            if code.split()[1] == "1":
                inside = True
            elif inside:
                inside, done = False, True
            continue
        if inside and (code.startswith("global_load") or (code.startswith("s_waitcnt") and "vmcnt(" in code)):
            window.append(" ".join(code.split()))

    def field(name):
        for line in body:
            m = re.match(r";\s*" + name + r":\s*(\d+)", line.strip())
            if m:
                return int(m.group(1))
        return -1
    lanes = sum(1 for line in body if re.match(r"\s*v_(writelane|readlane)_b32", line))

    def count(pattern):
        return sum(1 for line in body if re.match(r"\s*" + pattern + r"\b", line))
    return {"pk": count(r"v_pk_(fma|add|mul)_f32"), "mov": count(r"v_mov_b32_e32"), "nop": count(r"s_nop"),
            "window": window, "waits": sum(1 for w in window if w.startswith("s_waitcnt")),
            "loads": sum(1 for w in window if w.startswith("global_load")),
            "vgpr": field("NumVgprs"), "sgpr": field("TotalNumSgprs"), "scratch": field("ScratchSize"), "lanes": lanes}


def label(key):
    k, s, mode, pre, pair, stats, dhist = key
    flags = [n for n, f in (("PRE", pre), ("PAIR", pair), ("STATS", stats), ("DHIST", dhist)) if f]
    return f"pm_step_fast_kernel<{k},{s},{MODES.get(mode, mode)}{''.join(',' + f for f in flags)}>"


def main():
    args, root, asm, table, extra = sys.argv[1:], ROOT, [], False, []
    wanted = []
    while args:
        a = args.pop(0)
        if a == "--root":
            root = args.pop(0)
        elif a == "--asm":
            while args and not args[0].startswith("--") and not re.match(r"-?\d+,", args[0]):
                asm.append(args.pop(0))
        elif a == "--table":
            table = True
        elif a.startswith("-D"):
            extra.append(a)
        else:
            wanted.append(tuple(int(x) for x in a.split(",")))
    kernels = {}
    for path in asm or compile_units(root, extra):
        kernels.update(step_kernels(path))
    missing = [w for w in wanted if w not in kernels]
    if missing:
        raise SystemExit(f"not compiled in these units: {missing}")
    print(f"# {len(kernels)} instantiations of pm_step_fast_kernel" + (f", built with {' '.join(extra)}" if extra else ""))
    every = [describe(b) for b in kernels.values()]
    print(f"# all of them: {sum(1 for d in every if d['waits'])} with vmcnt waits inside the first priority window, "
          f"{sum(1 for d in every if d['vgpr'] > 128)} above 128 VGPRs (largest at or below: {max(d['vgpr'] for d in every if d['vgpr'] <= 128)}), "
          f"{sum(1 for d in every if d['scratch'])} with scratch ({sum(d['scratch'] for d in every)} B in all), "
          f"{sum(1 for d in every if d['lanes'])} with v_writelane/v_readlane ({sum(d['lanes'] for d in every)} in all), "
          f"largest SGPR count {max(d['sgpr'] for d in every)}")
    if table:
        print("# K S mode PRE PAIR STATS DHIST : loads and vmcnt waits in the first priority window, VGPRs, SGPRs, scratch bytes, lane moves; in the kernel: packed f32 operations, v_mov_b32_e32, s_nop")
    for key in wanted or sorted(kernels):
        d = describe(kernels[key])
        if table:
            print(f"{key[0]:2d} {key[1]} {MODES.get(key[2], key[2]):7s} {key[3]} {key[4]} {key[5]} {key[6]} : loads {d['loads']} waits {d['waits']} "
                  f"vgpr {d['vgpr']} sgpr {d['sgpr']} scratch {d['scratch']} lanes {d['lanes']} pk {d['pk']} mov {d['mov']} nop {d['nop']}")
            continue
        print(f"{label(key)}: {d['waits']} vmcnt waits among {d['loads']} loads in the first priority window; "
              f"VGPRs {d['vgpr']}, SGPRs {d['sgpr']}, scratch {d['scratch']} B, v_writelane/v_readlane {d['lanes']}; "
              f"packed f32 operations {d['pk']}, v_mov_b32_e32 {d['mov']}, s_nop {d['nop']}")
        for w in d["window"]:
            print("    " + w)


if __name__ == "__main__":
    main()
