#!/usr/bin/env python3
"""Compare two device-assembly files (hipcc --cuda-device-only -S) function by function.

    tools/asm_diff.py [--rename OLD=NEW ...] before.s after.s

A function is the text from `; -- Begin function NAME` to `; -- End function` (code and the .amdhsa_kernel
descriptor).  Functions are matched by mangled name, because the order of emission -- and with it the ordinal in
local labels -- follows the order in which host code names the instantiations.  Before comparing, the ordinal in
.LBB<n>_, .Lfunc_begin<n>, .Lfunc_end<n>, .Ltmp<n>, .LJTI<n>_ is replaced and `;` comments are dropped.
--rename OLD=NEW replaces OLD by NEW in the text of before.s first, names and bodies: a kernel renamed on purpose is
then compared with the body it had (a mangled name holds its length: 17fmat_total_kernel=19ransac_total_kernel).
Prints the counts and the first difference, and for every differing function its register, LDS and scratch lines and
the mnemonics that occur a different number of times; exit status 1 if the name sets or any body differ."""
import collections
import re
import sys

BEGIN = re.compile(r"; -- Begin function (\S+)")
SIZES = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_group_segment_fixed_size", ".amdhsa_private_segment_fixed_size")
LABEL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|Ltmp|LJTI)\d+")


def functions(path, renames=()):
    out, name, body = {}, None, []
    for line in open(path):
        for old, new in renames:
            line = line.replace(old, new)
        m = BEGIN.search(line)
        if m:
            name, body = m.group(1), []
        if name is None:
            continue
        code = LABEL.sub(r".\1N", line.split(";", 1)[0]).rstrip()
        if code:
            body.append(code)
        if "; -- End function" in line:
            out[name], name = body, None
    return out


def main():
    renames = []
    while sys.argv[1] == "--rename":
        renames.append(tuple(sys.argv[2].split("=", 1)))
        del sys.argv[1:3]
    a, b = functions(sys.argv[1], renames), functions(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differing = [n for n in sorted(set(a) & set(b)) if a[n] != b[n]]
    print(f"{sys.argv[2]}: functions {len(a)} -> {len(b)}, only before {len(only_a)}, only after {len(only_b)}, "
          f"compared {len(set(a) & set(b))}, differing {len(differing)}")
    for n in only_a[:3]:
        print("  only before:", n)
    for n in only_b[:3]:
        print("  only after: ", n)
    if differing:
        n = differing[0]
        i = next((i for i, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
        print(f"  first difference: {n}, line {i} of its body\n  - {a[n][i:i + 1]}\n  + {b[n][i:i + 1]}")
    for n in differing:
        ca, cb = (collections.Counter(x.split()[0] for x in f[n] if x[0] == "\t" and x[1] != ".") for f in (a, b))
        sizes = [[int(x.split()[1]) for k in SIZES for x in f[n] if x.split()[0] == k] for f in (a, b)]
        print(f"  {n}: lines {len(a[n])} -> {len(b[n])}, vgpr/sgpr/lds/scratch {sizes[0]} -> {sizes[1]}, mnemonic counts "
              f"{ {k: (ca[k], cb[k]) for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k]} or 'equal' }")
    return 1 if only_a or only_b or differing else 0


if __name__ == "__main__":
    sys.exit(main())
