#!/usr/bin/env python3
"""Compare two device-assembly files (hipcc --cuda-device-only -S) function by function.

    tools/asm_diff.py before.s after.s

A function is the text from `; -- Begin function NAME` to `; -- End function` (code and the .amdhsa_kernel
descriptor).  Functions are matched by mangled name, because the order of emission -- and with it the ordinal in
local labels -- follows the order in which host code names the instantiations.  Before comparing, the ordinal in
.LBB<n>_, .Lfunc_begin<n>, .Lfunc_end<n>, .Ltmp<n>, .LJTI<n>_ is replaced and `;` comments are dropped.
Prints the counts and the first difference; exit status 1 if the name sets or any body differ."""
import re
import sys

BEGIN = re.compile(r"; -- Begin function (\S+)")
LABEL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|Ltmp|LJTI)\d+")


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
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
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
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
    return 1 if only_a or only_b or differing else 0


if __name__ == "__main__":
    sys.exit(main())
