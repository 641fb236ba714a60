#!/usr/bin/env python3
"""Compare two tools/isa_snapshot.sh snapshots kernel by kernel:

    tools/isa_snapshot.sh /tmp/isa_a      # in a checkout of commit A
    tools/isa_snapshot.sh /tmp/isa_b      # in a checkout of commit B
    tools/isa_compare.py /tmp/isa_a /tmp/isa_b

A plain diff of the .isa files stops being readable once a translation unit gains a kernel: the
local labels carry the function's index within the unit (.LBB12_3, .Lfunc_end12), so every kernel
behind the new one differs in every label. Here each unit's .s is cut into its functions (from the
symbol's label to its .Lfunc_end), comments dropped and the index taken out of the labels (the long
branches' .Lpost_getpcN, numbered through the unit, likewise); per unit:
how many of A's kernels are instruction for instruction the same in B, which changed, which are gone
and how many B adds. Exit status 1 when a kernel of A changed or is gone."""
import glob
import os
import re
import sys


def functions(path):
    out, cur = {}, None
    for line in open(path):
        line = re.sub(r"\s*;.*$", "", line.rstrip("\n"))
        if not line.strip() or re.search(r"\.file|\.ident|__hip_cuid_|amdhsa\.target", line):
            continue
        m = re.match(r"^(_Z\w+):$", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if re.match(r"^\.Lfunc_end", line) or re.match(r"^\s*\.amdgpu_metadata", line):
            cur = None
        if cur:
            # (.Lpost_getpcN, the label of a long branch's s_getpc, counts through the whole unit as well)
            out[cur].append(re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_", ".LBB_", line)))
    return out


def main(a_dir, b_dir):
    bad = 0
    for a_path in sorted(glob.glob(os.path.join(a_dir, "*.s"))):
        unit = os.path.basename(a_path)
        b_path = os.path.join(b_dir, unit)
        a = functions(a_path)
        b = functions(b_path) if os.path.exists(b_path) else {}
        same = [k for k in a if b.get(k) == a[k]]
        changed = [k for k in a if k in b and b[k] != a[k]]
        gone = [k for k in a if k not in b]
        bad += len(changed) + len(gone)
        print(f"{unit[:-2]:24s} A {len(a):3d}  B {len(b):3d}  identical {len(same):3d}  "
              f"changed {len(changed)}  gone {len(gone)}  added {len([k for k in b if k not in a])}")
        for k in changed:
            print("  changed:", k)
        for k in gone:
            print("  gone:   ", k)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
