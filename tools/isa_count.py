#!/usr/bin/env python3
"""Static instruction counts of one kernel in a tools/isa_snapshot.sh dump, by issue class.

    tools/isa_count.py tools/build/isa/flock_rollout_w64.s env_rollout_w64ILi0ELi64EfLb1ELb1EE [other.s]

Counts every instruction between the kernel's label and its end once (no trip counts, both sides of
every branch): the difference between two snapshots of the same kernel is what a change to
straight-line code of the step removed or added. With a second file, prints both and the difference.
"""
import collections
import re
import sys

TRANS = ("v_rcp_", "v_rsq_", "v_sqrt_", "v_exp_", "v_log_", "v_sin_", "v_cos_")


def classes(op):
    out = []
    if op.startswith("v_"):
        out.append("VALU")
        if "_f64" in op:
            out.append("VALU f64")
        if op.startswith(TRANS):
            out.append("transcendental")
        if op.startswith("v_div_"):
            out.append("v_div_*")
        if op.startswith("v_cndmask"):
            out.append("v_cndmask")
        if op.startswith("v_mov_") or op.startswith("v_accvgpr"):
            out.append("v_mov")
        if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
            out.append("v_readlane/writelane")
        if op.startswith("v_cmp"):
            out.append("v_cmp")
    elif op.startswith("s_"):
        if not op.startswith(("s_waitcnt", "s_nop", "s_endpgm", "s_code_end")):
            out.append("SALU+branch")
    elif op.startswith("ds_"):
        out.append("LDS")
    elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        out.append("VMEM")
    return out


def count(path, kernel):
    c = collections.Counter()
    inside = False
    for line in open(path):
        s = line.split(";")[0].strip()
        if not inside:
            inside = s.endswith(":") and kernel in s and not s.startswith(".")
            continue
        if s.startswith(".Lfunc_end") or s.startswith(".section"):
            break
        m = re.match(r"([vs]_\w+|ds_\w+|global_\w+|buffer_\w+|flat_\w+|scratch_\w+)\b", s)
        if m:
            for k in classes(m.group(1)):
                c[k] += 1
    if not c:
        sys.exit(f"{path}: no kernel matching {kernel}")
    return c


def main():
    a = count(sys.argv[1], sys.argv[2])
    b = count(sys.argv[3], sys.argv[2]) if len(sys.argv) > 3 else None
    keys = ["VALU", "VALU f64", "transcendental", "v_div_*", "v_cndmask", "v_mov", "v_cmp", "v_readlane/writelane",
            "SALU+branch", "LDS", "VMEM"]
    for k in keys:
        if b is None:
            print(f"{k:22s} {a[k]:6d}")
        else:
            print(f"{k:22s} {a[k]:6d} {b[k]:6d} {b[k] - a[k]:+6d}")


if __name__ == "__main__":
    main()
