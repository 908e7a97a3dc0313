#!/usr/bin/env python3
"""Static instruction histogram of one kernel in the device assembly of a stage.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S [-D...] -o stage_align.s yaha_amd/csrc/device/stage_align.hip
    tools/rows_asm_hist.py stage_align.s _Z13k_ext_rows_pkILb0ELi256EEv7ExtArgs [more.s ...]

Prints, the files side by side: the kernel's resource figures (the assembler's comments behind the function) and the count of every vector-instruction
mnemonic -- in the row code of k_ext_rows_pk (the block that holds its sched_barriers), and in the whole function; for the pass loop the total over
every path.  (profiles/rows_sign_selectors.txt holds its output.)"""
import collections
import os
import re
import sys


def histogram(body):
    h = collections.Counter()
    for l in body:
        m = re.match(r"\s+([vs]_[a-z0-9_]+|ds_[a-z0-9_]+|global_[a-z0-9_]+|buffer_[a-z0-9_]+|scratch_[a-z0-9_]+|flat_[a-z0-9_]+)\b", l)
        if m:
            h[m.group(1)] += 1
    return h


def resources(body):
    keep = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize", "codeLenInByte")
    out = {}
    for l in body:
        m = re.match(r";\s*(\w+):\s*(\d+)", l)
        if m and m.group(1) in keep:
            out[m.group(1)] = int(m.group(2))
    return out


def regions(lines, start, end):
    """(row block, pass loop) of k_ext_rows_pk as line ranges: the row code is the stretch that holds the kernel's sched_barriers, from the label in front of
    the first to the first label or branch behind the last; the pass loop runs from the target of the first backward s_branch behind the row code to that branch."""
    sb = [i for i in range(start, end) if "sched_barrier" in lines[i]]
    if not sb:
        return None, None
    a = max(i for i in range(start, sb[0]) if lines[i].startswith(".LBB"))
    b = min(i for i in range(sb[-1], end) if lines[i].startswith(".LBB") or "s_cbranch" in lines[i])
    loop = None
    for i in range(sb[-1], end):
        m = re.match(r"\s+s_branch (\.LBB\d+_\d+)", lines[i])
        if m:
            t = next(j for j in range(start, end) if lines[j].startswith(m.group(1) + ":"))
            if t < sb[0]:
                loop = (t, i + 1)
                break
    return (a, b), loop


def vcount(h):
    return sum(n for m, n in h.items() if m.startswith("v_"))


def table(title, files, hs):
    print()
    print(title)
    print("%-28s" % "" + "".join("%16s" % os.path.basename(f)[:-2][-15:] for f in files))
    print("%-28s" % "vector instructions (v_*)" + "".join("%16d" % vcount(h) for h in hs))
    print("%-28s" % "scalar instructions (s_*)" + "".join("%16d" % sum(n for m, n in h.items() if m.startswith("s_")) for h in hs))
    for m in sorted(set().union(*hs), key=lambda m: (-max(h[m] for h in hs), m)):
        if m.startswith("v_"):
            print("%-28s" % m + "".join("%16d" % h[m] for h in hs))


def main():
    name = sys.argv[2]
    files = [sys.argv[1]] + sys.argv[3:]
    whole, rows, loops, rs = [], [], [], []
    for f in files:
        lines = open(f).read().split("\n")
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        whole.append(histogram(lines[start:end]))
        rs.append(resources(lines[end:end + 60]))
        rb, lp = regions(lines, start, end)
        rows.append(histogram(lines[rb[0]:rb[1]]) if rb else collections.Counter())
        loops.append(histogram(lines[lp[0]:lp[1]]) if lp else collections.Counter())
    print("kernel", name)
    print("%-28s" % "" + "".join("%16s" % os.path.basename(f)[:-2][-15:] for f in files))
    for k in ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "Occupancy", "LDSByteSize"):
        print("%-28s" % k + "".join("%16s" % r.get(k, "-") for r in rs))
    if any(rows):
        table("the row code (one straight block a pass: every lane, every pass)", files, rows)
        print()
        print("%-28s" % "pass loop, every path: v_*" + "".join("%16d" % vcount(h) for h in loops))
        print("%-28s" % "  of them v_readlane_b32" + "".join("%16d" % h["v_readlane_b32"] for h in loops))
    table("the whole kernel", files, whole)


if __name__ == "__main__":
    main()
