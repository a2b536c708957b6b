#!/usr/bin/env python3
"""Kernel-by-kernel instruction identity of two device assemblies of one translation unit (no GPU needed: hipcc cross-compiles).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=fast -w --offload-device-only -S csrc/gemm.hip -o new.s      (the product flags)
    ... the same at the parent commit -> parent.s
    tools/isa_compare.py parent.s new.s [-o profiles/NAME_isa.txt] [--diff KERNEL_SUBSTRING]

Per kernel: comments and assembler directives are stripped, the function index in .LBB<n>_<m> labels is normalised, and what is left (instructions and
labels) is compared line by line.  Columns: .vgpr_count, .sgpr_count, .private_segment_fixed_size (scratch), .group_segment_fixed_size (LDS) and
occupancy (waves per SIMD) from the code object metadata of the NEW assembly, instructions + labels at the parent and new, verdict:
SAME, DIFF (resources equal) or DIFF* (a resource differs: the parent's values follow), GONE / NEW.  For a kernel that differs, wf = waterfall loops
around an LDS-DMA (tools/check_isa.sh) at the parent -> new.  --diff prints the unified diff of the normalised streams of the kernels whose name contains
the substring.  Exit status 1 if a kernel is gone, new, or differs in a resource."""
import argparse
import collections
import difflib
import re
import subprocess
import sys

RES = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def parse(path):
    """symbol -> (normalised lines, waterfall loops, occupancy); symbol -> resources from the metadata"""
    body, wf, occ, cur, last, raw = collections.OrderedDict(), {}, {}, None, None, []
    meta, text = {}, open(path).read()
    for line in text.split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, raw = m.group(1), []
            body[cur], wf[cur] = [], 0
            continue
        if cur is None:
            m = re.match(r"; Occupancy: (\d+)", line)
            if m and last is not None:
                occ[last] = int(m.group(1))
            continue
        if line.startswith(".Lfunc_end"):
            last, cur = cur, None
            continue
        if "buffer_load_dwordx4" in line and " lds" in line and any("s_and_saveexec" in l for l in raw[-3:]):
            wf[cur] += 1
        raw.append(line)
        s = line.split(";")[0].strip()
        if not s or (s.startswith(".") and not s.startswith(".LBB")):
            continue
        body[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:      # one metadata entry per kernel
        name = re.search(r"\n    \.name:\s+(\S+)", blk)
        if name:
            meta[name.group(1)] = tuple(int(re.search(r"\n    \%s:\s+(\d+)" % k, "\n" + blk).group(1)) for k in RES)
    return body, wf, occ, meta


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [d.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "") for d in out]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("-o", "--out")
    ap.add_argument("--diff", default=None)
    a = ap.parse_args()
    (pb, pwf, pocc, pmeta), (nb, nwf, nocc, nmeta) = parse(a.parent), parse(a.new)
    kernels = [k for k in pb if k in pmeta] + [k for k in nb if k in nmeta and k not in pb]      # (device functions other than kernels have no metadata entry)
    rows, counts, bad = [], collections.Counter(), False
    for sym, name in sorted(zip(kernels, demangle(kernels)), key=lambda t: t[1]):
        if sym not in nb or sym not in pb:
            verdict = "GONE" if sym not in nb else "NEW"
            bad = True
            r, occ, n0, n1, note = (pmeta if sym in pmeta else nmeta)[sym], (pocc if sym in pocc else nocc).get(sym, 0), len(pb.get(sym, [])), len(nb.get(sym, [])), ""
        else:
            r, occ, n0, n1, note = nmeta[sym], nocc.get(sym, 0), len(pb[sym]), len(nb[sym]), ""
            if pb[sym] == nb[sym] and pmeta[sym] == r:
                verdict = "SAME"
            else:
                res_same = pmeta[sym] == r and pocc.get(sym) == nocc.get(sym)
                verdict = "DIFF" if res_same else "DIFF*"
                bad |= not res_same
                note = "  wf %d -> %d" % (pwf[sym], nwf[sym]) + ("" if res_same else "  parent: %s occ %s" % (" ".join(map(str, pmeta[sym])), pocc.get(sym)))
                if a.diff is not None and a.diff in name:
                    sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(pb[sym], nb[sym], "parent " + name, "new " + name, lineterm="", n=2))
        counts[verdict] += 1
        rows.append("%-50s %5d %5d %8d %7d %4d %8d %8d  %s%s" % (name, r[0], r[1], r[2], r[3], occ, n0, n1, verdict, note))
    head = "%-50s %5s %5s %8s %7s %4s %8s %8s  verdict" % ("kernel", "vgpr", "sgpr", "scratch", "lds", "occ", "n_parent", "n_new")
    summary = "%d kernels: %s" % (len(rows), ", ".join("%d %s" % (n, v) for v, n in sorted(counts.items())))
    text = "\n".join([head] + rows + ["", summary]) + "\n"
    if a.out:
        open(a.out, "w").write(text)
        print(summary)
    else:
        sys.stdout.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
