#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds of the device code, kernel by kernel.

Make the two listings with the library's flags (rvo3d_amd/_lib.py: HIPCC_FLAGS, without -shared) plus
    --cuda-device-only -S -Rpass-analysis=kernel-resource-usage -o NAME.s csrc/rvo3d_capi.hip
then
    tools/isa_diff.py OLD.s NEW.s [--only SUBSTRING] [--diff-lines N]

A kernel's text runs from its label to the end of its "Kernel info" comment block (code, kernel descriptor, resource
usage).  Local labels (.LBB<n>_<m> and BB<n>_<m> in comments, .Lfunc_end<n>, .Ltmp<n>) are replaced by a constant, since they count functions
across the whole file, and the blanks in front of a trailing comment by one (the assembler aligns those comments behind
the label, whose length changes with the numbers).  A kernel of NEW that OLD does not have is listed and does not count
(--strict: it does).  For a kernel that differs the script prints the resource lines and the counts of the
instructions that decide speed for both builds and the head of a unified diff.  Exit status 1 if any kernel differs
or exists on one side only.
"""
import argparse
import difflib
import re
import shutil
import subprocess
import sys

BEGIN = re.compile(r"^\s*\.protected\s+(\S+)\s*; -- Begin function")
LABEL = re.compile(r"(\.L)?BB\d+_\d+|\.Lfunc_(begin|end)\d+|\.Ltmp\d+")
COMMENT_GAP = re.compile(r"(?<=\S)[ \t]+;")
RESOURCE = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "LDSByteSize", "Occupancy",
            "codeLenInByte")
COUNTED = ("v_mfma", "buffer_load", "global_load", "ds_read", "ds_write", "s_waitcnt", "s_barrier", "scratch_")


def kernels(path):
    """{symbol: normalised lines} of every function in an assembly listing."""
    out, cur, info = {}, None, False
    with open(path) as f:
        for line in f:
            m = BEGIN.match(line)
            if m:
                cur, info = [], False
                out[m.group(1)] = cur
                continue
            if cur is None:
                continue
            info = info or line.startswith("; Kernel info:")
            if info and not line.startswith(";"):
                cur = None  # (behind the resource comments: the next function's section directives)
                continue
            cur.append(COMMENT_GAP.sub(" ;", LABEL.sub(".L", line.rstrip("\n"))))
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return {n: n for n in names}
    res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, res.stdout.splitlines()))


def facts(lines):
    res = {}
    for ln in lines:
        if ln.startswith("; "):
            key = ln[2:].split(":")[0].split("=")[0].strip()
            if key in RESOURCE:
                res[key] = ln[2:].strip()
    counts = {c: 0 for c in COUNTED}
    for ln in lines:
        op = ln.strip().split(" ")[0].split("\t")[0]
        for c in COUNTED:
            if op.startswith(c):
                counts[c] += 1
    return res, counts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--only", default="", help="compare only kernels whose demangled name contains this")
    ap.add_argument("--diff-lines", type=int, default=80, help="lines of unified diff printed per differing kernel")
    ap.add_argument("--strict", action="store_true", help="a kernel that only NEW has counts as a difference too")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    names = demangle(sorted(set(old) | set(new)))
    same = bad = 0
    for sym, nice in names.items():
        if a.only not in nice:
            continue
        if sym not in old or sym not in new:
            print(f"ONLY IN {'OLD' if sym in old else 'NEW'}  {nice}")
            bad += 1 if (sym in old or a.strict) else 0
            continue
        if old[sym] == new[sym]:
            print(f"identical  {nice}")
            same += 1
            continue
        bad += 1
        print(f"DIFFERENT  {nice}")
        (ro, co), (rn, cn) = facts(old[sym]), facts(new[sym])
        for k in RESOURCE:
            if ro.get(k) != rn.get(k):
                print(f"    resource  {ro.get(k)}  ->  {rn.get(k)}")
        for k in COUNTED:
            mark = "" if co[k] == cn[k] else "   <-- differs"
            print(f"    count  {k:12s} {co[k]:6d} {cn[k]:6d}{mark}")
        d = list(difflib.unified_diff(old[sym], new[sym], "old", "new", n=2, lineterm=""))
        for ln in d[:a.diff_lines]:
            print("    " + ln)
        if len(d) > a.diff_lines:
            print(f"    ... {len(d) - a.diff_lines} more diff lines")
    print(f"{same} identical, {bad} different or one-sided")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
