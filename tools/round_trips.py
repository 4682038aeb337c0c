#!/usr/bin/env python3
"""List the global loads of a kernel that are waited for almost at once: the serial memory round trips.

Make the listing as tools/isa_diff.py describes (the library's flags plus --cuda-device-only -S
-Rpass-analysis=kernel-resource-usage), then
    tools/round_trips.py LISTING.s SUBSTRING [--within N] [--quiet]

For every kernel whose demangled name contains SUBSTRING the script walks the instructions in listing order and
prints each global_load whose next `s_waitcnt vmcnt(k)` follows within N instructions AND covers it: vector memory
returns in order, so the wait covers the load when at most k vector-memory instructions (loads and stores alike)
were issued after it.  Such a load hides nothing behind its latency.  Then the totals: global loads, vmcnt waits,
loads with an immediate wait, registers and scratch.

The walk follows the listing, not the control flow: a load at the end of one block and a wait at the top of the next
count as neighbours although a branch may lie between them, and rare paths count like common ones.  Read the
printed neighbourhood before drawing conclusions.  A reporting aid, not a test.
"""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_diff import demangle, facts, kernels  # noqa: E402

VMCNT = re.compile(r"vmcnt\((\d+)\)")
VMEM = ("global_load", "global_store", "global_atomic", "buffer_load", "buffer_store", "buffer_atomic",
        "flat_load", "flat_store", "flat_atomic", "scratch_load", "scratch_store")


def instructions(lines):
    """(opcode, text) of every instruction of a kernel's code, up to its kernel descriptor."""
    out = []
    for ln in lines:
        s = ln.strip()
        if s.startswith(".amdhsa_kernel") or s.startswith(".section"):
            break
        if not s or s[0] in ".;" or s.endswith(":"):
            continue
        out.append((re.split(r"\s+", s, maxsplit=1)[0], s))
    return out


def round_trips(ins, within):
    """[(index of the load, index of the wait, k)] of the loads with an immediate covering wait."""
    hits = []
    for i, (op, _) in enumerate(ins):
        if not op.startswith("global_load"):
            continue
        later = 0
        for j in range(i + 1, min(i + 1 + within, len(ins))):
            opj, txt = ins[j]
            m = VMCNT.search(txt) if opj == "s_waitcnt" else None
            if m:
                if later <= int(m.group(1)):
                    hits.append((i, j, int(m.group(1))))
                break
            if opj.startswith(VMEM):
                later += 1
    return hits


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("only", help="report kernels whose demangled name contains this")
    ap.add_argument("--within", type=int, default=4, help="instructions between a load and its wait (default 4)")
    ap.add_argument("--quiet", action="store_true", help="totals only")
    a = ap.parse_args()
    ks = kernels(a.listing)
    names = demangle(sorted(ks))
    found = 0
    for sym, nice in names.items():
        if a.only not in nice:
            continue
        found += 1
        ins = instructions(ks[sym])
        hits = round_trips(ins, a.within)
        res, _ = facts(ks[sym])
        loads = sum(op.startswith("global_load") for op, _ in ins)
        waits = sum(op == "s_waitcnt" and VMCNT.search(txt) is not None for op, txt in ins)
        print(nice)
        if not a.quiet:
            for i, j, k in hits:
                print(f"  #{i:5d}  {ins[i][1]}")
                print(f"          +{j - i}: {ins[j][1]}")
        vg = res.get("NumVgprs", "NumVgprs: ?").split(":")[-1].strip()
        sc = res.get("ScratchSize", "ScratchSize: ?").split(":")[-1].strip()
        print(f"  global_load {loads}  vmcnt waits {waits}  loads with a wait within {a.within}: {len(hits)}  "
              f"VGPRs {vg}  scratch {sc}")
    if not found:
        print(f"no kernel matches {a.only!r}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
