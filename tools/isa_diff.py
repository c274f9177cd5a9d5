#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 code in two HIP objects: the check a
refactor makes that it left the compiled kernels alone.

Both objects are disassembled (spill_check.disassemble / kernels), every
instruction line is cut down to its text -- the address, the encoding and the
symbol name of a branch target go with the comment -- and the kernels are
paired by demangled name (c++filt).  Per kernel it prints "same", or the
instructions that differ, or that only one of the objects holds it.

Usage: isa_diff.py OLD.o NEW.o [RENAMES.json]
RENAMES.json: {"demangled name in OLD": "demangled name in NEW", ...} for
kernels the change renamed.  Exit status 1 if anything differs.
"""
import difflib
import json
import subprocess
import sys

import spill_check


def text(line):
    """An instruction line of llvm-objdump without its comment."""
    return " ".join(line.split("//")[0].split())


def compare(old, new):
    """[] if two kernels' instruction texts are equal, else what differs: the
    pairs at the same position for equal lengths, a unified diff otherwise."""
    a, b = [text(t) for _, t in old], [text(t) for _, t in new]
    if a == b:
        return []
    if len(a) == len(b):
        return [f"{k}: {x}  ->  {y}" for k, (x, y) in enumerate(zip(a, b)) if x != y]
    return [l for l in difflib.unified_diff(a, b, "old", "new", n=0, lineterm="")][2:]


def demangled(ks):
    """{demangled name: instructions} of spill_check.kernels' result."""
    names = list(ks)
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return {d.replace("(anonymous namespace)::", ""): ks[n] for n, d in zip(names, out.splitlines())}


def report(old, new, renames=None):
    """(lines to print, number of kernels that are not "same")"""
    renames = renames or {}
    old = {renames.get(n, n): (n, ins) for n, ins in old.items()}
    lines, bad = [], 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            lines.append(f"{name}: only in {'old' if name in old else 'new'}")
            bad += 1
            continue
        was, ins = old[name]
        head = name if was == name else f"{name} (was {was})"
        d = compare(ins, new[name])
        if not d:
            lines.append(f"{head}: same ({len(ins)} instructions)")
            continue
        bad += 1
        lines.append(f"{head}: {len(ins)} -> {len(new[name])} instructions, {len(d)} lines differ")
        lines += ["    " + l for l in d]
    return lines, bad


def main():
    if len(sys.argv) not in (3, 4):
        sys.exit(__doc__)
    renames = json.load(open(sys.argv[3])) if len(sys.argv) == 4 else {}
    old, new = (demangled(spill_check.kernels(spill_check.disassemble(p))) for p in sys.argv[1:3])
    lines, bad = report(old, new, renames)
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
