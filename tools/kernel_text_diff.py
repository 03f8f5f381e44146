#!/usr/bin/env python3
"""Is the device code of two builds the same?  The safety net of a host-only change.

    python tools/kernel_text_diff.py BUILD_DIR_A BUILD_DIR_B

Every ``*.hsaco`` of both build directories (mm-interleaved_amd/csrc/build of two checkouts) is disassembled with
``llvm-objdump -d`` and split at the symbol labels; addresses and the ``//`` encoding column are dropped, and per
translation unit the symbol sets and each symbol's instruction text are compared.  The order of the symbols within a unit
may differ (it follows the order of template instantiation on the host side); nothing else may.  Exit status 1 if a unit,
a symbol or a line differs.  Text is compared as text: no instruction is looked for.
"""
import glob
import os
import re
import subprocess
import sys

OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/lib/llvm/bin/llvm-objdump")
LABEL = re.compile(r"^[0-9a-f]+ <(.+)>:$")


def symbols(hsaco):
    """{symbol: [instruction text]} and the symbols in the file's order."""
    text = subprocess.run([OBJDUMP, "-d", hsaco], check=True, capture_output=True, text=True).stdout
    out, order, cur = {}, [], None
    for line in text.splitlines():
        m = LABEL.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
            order.append(m.group(1))
        elif cur is not None and line.strip():
            cur.append(" ".join(line.split("//")[0].split()))
    return out, order


def main(dir_a, dir_b):
    units_a, units_b = ({os.path.basename(p): p for p in glob.glob(os.path.join(d, "*.hsaco"))} for d in (dir_a, dir_b))
    bad = sorted(set(units_a) ^ set(units_b))
    for u in bad:
        print(f"{u}: only in {'A' if u in units_a else 'B'}")
    n_sym = n_lines = reordered = 0
    for unit in sorted(set(units_a) & set(units_b)):
        (a, order_a), (b, order_b) = symbols(units_a[unit]), symbols(units_b[unit])
        for s in sorted(set(a) ^ set(b)):
            print(f"{unit}: {s}: only in {'A' if s in a else 'B'}")
            bad.append(s)
        differ = [s for s in a if s in b and a[s] != b[s]]
        for s in differ:
            first = next((i for i, (x, y) in enumerate(zip(a[s], b[s])) if x != y), min(len(a[s]), len(b[s])))
            print(f"{unit}: {s}: differs from line {first}: {a[s][first:first + 1]} | {b[s][first:first + 1]}")
        bad += differ
        reordered += order_a != order_b and set(order_a) == set(order_b)
        n_sym += len(set(a) & set(b))
        n_lines += sum(len(v) for v in a.values())
        print(f"{unit}: {len(a)} symbols, {len(differ)} differ{', order differs' if order_a != order_b else ''}")
    print(f"{len(set(units_a) & set(units_b))} units, {n_sym} symbols compared, {n_lines} lines of instruction text, "
          f"{reordered} units with another symbol order, {len(bad)} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
