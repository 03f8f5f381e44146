#!/usr/bin/env python3
"""Compare the instruction streams of kernels in two device-assembly files (``make asm``: csrc/build/*.s).

    tools/asm_kernel_diff.py OLD.s NEW.s old_name=new_name [old_name=new_name ...]

A name is a substring of the mangled symbol (``clip_attn_fwd``, ``attn_train_fwd``); every symbol of OLD.s that holds
``old_name`` is matched with the symbol of NEW.s that holds ``new_name`` and has the same element type (the first ``DF16_`` or
``DF16b`` in the mangled name).  Per pair: identical / differs, the two line counts, and a unified diff of the
differing lines.  Comments are stripped; every mangled symbol inside an instruction is replaced by ``SYM`` and the function's
number is taken out of its local labels (``.LBB3_7`` -> ``.LBB_7``).
Exit status 1 if any pair differs or is missing.  Text is compared as text: no instruction is looked for.
(tools/kernel_text_diff.py compares whole builds whose symbols kept their names.)
"""
import difflib
import re
import sys

TYPES = {"DF16_": "fp16", "DF16b": "bf16"}


def elem_type(sym):
    found = sorted((sym.find(t), n) for t, n in TYPES.items() if t in sym)
    return found[0][1] if found else "-"


def kernels(path):
    """-> {symbol: [instruction and label lines]} for every function of the file"""
    out, cur = {}, None
    for line in open(path):
        line = re.sub(r"\s*(;|//).*", "", line.rstrip())
        m = re.match(r"^(_Z\w+):$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.strip():
            continue
        if re.match(r"^\s*\.Lfunc_end", line):
            cur = None
            continue
        if re.match(r"^\s+\.", line):                   # a directive
            continue
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", line.strip())))
    return out


def main(argv):
    if len(argv) < 4 or any("=" not in a for a in argv[3:]):
        sys.exit(__doc__)
    old, new = kernels(argv[1]), kernels(argv[2])
    bad = 0
    for pair in argv[3:]:
        on, nn = pair.split("=")
        for osym in sorted(s for s in old if on in s):
            ty = elem_type(osym)
            match = [s for s in new if nn in s and elem_type(s) == ty]
            if len(match) != 1:
                print(f"{on} {ty}: {len(match)} symbols with '{nn}' in {argv[2]}")
                bad += 1
                continue
            a, b = old[osym], new[match[0]]
            same = a == b
            bad += not same
            print(f"{on} -> {nn} {ty}: {'identical' if same else 'differs'} ({len(a)} / {len(b)} lines)")
            if not same:
                for d in difflib.unified_diff(a, b, "old", "new", n=0, lineterm=""):
                    print("    " + d)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
