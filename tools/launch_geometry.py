#!/usr/bin/env python3
"""The launch shapes of the four LDS-resident kernels (msda_fwd_mma / _wq / _q8, msda_taps_mma), pinned where they run.

    rocprofv3 --kernel-trace --output-format csv -d DIR_A -- env MMFS_MSDA_LIB=A.so python tools/launch_geometry.py
    rocprofv3 --kernel-trace --output-format csv -d DIR_B -- env MMFS_MSDA_LIB=B.so python tools/launch_geometry.py
    python tools/launch_geometry.py --compare DIR_A DIR_B

Run: the forward through "lds", "slices", "waves" and "auto" and the backward with taps "lds" and "auto" over SHAPES --
tiny pyramids (the launch shape depends on B, H, Nq, K, D, not on the image), each threshold of the launchers crossed once
from both sides on a device of 256 CUs (csrc/msda_mma_common.h; launch_q8 in csrc/msda_fwd_q8.hip).  One line per call
goes to stdout, so that two runs can be seen to have made the same calls.  The knobs (MMFS_*_LDS_KB, MMFS_MMA_GRID,
MMFS_MMA_PERSIST) come from the environment.

Compare: the kernel traces of two runs, launch by launch in dispatch order -- kernel name, grid, workgroup and LDS size
must be equal.  Exit status 1 if they are not.  (The trace's LDS column reads 0 for these kernels, whose LDS is all
dynamic, whatever was asked for: it can only show that nothing static appeared.  With MMFS_MMA_PERSIST=0 the grid is the number of runs and
shows the queries per run, which a persistent grid hides.)
"""
import csv
import glob
import os
import re
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

PYR = [(8, 8), (4, 4)]                    # S = 80: every level resident everywhere
BIG = [(37, 37), (4, 4)]                  # S = 1385 > 1356: launch_q8's "not all resident" run length (512)
# (what it crosses, B, H, D, Nq, P, pyramid); K = 2 P samples per query.  2 x 256 CUs = 512 runs is the mark throughout.
SHAPES = [
    ("runs of 256: 64 slabs x 8 = 512, persistent",            8, 8, 128, 2048, 8, PYR),
    ("runs of 128: 64 x 7 < 512 at 256; 64 x 14, persistent",  8, 8, 128, 1792, 8, PYR),
    ("runs of 128: 64 x 8 = 512 at 128",                       8, 8, 128, 897, 8, PYR),
    ("runs of 64: 64 x 7 < 512 at 128; 64 x 14",               8, 8, 128, 896, 8, PYR),
    ("enough_runs: 64 x 8 = 512 at 64",                        8, 8, 128, 449, 8, PYR),
    ("not enough runs: 64 x 7 = 448, one workgroup per run",   8, 8, 128, 448, 8, PYR),
    ("H = 6 does not divide 256 CUs: 66 x 8 = 528 runs, dealt", 11, 6, 128, 2048, 8, PYR),
    ("D = 64, runs of 256, persistent",                        8, 8, 64, 2048, 8, PYR),
    ("D = 64, runs of 64",                                     8, 8, 64, 896, 8, PYR),
    ("q8: 32 units x 8 runs of 1024 = 256: not shortened",     2, 8, 64, 8192, 8, PYR),
    ("q8: 32 x 7 < 256 at 1024: shortened to 896",             2, 8, 64, 7168, 8, PYR),
    ("q8: levels not all resident: runs of 512",               2, 8, 64, 8192, 8, BIG),
    ("K = 32 > 16: the query-wave kernel's multi-chunk variant", 8, 8, 128, 2048, 16, PYR),
]


def run():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "mm-interleaved_amd")]
    import torch
    import MultiScaleDeformableAttention as MSDA
    from mmfs_amd.levels import make_level_tables
    dev, dtype = "cuda", torch.bfloat16
    g = torch.Generator().manual_seed(0)
    for what, B, H, D, Nq, P, pyr in SHAPES:
        shapes, start, S = make_level_tables(pyr, 1, dev)
        L = len(pyr)
        value = torch.rand(B, S, H, D, generator=g).to(dev, dtype)
        loc = torch.rand(B, Nq, H, L, P, 2, generator=g).to(dev, dtype)
        attn = torch.softmax(torch.rand(B, Nq, H, L * P, generator=g), -1).reshape(B, Nq, H, L, P).to(dev, dtype)
        grad = torch.randn(B, Nq, H * D, generator=g).to(dev, dtype)
        for algo in ("lds", "slices", "waves", "auto"):
            MSDA._fwd_algo = algo
            try:
                MSDA.ms_deform_attn_forward(value, shapes, start, loc, attn, 1)
                note = "ran"
            except RuntimeError as e:
                note = "refused" if f"status {MSDA._E_UNSUPPORTED}" in str(e) else f"FAILED {e}"
            finally:
                MSDA._fwd_algo = "auto"
            print(f"{what}: B={B} H={H} D={D} Nq={Nq} K={L * P} S={S} forward {algo}: {note}")
        for taps in ("lds", "auto"):
            MSDA._taps_algo = taps
            try:
                MSDA.ms_deform_attn_backward(value, shapes, start, loc, attn, grad, 1)
                note = "ran"
            except RuntimeError as e:
                note = "refused" if f"status {MSDA._E_UNSUPPORTED}" in str(e) else f"FAILED {e}"
            finally:
                MSDA._taps_algo = "auto"
            print(f"{what}: B={B} H={H} D={D} Nq={Nq} K={L * P} S={S} backward taps {taps}: {note}")
        torch.cuda.synchronize()


def launches(trace_dir):
    """[(kernel, grid, workgroup, LDS bytes)] in dispatch order, from the kernel-trace csv files under trace_dir."""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path, newline="")):
            pick = lambda *names: next(r[n] for n in names if n in r)
            rows.append((int(pick("Dispatch_Id", "Start_Timestamp")), pick("Kernel_Name"),
                         tuple(int(pick(f"Grid_Size_{a}", f"Grid_Size{a}")) for a in "XYZ"),
                         tuple(int(pick(f"Workgroup_Size_{a}", f"Workgroup_Size{a}")) for a in "XYZ"),
                         int(pick("LDS_Block_Size", "Group_Segment_Size", "LDS_Block_Size_v"))))
    return [r[1:] for r in sorted(rows)]


def compare(dir_a, dir_b):
    a, b = launches(dir_a), launches(dir_b)
    resident = [r for r in a if any(k in r[0] for k in ("msda_fwd_mma", "msda_fwd_wq", "msda_fwd_q8", "msda_taps_mma"))]
    # (mangled names: the kernel and its template arguments, e.g. msda_fwd_wq IDF16bLi128ELb0E)
    short = lambda n: " ".join(re.search(r"(msda_(?:fwd_mma|fwd_wq|fwd_q8|taps_mma))(\w*?)EEv", n).groups()) if "EEv" in n else n[:48]
    shapes = sorted({(short(r[0]), r[1][0] // max(r[2][0], 1), r[3]) for r in resident})
    print(f"{len(a)} launches in A, {len(b)} in B; {len(resident)} of A's by the LDS-resident kernels, "
          f"{len(shapes)} distinct (kernel, workgroups, LDS bytes):")
    for k, n, lds in shapes:
        print(f"  {k:32s} {n:6d} workgroups  {lds:7d} bytes of LDS")
    bad = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
    for i, x, y in bad[:20]:
        print(f"launch {i} differs:\n  A {x}\n  B {y}")
    ok = not bad and len(a) == len(b) and len(resident) > 0
    print("launch sequences equal" if ok else "LAUNCH SEQUENCES DIFFER")
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 1:
        sys.exit(__doc__)
    run()
