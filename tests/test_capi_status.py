"""What every entry point of the op returns for a bad argument, pinned against tests/golden/capi_statuses.json.

A valid call of each ``mmfs_msda_*`` entry is faulted in one argument at a time (dtype code, one dimension, one NULL or
misaligned pointer, the workspace, the bank / flag words) and the status is compared with the one the library returned
when the file was recorded; the host-only queries are swept over every subset of the backward flag bits.  Pointers are
fake (distinct 4096-aligned numbers, never dereferenced): every pinned case returns before any launch -- its status is
negative, or MMFS_OK for a problem with a zero product -- so no GPU is needed, and the module skips itself where one is
visible (a library that wrongly let such a case through would hand a fake pointer to a kernel there; here it fails with
a positive HIP status).

The file holds case names and integers only, run-length encoded (``pack``): per entry the fault names once, then per base
shape and flag word the statuses in that order as [status, count] runs, null for a case that reaches a launch.  Recording (from the library the file is to describe):
    MMFS_MSDA_LIB=/path/to/libmmfs_msda.so python tests/test_capi_status.py
"""
import ctypes
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "capi_statuses.json")

if __name__ != "__main__" and torch.cuda.is_available():
    pytest.skip("fake device pointers: host-only checks, run where no GPU is visible", allow_module_level=True)

DIMS = ("B", "S", "H", "D", "L", "Nq", "P")
PYRAMID = ((64, 64), (32, 32), (16, 16), (8, 8))                    # 5440 pixels
# name -> (dtype code, dims, level table)
BASES = {
    "northstar": (2, dict(B=8, S=5440, H=8, D=128, L=4, Nq=4096, P=4), PYRAMID),
    "d64p8": (2, dict(B=8, S=5440, H=16, D=64, L=4, Nq=4096, P=8), PYRAMID),
    "d32": (1, dict(B=8, S=5440, H=8, D=32, L=4, Nq=4096, P=4), PYRAMID),
    "d24": (2, dict(B=8, S=5440, H=8, D=24, L=4, Nq=4096, P=4), PYRAMID),
    "l129": (2, dict(B=2, S=516, H=8, D=128, L=129, Nq=256, P=4), ((2, 2),) * 129),
    "p64": (2, dict(B=2, S=5440, H=8, D=128, L=4, Nq=1024, P=64), PYRAMID),
    "northstar_f32": (0, dict(B=8, S=5440, H=8, D=128, L=4, Nq=4096, P=4), PYRAMID),
    "northstar_f64": (3, dict(B=8, S=5440, H=8, D=128, L=4, Nq=4096, P=4), PYRAMID),
}
DTYPES = (0, 1, 2, 3, 9)
BWD_BITS = (1, 2, 4, 16, 32, 64, 128)           # MMFS_BWD_*: every flag bit of the backward that the header defines
# every subset, the bits most entries ignore (dense taps, lazy attn) changing fastest: long runs in the file
BWD_FLAG_WORDS = [sum(bit for i, bit in enumerate((4, 16, 64, 128, 32, 2, 1)) if m >> i & 1) for m in range(128)]

# entry -> (argument names in ABI order, flag words a base call is made with)
#   pointers: any other name; "ws" / "have": workspace and its size; "hs" / "ht": the hybrid's HOST level table
PTRS10 = ("value", "shapes", "start", "loc", "attn", "grad_out", "grad_value", "grad_loc", "grad_attn")
ENTRIES = {
    "mmfs_msda_forward": (("dtype", "value", "shapes", "start", "loc", "attn", "out") + DIMS + ("stream",), (None,)),
    "mmfs_msda_forward_flags": (("dtype", "value", "shapes", "start", "loc", "attn", "out") + DIMS + ("flags", "stream"),
                                (0,)),
    "mmfs_msda_forward_shared": (("dtype", "value", "shapes", "start", "loc", "attn", "out", "B", "Bv", "layout")
                                 + DIMS[1:] + ("flags", "stream"), (0,)),
    "mmfs_msda_forward_fp8": (("dtype", "q", "scale", "shapes", "start", "loc", "attn", "out", "B", "Bv", "layout")
                              + DIMS[1:] + ("stream",), (None,)),
    "mmfs_msda_backward": (("dtype",) + PTRS10 + ("ws", "have") + DIMS + ("flags", "stream"), (1, 0)),
    "mmfs_msda_backward_checked": (("dtype",) + PTRS10 + ("ws", "have") + DIMS + ("flags", "table_status", "stream"),
                                   (32, 1, 0)),
    "mmfs_msda_backward_taps": (("dtype", "value", "shapes", "start", "loc", "attn", "grad_out", "grad_loc", "grad_attn")
                                + DIMS + ("stream",), (None,)),
    "mmfs_msda_backward_value": (("dtype", "shapes", "start", "loc", "attn", "grad_out", "grad_value", "ws", "have")
                                 + DIMS + ("stream",), (None,)),
    "mmfs_msda_backward_value_prepare": (("dtype", "loc", "attn", "ws", "have") + DIMS + ("stream",), (None,)),
    "mmfs_msda_backward_value_sort": (("dtype", "shapes", "start", "ws", "have") + DIMS + ("stream",), (None,)),
    "mmfs_msda_backward_value_reduce": (("dtype", "grad_out", "grad_value", "ws", "have") + DIMS + ("stream",), (None,)),
    "mmfs_msda_backward_value_run": (("dtype", "shapes", "start", "grad_out", "grad_value", "ws", "have") + DIMS
                                     + ("stream",), (None,)),
    "mmfs_msda_backward_hybrid": (("dtype", "value", "shapes", "start", "hs", "ht") + PTRS10[3:] + ("ws", "have") + DIMS
                                  + ("flags", "stages", "stream"), (5,)),
    "mmfs_msda_backward_sorted": (("dtype",) + PTRS10 + ("ws", "have") + DIMS + ("blocks4", "flags", "stages", "stream"),
                                  (1,)),
}
NOT_POINTERS = set(DIMS) | {"dtype", "have", "Bv", "layout", "flags", "stages", "blocks4", "stream", "hs", "ht"}
# flag words tried on a base call (the refusals: a named kernel on a shape that has none, the hybrid without
# MMFS_BWD_DENSE_TAPS, the sorted route on a word that is not the canonical one, ...)
FLAG_FAULTS = {
    "mmfs_msda_forward_flags": range(16), "mmfs_msda_forward_shared": range(16),
    "mmfs_msda_backward": BWD_FLAG_WORDS, "mmfs_msda_backward_checked": BWD_FLAG_WORDS,
    "mmfs_msda_backward_hybrid": BWD_FLAG_WORDS, "mmfs_msda_backward_sorted": BWD_FLAG_WORDS,
}
LIM = 2 ** 31


class Tables:
    """Host level tables (real int64 arrays: the hybrid entries read them) of a base: its own, one with an empty level."""

    def __init__(self, levels):
        flat = [x for hw in levels for x in hw]
        starts = [sum(h * w for h, w in levels[:i]) for i in range(len(levels))]
        hole = list(flat)
        hole[2], hole[3] = 0, 0
        self.arrays = {"base": ((ctypes.c_int64 * len(flat))(*flat), (ctypes.c_int64 * len(starts))(*starts)),
                       "hole": ((ctypes.c_int64 * len(flat))(*hole), (ctypes.c_int64 * len(starts))(*starts))}
        self.blocks4 = sum(((h + 3) // 4) * ((w + 3) // 4) for h, w in levels)

    def pointers(self, which):
        if which == "null":
            return None, None
        hs, ht = self.arrays[which]
        return ctypes.cast(hs, ctypes.c_void_p).value, ctypes.cast(ht, ctypes.c_void_p).value


def workspace_need(lib, entry, dtype, dims, flags, tables):
    d = [dims[k] for k in DIMS]
    if entry == "mmfs_msda_backward_hybrid":
        return lib.mmfs_msda_backward_hybrid_workspace_bytes(dtype, *tables.pointers("base"), *d, flags)
    if entry == "mmfs_msda_backward_sorted":
        return lib.mmfs_msda_backward_sorted_workspace_bytes(dtype, *d, flags)
    return lib.mmfs_msda_backward_workspace_bytes(dtype, *d, 1 if flags is None else flags)


def base_call(lib, entry, dtype, dims, flags, tables):
    """{argument name: value} of a valid call."""
    names, _ = ENTRIES[entry]
    args = {}
    for i, n in enumerate(names):
        if n not in NOT_POINTERS:
            args[n] = 0x100000 * (i + 1)                      # distinct, 4096-aligned, never dereferenced
    args.update(dims, dtype=dtype, flags=flags, stream=None, Bv=dims["B"], layout=0, blocks4=tables.blocks4)
    args["stages"] = 31 if entry == "mmfs_msda_backward_hybrid" else 15
    args["hs"], args["ht"] = tables.pointers("base")
    if "ws" in names:
        args["have"] = workspace_need(lib, entry, dtype, dims, flags, tables)
    return args


def faults(entry, base, tables):
    """(name, {argument: value}) of every one-argument fault of a base call of ``entry``."""
    names, _ = ENTRIES[entry]
    for code in DTYPES:
        yield f"dtype={code}", {"dtype": code}
    for k in DIMS:
        for v in (-1, LIM, 0):
            yield f"{k}={v}", {k: v}
    yield "L*P>lim", {"L": 65536, "P": 32768}
    yield "H*D>lim", {"H": 65536, "D": 32768}
    yield "S=lim-2", {"S": LIM - 2}
    for n in names:
        if n in NOT_POINTERS:
            continue
        yield f"{n}=NULL", {n: None}
        if n != "ws":
            for off in (1, 2, 4, 8):
                yield f"{n}+{off}", {n: base[n] + off}
    if "ws" in names:
        yield "ws short", {"have": base["have"] - 1}
        yield "ws+8", {"ws": base["ws"] + 8}
    if "Bv" in names:
        yield "Bv=0", {"Bv": 0}
        yield "Bv=3", {"Bv": 3}
        yield "Bv=B/2", {"Bv": base["B"] // 2}
        yield "Bv=B/2 interleave", {"Bv": base["B"] // 2, "layout": 1}
        yield "layout=7", {"layout": 7}
    if "blocks4" in names:
        yield "blocks4=-1", {"blocks4": -1}
        yield "blocks4=0", {"blocks4": 0}
    if "hs" in names:
        for which in ("hole", "null"):
            hs, ht = tables.pointers(which)
            yield f"host table {which}", {"hs": hs, "ht": ht}
    for word in FLAG_FAULTS.get(entry, ()):
        yield f"flags={word}", {"flags": word}
    if "stages" in names:
        yield "stages=0", {"stages": 0}


def entry_statuses(lib, entry):
    """{case name: status} of the sweep of ``entry``, the cases the library lets through to a launch (positive status
    where there is no device) left out."""
    names, flag_words = ENTRIES[entry]
    names = [n for n in names]
    out = {}
    for bname, (dtype, dims, levels) in BASES.items():
        tables = Tables(levels)
        for flags in flag_words:
            base = base_call(lib, entry, dtype, dims, flags, tables)
            for fname, change in faults(entry, base, tables):
                args = dict(base, **change)
                if "have" in args and ("dtype" in change or set(change) & set(DIMS) or "flags" in change):
                    # a workspace that fits the call as made: the fault under test is the only one
                    # (the workspace queries are asked about non-empty problems only: mmfs_msda_backward_workspace_bytes
                    # divides by zero for B = 0 with MMFS_BWD_CANONICAL_LEVELS)
                    if all(0 < args[k] < LIM for k in DIMS) and args["L"] * args["P"] < LIM and args["H"] * args["D"] < LIM:
                        args["have"] = max(args["have"], workspace_need(lib, entry, args["dtype"], args, args["flags"], tables))
                key = f"{bname}/flags={flags}/{fname}"
                out[key] = getattr(lib, entry)(*[args[n] for n in names])
    return out


def cast_statuses(lib):
    f, out = lib.mmfs_msda_cast_from_f32, {}
    for code in DTYPES:
        out[f"dtype={code}"] = f(code, 0x100000, 0x200000, 4096, None)
    for n in (-1, 0, LIM):
        out[f"n={n}"] = f(2, 0x100000, 0x200000, n, None)
    out["src=NULL"] = f(2, None, 0x200000, 4096, None)
    out["dst=NULL"] = f(2, 0x100000, None, 4096, None)
    for off in (1, 2, 4, 8):
        out[f"src+{off}"] = f(2, 0x100000 + off, 0x200000, 4096, None)
        out[f"dst+{off}"] = f(2, 0x100000, 0x200000 + off, 4096, None)
    return {f"4096 elements/flags=None/{k}": v for k, v in out.items()}


def query_values(lib, query):
    """{base/dtype[/table]: [value for every subset of the backward flag bits]} of a host-only query."""
    out = {}
    if query == "mmfs_rmsnorm_backward_partials_rows":
        rows = (-1, 0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 4095, 4096, 32768, 8 * 4096, 2 ** 20, LIM, 2 ** 40)
        return {"rows": list(rows), "values": [lib.mmfs_rmsnorm_backward_partials_rows(r) for r in rows]}
    for bname, (_, dims, levels) in BASES.items():
        d = [dims[k] for k in DIMS]
        tables = Tables(levels)
        for code in DTYPES:
            if query == "mmfs_msda_backward_hybrid_workspace_bytes":
                for which in ("base", "hole", "null"):
                    out[f"{bname}/dtype={code}/{which}"] = [getattr(lib, query)(code, *tables.pointers(which), *d, w)
                                                            for w in BWD_FLAG_WORDS]
            else:
                out[f"{bname}/dtype={code}"] = [getattr(lib, query)(code, *d, w) for w in BWD_FLAG_WORDS]
    return out


QUERIES = ("mmfs_msda_backward_workspace_bytes", "mmfs_msda_backward_hybrid_workspace_bytes",
           "mmfs_msda_backward_sorted_workspace_bytes", "mmfs_msda_backward_taps_fused",
           "mmfs_rmsnorm_backward_partials_rows")
LAUNCHING = tuple(ENTRIES) + ("mmfs_msda_cast_from_f32",)


def zero_product(case):
    """The case names a problem with an empty tensor (a dimension or the element count at 0)."""
    return case.rsplit("/", 1)[-1] in {f"{k}=0" for k in DIMS} | {"n=0"}


def returns_before_launch(case, status):
    return status < 0 or (status == 0 and zero_product(case))


def sweep(lib, entry):
    return cast_statuses(lib) if entry == "mmfs_msda_cast_from_f32" else entry_statuses(lib, entry)


def rle(values):
    runs = []
    for v in values:
        if runs and runs[-1][0] == v:
            runs[-1][1] += 1
        else:
            runs.append([v, 1])
    return runs


def unrle(runs):
    return [v for v, n in runs for _ in range(n)]


def pack(cases):
    """{"base/flags=F/fault": status} -> {"faults": [names], base: {"flags=F": runs over the names, None where not pinned}}"""
    faults, groups = [], {}
    for case in cases:
        base, flags, fault = case.split("/", 2)
        groups.setdefault(base, {}).setdefault(flags, {})[fault] = cases[case]
        if fault not in faults:
            faults.append(fault)
    packed = {"faults": faults}
    for base, group in groups.items():
        runs = {f: rle([by.get(n) for n in faults]) for f, by in group.items()}
        packed[base] = next((b for b in packed if packed[b] == runs), runs)        # (the name of a base with the same statuses)
    return packed


def unpack(packed):
    return {f"{base}/{flags}/{fault}": status for base, group in packed.items() if base != "faults"
            for flags, runs in (packed[group] if isinstance(group, str) else group).items()
            for fault, status in zip(packed["faults"], unrle(runs)) if status is not None}


def pack_query(values):
    """{"base/rest": [values]} -> {base: {rest: runs, or the name of a ``rest`` of the base with the same runs}}"""
    out = {}
    for key, v in values.items():
        base, _, rest = key.partition("/")
        group = out.setdefault(base, {})
        group[rest] = next((r for r in group if group[r] == rle(v)), rle(v))
    return out


def unpack_query(packed):
    return {(f"{base}/{rest}" if rest else base): unrle(group[runs] if isinstance(runs, str) else runs)
            for base, group in packed.items() for rest, runs in group.items()}


def dump(gold, f):
    """One line per entry's fault names and per base shape."""
    compact = lambda v: json.dumps(v, separators=(",", ":"))
    sections = []
    for sec, body in gold.items():
        entries = [" %s: {\n%s\n }" % (json.dumps(name), ",\n".join(f"  {json.dumps(k)}: {compact(v)}" for k, v in rows.items()))
                   for name, rows in body.items()]
        sections.append("%s: {\n%s\n}" % (json.dumps(sec), ",\n".join(entries)))
    f.write("{\n" + ",\n".join(sections) + "\n}\n")


def record(lib):
    """The golden file's content from ``lib``.  A case the library lets through to a launch is not pinned (and must not
    be run where there is a GPU): only what returns before any launch goes into the file."""
    gold = {"statuses": {}, "queries": {}}
    for entry in LAUNCHING:
        got = sweep(lib, entry)
        kept = {c: s for c, s in got.items() if returns_before_launch(c, s)}
        assert all(s > 0 or (s == 0 and not zero_product(c)) for c, s in got.items() if c not in kept)
        print(f"{entry}: {len(kept)} cases pinned, {len(got) - len(kept)} reach a launch and are left out", file=sys.stderr)
        # (every swept case, so that the order of the fault names is the sweep's; None: not pinned)
        gold["statuses"][entry] = pack({c: kept.get(c) for c in got})
    for q in QUERIES:
        gold["queries"][q] = pack_query(query_values(lib, q))
    return gold


@pytest.fixture(scope="module")
def lib():
    from helpers import bound_library
    return bound_library()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        gold = json.load(f)
    return {"statuses": {e: unpack(p) for e, p in gold["statuses"].items()},
            "queries": {q: unpack_query(p) for q, p in gold["queries"].items()}}


def test_golden_file_holds_no_case_that_launches(golden):
    assert sorted(golden["statuses"]) == sorted(LAUNCHING) and sorted(golden["queries"]) == sorted(QUERIES)
    for entry, cases in golden["statuses"].items():
        assert len(cases) > 10, entry
        for case, status in cases.items():
            assert returns_before_launch(case, status), f"{entry}: {case}: recorded status {status}"


@pytest.mark.parametrize("entry", LAUNCHING)
def test_entry_statuses_are_the_recorded_ones(lib, golden, entry):
    want = golden["statuses"][entry]
    got = sweep(lib, entry)
    assert set(want) <= set(got), f"{entry}: cases of the file the sweep no longer makes: {sorted(set(want) - set(got))[:5]}"
    wrong = [f"{entry}: {c}: returned {got[c]}, recorded {s}" for c, s in want.items() if got[c] != s]
    # a case that was not pinned reached a launch when the file was recorded: it still must (positive status, no device)
    wrong += [f"{entry}: {c}: returned {s}, reached a launch when recorded" for c, s in got.items()
              if c not in want and returns_before_launch(c, s)]
    assert not wrong, "\n".join(wrong[:40] + [f"({len(wrong)} in all)"])


@pytest.mark.parametrize("query", QUERIES)
def test_host_only_queries_are_the_recorded_ones(lib, golden, query):
    want, got = golden["queries"][query], query_values(lib, query)
    assert sorted(want) == sorted(got)
    wrong = []
    for key, values in want.items():
        if key == "rows":
            assert values == got[key]
            continue
        words = BWD_FLAG_WORDS if key != "values" else want["rows"]
        wrong += [f"{query}: {key}: flags / rows {w}: returned {g}, recorded {v}"
                  for w, g, v in zip(words, got[key], values) if g != v]
        assert len(values) == len(got[key])
    assert not wrong, "\n".join(wrong[:40] + [f"({len(wrong)} in all)"])


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "mm-interleaved_amd"))
    import mmfs_abi
    recorded = record(mmfs_abi.bind(ctypes.CDLL(os.environ["MMFS_MSDA_LIB"])))
    with open(GOLDEN, "w") as f:
        dump(recorded, f)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes", file=sys.stderr)
