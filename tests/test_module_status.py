"""What the module's entry points (everything of include/mmfs_msda.h besides the op's ``mmfs_msda_*``) return for a bad
argument, pinned against tests/golden/module_statuses.json -- the sibling of tests/test_capi_status.py, whose encoding
of the file (``rle`` / ``pack`` / ``unpack`` / ``dump``) it uses.

Per launching entry a few valid base calls at the smallest shapes that reach each branch of its checks, and per base:
  one fault   every dtype code; every int64 argument at -1, 0, 2^31, one off the base value and at / one past every limit
              the code names (``LIMITS``); every option word over ``WORDS``; every pointer at NULL and +1, +2, +4, +8, +16, +32
              (a point row of the samplers is up to 64 bytes);
  two faults  the pairs of pointers (a, b) with a NULL and b off by 2 -- a before b in the ABI's order, and the mirror for
              the first and the last pointer --, and every int64 argument at -1 with every
              pointer at NULL and with every pointer off by 2 -- the ORDER in which an entry looks at its arguments.
The 19 host-only queries are swept over a grid of their arguments (``QUERY_GRIDS``).  No module entry takes a workspace
size (a workspace is a pointer like any other here).

Pointers are fake (distinct 4096-aligned numbers, never dereferenced) but for the three arguments that are HOST arrays by
contract -- ``level_hw`` of the dwconv entries, ``level_ptrs`` / ``level_hw`` of the bank entries -- which are real
ctypes arrays (faulted with NULL only).  Every pinned case returns before any launch: a negative status, or MMFS_OK for an
empty problem (an int64 argument at 0 or a NULL output nobody asked for); a case that reaches a launch is null in the file
and must still reach one (a positive HIP status: the module skips itself where a GPU is visible).  Every MMFS_*
environment variable is cleared and ``mmfs_env_reload`` called first: the tuning knobs change what some queries answer.

Recording (from the library the file is to describe):
    MMFS_MSDA_LIB=/path/to/libmmfs_msda.so python tests/test_module_status.py
"""
import ctypes
import hashlib
import itertools
import json
import os
import re
import sys

import pytest
import torch

from test_capi_status import dump, pack, pack_query, returns_before_launch, unpack, unpack_query

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "module_statuses.json")
HEADER = os.path.join(os.path.dirname(HERE), "include", "mmfs_msda.h")

if __name__ != "__main__" and torch.cuda.is_available():
    pytest.skip("fake device pointers: host-only checks, run where no GPU is visible", allow_module_level=True)

LIM = 2 ** 31
DTYPES = (-1, 0, 1, 2, 3, 9)
WORDS = (-1, 0, 1, 2, 3, 4, 5, 7, 8, 9, 14, 15, 16, 17)     # act, layout, mask, reduction, flags, n_levels, ...
# at and one past (the next value the other checks let through) every limit the entries name: P and R sets; n * L <= 64;
# kMaxLevels 8; kMaxNq 128; query_prep C <= 2048; pyramid H, W <= 2^12; kMaxNk 8192 and the longest RMS-norm row;
# 65535 slots / images; B, H <= 2^20; kLlamaMaxCap, kLlamaTrainMaxL, kMaxTokens, kMaxRows 2^22; C, kMaxVocab, B * H <= 2^24;
# bank tokens 2^28; 2^31 - 2 pixels; B * Lq <= 2^32; B * Lq * H <= 2^34; max_pos and the bias strides <= 2^40
LIMITS = (2, 3, 5, 8, 9, 16, 32, 33, 64, 65, 128, 129, 2048, 2056, 4096, 4098, 8192, 8193, 8200, 65535, 65536,
          2 ** 20, 2 ** 20 + 1, 2 ** 22, 2 ** 22 + 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 8, 2 ** 28, 2 ** 28 + 1, LIM - 2, LIM - 1,
          2 ** 32 + 1, 2 ** 34 + 1, 2 ** 40, 2 ** 40 + 1)


def prototypes():
    """{name: [(kind, argument name)]} of the header; kinds as in mmfs_abi.py (i int, l int64_t, u unsigned, f float, p pointer)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(HEADER).read(), flags=re.S)
    kinds = {"int": "i", "int64_t": "l", "unsigned": "u", "float": "f"}
    out = {}
    for name, args in re.findall(r"^(?:const char \*|\w+)\s*\b(mmfs_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        args = [" ".join(a.split()) for a in args.split(",") if a.strip() != "void"]
        out[name] = [("p", a.rsplit("*", 1)[1].strip()) if "*" in a else (kinds[a.rsplit(" ", 1)[0]], a.rsplit(" ", 1)[1])
                     for a in args]
    return out


PROTOS = prototypes()
_KEEP = []                                           # the host arrays, alive as long as the module


def host_i64(*values, n=16):
    a = (ctypes.c_int64 * n)(*values)
    _KEEP.append(a)
    return ("host", ctypes.cast(a, ctypes.c_void_p).value)


def host_ptrs(count, n=8):
    a = (ctypes.c_void_p * n)(*[0x7000000 + 0x10000 * i for i in range(count)])
    _KEEP.append(a)
    return ("host", ctypes.cast(a, ctypes.c_void_p).value)


HW23 = host_i64(2, 3)                                # one level of 2 x 3 tokens
HW23_12 = host_i64(2, 3, 1, 2)                       # two levels, 8 tokens
BANK_HW = host_i64(6, 2, n=8)
BANK_PTRS = host_ptrs(2)

# ---- base calls: {entry: {base name: {argument: value}}}.  A pointer that is not named gets a fake address; None is NULL.
_PLAN = dict(N=2, Lq=3, H=2, L=2, n=2, M=5, Lr=1, Nr=1, ld_off=0, ld_att=0, ld_toff=0, ld_tatt=0, q_grads_in_storage_type=0,
             S=20, D=16, Nv=2, layout=0)
PLAN_BASES = {
    "p4_bf16": dict(_PLAN, dtype=2, P=4),
    "p8_f16_strided": dict(_PLAN, dtype=1, P=8, Lr=3, Nr=2, ld_off=48, ld_att=40, ld_toff=48, ld_tatt=40,
                           q_grads_in_storage_type=1, D=64),
    "p16_f32": dict(_PLAN, dtype=0, P=16, D=8),
    "p4_interleave": dict(_PLAN, dtype=2, P=4, N=4, Nv=2, layout=1, token=None, q_grads_in_storage_type=1),
}
_DEFORM = dict(N=2, Lq=3, H=2, L=2, Nr=1, Lref=1, R=2, ld_off=0, ld_att=0, S=20)
DEFORM_BASES = {
    "p4_bf16": dict(_DEFORM, dtype=2, P=4, D=16),
    "p8_f16_strided": dict(_DEFORM, dtype=1, P=8, Nr=2, Lref=2, R=4, ld_off=80, ld_att=40, D=64),
    "p2_f32": dict(_DEFORM, dtype=0, P=2, D=8),
}
_DWCONV = {"none_bf16": dict(dtype=2, level_hw=HW23, B=2, N=6, C=8, L=1, act=0),
           "gelu_f32_two_levels": dict(dtype=0, level_hw=HW23_12, B=2, N=8, C=4, L=2, act=1),
           "none_no_bias": dict(dtype=1, level_hw=HW23, B=1, N=6, C=16, L=1, act=0, bias=None, pre=None, grad_bias=None)}
_PYR = dict(dtype=2, B=2, H=2, W=2, C=8)
PYRAMID_BASES = {"mask1_nchw": dict(_PYR, levels=1, c1_layout=0), "mask14": dict(_PYR, levels=14, c1_layout=0),
                 "mask15_nhwc": dict(_PYR, levels=15, c1_layout=1), "mask15_nchw_f32": dict(_PYR, dtype=0, C=4, levels=15, c1_layout=0)}
_EMBED = dict(dtype=2, text_dtype=2, soi_token_id=8, rows=6, L=3, C=8, n_vis=4, n_images=2)
EMBED_BASES = {"text_T": _EMBED, "text_f32": dict(_EMBED, dtype=1, text_dtype=0), "no_vis": dict(_EMBED, n_vis=0, n_images=0)}
_CTX = dict(dtype=2, B=2, L=3, C=8, n_images=2, max_len=4, seq_len=5)
CONTEXT_BASES = {"bf16": _CTX, "f32": dict(_CTX, dtype=0, C=4), "no_images": dict(_CTX, n_images=0)}
_LOSS = dict(dtype=2, B=2, L=4, V=10, first=1, n=2, ignore_index=-100)
LOSS_BASES = {"none": dict(_LOSS, reduction=0), "sum_f32": dict(_LOSS, dtype=0, reduction=1), "mean": dict(_LOSS, reduction=2)}
_QK = dict(dtype=2, B=2, H=2, D=64, Nq=3, Nk=5, eps=1e-5, norm_dtype=0, bias_dtype=0, bias_stride=5)
_NO_NORM = dict(q_norm_weight=None, q_norm_bias=None, k_norm_weight=None, k_norm_bias=None, partials=None, grad_params=None)
QK_BASES = {"norm_f32_bias_f32": _QK, "norm_T_bias_T": dict(_QK, dtype=1, norm_dtype=1, bias_dtype=1, bias_stride=0),
            "no_norm_no_bias": dict(_QK, **_NO_NORM, key_bias=None), "no_norm_bias_T": dict(_QK, **_NO_NORM, bias_dtype=2)}
_LLAMA = dict(dtype=2, B=2, Lq=3, L=3, H=2, D=128, cap=8, kv_bound=5, max_pos=16, flags=0, bias_dtype=0, bias_stride=8,
              bias_len=5, bias_batch_stride=0, bias_query_stride=0)
_NO_ROPE = dict(max_pos=0, cos_table=None, sin_table=None)
LLAMA_BASES = {"bf16_no_bias": dict(_LLAMA, bias=None), "f16_bias_f32": dict(_LLAMA, dtype=1, flags=1, bias_query_stride=8,
                                                                              bias_batch_stride=24),
               "bf16_bias_T": dict(_LLAMA, bias_dtype=2, bias_stride=0, flags=2, **_NO_ROPE),
               "f16_visit_all_causal": dict(_LLAMA, dtype=1, flags=3, bias=None)}
_BANK = dict(n_levels=2, level_hw=BANK_HW, n_img=2, C=8, n_slots=3)
BANK_BASES = {"bf16": dict(_BANK, dtype=2), "f32": dict(_BANK, dtype=0)}
for _b in BANK_BASES.values():
    _b["level_ptrs"] = _b["grad_level_ptrs"] = BANK_PTRS
NORM_BASES = {"bf16_one_vector": dict(dtype=2, rows=3, C=512, eps=1e-6), "bf16_longest": dict(dtype=2, rows=3, C=8192, eps=1e-6),
              "f32_one_vector": dict(dtype=0, rows=3, C=256, eps=1e-6)}
_QUERY = dict(dtype=2, B=2, C=8, HW=8, eps=1e-5)
QUERY_BASES = {"bf16": _QUERY, "f16_no_stats": dict(_QUERY, dtype=1, C=2048, HW=16, mean=None, rstd=None, pos=None)}
_LIN = dict(dtype=2, M=2, N=5, K=8, ldx=8, ldy=5, ldr=5)
LINEAR_BASES = {"m2_packed": _LIN, "m8_f16_strided": dict(_LIN, dtype=1, M=8, K=16, ldx=24, ldy=8, ldr=8),
                "no_bias_no_residual": dict(_LIN, bias=None, residual=None, ldr=0)}
def without(bases, *names):
    return {k: v for k, v in bases.items() if k not in names}


BASES = {
    # (the bank layouts: the two entries that take one)
    **{e: without(PLAN_BASES, "p4_interleave") for e in (
        "mmfs_plan_forward", "mmfs_plan_backward", "mmfs_plan_forward_heads", "mmfs_plan_backward_heads", "mmfs_sample_forward",
        "mmfs_sample_forward_token", "mmfs_sample_forward_heads")},
    "mmfs_sample_forward_heads_shared": PLAN_BASES,
    "mmfs_sample_forward_heads_fp8": {**PLAN_BASES, "p4_bf16_d256": dict(PLAN_BASES["p4_bf16"], D=256)},
    "mmfs_bank_quantize_fp8": {"bf16": dict(dtype=2, nbanks=2, Bv=2, R=3, C=32), "f32": dict(dtype=0, nbanks=1, Bv=1, R=1, C=16)},
    **{e: DEFORM_BASES for e in ("mmfs_deform_plan_forward", "mmfs_deform_plan_backward", "mmfs_deform_sample_forward")},
    "mmfs_dwconv_tokens_forward": _DWCONV, "mmfs_dwconv_tokens_backward": _DWCONV,
    "mmfs_pyramid_head_forward": PYRAMID_BASES, "mmfs_pyramid_head_backward": PYRAMID_BASES,
    "mmfs_sequence_index": {"images": dict(B=2, L=3, image_token_id=7, soi_token_id=8, n_vis=4, n_images=2),
                            "text_only": dict(B=2, L=3, image_token_id=7, soi_token_id=8, n_vis=0, n_images=0)},
    "mmfs_sequence_embed_forward": EMBED_BASES, "mmfs_sequence_embed_backward": EMBED_BASES,
    "mmfs_sequence_context_forward": CONTEXT_BASES, "mmfs_sequence_context_backward": CONTEXT_BASES,
    "mmfs_text_loss_forward": LOSS_BASES, "mmfs_text_loss_backward": LOSS_BASES,
    "mmfs_qk_attn_forward": QK_BASES, "mmfs_qk_attn_backward": QK_BASES,
    # (the four flag words: the prefill; a bias: it and the decode step; the rotary tables: all but the training forward)
    "mmfs_llama_attn_prefill": LLAMA_BASES,
    **{e: without(LLAMA_BASES, "f16_visit_all_causal") for e in (
        "mmfs_llama_attn_rope_append", "mmfs_llama_attn_decode", "mmfs_llama_attn_train_rope", "mmfs_llama_attn_train_backward")},
    "mmfs_llama_attn_train_forward": without(LLAMA_BASES, "f16_visit_all_causal", "bf16_bias_T"),
    "mmfs_bank_gather": BANK_BASES, "mmfs_bank_scatter": BANK_BASES,
    "mmfs_rmsnorm_forward": NORM_BASES, "mmfs_rmsnorm_backward": NORM_BASES, "mmfs_rmsnorm_backward_partials": NORM_BASES,
    "mmfs_query_prep": QUERY_BASES, "mmfs_tokens_add": QUERY_BASES,
    "mmfs_linear_small": LINEAR_BASES, "mmfs_linear_small_add": LINEAR_BASES,
}
LAUNCHING = tuple(BASES)

# ---- the host-only queries: {query: one tuple of values per argument}; "hw" / "null": the dwconv level table
_C16 = (-1, 0, 1, 4, 8, 12, 16, 2 ** 24, 2 ** 24 + 8)
_BH = (-1, 0, 1, 2 ** 12, 2 ** 13, 2 ** 20, 2 ** 20 + 1)
_LEVEL = tuple(range(-1, 7))
QUERY_GRIDS = {
    "mmfs_sample_forward_groups": (DTYPES, (-1, 0, 1, 8, 9), (0, 4, 8, 12, 16, 24, 64, 128, 256, 512, 1024), (0, 1, 4, 32, 33, 64, 65),
                                   (2, 4, 8, 16)),
    "mmfs_deform_plan_supported": (DTYPES, (-1, 0, 1, 8, 9), (1, 2, 3, 4, 8, 16), (1, 2, 3, 4, 5),
                                   (0, 4, 8, 16, 24, 32, 64, 128, 256, 512, 1024)),
    "mmfs_dwconv_tokens_supported": (DTYPES, _C16, (0, 1, 8, 9), (-1, 0, 1, 2, 3)),
    "mmfs_dwconv_tokens_backward_workspace_bytes": (DTYPES, ("hw", "null"), (-1, 0, 2, LIM), (-1, 0, 6, 8, LIM),
                                                    (-1, 0, 4, 8, 2 ** 24, 2 ** 24 + 8), (0, 1, 2, 3, 9), (0, 1, 2)),
    "mmfs_pyramid_head_supported": (DTYPES, (-1, 0, 4, 8, 12), (0, 1, 2, 3, 4, 4096, 4098), (0, 1, 2, 3, 4, 4096, 4098),
                                    tuple(range(-1, 18))),
    "mmfs_sequence_supported": (DTYPES, _C16),
    "mmfs_sequence_context_backward_workspace_bytes": (DTYPES, _C16, (-1, 0, 1, 2 ** 22, 2 ** 22 + 1)),
    "mmfs_text_loss_supported": (DTYPES, (-1, 0, 1, 2, 2 ** 24, 2 ** 24 + 1)),
    "mmfs_qk_attn_supported": (DTYPES, (0, 32, 64, 128), (0, 1, 128, 129), (0, 1, 8192, 8193)),
    "mmfs_llama_attn_supported": (DTYPES, (0, 64, 128, 256), (0, 1, 8, 9, 2 ** 22, 2 ** 22 + 1), (0, 1, 8, 2 ** 22, 2 ** 22 + 1)),
    "mmfs_llama_attn_decode_keys": (_LEVEL,),
    "mmfs_llama_attn_decode_workspace_bytes": (_BH, _BH, (0, 1, 2, 255, 256, 257, 511, 512, 513, 1024, 1025, 2 ** 22, 2 ** 22 + 1)),
    "mmfs_llama_attn_prefill_tiles": (_LEVEL,),
    "mmfs_llama_attn_train_supported": (DTYPES, (0, 64, 128, 256), (-1, 0, 1, 2 ** 22, 2 ** 22 + 1)),
    "mmfs_llama_attn_train_tiles": (_LEVEL,),
    "mmfs_llama_attn_train_workspace_bytes": (_BH, _BH, (-1, 0, 1, 2 ** 22, 2 ** 22 + 1)),
    "mmfs_rmsnorm_supported": (DTYPES, (-1, 0, 1, 4, 8, 12, 256, 512, 4096, 4100, 4104, 8192, 8200, 16384)),
    "mmfs_query_prep_supported": (DTYPES, (-1, 0, 4, 8, 12, 2048, 2056), (-1, 0, 4, 8, 12)),
    "mmfs_linear_small_supported": (DTYPES, (0, 1, 4, 5, 8, 9), (0, 1, 0x3fffffff, 0x40000000), (0, 4, 8, 12, 4096, 4104, 8192, 8200)),
}
QUERIES = tuple(QUERY_GRIDS)


def is_dtype(name):
    return name.endswith("dtype")


def base_call(entry, base):
    """{argument name: value} of a valid call, and the names of its fake pointers / of all its pointers."""
    args, fake, ptrs = {}, [], []
    for i, (kind, name) in enumerate(PROTOS[entry]):
        if name == "stream":
            args[name] = None
        elif kind != "p":
            args[name] = base[name]
        else:
            v = base.get(name, 0x100000 * (i + 1))           # distinct, 4096-aligned, never dereferenced
            ptrs.append(name)
            if isinstance(v, tuple):
                v = v[1]                                     # a host array: NULL is its only fault
            elif v is not None:
                fake.append(name)
            args[name] = v
    return args, fake, ptrs


def faults(entry, base):
    """(name, {argument: value}) of every fault of a base call: one argument at a time, then two."""
    args, fake, ptrs = base_call(entry, base)
    yield "base", {}                                         # (P = 16 is a base the sample entries refuse as a whole)
    for kind, name in PROTOS[entry]:
        if kind in "iu":
            for v in (DTYPES if is_dtype(name) else WORDS):
                yield f"{name}={v}", {name: v % 2 ** 32 if kind == "u" else v}
        elif kind == "l":
            for off in (-1, 1, 2):
                yield f"{name}{off:+d}", {name: args[name] + off}
            # (a stride or leading dimension: 0, one short and off its vector are above; its own limits are 2^31 - 1 and 2^40)
            stride = name.startswith("ld") or "stride" in name
            for v in sorted({-1, 0, 1, LIM} | set(LIMITS[-5:] if stride else LIMITS)):
                yield f"{name}={v}", {name: v}
    for name in ptrs:
        yield f"{name}=NULL", {name: None}
    for off in (1, 2, 4, 8, 16, 32):
        for name in fake:
            yield f"{name}+{off}", {name: args[name] + off}
    for i, a in enumerate(ptrs):                             # (a, b) with a before b in the ABI's order, and the mirror
        for b in fake:                                       # for the first and the last pointer
            if ptrs.index(b) > i or (a != b and (i in (0, len(ptrs) - 1) or b in (ptrs[0], ptrs[-1]))):
                yield f"{a}=NULL,{b}+2", {a: None, b: args[b] + 2}
    for kind, name in PROTOS[entry]:
        if kind == "l":
            for p in ptrs:
                yield f"{name}=-1,{p}=NULL", {name: -1, p: None}
            for p in fake:
                yield f"{name}=-1,{p}+2", {name: -1, p: args[p] + 2}


def fault_names(entry):
    """The fault names of an entry's bases, each once, in the order of the sweep: the columns of the file's runs."""
    return list(dict.fromkeys(fname for base in BASES[entry].values() for fname, _ in faults(entry, base)))


def names_mark(names):
    """What the file keeps in the place of the names (they are the sweep's own): how many, and a digest of them."""
    return [len(names), hashlib.sha1("\n".join(names).encode()).hexdigest()[:12]]


def empty_problem(entry, args):
    """MMFS_OK without a launch: an int64 argument is 0, or a NULL pointer stands for an output nobody asked for."""
    return any(args[name] in (0, None) for kind, name in PROTOS[entry] if kind in "lp" and name != "stream")


def sweep(lib, entry):
    """{case: (status, it returned before any launch)}"""
    out, names = {}, [name for _, name in PROTOS[entry]]
    fn = getattr(lib, entry)
    for bname, base in BASES[entry].items():
        args, _, _ = base_call(entry, base)
        for fname, change in faults(entry, base):
            call = dict(args, **change)
            status = fn(*[call[n] for n in names])
            case = f"{bname}/{2 if ',' in fname else 1}/{fname}"
            out[case] = (status, returns_before_launch(case, status) or (status == 0 and empty_problem(entry, call)))
    return out


def query_values(lib, query):
    """{first argument[/last argument]: [value over the grid of the arguments between them]} -- the last argument is often
    an option word whose valid values answer alike: the file then holds their runs once"""
    fn, grid, out = getattr(lib, query), QUERY_GRIDS[query], {}
    table = {"hw": HW23_12[1], "null": None}
    for first in grid[0]:
        for last in (grid[-1] if len(grid) > 1 else ((),)):
            calls = [(first,) + mid + (() if last == () else (last,)) for mid in itertools.product(*grid[1:-1])]
            out["/".join(str(h) for h in (first, last) if h != ())] = [
                fn(*[table.get(v, v) if isinstance(v, str) else v for v in call]) for call in calls]
    return out


def clear_environment(lib):
    """Every MMFS_* variable but the library's path goes (-> what to put back) and the library reads its knobs again."""
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("MMFS_") and k != "MMFS_MSDA_LIB"}
    lib.mmfs_env_reload()
    return saved


def record(lib):
    """The golden file's content from ``lib``; only what returns before any launch goes into the file."""
    gold, pinned, launched = {"statuses": {}, "queries": {}}, 0, 0
    for entry in LAUNCHING:
        got = sweep(lib, entry)
        for case, (status, before) in got.items():
            assert before or status > 0, f"{entry}: {case}: MMFS_OK from a call that is no empty problem"
        kept = sum(before for _, before in got.values())
        pinned, launched = pinned + kept, launched + len(got) - kept
        print(f"{entry}: {kept} cases pinned, {len(got) - kept} reach a launch and are left out", file=sys.stderr)
        packed = pack({c: s if before else None for c, (s, before) in got.items()})
        assert packed["faults"] == fault_names(entry)
        gold["statuses"][entry] = dict(packed, faults=names_mark(packed["faults"]))
    for q in QUERIES:
        values = query_values(lib, q)
        pinned += sum(len(v) for v in values.values())
        gold["queries"][q] = pack_query(values)
    print(f"{pinned} cases pinned in all, {launched} reach a launch", file=sys.stderr)
    return gold


@pytest.fixture(scope="module")
def lib():
    from helpers import bound_library
    lib = bound_library()
    saved = clear_environment(lib)
    yield lib
    os.environ.update(saved)
    lib.mmfs_env_reload()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        gold = json.load(f)
    return {"statuses": gold["statuses"], "queries": {q: unpack_query(p) for q, p in gold["queries"].items()}}


def test_sweep_covers_the_module():
    """Every prototype of the header besides the op's and the library's own (version, environment, debug) is swept."""
    swept = set(LAUNCHING) | set(QUERIES) | {"mmfs_rmsnorm_backward_partials_rows"}    # (that one: test_capi_status.py)
    rest = {n for n in PROTOS if not n.startswith(("mmfs_msda_", "mmfs_env_", "mmfs_debug_"))}
    assert swept == rest and len(LAUNCHING) == 41 and len(QUERIES) == 19


def test_golden_file_holds_no_case_that_launches(golden):
    assert sorted(golden["statuses"]) == sorted(LAUNCHING) and sorted(golden["queries"]) == sorted(QUERIES)
    for entry, packed in golden["statuses"].items():
        runs = [run for base, group in packed.items() if isinstance(group, dict) for row in group.values() for run in row]
        assert sum(n for status, n in runs if status is not None) > 10, entry
        assert all(status is None or status <= 0 for status, _ in runs), entry


@pytest.mark.parametrize("entry", LAUNCHING)
def test_entry_statuses_are_the_recorded_ones(lib, golden, entry):
    packed, names = golden["statuses"][entry], fault_names(entry)
    assert packed["faults"] == names_mark(names), f"{entry}: the sweep's cases are not the ones the file was recorded with"
    want = unpack(dict(packed, faults=names))
    got = sweep(lib, entry)
    assert set(want) <= set(got), f"{entry}: cases of the file the sweep no longer makes: {sorted(set(want) - set(got))[:5]}"
    wrong = [f"{entry}: {c}: returned {got[c][0]}, recorded {s}" for c, s in want.items() if got[c][0] != s]
    # a case that was not pinned reached a launch when the file was recorded: it still must (positive status, no device)
    wrong += [f"{entry}: {c}: returned {s}, reached a launch when recorded" for c, (s, _) in got.items()
              if c not in want and s <= 0]
    assert not wrong, "\n".join(wrong[:40] + [f"({len(wrong)} in all)"])


@pytest.mark.parametrize("query", QUERIES)
def test_host_only_queries_are_the_recorded_ones(lib, golden, query):
    want, got = golden["queries"][query], query_values(lib, query)
    assert sorted(want) == sorted(got)
    rest = list(itertools.product(*QUERY_GRIDS[query][1:-1]))
    wrong = [f"{query}: {key}/{'/'.join(map(str, r))}: returned {g}, recorded {v}"
             for key, values in want.items() for r, g, v in zip(rest, got[key], values) if g != v]
    assert all(len(want[k]) == len(got[k]) for k in want)
    assert not wrong, "\n".join(wrong[:40] + [f"({len(wrong)} in all)"])


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "mm-interleaved_amd"))
    import mmfs_abi
    library = mmfs_abi.bind(ctypes.CDLL(os.environ["MMFS_MSDA_LIB"]))
    clear_environment(library)
    recorded = record(library)
    with open(GOLDEN, "w") as f:
        dump(recorded, f)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes", file=sys.stderr)
