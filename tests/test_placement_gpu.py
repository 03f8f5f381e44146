"""GPU: the op and the kernels around it with their operands where a caller may put them, not where torch's allocator does.

B.  The op at the least alignment its C contract takes (csrc/msda_capi.hip ``check_tensors``): ``sampling_loc`` and
    ``attn_weight`` one element past a 16-byte boundary (a view into a flat buffer), ``attn_weight`` at 4 mod 8, and --
    for a head width whose rows are no multiple of 16 bytes (``row_align``: D = 6) -- ``value``, ``out``, ``grad_out`` and
    ``grad_value`` one element off as well.  Every route of the forward and the backward, every placement: the oracle's
    per-element bound; the forward, grad_loc and grad_attn bit-equal to the aligned run (alignment changes how operands
    are loaded, not the arithmetic); grad_value with a misaligned loc bit-equal to the aligned run under
    MMFS_SORT_REPACK=1 (the same re-pack branch on the same numbers); inputs untouched, no byte outside any tensor.
C.  Exact extents: each wrapper under mmfs_amd/functions and the op through the shim, with every output and workspace they
    allocate placed between guard bands (tests/helpers.py ``guarded_allocations``) and every input between 0xFF bands.

About grad_value's bits: the cell sort hands out a cell's slots by LDS atomics, so across waves the order of a pixel's fp32
sum is not fixed from run to run (tests/test_stress_gpu.py).  With at most 64 queries every sample of a slice sits in ONE
wave and the order is the lanes': equality of grad_value is asserted at such shapes only, the bound everywhere."""
import functools

import numpy as np
import pytest
import torch

from helpers import (OUTPUT_GUARD, OUTPUTS, assert_bit_equal, assert_guards_intact, assert_no_poison, assert_payload_unchanged,
                     assert_within_bounds, bound_ratios, error_bounds, make_inputs, near_crossing, placed, poison, run_placed,
                     KINDS, MAX_LEFT_OUT, ODD_D, OP_DTYPES)

pytestmark = pytest.mark.gpu
DEV = "cuda"
name = lambda dtype: str(dtype)[6:]


@functools.lru_cache(maxsize=None)
def case(dtype, D, kind="ragged"):
    """(inputs, bounds) of the oracle for one input set, computed once and left unchanged."""
    x = KINDS[kind](dtype, D)
    assert float(np.mean(near_crossing(x))) <= MAX_LEFT_OUT
    return x, error_bounds(x, dtype)[0]


def held(got, dtype, D, what, kind="ragged"):
    x, bounds = case(dtype, D, kind)
    outputs = tuple(n for n, g in zip(OUTPUTS, got) if g is not None)
    res = bound_ratios([None if g is None else g.double().cpu().numpy() for g in got], x, dtype, outputs, bounds=bounds)
    print(f"PLACEMENT-BOUND {name(dtype)} D{D} {what}: " + " ".join(f"{n}={r[0]:.3g}" for n, r in res.items()))
    bad = {n: r for n, r in res.items() if not r[0] <= 1.0}
    assert not bad, f"{what}: per-element bound broken: " + "; ".join(
        f"{n} {r[0]:.3g} x the bound at {r[1]} (err {r[2]:.3e}, bound {r[3]:.3e})" for n, r in bad.items())


def storage(x, dtype):
    """The op's arguments as CPU tensors of the storage type (the level tables int64), by name."""
    f = lambda t: t.to(dtype)
    B, Nq = x["loc"].shape[:2]
    return dict(value=f(x["value"]), shapes=x["shapes"], start=x["start"], loc=f(x["loc"]), attn=f(x["attn"]),
                grad=f(x["grad"]).reshape(B, Nq, -1))


def op_call(monkeypatch, attrs=None, env=None, backward=True, registered=True):
    """-> fn(value, shapes, start, loc, attn, grad) -> [out, grad_value, grad_loc, grad_attn] through the shim, with the
    shim's switches ``attrs`` and the knobs ``env`` set for the call and the level table registered."""
    import MultiScaleDeformableAttention as MSDA

    def fn(value, shapes, start, loc, attn, grad):
        with monkeypatch.context() as m:
            m.setattr(MSDA, "_ws_cache", {})
            for k, v in (attrs or {}).items():
                m.setattr(MSDA, k, v)
            for k, v in (env or {}).items():
                m.setenv(k, v)
            if registered:
                MSDA.register_level_tables(shapes, start, value.shape[1])
            out = MSDA.ms_deform_attn_forward(value, shapes, start, loc, attn, 1)
            grads = MSDA.ms_deform_attn_backward(value, shapes, start, loc, attn, grad, 1) if backward else [None] * 3
            torch.cuda.synchronize()
        return [out, *grads]
    return fn


def placements(dtype):
    es = torch.empty((), dtype=dtype).element_size()
    p = {"loc+1": dict(loc=es), "attn+1": dict(attn=es), "loc+1 attn+1": dict(loc=es, attn=es)}
    if es != 4:
        p["attn at 4 mod 8"] = dict(attn=4)
    return p


# ---------------------------------------------------------------------------------------------------- B: the forward
FWD = [("auto", 32), ("gather", 32), ("auto", 128), ("gather", 128), ("lds", 128), ("slices", 128), ("waves", 128)]


# (the LDS-resident formulations serve 16-bit storage only: msda_mma_common.h resident_shape_supported)
FWD_CASES = [(a, d, t) for a, d in FWD for t in OP_DTYPES if not (a in ("lds", "slices", "waves") and t == torch.float32)]


@pytest.mark.parametrize("algo,D,dtype", FWD_CASES, ids=[f"{a}-D{d}-{name(t)}" for a, d, t in FWD_CASES])
def test_forward_takes_loc_and_attn_at_element_alignment(algo, D, dtype, monkeypatch):
    x, _ = case(dtype, D)
    fn = op_call(monkeypatch, attrs=dict(_fwd_algo=algo), backward=False)
    aligned = None
    for what, leads in {"aligned": {}, **placements(dtype)}.items():
        got, plain, rec = run_placed(monkeypatch, fn, storage(x, dtype), leads=leads)      # (asserts bit-equality to ``plain``)
        held(got, dtype, D, f"forward {algo}, {what}")
        aligned = aligned if aligned is not None else got
        assert_bit_equal(got[0], aligned[0], f"forward {algo}, {what} against the aligned run")


# ---------------------------------------------------------------------------------------------------- B: the backward
BWD_ROUTES = {
    "auto": dict(),
    "atomic": dict(attrs=dict(_bwd_algo="atomic")),
    "hybrid off": dict(attrs=dict(_hybrid=False)),
    "value block": dict(env=dict(MMFS_VALUE_ALGO="block")),
    "value pixel": dict(env=dict(MMFS_VALUE_ALGO="pixel")),
    "sorted taps": dict(attrs=dict(_taps_prefer_sorted=True)),
    # (the grad_value half's opening job hosted by msda_taps_mma, or a launch of its own: heads of 128 channels on that kernel)
    "prepare on its own": dict(env=dict(MMFS_PREPARE_IN_TAPS="0"), attrs=dict(_taps_algo="lds"), D=128),
    "prepare in taps": dict(env=dict(MMFS_PREPARE_IN_TAPS="1"), attrs=dict(_taps_algo="lds"), D=128),
    "pairs off": dict(env=dict(MMFS_TILE_PAIR="0")),
    "pairs on": dict(env=dict(MMFS_TILE_PAIR="1")),
}


# 16-bit storage only: the sorted taps route (csrc/msda_bwd_block.hip taps_sorted_supported), msda_taps_mma, the tile reduce's pairs
HALF_ONLY = ("sorted taps", "prepare on its own", "prepare in taps", "pairs off", "pairs on")
BWD_CASES = [(r, t) for r in sorted(BWD_ROUTES) for t in OP_DTYPES if not (r in HALF_ONLY and t == torch.float32)]


@pytest.mark.parametrize("route,dtype", BWD_CASES, ids=[f"{r}-{name(t)}" for r, t in BWD_CASES])
def test_backward_takes_loc_and_attn_at_element_alignment(route, dtype, monkeypatch):
    """33 queries: one wave of the sort holds a slice's samples, so grad_value's bits are fixed (module docstring)."""
    import MultiScaleDeformableAttention as MSDA
    r = BWD_ROUTES[route]
    D, attrs, env = r.get("D", 32), r.get("attrs", {}), r.get("env", {})
    x, _ = case(dtype, D)
    fn = op_call(monkeypatch, attrs=attrs, env=env)
    sorted_before = MSDA.route_counts["sorted"]
    aligned, _, _ = run_placed(monkeypatch, fn, storage(x, dtype), bit_equal=False)
    if route == "sorted taps":
        assert MSDA.route_counts["sorted"] == sorted_before + 2, "the sorted route refused: the case tests nothing"
    held(aligned, dtype, D, f"backward {route}, aligned")
    repacked, _, _ = run_placed(monkeypatch, op_call(monkeypatch, attrs=attrs, env=dict(env, MMFS_SORT_REPACK="1")),
                                storage(x, dtype), bit_equal=False)
    held(repacked, dtype, D, f"backward {route}, aligned, MMFS_SORT_REPACK=1")
    for what, leads in placements(dtype).items():
        got, plain, rec = run_placed(monkeypatch, fn, storage(x, dtype), leads=leads, bit_equal=False)
        held(got, dtype, D, f"backward {route}, {what}")
        for k, n in ((0, "out"), (2, "grad_loc"), (3, "grad_attn")):
            assert_bit_equal(got[k], aligned[k], f"backward {route}, {what}: {n} against the aligned run")
        if route != "atomic":                              # (float atomics: any order, the bound alone)
            assert_bit_equal(got[1], repacked[1], f"backward {route}, {what}: grad_value against the aligned run under MMFS_SORT_REPACK=1")


# ---------------------------------------------------------------------------------------------------- B: element-aligned rows
# ODD_D = 6: rows of 12 bytes (16-bit storage) and 24 bytes (fp32) -- ``row_align`` is the element size for all three types
def odd_width_call(dtype, t, lead_out):
    """The forward and the one-call backward through the C entries (the shim would re-align ``value`` and ``grad_output``) on the
    device tensors ``t``; outputs placed ``lead_out`` bytes off between guards.  -> the four output handles."""
    import MultiScaleDeformableAttention as MSDA
    code, dev = MSDA._DTYPE_CODE[dtype], torch.device(DEV, 0)
    B, S, H, D = t["value"].shape
    Nq, L, P = t["loc"].shape[1], t["loc"].shape[3], t["loc"].shape[4]
    dims = (B, S, H, D, L, Nq, P)
    outs = [placed(torch.zeros(s, dtype=dtype), lead_out, OUTPUT_GUARD, DEV, name=n)
            for n, s in (("out", (B, Nq, H * D)), ("grad_value", t["value"].shape), ("grad_loc", t["loc"].shape), ("grad_attn", t["attn"].shape))]
    for h in outs:
        poison(h.t)
    flags = MSDA._BWD_CANONICAL_LEVELS
    ws_bytes = MSDA._lib.mmfs_msda_backward_workspace_bytes(code, *dims, flags)
    ws = placed(torch.zeros(max(ws_bytes, 16), dtype=torch.uint8), 0, OUTPUT_GUARD, DEV, name="workspace")
    poison(ws.t)
    ptr = lambda k: t[k].data_ptr()
    MSDA._call("msda_fwd", "mmfs_msda_forward_flags", dev, code, ptr("value"), ptr("shapes"), ptr("start"), ptr("loc"), ptr("attn"),
               outs[0].t.data_ptr(), *dims, 0)
    MSDA._call("msda_bwd", "mmfs_msda_backward_checked", dev, code, ptr("value"), ptr("shapes"), ptr("start"), ptr("loc"), ptr("attn"),
               ptr("grad"), outs[1].t.data_ptr(), outs[2].t.data_ptr(), outs[3].t.data_ptr(), ws.t.data_ptr() if ws_bytes else None,
               ws_bytes, *dims, flags, None)
    torch.cuda.synchronize()
    assert_guards_intact(ws, *outs)
    return outs


@pytest.mark.parametrize("dtype", OP_DTYPES, ids=name)
def test_rows_of_no_16_byte_multiple_take_every_operand_at_element_alignment(dtype):
    """D = 6: the scalar forward and the float-atomic backward (no vector path for that width), which the contract lets start
    anywhere an element may -- value, out, grad_out, grad_value, loc, attn, grad_loc and grad_attn all one element past a
    16-byte boundary.  The 16-bit grad_value is cast from the fp32 accumulator by a kernel that stored 8 bytes at a time
    whatever the pointer (csrc/msda_bwd.hip ``cast_kernel``): fixed with this test.  Out, grad_loc and grad_attn are one
    thread's sums: bit-equal to the aligned run; grad_value is float atomics: the bound."""
    es = torch.empty((), dtype=dtype).element_size()
    x, _ = case(dtype, ODD_D)
    results = {}
    for what, lead in (("aligned", 0), ("one element off", es)):
        hs = {k: placed(v, lead if v.is_floating_point() else 0, device=DEV, name=k) for k, v in storage(x, dtype).items()}
        outs = odd_width_call(dtype, {k: h.t for k, h in hs.items()}, lead)
        assert all(h.t.data_ptr() % 16 == lead for h in outs)
        assert_guards_intact(*hs.values())
        assert_payload_unchanged(*hs.values())
        for h in outs:
            assert_no_poison(h.t, h.name)
        results[what] = [h.t for h in outs]
        held(results[what], dtype, ODD_D, f"odd width, {what}")
    for k in (0, 2, 3):
        assert_bit_equal(results["one element off"][k], results["aligned"][k], f"odd width: {OUTPUTS[k]} against the aligned run")


@pytest.mark.parametrize("dtype", OP_DTYPES, ids=name)
@pytest.mark.parametrize("lead_elems", [0, 1, 7])
def test_nothing_to_sample_zero_fills_an_output_that_starts_anywhere(dtype, lead_elems):
    """No level (L = 0): the forward's value is 0, written by ``zero_fill`` (csrc/msda_bwd.hip) as head bytes, 16-byte body and
    tail bytes around the first 16-byte boundary -- for an ``out`` of 33 x 2 x 6 elements that starts 0, 1 and 7 elements past
    one: every byte of it +0, none outside it."""
    import MultiScaleDeformableAttention as MSDA
    es = torch.empty((), dtype=dtype).element_size()
    B, S, H, D, L, Nq, P = 1, 41, 2, ODD_D, 0, 33, 4
    out = placed(torch.zeros(B, Nq, H * D, dtype=dtype), lead_elems * es, OUTPUT_GUARD, DEV, name="out")
    poison(out.t)
    value = torch.ones(B, S, H, D, dtype=dtype, device=DEV)
    MSDA._call("msda_fwd", "mmfs_msda_forward_flags", torch.device(DEV, 0), MSDA._DTYPE_CODE[dtype], value.data_ptr(), None, None, None,
               None, out.t.data_ptr(), B, S, H, D, L, Nq, P, 0)
    torch.cuda.synchronize()
    assert_guards_intact(out)
    assert_bit_equal(out.t, torch.zeros_like(out.t), "out")


# ---------------------------------------------------------------------------------------------------- C: the op's extents
EXTENT_ROUTES = {k: BWD_ROUTES[k] for k in ("auto", "atomic", "hybrid off", "value block", "value pixel", "sorted taps", "pairs off")}
EXTENT_CASES = [("ragged", 32), ("hot", 64), ("pair", 32)]


EXTENTS = [(r, k, d, t) for r in sorted(EXTENT_ROUTES) for k, d in EXTENT_CASES for t in OP_DTYPES
           if not (r in HALF_ONLY and t == torch.float32)]


@pytest.mark.parametrize("route,kind,D,dtype", EXTENTS, ids=[f"{r}-{k}-{name(t)}" for r, k, d, t in EXTENTS])
def test_op_writes_inside_its_outputs_and_its_workspace(route, kind, D, dtype, monkeypatch):
    """The shim's forward and backward with ``out``, the three gradients and the planned workspace between guard bands and
    every input between 0xFF bands: the ragged shape, the hot spot whose block list is cut into chunks, and the one pair of
    whole blocks -- the workspace's data-dependent writers.  Out, grad_loc, grad_attn: the bits of ordinary allocations;
    grad_value: those too where one wave holds a slice's samples, the bound elsewhere (module docstring) and on the
    float-atomic route."""
    r = EXTENT_ROUTES[route]
    x, _ = case(dtype, D, kind)
    fn = op_call(monkeypatch, attrs=r.get("attrs", {}), env=r.get("env", {}))
    got, plain, rec = run_placed(monkeypatch, fn, storage(x, dtype), bit_equal=False)
    assert len(rec.records) >= 4 and rec.pass_through_count == 0
    held(got, dtype, D, f"extents {route}", kind)
    for k in (0, 2, 3):
        assert_bit_equal(got[k], plain[k], f"extents {route} {kind}: {OUTPUTS[k]} against ordinary allocations")
    if route != "atomic" and x["loc"].shape[1] <= 64:
        assert_bit_equal(got[1], plain[1], f"extents {route} {kind}: grad_value against ordinary allocations")


# ---------------------------------------------------------------------------------------------------- C: the row gather's walks
def walk_cases():
    from test_op_gpu import WALKS                            # (the list of test_row_gather_walks_at_their_smallest, not a copy)
    return [(t, D, live) for t, D, _ in WALKS for live in (0, 5)]


@pytest.mark.parametrize("dtype,D,live", walk_cases(), ids=lambda v: name(v) if isinstance(v, torch.dtype) else str(v))
def test_row_gather_walks_write_inside_their_output(dtype, D, live, monkeypatch):
    """The op's row gather at the walks of tests/test_op_gpu.py (WALKS): 1, 4 and 64 lanes per query, three queries (a ragged
    tile) of 8 samples each of which the first ``live`` weigh something, the middle query nothing at all -- ``out`` between guard
    bands, every input between 0xFF bands (a walk that reads a record or a row it should skip meets NaN), the oracle's bound,
    and the bits of ordinary allocations."""
    x = make_inputs(1, 1, D, 3, 4, [(3, 5), (2, 2)], seed=41, loc_range=(0.1, 0.9), dtype=dtype)
    keep = torch.zeros(1, 3, 1, 8, dtype=torch.float64)
    keep[..., :live] = 1.0
    keep[:, 1] = 0.0
    x["attn"] = x["attn"] * keep.reshape(1, 3, 1, 2, 4)
    got, plain, rec = run_placed(monkeypatch, op_call(monkeypatch, attrs=dict(_fwd_algo="gather"), backward=False), storage(x, dtype))
    assert len(rec.records) >= 1 and rec.pass_through_count == 0
    assert_within_bounds([got[0].double().cpu().numpy(), None, None, None], x, dtype, f"walk D{D}, {live} live", outputs=("out",))
    if live == 0:
        assert_bit_equal(got[0], torch.zeros_like(got[0]), "out of queries that weigh nothing")


# ---------------------------------------------------------------------------------------------------- C: the kernels around the op
# One or two calls of each wrapper under mmfs_amd/functions at the smallest ragged shapes their own test files name, forward
# and backward, through ``run_placed``: inputs between 0xFF bands, every output and workspace the wrapper allocates between
# 0xA5 bands, nothing returned left poisoned, nothing passed through unplaced, and the bits of the same call on ordinary
# allocations (results of float atomics excepted, each named where it is left out).
HALVES = [torch.bfloat16, torch.float16]


def rnd(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *shape, scale=1.0, shift=0.0: torch.randn(*shape, generator=g) * scale + shift


def differentiated(call, wrt, up="up", extra=0):
    """-> fn(**tensors) for ``run_placed``: ``call(t)`` (a tensor, or a tuple whose first ``1 + extra`` entries are returned
    and whose first entry is differentiated) on leaves of ``wrt``, backward from ``t[up]`` -> [outputs..., gradients...]."""
    def fn(**t):
        t = {k: (v.detach().requires_grad_(True) if k in wrt else v) for k, v in t.items()}
        out = call(t)
        outs = list(out[:1 + extra]) if isinstance(out, (tuple, list)) else [out]
        outs[0].backward(t[up])
        torch.cuda.synchronize()
        return [o.detach() for o in outs] + [t[k].grad for k in wrt]
    return fn


def family(monkeypatch, fn, inputs, min_records, bit_equal=True):
    got, plain, rec = run_placed(monkeypatch, fn, inputs, bit_equal=bit_equal)
    assert len(rec.records) >= min_records and rec.pass_through_count == 0, (len(rec.records), rec.passed_through)
    return got, plain


@pytest.mark.parametrize("dtype", OP_DTYPES, ids=name)
@pytest.mark.parametrize("case_index", [2, 3])
def test_bank_writes_inside_its_outputs(case_index, dtype, monkeypatch):
    from mmfs_amd.functions import BankGatherFunction
    from test_bank_gpu import CASES
    n_img, C, shapes, slots = CASES[case_index]
    r = rnd(7)
    levels = {f"level{i}": r(n_img, C, h, w).to(dtype) for i, (h, w) in enumerate(shapes)}
    inputs = dict(levels, src=torch.tensor(slots), up=r(len(slots), sum(h * w for h, w in shapes), C).to(dtype))
    call = lambda t: BankGatherFunction.apply(t["src"], *[t[k] for k in levels])
    family(monkeypatch, differentiated(call, tuple(levels)), inputs, 1 + len(levels))


@pytest.mark.parametrize("dtype", OP_DTYPES, ids=name)
def test_rmsnorm_writes_inside_its_outputs(dtype, monkeypatch):
    from mmfs_amd.functions import RMSNormFunction
    r = rnd(11)
    inputs = dict(x=r(5, 72, scale=3.0).to(dtype), w=(torch.rand(72) + 0.5).to(dtype), up=r(5, 72).to(dtype))
    family(monkeypatch, differentiated(lambda t: RMSNormFunction.apply(t["x"], t["w"], 1e-6), ("x", "w")), inputs, 4)   # y, rstd, gx, parts


@pytest.mark.parametrize("dtype", HALVES, ids=name)
def test_layout_kernels_write_inside_their_outputs(dtype, monkeypatch):
    """The (2, 64, 5, 8) layout shape: 40 pixels are one ragged tile of mmfs_query_prep; mmfs_tokens_add's tiles likewise."""
    from mmfs_amd.functions.query_func import QueryPrepFunction, TokensAddFunction
    B, C, H, W = 2, 64, 5, 8
    r = rnd(13)
    inputs = dict(sample=r(B, C, H, W, scale=1.5, shift=0.3).to(dtype), weight=r(C, scale=0.2, shift=1.0).to(dtype),
                  bias=r(C, scale=0.1).to(dtype), pos=r(H * W, C).to(dtype), up=r(B, H * W, C).to(dtype))
    call = lambda t: QueryPrepFunction.apply(t["sample"], t["weight"], t["bias"], 1e-6, t["pos"])
    family(monkeypatch, differentiated(call, ("sample", "weight", "bias", "pos")), inputs, 3)                 # q, mean, rstd
    inputs = dict(tokens=r(B, H * W, C).to(dtype), residual=r(B, C, H, W).to(dtype), up=r(B, C, H, W).to(dtype))
    family(monkeypatch, differentiated(lambda t: TokensAddFunction.apply(t["tokens"], t["residual"]), ("tokens", "residual")), inputs, 1)


@pytest.mark.parametrize("dtype", HALVES, ids=name)
def test_small_linear_writes_inside_its_output(dtype, monkeypatch):
    """mmfs_linear_small_add: 3 token rows (a partly filled tile of 4), 40 outputs, K = 72, bias and residual."""
    from mmfs_amd.functions.linear_func import small_linear
    r = rnd(17)
    inputs = dict(x=r(3, 72).to(dtype), weight=r(40, 72, scale=0.1).to(dtype), bias=r(40).to(dtype), residual=r(3, 40).to(dtype))

    def fn(x, weight, bias, residual):
        with torch.no_grad():
            y = small_linear(x, weight, bias, residual)
        torch.cuda.synchronize()
        return y
    family(monkeypatch, fn, inputs, 1)               # (the kernel's route alone allocates ``y`` here: F.linear would record nothing)


@pytest.mark.parametrize("dtype", HALVES, ids=name)
@pytest.mark.parametrize("side", [-1, 1], ids=["tile-1", "tile+1"])
def test_clip_attention_writes_inside_its_outputs(side, dtype, monkeypatch):
    from clip_attn_refs import draw
    from mmfs_amd.functions.clip_attn_func import CLIP_TILES, ClipAttentionFunction
    B, H, L = 1, 2, CLIP_TILES[1] + side                                    # one key more / less than a key tile
    q, k, v, up = draw(31 + L, L, dtype, B, H)
    call = lambda t: ClipAttentionFunction.apply(t["q"], t["k"], t["v"], H)
    family(monkeypatch, differentiated(call, ("q", "k", "v")), dict(q=q, k=k, v=v, up=up), 6)        # context, lse, dq, dk, dv, delta


@pytest.mark.parametrize("dtype", HALVES, ids=name)
@pytest.mark.parametrize("side", [-1, 1], ids=["tile-1", "tile+1"])
def test_llama_training_attention_writes_inside_its_outputs(side, dtype, monkeypatch):
    from llama_train_refs import draw
    from mmfs_amd.functions.llama_attn_func import rope_table
    from mmfs_amd.functions.llama_train_func import TRAIN_TILES, llama_attn_train
    B, H, L = 1, 2, TRAIN_TILES[1] + side
    q, k, v, up, pos = draw(11 + L, L, dtype, B, H)
    cos, sin = rope_table(128, L + 32)
    call = lambda t: llama_attn_train(t["q"], t["k"], t["v"], t["pos"], t["cos"], t["sin"], H)
    inputs = dict(q=q, k=k, v=v, up=up, pos=pos, cos=cos.float().contiguous(), sin=sin.float().contiguous())
    family(monkeypatch, differentiated(call, ("q", "k", "v")), inputs, 8)        # q_rot, k_rot, context, lse, dq, dk, dv, delta


def qk_shapes():
    """The library exports no tile tuple for this kernel: its own test file's shapes on either side of 16 queries / 32 keys."""
    from test_qk_attn_gpu import SHAPES
    return [s[:2] for s in SHAPES if s[:2] in ((15, 31), (17, 33))]


@pytest.mark.parametrize("dtype", HALVES, ids=name)
@pytest.mark.parametrize("Nq,Nk", qk_shapes())
def test_qk_norm_attention_writes_inside_its_outputs(Nq, Nk, dtype, monkeypatch):
    """The Q-Former's attention one query and one key below and above its tiles (15 x 31, 17 x 33: SHAPES of
    tests/test_qk_attn_gpu.py), per-head LayerNorm of q and k (fp32 parameters, read where they lie) and a key bias."""
    from mmfs_amd.functions import QKNormAttentionFunction
    B, H = 1, 2
    r = rnd(19)
    inputs = dict(q=r(B, Nq, H * 64).to(dtype), k=r(B, Nk, H * 64, scale=1.5, shift=0.25).to(dtype), v=r(B, Nk, H * 64).to(dtype),
                  qw=r(64, scale=0.2, shift=1.0), qb=r(64, scale=0.1), kw=r(64, scale=0.2, shift=1.0), kb=r(64, scale=0.1),
                  key_bias=r(B, Nk), up=r(B, Nq, H * 64).to(dtype))
    call = lambda t: QKNormAttentionFunction.apply(t["q"], t["k"], t["v"], t["qw"], t["qb"], t["kw"], t["kb"], 1e-6, t["key_bias"], H)
    family(monkeypatch, differentiated(call, ("q", "k", "v", "qw", "qb", "kw", "kb"), extra=1), inputs, 7)


@pytest.mark.parametrize("dtype", OP_DTYPES, ids=name)
@pytest.mark.parametrize("act", ["none", "gelu"])
def test_dwconv_writes_inside_its_outputs(act, dtype, monkeypatch):
    """Two maps, 3 x 5 and 2 x 2 (19 tokens), 8 channels -- one 16-byte vector of 16-bit storage, two of fp32."""
    from mmfs_amd.functions import DWConvTokensFunction
    B, C, maps = 2, 8, ((3, 5), (2, 2))
    r = rnd(23)
    inputs = dict(x=r(B, 19, C).to(dtype), weight=r(C, 1, 3, 3, scale=0.3).to(dtype), bias=r(C, scale=0.1).to(dtype), up=r(B, 19, C).to(dtype))
    call = lambda t: DWConvTokensFunction.apply(t["x"], t["weight"], t["bias"], maps, act)
    family(monkeypatch, differentiated(call, ("x", "weight", "bias")), inputs, 5)


@pytest.mark.parametrize("dtype", OP_DTYPES, ids=name)
@pytest.mark.parametrize("reduction", ["none", "mean"])
def test_text_loss_writes_inside_its_outputs(reduction, dtype, monkeypatch):
    """Rows of 9 classes (one more than a vector of 16-bit logits), the scored rows starting at token 2, one label ignored and
    one out of range."""
    from mmfs_amd.functions.text_loss_func import TextLossFunction
    B, L, V, first, n = 2, 5, 9, 2, 3
    r = rnd(29)
    labels = torch.tensor([[1, -100, 8], [0, 9, 4]])
    inputs = dict(logits=r(B, L, V, scale=4.0).to(dtype), labels=labels, up=r(B, n) if reduction == "none" else r(()).reshape(()))
    call = lambda t: TextLossFunction.apply(t["logits"], t["labels"], first, -100, reduction)
    family(monkeypatch, differentiated(call, ("logits",), extra=1), inputs, 3)


@pytest.mark.parametrize("dtype", OP_DTYPES, ids=name)
def test_fp8_quantiser_writes_inside_its_outputs(dtype, monkeypatch):
    """A bank of 41 rows (not a multiple of the 64 rows a lane folds) and 2 x 16 channels, two bank rows."""
    import MultiScaleDeformableAttention as MSDA
    inputs = dict(x=rnd(31)(2, 41, 2, 16).to(dtype))

    def fn(x):
        q, scale = MSDA.quantize_bank_fp8(x)
        torch.cuda.synchronize()
        return q, scale
    got, _ = family(monkeypatch, fn, inputs, 2)
    want = MSDA.quantize_bank_fp8_reference(inputs["x"])          # (on the CPU: an IEEE division, as the kernel's)
    assert_bit_equal(got[0].cpu(), want[0], "q against the rule")
    assert_bit_equal(got[1].cpu(), want[1], "scale against the rule")


def plan_tensors(dtype, seed, Lq, H, L, P, n, N=2, M=12):
    r = rnd(seed)
    g = torch.Generator().manual_seed(seed + 1)
    return dict(off_q=r(N, Lq, H * P * 2, scale=2.0).to(dtype), att_q=(torch.rand(N, Lq, H * L * P, generator=g) * 8 - 4).to(dtype),
                off_tab=r(M, H * P * 2).to(dtype), att_tab=(torch.rand(M, H * L * P, generator=g) * 8 - 4).to(dtype),
                relpos=torch.randint(1, M, (N, Lq, n), generator=g), ref=torch.rand(N, Lq, 2, generator=g),
                ratios=torch.rand(L, generator=g) * 1.5 + 0.5)


@pytest.mark.parametrize("dtype", OP_DTYPES, ids=name)
def test_plan_writes_inside_its_outputs(dtype, monkeypatch):
    """mmfs_plan_forward / _backward: 5 queries (fewer than a run of 8), 3 heads, 2 images of 2 levels, P = 4.  The two table
    gradients are float atomics into a zeroed table (csrc/mmfs_plan.hip): extents and poison, not bits."""
    from mmfs_amd.functions import MMFSPlanFunction
    Lq, H, L, P, n = 5, 3, 2, 4, 2
    t0 = plan_tensors(dtype, 37, Lq, H, L, P, n)
    r = rnd(39)
    inputs = dict(t0, shapes=torch.tensor([(3, 5), (2, 2), (7, 4), (1, 6)]), g_loc=r(2, Lq, H, n * L, P, 2).to(dtype),
                  g_attn=r(2, Lq, H, n * L, P).to(dtype), g_sink=r(2, Lq, H))
    wrt = ("off_q", "att_q", "off_tab", "att_tab")

    def fn(**t):
        t = {k: (v.detach().requires_grad_(True) if k in wrt else v) for k, v in t.items()}
        loc, attn, sink = MMFSPlanFunction.apply(t["off_q"], t["att_q"], t["off_tab"], t["att_tab"], t["relpos"], t["ref"], t["shapes"],
                                                 t["ratios"], H, L, P)
        torch.autograd.backward([loc, attn, sink], [t["g_loc"], t["g_attn"], t["g_sink"]])
        torch.cuda.synchronize()
        return [loc.detach(), attn.detach(), sink.detach()] + [t[k].grad for k in wrt]
    got, plain = family(monkeypatch, fn, inputs, 7, bit_equal=False)
    for i, what in enumerate(("loc", "attn", "sink", "d_off_q", "d_att_q")):
        assert_bit_equal(got[i], plain[i], f"plan {what} against ordinary allocations")


@pytest.mark.parametrize("dtype", OP_DTYPES, ids=name)
def test_heads_plan_writes_inside_its_outputs(dtype, monkeypatch):
    """MMFSHeadsPlanFunction (mmfs_plan_forward_heads / mmfs_plan_backward_heads): the two query heads stacked in one row of
    C = 64 columns (4 heads, 2 levels, P = 4) and the two tables likewise, read -- and their gradients written -- as column
    ranges at a row stride of C: ``d_both`` (the storage type) and ``d_tabs`` (fp32, zeroed, float atomics: extents and poison,
    not bits) between guard bands.  5 queries, 2 images."""
    from mmfs_amd.functions.mmfs_plan_func import MMFSHeadsPlanFunction
    Lq, H, L, P, n = 5, 4, 2, 4, 2
    t0 = plan_tensors(dtype, 67, Lq, H, L, P, n)
    r = rnd(69)
    inputs = dict(both=torch.cat((t0["off_q"], t0["att_q"]), -1), tabs=torch.cat((t0["off_tab"], t0["att_tab"]), -1), relpos=t0["relpos"],
                  ref=t0["ref"], ratios=t0["ratios"], shapes=torch.tensor([(3, 5), (2, 2), (7, 4), (1, 6)]),
                  g_loc=r(2, Lq, H, n * L, P, 2).to(dtype), g_attn=r(2, Lq, H, n * L, P).to(dtype), g_sink=r(2, Lq, H))

    def fn(both, tabs, relpos, ref, ratios, shapes, g_loc, g_attn, g_sink):
        both, tabs = both.detach().requires_grad_(True), tabs.detach().requires_grad_(True)
        loc, attn, sink = MMFSHeadsPlanFunction.apply(both, tabs, relpos, ref, shapes, ratios, H, L, P)
        torch.autograd.backward([loc, attn, sink], [g_loc, g_attn, g_sink])
        torch.cuda.synchronize()
        return [loc.detach(), attn.detach(), sink.detach(), both.grad, tabs.grad]
    got, plain = family(monkeypatch, fn, inputs, 5, bit_equal=False)             # loc, attn, sink, d_both, d_tabs
    for i, what in enumerate(("loc", "attn", "sink", "d_both")):
        assert_bit_equal(got[i], plain[i], f"heads plan {what} against ordinary allocations")


def front_end_walks():
    from test_front_end_gpu import SAMPLER_WALKS             # (the list of test_fused_sampler_walks_at_their_smallest, not a copy)
    return [(t, D, live) for t, D, _ in SAMPLER_WALKS for live in (0, 5)]


@pytest.mark.parametrize("dtype,D,live", front_end_walks(), ids=lambda v: name(v) if isinstance(v, torch.dtype) else str(v))
def test_fused_sampler_writes_inside_its_outputs(dtype, D, live, monkeypatch):
    """mmfs_sample_forward at the walks of tests/test_front_end_gpu.py (SAMPLER_WALKS): three queries of one head, levels 3 x 5
    and 2 x 2, P = 4, the first ``live`` of a query's 8 samples weighing something (a logit of -1e4 is a weight of exactly 0)."""
    from mmfs_amd.functions.mmfs_plan_func import mmfs_sample_forward
    monkeypatch.setenv("MMFS_SAMPLE_DECODE", "0")            # (3 queries are decode-sized: this is about mmfs_sample_fwd)
    Lq, H, L, P, n, N = 3, 1, 2, 4, 1, 2
    t0 = plan_tensors(dtype, 41, Lq, H, L, P, n)
    t0["att_q"][..., live:] = -1e4
    shapes = torch.tensor([(3, 5), (2, 2)])
    inputs = dict(t0, shapes=shapes, start=torch.tensor([0, 15]), value=torch.rand(N, 19, H, D, generator=torch.Generator().manual_seed(5)).to(dtype),
                  token=rnd(43)(H, D).to(dtype))

    def fn(value, shapes, start, off_q, att_q, off_tab, att_tab, relpos, ref, ratios, token):
        res = mmfs_sample_forward(value, shapes, start, off_q, att_q, off_tab, att_tab, relpos, ref, ratios, H, L, P, token=token)
        assert res is not None
        torch.cuda.synchronize()
        return list(res[:2])
    family(monkeypatch, fn, inputs, 2)


@pytest.mark.parametrize("dtype", OP_DTYPES, ids=name)
def test_deform_plan_and_sampler_write_inside_their_outputs(dtype, monkeypatch):
    """The ViT-Adapter's front end: 5 queries, 3 heads, levels 3 x 5 and 2 x 2, P = 4, the two heads' columns stacked in one row
    (72 columns: the ranges are read and written as they lie) -- DeformPlanFunction forward and backward, and the fused
    deform_sample_forward on the same arguments."""
    from mmfs_amd.functions import DeformPlanFunction, deform_sample_forward
    N, Lq, H, L, P, D = 2, 5, 3, 2, 4, 32
    r = rnd(47)
    g = torch.Generator().manual_seed(48)
    inputs = dict(both=r(N, Lq, H * L * P * 3).to(dtype), ref=torch.rand(N, Lq, L, 2, generator=g), shapes=torch.tensor([(3, 5), (2, 2)]),
                  g_loc=r(N, Lq, H, L, P, 2).to(dtype), g_attn=r(N, Lq, H, L, P).to(dtype))

    def plan(both, ref, shapes, g_loc, g_attn):
        both = both.detach().requires_grad_(True)
        loc, attn = DeformPlanFunction.apply(both, ref, shapes, H, L, P)
        torch.autograd.backward([loc, attn], [g_loc, g_attn])
        torch.cuda.synchronize()
        return [loc.detach(), attn.detach(), both.grad]
    family(monkeypatch, plan, inputs, 3)
    inputs = dict(both=inputs["both"], ref=inputs["ref"], shapes=inputs["shapes"], start=torch.tensor([0, 15]),
                  value=torch.rand(N, 19, H, D, generator=g).to(dtype))

    def sample(value, shapes, start, both, ref):
        out = deform_sample_forward(value, shapes, start, both, ref, H, L, P)
        assert out is not None
        torch.cuda.synchronize()
        return out
    family(monkeypatch, sample, inputs, 1)


def adapter_walks():
    from test_vit_adapter_gpu import SAMPLER_WALKS           # (the list of test_fused_sampler_walk_at_its_smallest, not a copy)
    return [(t, D, live, R) for t, D, _ in SAMPLER_WALKS for live, R in ((1, 2), (5, 4))]


@pytest.mark.parametrize("dtype,D,live,R", adapter_walks(), ids=lambda v: name(v) if isinstance(v, torch.dtype) else str(v))
def test_deform_sampler_walks_write_inside_their_output(dtype, D, live, R, monkeypatch):
    """deform_sample_forward at the walks of tests/test_vit_adapter_gpu.py (SAMPLER_WALKS): three queries of one head, levels
    3 x 5 and 2 x 2, P = 4, the first ``live`` of a query's 8 samples weighing something (the odd prologue alone; one loop
    trip), reference points of 2 and of 4 numbers."""
    from mmfs_amd.functions import deform_sample_forward
    N, Lq, H, L, P = 2, 3, 1, 2, 4
    r = rnd(71 + live)
    g = torch.Generator().manual_seed(73)
    both = r(N, Lq, H * L * P * 3)
    both[..., H * L * P * 2 + live:] = -1e4
    ref = torch.rand(N, Lq, L, R, generator=g)
    if R == 4:
        ref[..., 2:] = ref[..., 2:] * 0.5 + 0.1                 # (box width and height)
    inputs = dict(both=both.to(dtype), ref=ref, shapes=torch.tensor([(3, 5), (2, 2)]), start=torch.tensor([0, 15]),
                  value=torch.rand(N, 19, H, D, generator=g).to(dtype))

    def sample(value, shapes, start, both, ref):
        out = deform_sample_forward(value, shapes, start, both, ref, H, L, P)
        assert out is not None
        torch.cuda.synchronize()
        return out
    family(monkeypatch, sample, inputs, 1)


@pytest.mark.parametrize("dtype", OP_DTYPES, ids=name)
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_pyramid_head_writes_inside_its_outputs(layout, dtype, monkeypatch):
    """The adapter's output pyramid at H = W = 2 (levels of 64, 16, 4 and 1 tokens), 8 channels, every level, with position
    tables; c1 contiguous and channels_last -- whose gradient the wrapper allocates with that memory format
    (pyramid_func.py): reproduced inside the guarded buffer with its strides, not passed through."""
    from mmfs_amd.functions import PyramidHeadFunction, pyramid_head_supported
    B, H, W, C, mask = 2, 2, 2, 8, 15
    r = rnd(53)
    c1_shape = (B, C, 4 * H, 4 * W) if layout == "nchw" else (B, 4 * H, 4 * W, C)
    inputs = dict(c=r(B, 21 * H * W // 4, C).to(dtype), x1=r(B, H * W, C).to(dtype), x2=r(B, H * W, C).to(dtype), x3=r(B, H * W, C).to(dtype),
                  x4=r(B, H * W, C).to(dtype), adapter_up=r(B, 4 * H * W, 4 * C).to(dtype), c1=r(*c1_shape).to(dtype),
                  pos0=r(16 * H * W, C), pos1=r(4 * H * W, C), pos2=r(H * W, C), pos3=r(H * W // 4, C), up=r(B, 85 * H * W // 4, C).to(dtype))
    wrt = ("c", "x1", "x2", "x3", "x4", "adapter_up", "c1")

    def call(t):
        c1 = t["c1"] if layout == "nchw" else t["c1"].permute(0, 3, 1, 2)
        pos = [t[f"pos{l}"] for l in range(4)]
        assert pyramid_head_supported(t["c"], [t[f"x{l}"] for l in range(1, 5)], c1, pos, H, W, mask)
        return PyramidHeadFunction.apply(t["c"], t["x1"], t["x2"], t["x3"], t["x4"], t["adapter_up"], c1, pos, H, W, mask)
    family(monkeypatch, differentiated(call, wrt), inputs, 7)             # out, four gx, g_up, g_c1


@pytest.mark.parametrize("dtype", OP_DTYPES, ids=name)
def test_sequence_kernels_write_inside_their_outputs(dtype, monkeypatch):
    """The "sparse_edges" layout of tests/test_sequence.py (2 x 40 tokens; image tokens and <soi> at the first and last
    column): the index tables and mm_embeds with its three gradients, then the image decoder's context (three slots for
    two <soi>: one is padding) with the gradients of the features, the weight and the bias."""
    import types
    from mmfs_amd import sequence as seq
    from test_sequence import index_layouts
    _, ids, image_id, soi_id = [l for l in index_layouts() if l[0] == "sparse_edges"][0]
    B, L, C = ids.shape[0], ids.shape[1], 16
    n_vis = int((ids == image_id).sum())
    r = rnd(59)
    inputs = dict(text=r(B, L, C).to(dtype), vis=r(n_vis, C).to(dtype), soi=r(1, C).to(dtype), ids=ids, up=r(B, L, C).to(dtype))
    call = lambda t: seq.assemble_mm_embeds(t["text"], t["ids"], t["vis"], t["soi"], image_token_id=image_id, soi_token_id=soi_id,
                                            route="kernels")
    family(monkeypatch, differentiated(call, ("text", "vis", "soi")), inputs, 5)                     # the tables, mm_embeds, three gradients
    n_images, C_out = 3, 16
    inputs = dict(x=r(B, L, C).to(dtype), weight=r(C_out, C, scale=0.3).to(dtype), bias=r(C_out, scale=0.1).to(dtype), ids=ids,
                  up=r(n_images, L, C_out).to(dtype))

    def context(t):
        proj = types.SimpleNamespace(weight=t["weight"], bias=t["bias"])
        return seq.prepare_context_features_for_image_decoder(t["x"], t["ids"], proj, soi_token_id=soi_id, n_images=n_images, seq_len=64,
                                                              max_len=L, route="kernels")
    family(monkeypatch, differentiated(context, ("x", "weight", "bias"), extra=1), inputs, 4)        # the tables, features, mask, the gathered gradient


def llama_cache(dtype, B, H, cap, held, seed):
    r = rnd(seed)
    keys, values = r(B, H, cap, 128, scale=1.5, shift=0.25).to(dtype), r(B, H, cap, 128).to(dtype)
    keys[:, :, held:], values[:, :, held:] = 0, 0
    return dict(keys=keys, values=values, length=torch.tensor([held], dtype=torch.int32),
                src_row=torch.arange(B, dtype=torch.int32).view(B, 1).repeat(1, cap).contiguous())


@pytest.mark.parametrize("dtype", HALVES, ids=name)
@pytest.mark.parametrize("side", [-1, 1], ids=["tile-1", "tile+1"])
@pytest.mark.parametrize("step", ["prefill", "decode"])
def test_llama_cache_attention_writes_inside_its_outputs(step, side, dtype, monkeypatch):
    """llama_rope_append + llama_attn_prefill (three new tokens, causal) and llama_rope_append + llama_attn_decode (one new
    token), each with one key less and one key more than its key tile in all (the library's PREFILL_TILES[2]; WAVE_KEYS, the
    keys of a wave of the decode): the cache, written in place, between guard bands as well -- the new keys, values and rows
    land in their slots and nowhere else."""
    from mmfs_amd.functions import llama_attn_func as F
    B, H, cap = 2, 2, 256
    Lq, tile = (3, F.PREFILL_TILES[2]) if step == "prefill" else (1, F.WAVE_KEYS)
    held = tile + side - Lq                                  # (held + Lq keys are attended)
    assert 0 < held and held + Lq <= cap
    r = rnd(61)
    cos, sin = F.rope_table(128, cap + 8)
    inputs = dict(llama_cache(dtype, B, H, cap, held, 63), q=r(B, Lq, H * 128).to(dtype), k=r(B, Lq, H * 128, scale=1.5, shift=0.25).to(dtype),
                  v=r(B, Lq, H * 128).to(dtype), pos=(torch.arange(Lq) + held).view(1, Lq).repeat(B, 1), cos=cos, sin=sin)

    def fn(keys, values, length, src_row, q, k, v, pos, cos, sin):
        assert F.llama_attn_supported(q, H, cap)
        q_rot = F.llama_rope_append(q, k, v, pos, cos, sin, keys, values, length, src_row)
        if step == "prefill":
            out = F.llama_attn_prefill(q_rot, keys, values, length, src_row, causal=True)
        else:
            out = F.llama_attn_decode(q_rot, keys, values, length, src_row)
        torch.cuda.synchronize()
        return [q_rot, out, keys, values, src_row]
    got, plain, rec = run_placed(monkeypatch, fn, inputs, writes=("keys", "values", "src_row"))
    assert len(rec.records) >= 2 and rec.pass_through_count == 0
    # the slots behind the new tokens are untouched: still the zeros they were given
    assert not bool(got[2][:, :, held + Lq:].any()) and not bool(got[3][:, :, held + Lq:].any())
    assert bool(got[2][:, :, held:held + Lq].any()) and torch.equal(got[2][:, :, :held].cpu(), inputs["keys"][:, :, :held])
