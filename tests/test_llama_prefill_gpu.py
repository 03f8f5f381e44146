"""The LLM's self-attention over a prompt (csrc/mmfs_llama_prefill.hip) on the device, through mmfs_amd.llama_attn_prefill
and mmfs_amd.LlamaSelfAttention.

The context is held element by element to fp64 on the stored q_rot, keys and values under the bounds of
csrc/mmfs_llama_attn.hip's header with n = held + Lq (tests/llama_attn_refs.py, handed the mask clamped at finfo(T).min);
the framework's statement in T on the same inputs is held to the SAME bounds.  B = 2, H = 3 (an odd head count catches a
wrong head stride), the capacity is no multiple of any tile; cache slots at or behind n hold NaN and outputs are poisoned
before the kernel runs.  The (held, Lq) pairs sit at the edges of the kernel's tiles, read from the library.

Worst bound ratios measured on an MI355X are kept in profiles/llama_attn.md."""
import types

import pytest
import torch

from attn_score_families import CACHE_FAMILIES, prefill_case
from front_end_refs import worst
from helpers import poison_allocations
from llama_attn_refs import attend64
from llama_train_refs import row_error
from llama_prefill_refs import clamped, hf_mask, left_padded, padding_row

import mmfs_amd
from mmfs_amd.llama_attn import LlamaKVCache, LlamaSelfAttention

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.bfloat16, torch.float16]
B, H, MAX_POS = 2, 3, 512
from mmfs_amd.functions.llama_attn_func import PREFILL_TILES  # noqa: E402  (the library's own: a retuned kernel moves the cases)
W, G, K = PREFILL_TILES
CASES = [(0, 2), (0, W - 1), (0, W + 1), (3, G - 1), (0, G + 1), (K - 1, 2), (K + 1, W), (2 * K + 1, 2 * G + 1)]
# every kv above is odd or twice an odd number, and a mask with a row per query whose rows start 4 elements aligned is
# read 4 keys a lane: one case with kv = 4 * 49, its last tile 4 keys wide
CASES.append((K + 3, G + 1))
assert (K + 3 + G + 1) % 4 == 0
ids = dict(ids=lambda d: str(d).split(".")[1])
case_ids = dict(ids=lambda c: f"{c[0]}+{c[1]}")


def func():
    from mmfs_amd.functions import llama_attn_func
    return llama_attn_func


_TABLES = []


def tables():
    if not _TABLES:                                     # (made once: a graph capture must not meet the host-to-device copy)
        _TABLES.extend(mmfs_amd.rope_table(128, MAX_POS, device=DEV))
    return tuple(_TABLES)


def module(heads, dtype, max_pos=MAX_POS):
    cfg = types.SimpleNamespace(hidden_size=heads * 128, num_attention_heads=heads, max_position_embeddings=max_pos)
    return LlamaSelfAttention(cfg).to(DEV, dtype).eval()


def hold(tag, got, ref, bound, report):
    w = worst(got.detach().cpu(), ref, bound)
    report.append((tag, w[0]))
    assert w[0] <= 1.0, (f"{tag}: |got - ref| / bound = {w[0]:.3g} at {w[1]}: got {w[2]!r}, ref {w[3]!r}, bound {w[4]:.3g}")


def show(report):
    by_kind = {}
    for what, ratio in report:
        by_kind[what] = max(by_kind.get(what, 0.0), ratio)
    print("worst |got - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(by_kind.items())))


def cap_of(n):
    cap = n + 5
    return cap if cap % 8 else cap + 1                  # no multiple of any tile


def pads_of(n, held):
    return min(n - 1, max(n // 3, held) + 1)            # the first query of row 1 is a padded one


def appended(held, Lq, dtype, batch=B, seed=0):
    """a cache of ``held`` random tokens (NaN behind them) with Lq more appended by the kernel -> (cache, q_rot)"""
    gen = torch.Generator().manual_seed(1000 * held + Lq + seed)
    n = held + Lq
    cache = LlamaKVCache(1, batch, H, cap_of(n), 128, dtype, DEV)
    cache.store.fill_(float("nan"))
    cache.store[:, 0, :, :, :held] = (torch.randn(1, batch, H, held, 128, generator=gen) * 1.5 + 0.25).to(DEV, dtype)
    cache.store[:, 1, :, :, :held] = torch.randn(1, batch, H, held, 128, generator=gen).to(DEV, dtype)
    cache.set_length(held)
    q, k, v = draw_tokens(gen, batch, Lq, dtype)
    cos, sin = tables()
    pos = torch.arange(held, n, device=DEV)[None].expand(batch, -1).contiguous()
    q_rot = mmfs_amd.llama_rope_append(q, k, v, pos, cos, sin, cache[0].keys, cache[0].values, cache.length, cache.src_row)
    return cache, q_rot


def draw_tokens(gen, batch, Lq, dtype):
    q = torch.randn(batch, Lq, H * 128, generator=gen).to(DEV, dtype)
    k = (torch.randn(batch, Lq, H * 128, generator=gen) * 1.5 + 0.25).to(DEV, dtype)
    v = torch.randn(batch, Lq, H * 128, generator=gen).to(DEV, dtype)
    return q, k, v


def logical(cache, n):
    """the reference's key / value tensors [B, H, n, 128] of layer 0 with n tokens"""
    layer = cache[0]
    layer.pending = n - cache.host_length
    keys, values = layer[0], layer[1]
    layer.pending = 0
    return keys, values


def prefill(cache, q_rot, bias=None, causal=False, visit_all=None):
    layer = cache[0]
    if visit_all is None:
        return mmfs_amd.llama_attn_prefill(q_rot, layer.keys, layer.values, cache.length, cache.src_row, bias, causal)
    return func()._attn_prefill(q_rot, layer.keys, layer.values, cache.length, cache.src_row, bias, causal, visit_all)


def masks_of(held, Lq, dtype):
    """the four mask kinds -> {kind: (what the kernel is handed, causal flag, the full mask [B or 1, 1, Lq, n] or None)}"""
    n = held + Lq
    gen = torch.Generator().manual_seed(77 * n + held)
    attention = left_padded(B, n, pads_of(n, held))
    hf = hf_mask(attention, Lq, dtype)
    shared = (torch.randn(1, 1, Lq, n, generator=gen) * 2).to(dtype).float()
    return {"none": (None, False, None), "hf": (hf.to(DEV), False, hf), "fp32 shared": (shared.to(DEV), False, shared),
            "row + causal": (padding_row(attention, dtype).to(DEV), True, hf)}


_SHARED = {}


def shared_case(held, Lq, dtype):
    """per (held, Lq, T), made once and left unchanged: the appended cache, q_rot, the masks and the fp64 references"""
    key = (held, Lq, dtype)
    if key not in _SHARED:
        cache, q_rot = appended(held, Lq, dtype)
        keys, values = logical(cache, held + Lq)
        masks = masks_of(held, Lq, dtype)
        refs = {}
        for kind in ("none", "hf", "fp32 shared"):
            refs[kind] = attend64(q_rot, keys, values, H, mask=clamped(masks[kind][2], dtype), dtype=dtype)
        refs["row + causal"] = refs["hf"]
        _SHARED[key] = (cache, q_rot, masks, refs)
    return _SHARED[key]


# ------------------------------------------------------------------ bounds
@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("case", CASES, **case_ids)
def test_prefill_and_the_framework_statement_hold_the_bounds(case, dtype, monkeypatch):
    held, Lq = case
    n = held + Lq
    cache, q_rot, masks, refs = shared_case(held, Lq, dtype)
    keys, values = logical(cache, n)
    assert bool(torch.isnan(cache.store[0, :, :, :, n:]).all())             # the slots behind n are poison
    if pads_of(n, held) > held + 1:
        assert bool(torch.isinf(masks["hf"][2][1]).any())                   # HF's sum of two finfo.min
    m = module(H, dtype)
    poison_allocations(monkeypatch)
    report = []
    for kind, (bias, causal, full) in masks.items():
        r = refs[kind]
        assert bool(torch.isfinite(r["context"]).all())
        ctx = prefill(cache, q_rot, bias, causal)
        assert ctx.shape == q_rot.shape and ctx.dtype == dtype
        hold(f"kernel {kind}", ctx, r["context"], r["E_context"], report)
        if kind != "row + causal":
            fw_mask = None if full is None else full.to(DEV, dtype).expand(B, 1, Lq, n)
            fw = m._attend(q_rot.view(B, Lq, H, 128).transpose(1, 2), keys, values, fw_mask, False)[0]
            hold(f"framework {kind}", fw, r["context"], r["E_context"], report)
    show(report)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_one_new_token_agrees_with_the_decode_kernel_under_the_bounds(dtype, monkeypatch):
    held = K + 1
    cache, q_rot = appended(held, 1, dtype)
    keys, values = logical(cache, held + 1)
    gen = torch.Generator().manual_seed(5)
    bias = (torch.randn(B, 1, 1, held + 1, generator=gen) * 2).to(dtype)
    bias[1, ..., :3] = torch.finfo(dtype).min
    r = attend64(q_rot, keys, values, H, mask=bias.double(), dtype=dtype)
    poison_allocations(monkeypatch)
    report = []
    ctx = prefill(cache, q_rot, bias.to(DEV))
    dec = mmfs_amd.llama_attn_decode(q_rot, cache[0].keys, cache[0].values, cache.length, cache.src_row, bias.to(DEV).reshape(B, -1))
    hold("prefill", ctx, r["context"], r["E_context"], report)
    hold("decode", dec, r["context"], r["E_context"], report)
    show(report)


# ------------------------------------------------------------------ the causal flag, the skip rule
@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("case", CASES, **case_ids)
def test_the_causal_flag_is_the_materialised_mask_and_skipping_moves_no_bit(case, dtype, monkeypatch):
    held, Lq = case
    n = held + Lq
    cache, q_rot, masks, refs = shared_case(held, Lq, dtype)
    row, _, full = masks["row + causal"]
    poison_allocations(monkeypatch)
    flagged = prefill(cache, q_rot, row, True)
    materialised = prefill(cache, q_rot, full.to(DEV), False)
    assert torch.equal(flagged.view(torch.int16), materialised.view(torch.int16))
    # the padded query rows of row 1: the mean of all n value rows, within the bound, and finite
    pads = pads_of(n, held)
    padded = [j for j in range(Lq) if held + j < pads]
    assert padded and bool(torch.isfinite(flagged).all())
    values = logical(cache, n)[1]
    want = values[1].double().mean(1).reshape(-1).cpu()
    bound = refs["hf"]["E_context"][1, padded]
    assert float((refs["hf"]["context"][1, padded] - want).abs().max()) <= 1e-12
    assert bool(((flagged[1, padded].double().cpu() - want).abs() <= bound).all())
    # default against VISIT_ALL: the causal cases and the left-padded one
    for bias, causal in ((row, True), (row[:1] * 0, True), (None, True), (full.to(DEV), False)):
        a = prefill(cache, q_rot, bias, causal, visit_all=False)
        b = prefill(cache, q_rot, bias, causal, visit_all=True)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (causal, None if bias is None else tuple(bias.shape))
    assert torch.equal(flagged.view(torch.int16), prefill(cache, q_rot, row, True, visit_all=True).view(torch.int16))


# ------------------------------------------------------------------ peaked, drifting and sink rows
@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("name", CACHE_FAMILIES, ids=lambda n: n.replace(" ", "_"))
def test_prefill_holds_the_bounds_and_the_row_measure_at_drifting_and_sink_rows(name, dtype, monkeypatch):
    """held = K + 1, Lq = 2 G + 1, the family over the held and the appended keys, appended at position 0
    (tests/attn_score_families.py): the running maximum rises at every key tile, or later tiles underflow, or one key holds
    the weight.  No mask, and the padding row with the causal flag; skipping tiles moves no bit.  Beside the per-element
    bounds the kernel's context is held row by row to 8 u of the row's norm (llama_train_refs.row_error;
    tests/test_attn_families.py: a host model of the kernel's roundings measures 0.1)."""
    case = prefill_case(name, dtype, PREFILL_TILES)
    held, Lq = case["held"], case["Lq"]
    n = held + Lq
    assert (held, Lq) == (K + 1, 2 * G + 1)
    cache = LlamaKVCache(1, B, H, cap_of(n), 128, dtype, DEV)
    cache.store.fill_(float("nan"))
    cache.store[0, 0, :, :, :held] = case["keys"][:, :, :held].to(DEV)
    cache.store[0, 1, :, :, :held] = case["values"][:, :, :held].to(DEV)
    cache.set_length(held)
    cos, sin = tables()
    pos = torch.zeros(B, Lq, dtype=torch.long, device=DEV)
    q_rot = mmfs_amd.llama_rope_append(case["q"].to(DEV), case["k"].to(DEV), case["v"].to(DEV), pos, cos, sin, cache[0].keys,
                                       cache[0].values, cache.length, cache.src_row)
    keys, values = logical(cache, n)
    # position 0 rotates nothing: q_rot and the cache hold the host's rows, bit for bit
    assert torch.equal(q_rot.cpu(), case["q"]) and torch.equal(keys.cpu(), case["keys"]) and torch.equal(values.cpu(), case["values"])
    masks = masks_of(held, Lq, dtype)
    poison_allocations(monkeypatch)
    report, rows = [], {}
    for kind in ("none", "row + causal"):
        bias, causal, full = masks[kind]
        r = attend64(q_rot, keys, values, H, mask=clamped(full, dtype), dtype=dtype)
        ctx = prefill(cache, q_rot, bias, causal)
        hold(f"kernel {name} {kind}", ctx, r["context"], r["E_context"], report)
        rows[kind] = row_error(ctx, r["context"], dtype)
        if kind == "none":
            fw = module(H, dtype)._attend(q_rot.view(B, Lq, H, 128).transpose(1, 2), keys, values, None, False)[0]
            hold(f"framework {name} {kind}", fw, r["context"], r["E_context"], report)
        a = prefill(cache, q_rot, bias, causal, visit_all=False)
        b = prefill(cache, q_rot, bias, causal, visit_all=True)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(a.view(torch.int16), ctx.view(torch.int16)), kind
    show(report)
    print(f"worst row error / (8 u (|row| + floor)), kernel {name}: " + ", ".join(f"{t} {x:.3f}" for t, x in rows.items()))
    assert max(rows.values()) <= 1.0, rows


# ------------------------------------------------------------------ the cache is read only; indirection; graphs
@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_the_cache_its_rows_and_its_length_are_untouched(dtype, monkeypatch):
    held, Lq = K + 1, W
    cache, q_rot, masks, _ = shared_case(held, Lq, dtype)
    store, rows, length = cache.store.clone(), cache.src_row.clone(), cache.length.clone()
    poison_allocations(monkeypatch)
    for bias, causal, _ in masks.values():
        prefill(cache, q_rot, bias, causal)
    torch.cuda.synchronize()
    assert torch.equal(cache.store.view(torch.int16), store.view(torch.int16))
    assert torch.equal(cache.src_row, rows) and torch.equal(cache.length, length) and int(cache.length) == held


def fill(cache, gen, held):
    batch = cache.batch
    cache.store.fill_(float("nan"))
    cache.store[:, 0, :, :, :held] = (torch.randn(1, batch, H, held, 128, generator=gen) * 1.5 + 0.25).to(DEV, cache.dtype)
    cache.store[:, 1, :, :, :held] = torch.randn(1, batch, H, held, 128, generator=gen).to(DEV, cache.dtype)
    cache.set_length(held)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_after_a_reorder_a_chunk_reads_the_rows_an_index_select_would_copy(dtype, monkeypatch):
    gen = torch.Generator().manual_seed(51)
    batch, held, Lq = 3, K + 1, W + 1
    n = held + Lq
    cache = LlamaKVCache(1, batch, H, cap_of(n), 128, dtype, DEV)
    fill(cache, gen, held)
    beam = torch.tensor([2, 2, 0], device=DEV)
    copied = LlamaKVCache(1, batch, H, cap_of(n), 128, dtype, DEV)        # what _reorder_cache makes: the rows themselves
    copied.store.copy_(cache.store.index_select(2, beam))
    copied.set_length(held)
    cache.reorder(beam)
    assert not cache.identity and copied.identity
    q, k, v = draw_tokens(gen, batch, Lq, dtype)
    cos, sin = tables()
    pos = torch.arange(held, n, device=DEV)[None].expand(batch, -1).contiguous()
    attention = torch.ones(batch, n)
    attention[1, :held + 2] = 0
    row = padding_row(attention, dtype).to(DEV)
    poison_allocations(monkeypatch)
    out = []
    for c in (cache, copied):
        q_rot = mmfs_amd.llama_rope_append(q, k, v, pos, cos, sin, c[0].keys, c[0].values, c.length, c.src_row)
        out.append((q_rot, prefill(c, q_rot, row, True), prefill(c, q_rot, None, False)))
    for a, b in zip(*out):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    keys, values = logical(copied, n)
    assert torch.equal(logical(cache, n)[0], keys)
    r = attend64(out[0][0], keys, values, H, mask=clamped(hf_mask(attention, Lq, dtype), dtype), dtype=dtype)
    hold("kernel after a reorder", out[0][1], r["context"], r["E_context"], [])


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_two_eager_runs_and_a_replayed_graph_agree_bit_for_bit(dtype, monkeypatch):
    gen = torch.Generator().manual_seed(41)
    held, Lq = K + 1, G + 1
    n = held + Lq
    cache = LlamaKVCache(1, B, H, cap_of(n), 128, dtype, DEV)
    fill(cache, gen, held)
    store0 = cache.store.clone()
    q, k, v = draw_tokens(gen, B, Lq, dtype)
    cos, sin = tables()
    pos = torch.arange(held, n, device=DEV)[None].expand(B, -1).contiguous()
    row = padding_row(left_padded(B, n, pads_of(n, held)), dtype).to(DEV)
    poison_allocations(monkeypatch)

    def rewind():
        cache.store.copy_(store0)
        cache.set_length(held)

    def step():
        q_rot = mmfs_amd.llama_rope_append(q, k, v, pos, cos, sin, cache[0].keys, cache[0].values, cache.length, cache.src_row)
        return prefill(cache, q_rot, row, True)

    runs = []
    for _ in range(2):
        rewind()
        runs.append((step().clone(), cache.store.clone()))
    assert torch.equal(runs[0][0].view(torch.int16), runs[1][0].view(torch.int16)) and bool(torch.isfinite(runs[0][0]).all())
    assert torch.equal(runs[0][1].view(torch.int16), runs[1][1].view(torch.int16))
    rewind()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    rewind()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), runs[0][0].view(torch.int16))
    assert torch.equal(cache.store.view(torch.int16), runs[0][1].view(torch.int16)) and int(cache.length) == held


# ------------------------------------------------------------------ the module
@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_the_module_runs_a_prompt_through_the_prefill_kernel_unless_told_otherwise(dtype, monkeypatch):
    gen = torch.Generator().manual_seed(61)
    held, Lq = 3, W + 1
    n = held + Lq
    m = module(H, dtype)
    with torch.no_grad():
        m.o_proj.weight.copy_(torch.eye(H * 128))                           # the module's output IS the context, bit for bit
    cache = LlamaKVCache(1, B, H, cap_of(n), 128, dtype, DEV)
    fill(cache, gen, held)
    hidden = (torch.randn(B, Lq, H * 128, generator=gen) * 0.5).to(DEV, dtype)
    pos = torch.arange(held, n, device=DEV)[None].expand(B, -1).contiguous()
    mask = hf_mask(left_padded(B, n, pads_of(n, held)), Lq, dtype).to(DEV)
    assert bool(torch.isinf(mask).any())
    poison_allocations(monkeypatch)

    def took(**kw):
        cache.set_length(held)                                              # (the same prompt again)
        before = dict(func().launches)
        with torch.no_grad():
            out = m(hidden, attention_mask=mask, position_ids=pos, past_key_value=cache[0], use_cache=True, **kw)
        assert m.last_route == "kernels" and out[2] is cache[0] and cache[0].pending == Lq
        return out[0], tuple(func().launches[c] - before[c] for c in ("append", "prefill", "decode"))

    m.prefill_kernel = True
    kernel, counts = took()
    assert counts == (1, 1, 0) and m.last_prefill == "kernel"
    m.prefill_kernel = False
    ops, counts = took()
    assert counts == (1, 0, 0) and m.last_prefill == "framework ops"
    m.prefill_kernel = None
    from mmfs_amd import llama_attn
    _, counts = took()
    want = Lq >= llama_attn.PREFILL_KERNEL_MIN_TOKENS
    assert counts == (1, int(want), 0) and m.last_prefill == ("kernel" if want else "framework ops")
    assert bool(torch.isfinite(kernel).all()) and bool(torch.isfinite(ops).all())
    # both against fp64 on what the module stored: q_rot again from the same kernel (into a scratch cache), the cache's rows
    with torch.no_grad():
        q, k, v = m.q_proj(hidden), m.k_proj(hidden), m.v_proj(hidden)
    scratch = LlamaKVCache(1, B, H, cap_of(n), 128, dtype, DEV)
    scratch.set_length(held)
    cos, sin = m.rope(DEV, cache.cap)
    q_rot = mmfs_amd.llama_rope_append(q, k, v, pos, cos, sin, scratch[0].keys, scratch[0].values, scratch.length, scratch.src_row)
    keys, values = logical(cache, n)
    assert torch.equal(scratch[0].keys[:, :, held:n], keys[:, :, held:n])
    r = attend64(q_rot, keys, values, H, mask=clamped(mask.cpu(), dtype), dtype=dtype)
    report = []
    hold("module, kernel", kernel, r["context"], r["E_context"], report)
    hold("module, framework ops", ops, r["context"], r["E_context"], report)
    show(report)
    m.prefill_kernel = "yes"
    with pytest.raises(ValueError):
        took()


def test_the_function_refuses_tensors_the_kernel_would_read_out_of_bounds():
    dtype = torch.bfloat16
    cache, q_rot = appended(4, 5, dtype)
    keys, values = cache[0].keys, cache[0].values
    n = 9
    good = dict(keys=keys, values=values, length=cache.length, src_row=cache.src_row, bias=None)
    for bad in (dict(keys=keys[:, :, :10]), dict(values=values.float()), dict(src_row=cache.src_row.long()),
                dict(length=cache.length.cpu()), dict(bias=torch.zeros(5, device=DEV)), dict(bias=torch.zeros(B, 3, n, device=DEV)),
                dict(bias=torch.zeros(B, 2, 5, n, device=DEV)), dict(bias=torch.zeros(3, 1, n, device=DEV)),
                dict(bias=torch.zeros(B, 1, cache.cap + 1, device=DEV))):
        args = dict(good)
        args.update(bad)
        with pytest.raises(RuntimeError):
            mmfs_amd.llama_attn_prefill(q_rot, args["keys"], args["values"], args["length"], args["src_row"], args["bias"])
    # views pass as they lie: an expanded batch row, an expanded query row, rows an odd number of elements apart
    wide = torch.zeros(B, 5, n + 2, device=DEV, dtype=dtype)
    base = prefill(cache, q_rot)
    for bias in (torch.zeros(1, 1, n, device=DEV).expand(B, 5, n), wide[:, :, 1:n + 1], torch.zeros(B, 1, 5, n, device=DEV),
                 torch.zeros(B, 5, 2 * n, device=DEV)[:, :, ::2]):
        assert torch.equal(prefill(cache, q_rot, bias).view(torch.int16), base.view(torch.int16))
    # rows 4 elements aligned (4 keys a lane) against the same numbers in rows 13 apart (key by key): a group of 4 that
    # crosses the live keys (12 > n = 9), and one that crosses the end of the bias (6)
    gen = torch.Generator().manual_seed(3)
    aligned = (torch.randn(B, 5, 12, generator=gen) * 2).to(dtype)
    aligned[1, :, :2] = torch.finfo(dtype).min
    for T in (dtype, torch.float32):
        for width in (12, 6):
            a4 = aligned.to(DEV, T)[:, :, :width]
            odd = torch.zeros(B, 5, 13, device=DEV, dtype=T)[:, :, :min(width, n)]
            odd.copy_(a4[:, :, :min(width, n)])
            assert a4.stride(1) % 4 == 0 and odd.stride(1) % 4 == 1
            got, want = prefill(cache, q_rot, a4), prefill(cache, q_rot, odd)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and not torch.equal(got, base)
