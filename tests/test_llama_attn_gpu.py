"""The LLM's self-attention at decode (csrc/mmfs_llama_attn.hip) on the device, through mmfs_amd.llama_rope_append /
llama_attn_decode, mmfs_amd.LlamaKVCache and mmfs_amd.LlamaSelfAttention.

The rotated q, the cache rows and the context are held element by element to fp64 on the stored inputs under the bounds
of the kernel file's header (tests/llama_attn_refs.py states them; tests/test_llama_attn.py pins that statement to the
reference's fixtures); the framework route's result in the storage type on the same inputs is held to the SAME bounds, so
a bound is one the reference statement itself meets.  Outputs are poisoned before the kernels run: an element nobody
wrote is NaN.  H = 3 (an odd head count catches a wrong head stride), B = 2; the cache's capacity is no multiple of any
tile size.

Worst bound ratios measured on an MI355X are kept in profiles/llama_attn.md."""
import types

import numpy as np
import pytest
import torch

from attn_score_families import CACHE_FAMILIES, decode_case
from front_end_refs import worst
from helpers import load_golden, poison_allocations
from llama_attn_refs import attend64, linear64, rope64
from llama_train_refs import row_error

import mmfs_amd
from mmfs_amd.llama_attn import LlamaKVCache, LlamaSelfAttention, rotate_half

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.bfloat16, torch.float16]
B, H, MAX_POS = 2, 3, 96
from mmfs_amd.functions.llama_attn_func import SPLIT_KEYS, WAVE_KEYS  # noqa: E402  (the library's own: keys of a wave; of a
#                                                                       workgroup, which is a split -- a retuned kernel moves the cases)
# 1, 2, one below / at / one above the keys of a wave and of a workgroup (= split); 513 leaves the third split one key
KV_LENS = [1, 2, WAVE_KEYS - 1, WAVE_KEYS, WAVE_KEYS + 1, SPLIT_KEYS - 1, SPLIT_KEYS, SPLIT_KEYS + 1, 2 * SPLIT_KEYS + 1]
ids = dict(ids=lambda d: str(d).split(".")[1])


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


def hold(tag, name, got, ref, bound, report):
    w = worst(got.detach().cpu(), ref, bound)
    report.append((f"{tag} {name}", w[0]))
    assert w[0] <= 1.0, (f"{tag} {name}: |got - ref| / bound = {w[0]:.3g} at {w[1]}: got {w[2]!r}, ref {w[3]!r}, bound {w[4]:.3g}")


def show(report):
    by_kind = {}
    for what, ratio in report:
        by_kind[what] = max(by_kind.get(what, 0.0), ratio)
    print("worst |got - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(by_kind.items())))


def filled_cache(gen, batch, heads, cap, n, dtype, layers=1):
    """a cache whose first ``n`` slots hold random rows; everything behind them is NaN"""
    cache = LlamaKVCache(layers, batch, heads, cap, 128, dtype, DEV)
    cache.store.fill_(float("nan"))
    cache.store[:, 0, :, :, :n] = (torch.randn(layers, batch, heads, n, 128, generator=gen) * 1.5 + 0.25).to(DEV, dtype)
    cache.store[:, 1, :, :, :n] = torch.randn(layers, batch, heads, n, 128, generator=gen).to(DEV, dtype)
    cache.set_length(n)
    return cache


def draw_tokens(gen, batch, Lq, heads, dtype):
    q = torch.randn(batch, Lq, heads * 128, generator=gen).to(DEV, dtype)
    k = (torch.randn(batch, Lq, heads * 128, generator=gen) * 1.5 + 0.25).to(DEV, dtype)
    v = torch.randn(batch, Lq, heads * 128, generator=gen).to(DEV, dtype)
    return q, k, v


def framework_rope(x, pos, cos, sin, heads):
    """the reference's apply_rotary_pos_emb in T (the table rounded to T, two products and a sum in T)"""
    Bx, L, _ = x.shape
    xh = x.view(Bx, L, heads, 128)
    c = torch.cat((cos, cos), -1).to(x.dtype)[pos][:, :, None, :]
    s = torch.cat((sin, sin), -1).to(x.dtype)[pos][:, :, None, :]
    return ((xh * c) + (rotate_half(xh) * s)).reshape(Bx, L, heads * 128)


# ------------------------------------------------------------------ append
@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("Lq", [1, 5, 64])
@pytest.mark.parametrize("start", ["0", "3", "cap-Lq"])
def test_append_holds_the_rope_bound_and_touches_nothing_else(start, Lq, dtype, monkeypatch):
    cap = 77
    length = {"0": 0, "3": 3, "cap-Lq": cap - Lq}[start]
    gen = torch.Generator().manual_seed(100 * Lq + length)
    cos, sin = tables()
    cache = LlamaKVCache(1, B, H, cap, 128, dtype, DEV)
    cache.store.copy_(torch.randn(cache.store.shape, generator=gen).to(DEV, dtype))
    cache.src_row.fill_(-7)
    cache.set_length(length)
    before, rows_before = cache.store.clone(), cache.src_row.clone()
    q, k, v = draw_tokens(gen, B, Lq, H, dtype)
    pos = torch.randint(0, MAX_POS, (B, Lq), generator=gen)
    pos[0, 0], pos[-1, -1] = 0, MAX_POS - 1
    pos = pos.to(DEV)
    poison_allocations(monkeypatch)
    q_rot = mmfs_amd.llama_rope_append(q, k, v, pos, cos, sin, cache[0].keys, cache[0].values, cache.length, cache.src_row)
    report = []
    want_q, E_q = rope64(q, pos, cos, sin, H, dtype)
    want_k, E_k = rope64(k, pos, cos, sin, H, dtype)
    assert q_rot.shape == q.shape and q_rot.dtype == dtype
    hold("kernels", "q_rot", q_rot, want_q, E_q, report)
    hold("framework", "q_rot", framework_rope(q, pos, cos, sin, H), want_q, E_q, report)
    new_k = cache[0].keys[:, :, length:length + Lq].transpose(1, 2).reshape(B, Lq, H * 128)
    hold("kernels", "keys", new_k, want_k, E_k, report)
    hold("framework", "keys", framework_rope(k, pos, cos, sin, H), want_k, E_k, report)
    assert torch.equal(cache[0].values[:, :, length:length + Lq].transpose(1, 2).reshape(B, Lq, H * 128), v)
    assert cache.src_row[:, length:length + Lq].tolist() == [[b] * Lq for b in range(B)]
    # every other slot, every other src_row entry and the length word: bit-untouched
    outside = torch.ones(cap, dtype=torch.bool, device=DEV)
    outside[length:length + Lq] = False
    assert torch.equal(cache.store[..., outside, :].view(torch.int16), before[..., outside, :].view(torch.int16))
    assert torch.equal(cache.src_row[:, outside], rows_before[:, outside]) and int(cache.length) == length
    show(report)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_a_position_outside_the_table_is_nan_in_that_token_s_q_and_k_alone(dtype, monkeypatch):
    gen = torch.Generator().manual_seed(11)
    cos, sin = tables()
    cache = filled_cache(gen, B, H, 21, 4, dtype)
    q, k, v = draw_tokens(gen, B, 5, H, dtype)
    pos = torch.tensor([[0, 1, MAX_POS, 3, 4], [5, -1, 7, 8, 1 << 40]], device=DEV)
    poison_allocations(monkeypatch)
    q_rot = mmfs_amd.llama_rope_append(q, k, v, pos, cos, sin, cache[0].keys, cache[0].values, cache.length, cache.src_row)
    bad = ((pos < 0) | (pos >= MAX_POS))
    new_k = cache[0].keys[:, :, 4:9].transpose(1, 2)                       # [B, 5, H, 128]
    assert torch.equal(torch.isnan(q_rot), bad[:, :, None].expand_as(q_rot))
    assert torch.equal(torch.isnan(new_k), bad[:, :, None, None].expand_as(new_k))
    assert torch.equal(cache[0].values[:, :, 4:9].transpose(1, 2).reshape(B, 5, H * 128), v)
    want, E = rope64(q, pos, cos, sin, H, dtype)
    keep = ~bad.cpu()[:, :, None].expand_as(want)
    report = []
    hold("kernels", "q_rot", torch.where(keep, q_rot.cpu().double(), 0.0), torch.where(keep, want, 0.0), torch.where(keep, E, 1.0), report)


# ------------------------------------------------------------------ decode
def decode_both_routes(cache, q, k, v, pos, mask, report, tag=""):
    """one step on layer 0 of ``cache`` (append + decode; the cache does not advance): the kernels and the framework's
    statement in T on the same stored q_rot, keys and values, both against fp64 under the bounds -> (context, r)"""
    cos, sin = tables()
    layer, dtype = cache[0], q.dtype
    heads = cache.heads
    q_rot = mmfs_amd.llama_rope_append(q, k, v, pos, cos, sin, layer.keys, layer.values, cache.length, cache.src_row)
    bias = None if mask is None else mask.reshape(mask.shape[0], mask.shape[3])
    ctx = mmfs_amd.llama_attn_decode(q_rot, layer.keys, layer.values, cache.length, cache.src_row, bias, cache.host_length + 1)
    layer.pending = 1
    keys, values = layer[0], layer[1]
    layer.pending = 0
    assert ctx.shape == q.shape and ctx.dtype == dtype and keys.shape[2] == cache.host_length + 1
    r = attend64(q_rot, keys, values, heads, mask=mask, dtype=dtype)
    hold("kernels", "context" + tag, ctx, r["context"], r["E_context"], report)
    m = module(heads, dtype)
    full = None if mask is None else mask.to(dtype).expand(q.shape[0], 1, 1, -1)
    fw = m._attend(q_rot.view(q.shape[0], 1, heads, 128).transpose(1, 2), keys, values, full, False)[0]
    hold("framework", "context" + tag, fw, r["context"], r["E_context"], report)
    return ctx, r


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("kv", KV_LENS)
def test_decode_holds_the_bounds_at_every_key_count(kv, dtype, monkeypatch):
    """no bias; a bias per row in T (row 1 with a left-padded prefix of masked keys); one shared row in fp32"""
    gen = torch.Generator().manual_seed(7 * kv)
    cache = filled_cache(gen, B, H, kv + 3, kv - 1, dtype)
    low = torch.finfo(dtype).min
    rows = (torch.randn(B, 1, 1, kv, generator=gen) * 2).to(dtype)
    rows[1, ..., :min(3, kv - 1)] = low
    shared = (torch.randn(1, 1, 1, kv, generator=gen) * 2).to(dtype).float()
    if kv > 1:
        shared[..., kv // 2] = low
    pos = torch.tensor([[kv - 1], [max(kv - 4, 0)]], device=DEV) % MAX_POS
    poison_allocations(monkeypatch)
    report = []
    for tag, mask in ((" plain", None), (" rows", rows.to(DEV)), (" shared", shared.to(DEV))):
        q, k, v = draw_tokens(gen, B, 1, H, dtype)
        decode_both_routes(cache, q, k, v, pos, mask, report, tag)
    show(report)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_one_key_left_and_every_key_masked(dtype, monkeypatch):
    """row 0 keeps key 77 alone: its value row, bit for bit; row 1 masks every key: the mean of its values"""
    gen = torch.Generator().manual_seed(31)
    kv = 300
    cache = filled_cache(gen, B, H, kv + 5, kv - 1, dtype)
    mask = torch.full((B, 1, 1, kv), torch.finfo(dtype).min, dtype=dtype)
    mask[0, ..., 77] = 0
    q, k, v = draw_tokens(gen, B, 1, H, dtype)
    poison_allocations(monkeypatch)
    report = []
    ctx, r = decode_both_routes(cache, q, k, v, torch.tensor([[5], [9]], device=DEV), mask.to(DEV), report)
    values = cache.store[0, 1, :, :, :kv]                                   # [B, H, kv, 128]
    assert torch.equal(ctx[0, 0], values[0, :, 77].reshape(-1))
    want = values[1].double().mean(1).reshape(-1).cpu()
    assert float((r["context"][1, 0] - want).abs().max()) <= 1e-12
    assert bool(((ctx[1, 0].double().cpu() - want).abs() <= r["E_context"][1, 0]).all())
    show(report)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_a_row_of_minus_infinity_is_nan_as_the_framework_s(dtype, monkeypatch):
    gen = torch.Generator().manual_seed(32)
    kv = 70
    cache = filled_cache(gen, B, H, kv + 5, kv - 1, dtype)
    mask = torch.zeros(B, 1, 1, kv, dtype=dtype)
    mask[0] = -float("inf")
    mask[1, ..., :64] = -float("inf")                                       # a whole first wave: must not poison the merge
    q, k, v = draw_tokens(gen, B, 1, H, dtype)
    cos, sin = tables()
    poison_allocations(monkeypatch)
    q_rot = mmfs_amd.llama_rope_append(q, k, v, torch.tensor([[5], [9]], device=DEV), cos, sin, cache[0].keys, cache[0].values,
                                       cache.length, cache.src_row)
    ctx = mmfs_amd.llama_attn_decode(q_rot, cache[0].keys, cache[0].values, cache.length, cache.src_row, mask.reshape(B, kv).to(DEV))
    assert bool(torch.isnan(ctx[0]).all()) and not bool(torch.isnan(ctx[1]).any())
    keys, values = cache.store[0, 0, 1:, :, :kv], cache.store[0, 1, 1:, :, :kv]
    r = attend64(q_rot[1:], keys, values, H, mask=mask[1:], dtype=dtype)
    hold("kernels", "context", ctx[1:], r["context"], r["E_context"], [])


# ------------------------------------------------------------------ peaked, drifting and sink rows
@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("name", CACHE_FAMILIES, ids=lambda n: n.replace(" ", "_"))
def test_decode_holds_the_bounds_and_the_row_measure_at_partial_maxima_far_apart(name, dtype, monkeypatch):
    """kv = 2 SPLIT_KEYS + 1 at position 0 (tests/attn_score_families.py): the waves' and the splits' partial maxima lie up to 45
    apart (``rising``, ``falling``), or one key of the first and of the middle split holds the weight (``sink``); then plain
    unit-normal keys under an fp32 bias that rises by 0.25 a key.  Beside the per-element bounds, which admit half of p at
    |s| = 40 in bf16, the kernel's context is held row by row to 8 u of the row's norm (llama_train_refs.row_error;
    tests/test_attn_families.py: a host model of the kernel's roundings measures 0.06, partials merged without exp(m_j - M) 24
    or more)."""
    poison_allocations(monkeypatch)
    report, rows = [], {}
    for tag, case in ((" " + name, decode_case(name, dtype, SPLIT_KEYS)), (" rising bias", decode_case("bias", dtype, SPLIT_KEYS))):
        keys, values = case["keys"], case["values"]
        kv = keys.shape[2]
        assert kv == 2 * SPLIT_KEYS + 1 and keys.shape[:2] == (B, H)
        cache = LlamaKVCache(1, B, H, kv + 3, 128, dtype, DEV)
        cache.store.fill_(float("nan"))
        cache.store[0, 0, :, :, :kv - 1] = keys[:, :, :kv - 1].to(DEV)
        cache.store[0, 1, :, :, :kv - 1] = values[:, :, :kv - 1].to(DEV)
        cache.set_length(kv - 1)
        pos = torch.zeros(B, 1, dtype=torch.long, device=DEV)
        mask = None if case["bias"] is None else case["bias"].to(DEV)
        ctx, r = decode_both_routes(cache, case["q"].to(DEV), case["k"].to(DEV), case["v"].to(DEV), pos, mask, report, tag)
        # position 0 rotates nothing: the cache holds the host's rows, bit for bit
        assert torch.equal(cache.store[0, 0, :, :, :kv].cpu(), keys) and torch.equal(cache.store[0, 1, :, :, :kv].cpu(), values)
        rows[tag] = row_error(ctx, r["context"], dtype)
    show(report)
    print("worst row error / (8 u (|row| + floor)), kernels:" + ",".join(f"{t} {x:.3f}" for t, x in rows.items()))
    assert max(rows.values()) <= 1.0, rows


# ------------------------------------------------------------------ the reference's fixtures through the module
def mask_in(dtype, mask):
    """HF writes finfo(T).min where the fixture has finfo(float32).min (or their sum: the clamp brings it back)"""
    return torch.where(mask < 0, torch.finfo(dtype).min, 0.0).to(DEV, dtype)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("case", ["prefill_decode", "all_masked_row", "decode_beams"])
def test_goldens_end_to_end_through_the_module(case, dtype, monkeypatch):
    """The fixture's inputs and parameters are exact in T.  Every call's output, and the returned handle's keys and values,
    against the reference's fp64 tensors, under the header's bounds with what the Linear layers and the rope round
    carried along (llama_attn_refs: E_q, E_k, E_v).  Query rows at padded positions are left out: all their keys are
    masked, once or twice, and the two finfo.min levels of the fp64 fixture are one level in T."""
    g = {n: torch.from_numpy(np.asarray(a)) for n, a in load_golden("llama_attn_" + case).items()}
    W = {n[len("param."):]: a.double() for n, a in g.items() if n.startswith("param.")}
    calls = ["prefill"] + [f"step{i}" for i in range(sum(1 for n in g if n.startswith("step") and n.endswith(".out")))]
    batch = g["prefill.hidden_states"].shape[0]
    m = module(2, dtype, max_pos=64)
    m.load_state_dict({n: a.to(dtype) for n, a in W.items()}, strict=True)
    cos, sin = mmfs_amd.rope_table(128, 64)
    cache = LlamaKVCache(2, batch, 2, 13, 128, dtype, DEV)
    cache.store.fill_(float("nan"))
    poison_allocations(monkeypatch)
    report, E_K, E_V = [], None, None
    before = dict(func().launches)
    for i, call in enumerate(calls):
        h64, mask64, pos = g[call + ".hidden_states"].double(), g[call + ".mask"], g[call + ".position_ids"]
        mask = mask_in(dtype, mask64)
        with torch.no_grad():
            out, weights, present = m(h64.to(DEV, dtype), attention_mask=mask, position_ids=pos.to(DEV), past_key_value=cache[1],
                                      use_cache=True)
        assert m.last_route == "kernels" and weights is None and present is cache[1]
        # the fp64 chain with its bounds
        (q64, E_q0), (k64, E_k0), (v64, E_v0) = (linear64(h64, W[n + "_proj.weight"], dtype) for n in "qkv")
        q_rot, E_q = rope64(q64, pos, cos, sin, 2, dtype, E_x=E_q0)
        _, E_k = rope64(k64, pos, cos, sin, 2, dtype, E_x=E_k0)
        L = h64.shape[1]
        E_k, E_v = (t.reshape(batch, L, 2, 128).transpose(1, 2) for t in (E_k, E_v0))
        E_K = E_k if E_K is None else torch.cat((E_K, E_k), dim=2)
        E_V = E_v if E_V is None else torch.cat((E_V, E_v), dim=2)
        keys64, values64 = g[call + ".keys"], g[call + ".values"]
        hold("kernels", "keys", present[0], keys64, E_K, report)
        hold("kernels", "values", present[1], values64, E_V, report)
        r = attend64(q_rot, keys64, values64, 2, mask=mask.cpu().double(), dtype=dtype, E_q=E_q, E_k=E_K, E_v=E_V)
        want, E_out = linear64(r["context"], W["o_proj.weight"], dtype, E_x=r["E_context"])
        padded = torch.zeros(batch, L, 1, dtype=torch.bool)
        if L > 1:                                                           # the prompt: a query whose own key is masked
            padded = (mask64.diagonal(offset=mask64.shape[3] - L, dim1=2, dim2=3) < 0).reshape(batch, L, 1)
        assert float(((want - g[call + ".out"]).abs() * ~padded).max()) <= 1e-12 * float(g[call + ".out"].abs().max())
        got = torch.where(padded, want, out.cpu().double())
        hold("kernels", "out", got, want, E_out, report)
        cache.advance()
        assert present[0].shape[2] == cache.host_length == keys64.shape[2]
        if "beam_idx" in g and int(g["reorder_after"]) == i:
            cache.reorder(g["beam_idx"].to(DEV))
            E_K, E_V = E_K.index_select(0, g["beam_idx"]), E_V.index_select(0, g["beam_idx"])
    steps = len(calls) - 1
    assert func().launches["append"] - before["append"] == len(calls) and func().launches["decode"] - before["decode"] == 2 * steps
    assert torch.isnan(cache.store[0]).all()                               # layer 0 was nobody's
    show(report)


# ------------------------------------------------------------------ reproducibility, graphs, indirection
def three_steps(gen, dtype, kv0, cap):
    cache = filled_cache(gen, B, H, cap, kv0, dtype)
    steps = [draw_tokens(gen, B, 1, H, dtype) + (torch.tensor([[(kv0 + i) % MAX_POS], [(kv0 + i + 7) % MAX_POS]], device=DEV),)
             for i in range(3)]
    bias = torch.zeros(B, cap, device=DEV)
    bias[:, :kv0 + 3] = (torch.randn(B, kv0 + 3, generator=gen) * 2).to(DEV)
    bias[1, :3] = torch.finfo(dtype).min
    return cache, steps, bias, cache.store.clone()


def one_step(cache, q, k, v, pos, bias, bound):
    cos, sin = tables()
    q_rot = mmfs_amd.llama_rope_append(q, k, v, pos, cos, sin, cache[0].keys, cache[0].values, cache.length, cache.src_row)
    ctx = mmfs_amd.llama_attn_decode(q_rot, cache[0].keys, cache[0].values, cache.length, cache.src_row, bias, bound)
    cache.advance(1)
    return ctx


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_two_eager_runs_and_a_replayed_graph_agree_bit_for_bit(dtype, monkeypatch):
    """three steps from SPLIT_KEYS - 2 keys: the live keys cross a workgroup's range.  The graph (append + decode + advance)
    is captured at 254 with the grid cut for the whole capacity and replayed at 254, 255, 256 on static inputs; the
    eager steps cut their grids from the mirror.  The bits are the same."""
    kv0, cap = SPLIT_KEYS - 2, 2 * SPLIT_KEYS + 89
    gen = torch.Generator().manual_seed(41)
    cache, steps, bias, store0 = three_steps(gen, dtype, kv0, cap)
    tables()
    poison_allocations(monkeypatch)

    def rewind():
        cache.store.copy_(store0)
        cache.set_length(kv0)

    runs = []
    for _ in range(2):
        rewind()
        runs.append(([one_step(cache, *s, bias, cache.host_length + 1).clone() for s in steps], cache.store.clone()))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert torch.equal(runs[0][1].view(torch.int16), runs[1][1].view(torch.int16))
    # the graph
    static = [t.clone() for t in steps[0]]
    rewind()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one_step(cache, *static, bias, cap)
    torch.cuda.current_stream().wait_stream(side)
    rewind()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = one_step(cache, *static, bias, cap)
    cache.set_length(kv0)                                                   # (the capture moved the mirror, not the device word)
    for i, s in enumerate(steps):
        for dst, src in zip(static, s):
            dst.copy_(src)
        out.fill_(float("nan"))
        graph.replay()
        cache.advance_host(1)
        torch.cuda.synchronize()
        assert torch.equal(out, runs[0][0][i]), i
    assert int(cache.length) == kv0 + 3 == cache.host_length
    assert torch.equal(cache.store.view(torch.int16), runs[0][1].view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_after_a_reorder_decode_reads_the_rows_an_index_select_would_copy(dtype, monkeypatch):
    gen = torch.Generator().manual_seed(51)
    batch, kv0, cap = 3, 70, 333
    cache = filled_cache(gen, batch, H, cap, kv0, dtype)
    beam = torch.tensor([2, 2, 0], device=DEV)
    copied = LlamaKVCache(1, batch, H, cap, 128, dtype, DEV)              # what _reorder_cache makes: the rows themselves
    copied.store.copy_(cache.store.index_select(2, beam))
    copied.set_length(kv0)
    cache.reorder(beam)
    assert not cache.identity and copied.identity
    assert torch.equal(cache[0][0], copied[0][0]) and torch.equal(cache[0][1], copied[0][1])
    poison_allocations(monkeypatch)
    report = []
    for i in range(2):
        q, k, v = draw_tokens(gen, batch, 1, H, dtype)
        pos = torch.full((batch, 1), kv0 + i, device=DEV) % MAX_POS
        mask = (torch.randn(batch, 1, 1, kv0 + i + 1, generator=gen)).to(DEV, dtype)
        a, _ = decode_both_routes(cache, q, k, v, pos, mask, report)
        b, _ = decode_both_routes(copied, q, k, v, pos, mask, [])
        assert torch.equal(a, b), i
        cache.advance(1)
        copied.advance(1)
        assert torch.equal(cache[0][0], copied[0][0])
    # a second reorder composes with the first
    beam2 = torch.tensor([1, 0, 0], device=DEV)
    copied.store.copy_(copied.store.index_select(2, beam2))
    cache.reorder(beam2)
    assert torch.equal(cache[0][0], copied[0][0]) and torch.equal(cache[0][1], copied[0][1])
    q, k, v = draw_tokens(gen, batch, 1, H, dtype)
    pos = torch.full((batch, 1), 5, device=DEV)
    assert torch.equal(decode_both_routes(cache, q, k, v, pos, None, report)[0], decode_both_routes(copied, q, k, v, pos, None, [])[0])
    show(report)


def test_the_module_takes_the_kernels_only_with_a_cache_handle_and_nothing_more_asked(monkeypatch):
    dtype = torch.bfloat16
    poison_allocations(monkeypatch)
    gen = torch.Generator().manual_seed(61)
    m = module(H, dtype)
    cache = LlamaKVCache(1, B, H, 40, 128, dtype, DEV)
    prompt = torch.randn(B, 6, H * 128, generator=gen).to(DEV, dtype)
    token = torch.randn(B, 1, H * 128, generator=gen).to(DEV, dtype)
    causal = torch.full((6, 6), torch.finfo(dtype).min, dtype=dtype, device=DEV).triu(1)[None, None].expand(B, 1, 6, 6)
    pos = torch.arange(6, device=DEV)[None].expand(B, -1)

    def took(x, **kw):
        cache.set_length(cache.host_length)                                 # (the same step again: what the last call appended is dropped)
        before = dict(func().launches)
        out = m(x, **kw)
        return m.last_route, func().launches["append"] - before["append"], func().launches["decode"] - before["decode"], out

    with torch.no_grad():
        route, a, d, out = took(prompt, attention_mask=causal, position_ids=pos, past_key_value=cache[0], use_cache=True)
        assert (route, a, d) == ("kernels", 1, 0) and out[2] is cache[0] and out[1] is None         # the prefill: append + framework ops
        cache.advance()
        assert cache.host_length == 6 == int(cache.length) and out[2][0].shape == (B, H, 6, 128)
        fw = took(prompt, attention_mask=causal, position_ids=pos, use_cache=True)
        assert fw[:3] == ("framework", 0, 0) and isinstance(fw[3][2], tuple)
        assert float((out[0].float() - fw[3][0].float()).abs().max()) <= 0.05 * float(fw[3][0].float().abs().max())
        step = dict(position_ids=torch.full((B, 1), 6, device=DEV), use_cache=True)
        zero = torch.zeros(B, 1, 1, 7, dtype=dtype, device=DEV)
        assert took(token, attention_mask=zero, past_key_value=cache[0], **step)[:3] == ("kernels", 1, 2)
        assert took(token, attention_mask=zero[:1], past_key_value=cache[0], **step)[:3] == ("kernels", 1, 2)     # a shared row
        assert took(token, past_key_value=cache[0], **step)[:3] == ("kernels", 1, 2)
        wide = torch.zeros(B, 1, 1, 40, dtype=dtype, device=DEV)                                                # up to the capacity
        assert took(token, attention_mask=wide, past_key_value=cache[0], **step)[:3] == ("kernels", 1, 2)
        assert took(token, attention_mask=wide[..., :23], past_key_value=cache[0], **step)[:3] == ("kernels", 1, 2)
        assert m._kernel_reason(token, token, torch.zeros(B, 1, 1, 41, dtype=dtype, device=DEV), cache[0], False, True) is not None
        assert took(token, attention_mask=zero, past_key_value=fw[3][2], **step)[:3] == ("framework", 0, 0)       # a tuple cache
        # a handle on the framework route: the token goes into the cache all the same and the handle comes back
        kept = took(token, attention_mask=zero, past_key_value=cache[0], **step)[3]
        row = cache.store[0, :, :, :, 6].clone()
        cache.store[0, :, :, :, 6] = float("nan")
        route, a, d, out = took(token, attention_mask=zero, past_key_value=cache[0], output_attentions=True, **step)
        assert (route, a, d) == ("framework", 0, 0) and out[2] is cache[0] and cache[0].pending == 1 and out[1].shape == (B, H, 1, 7)
        assert float((cache.store[0, :, :, :, 6].float() - row.float()).abs().max()) <= 0.05 * float(row.float().abs().max())
        assert float((out[0].float() - kept[0].float()).abs().max()) <= 0.05 * float(kept[0].float().abs().max())
        assert m._kernel_reason(token, token, zero[..., :5], cache[0], False, True) == "a mask that is not [B or 1, 1, q_len or 1, kv_len]"
        assert m._kernel_reason(token, token, zero.expand(B, 3, 1, 7), cache[0], False, True) is not None
        with torch.autocast("cuda", dtype=dtype):
            assert took(token, attention_mask=zero, past_key_value=cache[0], **step)[:3] == ("framework", 0, 0)
    assert took(token, attention_mask=zero, past_key_value=cache[0], **step)[:3] == ("framework", 0, 0)       # grad mode
    assert m.last_reason == "tensors that require grad"
    with torch.no_grad():
        m.route = "kernels"
        with pytest.raises(RuntimeError):
            m(token, attention_mask=zero, past_key_value=cache[0], output_attentions=True, **step)
        m.route = None
        cache.set_length(40)
        with pytest.raises(RuntimeError):
            m(token, past_key_value=cache[0], **step)                       # past the capacity: raised on the host


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_a_step_captured_through_the_module_replays_at_later_lengths(dtype, monkeypatch):
    """The module's own capture branch: a static mask of the capacity's width, static hidden states and positions, the
    grid cut for the capacity; forward + cache.advance() captured at SPLIT_KEYS - 2 keys and replayed three times equals
    three eager calls bit for bit.  The positions lie behind max_position_embeddings: the kernel route's table covers the
    cache's capacity, as the framework route's grows."""
    kv0, cap, max_pos = SPLIT_KEYS - 2, SPLIT_KEYS + 45, 64
    gen = torch.Generator().manual_seed(71)
    m = module(H, dtype, max_pos=max_pos)
    cache = filled_cache(gen, B, H, cap, kv0, dtype)
    store0 = cache.store.clone()
    hidden = [torch.randn(B, 1, H * 128, generator=gen).to(DEV, dtype) for _ in range(3)]
    mask = torch.zeros(B, 1, 1, cap, dtype=dtype, device=DEV)
    mask[1, ..., :3] = torch.finfo(dtype).min
    static_h, static_pos = hidden[0].clone(), torch.zeros(B, 1, dtype=torch.long, device=DEV)

    def rewind():
        cache.store.copy_(store0)
        cache.set_length(kv0)

    def step(h, pos, attention_mask):
        out = m(h, attention_mask=attention_mask, position_ids=pos, past_key_value=cache[0], use_cache=True)
        assert m.last_route == "kernels" and out[2] is cache[0]
        cache.advance()
        return out[0]

    poison_allocations(monkeypatch)
    with torch.no_grad():
        eager = []
        for i, h in enumerate(hidden):
            n = kv0 + i
            eager.append(step(h, torch.full((B, 1), n, device=DEV), mask[..., :n + 1]).clone())
        assert all(bool(torch.isfinite(t).all()) for t in eager) and m.rope(DEV)[0].shape[0] >= cap > max_pos
        fw = m._framework(m.q_proj(hidden[2]), m.k_proj(hidden[2]), m.v_proj(hidden[2]), mask[..., :kv0 + 3],
                          torch.full((B, 1), kv0 + 2, device=DEV), (cache.store[0, 0, :, :, :kv0 + 2], cache.store[0, 1, :, :, :kv0 + 2]),
                          False, False)[0]
        assert float((fw.float() - eager[2].float()).abs().max()) <= 0.05 * float(fw.float().abs().max())
        final = cache.store.clone()
        rewind()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step(static_h, static_pos, mask)
        torch.cuda.current_stream().wait_stream(side)
        rewind()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step(static_h, static_pos, mask)
        cache.set_length(kv0)                                               # (the capture moved the mirror, not the device word)
        for i, h in enumerate(hidden):
            static_h.copy_(h)
            static_pos.fill_(kv0 + i)
            out.fill_(float("nan"))
            graph.replay()
            cache.advance_host(1)
            torch.cuda.synchronize()
            assert torch.equal(out, eager[i]), i
    assert int(cache.length) == kv0 + 3 == cache.host_length
    assert torch.equal(cache.store.view(torch.int16), final.view(torch.int16))


def test_the_functions_refuse_tensors_the_kernels_would_read_out_of_bounds():
    dtype = torch.bfloat16
    gen = torch.Generator().manual_seed(81)
    cos, sin = tables()
    cache = filled_cache(gen, B, H, 20, 4, dtype)
    q, k, v = draw_tokens(gen, B, 1, H, dtype)
    pos = torch.zeros(B, 1, dtype=torch.long, device=DEV)
    keys, values = cache[0].keys, cache[0].values
    good = (q, k, v, pos, cos, sin, keys, values, cache.length, cache.src_row)

    def with_(**kw):
        names = ("q", "k", "v", "pos", "cos", "sin", "keys", "values", "length", "src_row")
        return [kw.get(n, t) for n, t in zip(names, good)]

    for bad in (dict(cos=cos[:, :32].contiguous()), dict(cos=cos.double()), dict(sin=sin.cpu()), dict(cos=cos[::2]),
                dict(keys=keys[:, :, :10]), dict(values=values.float()), dict(keys=keys[:, :2].contiguous()),
                dict(length=cache.length.long()), dict(src_row=cache.src_row[:, :10]), dict(src_row=cache.src_row.long()),
                dict(k=k[:, :, :128]), dict(q=q.float()), dict(pos=torch.zeros(3, 7, dtype=torch.long, device=DEV))):
        with pytest.raises(RuntimeError):
            mmfs_amd.llama_rope_append(*with_(**bad))
    q_rot = mmfs_amd.llama_rope_append(*good)
    for bad in (dict(keys=keys[:, :, :10]), dict(src_row=cache.src_row.long()), dict(length=cache.length.cpu())):
        args = dict(keys=keys, values=values, length=cache.length, src_row=cache.src_row)
        args.update(bad)
        with pytest.raises(RuntimeError):
            mmfs_amd.llama_attn_decode(q_rot, args["keys"], args["values"], args["length"], args["src_row"])
    with pytest.raises(RuntimeError):
        mmfs_amd.llama_attn_decode(torch.cat((q_rot, q_rot), 1), keys, values, cache.length, cache.src_row)
    with pytest.raises(RuntimeError):
        mmfs_amd.llama_attn_decode(q_rot, keys, values, cache.length, cache.src_row, torch.zeros(5, device=DEV))
    assert bool(torch.isfinite(mmfs_amd.llama_attn_decode(q_rot, keys, values, cache.length, cache.src_row)).all())
