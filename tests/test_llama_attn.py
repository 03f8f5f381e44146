"""The LLM's self-attention in text generation (mmfs_amd/llama_attn.py, csrc/mmfs_llama_attn.hip), host side: the fp64
statement the GPU tests compare with (tests/llama_attn_refs.py) and the module's framework route in fp64 against the
reference's fixtures (tests/golden/llama_attn_*.npz, made by tests/golden/make_golden_llama_attn.py from the reference's
LlamaAttention with its tuple cache), the cache's host logic with a host-side emulation of the append kernel, the
conditions that keep a call on the framework route, and the C ABI's declarations and argument checks (every one returns
before a launch, so they are safe without a GPU)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from helpers import load_golden
from llama_attn_refs import attend64, linear64, rope64

import mmfs_amd
from mmfs_amd.llama_attn import LlamaKVCache, LlamaKVLayer, LlamaSelfAttention

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmfs_msda.h")
NAMES = ("mmfs_llama_attn_supported", "mmfs_llama_attn_rope_append", "mmfs_llama_attn_decode_keys",
         "mmfs_llama_attn_decode_workspace_bytes", "mmfs_llama_attn_decode")
CASES = ("prefill_decode", "all_masked_row", "decode_beams")
WEIGHTS = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "o_proj.weight")
HEADS, HIDDEN, MAX_POS = 2, 256, 64
BAR = 1e-12
F64 = torch.float64


def fixture(case):
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in load_golden("llama_attn_" + case).items()}
    for k, v in g.items():
        if v.dtype in (torch.float16, torch.float32):
            g[k] = v.double()                                   # (stored narrower where that is lossless)
    return g


def calls_of(g):
    return ["prefill"] + [f"step{i}" for i in range(sum(1 for k in g if re.fullmatch(r"step\d+\.out", k)))]


def config(**more):
    return types.SimpleNamespace(hidden_size=HIDDEN, num_attention_heads=HEADS, max_position_embeddings=MAX_POS, **more)


def module_of(g, dtype=F64):
    m = LlamaSelfAttention(config())
    m.load_state_dict({k[len("param."):]: v for k, v in g.items() if k.startswith("param.")}, strict=True)
    return m.to(dtype).eval()


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def reordered(g, call, past):
    """the reference's _reorder_cache after ``call``, where the fixture has one"""
    if "beam_idx" in g and calls_of(g)[int(g["reorder_after"])] == call:
        return tuple(t.index_select(0, g["beam_idx"]) for t in past)
    return past


# ------------------------------------------------------------------ the fp64 statement of the GPU tests
@pytest.mark.parametrize("case", CASES)
def test_the_written_out_fp64_statement_matches_the_fixture(case):
    """tests/llama_attn_refs.py (rope, attention) between the fixture's Linear layers, the reference's cat as the cache"""
    g = fixture(case)
    cos, sin = mmfs_amd.rope_table(128, MAX_POS)
    assert cos.dtype == torch.float32 and cos.shape == (MAX_POS, 64)
    past = None
    for call in calls_of(g):
        h, pos = g[call + ".hidden_states"], g[call + ".position_ids"]
        q, k, v = (linear64(h, g["param." + n], F64)[0] for n in WEIGHTS[:3])
        q_rot, E = rope64(q, pos, cos, sin, HEADS, F64)
        k_rot, _ = rope64(k, pos, cos, sin, HEADS, F64)
        assert bool(torch.isfinite(E).all()) and bool((E >= 0).all())
        B, L, _ = h.shape
        k_new, v_new = (t.reshape(B, L, HEADS, 128).transpose(1, 2) for t in (k_rot, v))
        keys = k_new if past is None else torch.cat((past[0], k_new), dim=2)
        values = v_new if past is None else torch.cat((past[1], v_new), dim=2)
        assert rel(keys, g[call + ".keys"]) <= BAR and rel(values, g[call + ".values"]) <= BAR, call
        r = attend64(q_rot, keys, values, HEADS, mask=g[call + ".mask"], dtype=F64)
        out = linear64(r["context"], g["param.o_proj.weight"], F64)[0]
        assert rel(out, g[call + ".out"]) <= BAR, call
        assert bool(torch.isfinite(r["E_context"]).all()) and bool((r["E_context"] >= 0).all())
        past = reordered(g, call, (keys, values))


def test_rope_table_is_the_reference_s_cache():
    """the fixture's keys of a prompt whose positions are 0 .. 4 pin the table: k_rot / k per pair is (cos, sin)"""
    cos, sin = mmfs_amd.rope_table(128, 2048)
    inv = 1.0 / (10000 ** (torch.arange(0, 128, 2).float() / 128))
    freqs = torch.outer(torch.arange(2048, dtype=torch.float32), inv)
    assert torch.equal(cos, freqs.cos()) and torch.equal(sin, freqs.sin())
    assert cos.dtype == torch.float32 and cos.shape == (2048, 64) and cos.is_contiguous()
    c5, _ = mmfs_amd.rope_table(128, 8, base=500)
    assert c5.shape == (8, 64) and not torch.equal(c5, cos[:8])


# ------------------------------------------------------------------ the framework route against the fixtures, fp64
@pytest.mark.parametrize("case", CASES)
def test_framework_route_against_the_fixture(case):
    g = fixture(case)
    m = module_of(g)
    assert list(m.state_dict()) == list(WEIGHTS)
    past = None
    with torch.no_grad():
        for call in calls_of(g):
            out, weights, past = m(g[call + ".hidden_states"], attention_mask=g[call + ".mask"],
                                   position_ids=g[call + ".position_ids"], past_key_value=past, use_cache=True)
            assert m.last_route == "framework" and weights is None and isinstance(past, tuple) and len(past) == 2
            assert out.dtype == F64 and rel(out, g[call + ".out"]) <= BAR, call
            assert past[0].shape == g[call + ".keys"].shape and past[1].shape == g[call + ".values"].shape
            assert rel(past[0], g[call + ".keys"]) <= BAR and rel(past[1], g[call + ".values"]) <= BAR
            past = reordered(g, call, past)
        h, mask, pos = (g["prefill." + n] for n in ("hidden_states", "mask", "position_ids"))
        out, weights, present = m(h, attention_mask=mask, position_ids=pos, output_attentions=True)
        assert present is None and weights.shape == (h.shape[0], HEADS, h.shape[1], h.shape[1])
        assert rel(out, g["prefill.out"]) <= BAR
        with pytest.raises(ValueError):
            m(h, attention_mask=mask[:, :, :1], position_ids=pos)                       # the reference's size check


def test_the_fixtures_hold_what_they_are_for():
    g = fixture("prefill_decode")
    low = torch.finfo(torch.float32).min
    assert g["prefill.hidden_states"].shape == (2, 7, HIDDEN) and g["prefill.mask"].shape == (2, 1, 7, 7)
    assert g["prefill.position_ids"].tolist() == [[0, 1, 2, 3, 4, 5, 6], [1, 1, 1, 0, 1, 2, 3]]
    assert calls_of(g) == ["prefill", "step0", "step1", "step2"] and g["step2.keys"].shape == (2, HEADS, 10, 128)
    assert g["step1.mask"].shape == (2, 1, 1, 9) and float(g["step1.mask"][0].abs().max()) == 0.0
    assert (g["step1.mask"][1, 0, 0, :3] == low).all() and (g["step1.mask"][1, 0, 0, 3:] == 0).all()
    assert g["step1.position_ids"].tolist() == [[8], [5]]
    g = fixture("all_masked_row")
    assert (g["step0.mask"][1] == low).all() and float(g["step0.mask"][0].abs().max()) == 0.0
    want = g["step0.values"][1].mean(1).reshape(1, HIDDEN) @ g["param.o_proj.weight"].T
    assert float((g["step0.out"][1] - want).abs().max()) <= 1e-13
    g = fixture("decode_beams")
    assert g["beam_idx"].tolist() == [2, 2, 0] and int(g["reorder_after"]) == 1 and g["step2.keys"].shape == (3, HEADS, 8, 128)
    # after the reorder, logical rows 0 and 1 share beam 2's first six tokens and differ in the seventh
    assert torch.equal(g["step1.keys"][0, :, :6], g["step0.keys"][2]) and torch.equal(g["step1.keys"][1, :, :6], g["step0.keys"][2])
    assert not torch.equal(g["step1.keys"][0, :, 6], g["step1.keys"][1, :, 6])
    for case in CASES:                                  # inputs and parameters are exact in both 16-bit types
        g = fixture(case)
        for name, t in g.items():
            if name.startswith("param.") or name.endswith(".hidden_states"):
                assert torch.equal(t.bfloat16().double(), t) and torch.equal(t.half().double(), t), name


# ------------------------------------------------------------------ the cache on the host
def append_on_the_host(layer, k_rot, v):
    """what llama_rope_append does to the cache, in framework ops: rows [B, L, H 128] to slots length + j of physical row b"""
    cache = layer.cache
    B, L, _ = k_rot.shape
    start = int(cache.length)
    cache.reserve(layer, L)
    layer.keys[:, :, start:start + L] = k_rot.reshape(B, L, cache.heads, 128).transpose(1, 2)
    layer.values[:, :, start:start + L] = v.reshape(B, L, cache.heads, 128).transpose(1, 2)
    cache.src_row[:, start:start + L] = torch.arange(B, dtype=torch.int32)[:, None]


@pytest.mark.parametrize("case", CASES)
def test_cache_host_logic_with_a_host_side_append(case):
    g = fixture(case)
    B, cap = g["prefill.hidden_states"].shape[0], 11
    cos, sin = mmfs_amd.rope_table(128, MAX_POS)
    cache = LlamaKVCache(2, B, HEADS, cap, 128, F64, "cpu")
    cache.store.fill_(float("nan"))
    assert len(cache) == 2 and isinstance(cache[1], LlamaKVLayer) and len(cache[1]) == 2 and cache[0][0].shape == (B, HEADS, 0, 128)
    assert cache.src_row.dtype == torch.int32 and cache.src_row.tolist() == [[b] * cap for b in range(B)] and int(cache.length) == 0
    for call in calls_of(g):
        h, pos = g[call + ".hidden_states"], g[call + ".position_ids"]
        k, v = (linear64(h, g["param." + n], F64)[0] for n in WEIGHTS[1:3])
        before = cache.host_length
        for layer in cache:
            append_on_the_host(layer, rope64(k, pos, cos, sin, HEADS, F64)[0], v)
            keys, values = layer                                                # (a handle unpacks like the reference's tuple)
            assert keys.shape == g[call + ".keys"].shape and layer[0].shape[2] == before + h.shape[1]
            assert rel(keys, g[call + ".keys"]) <= BAR and rel(values, g[call + ".values"]) <= BAR, call
            if cache.identity:
                assert keys.data_ptr() == layer.keys.data_ptr()                 # a view, not a copy
        assert cache.host_length == before and int(cache.length) == before     # nothing counts before advance
        cache.advance()
        assert cache.host_length == before + h.shape[1] == int(cache.length) and cache[0].pending == 0
        assert cache[0][0].shape[2] == cache.host_length                        # what LlamaModel.forward reads as the past length
        if "beam_idx" in g and calls_of(g)[int(g["reorder_after"])] == call:
            store = cache.store.clone()
            cache.reorder(g["beam_idx"])
            assert not cache.identity and torch.equal(torch.nan_to_num(cache.store), torch.nan_to_num(store))   # rows stay put
            assert cache.src_row[:, :cache.host_length].tolist() == [[int(b)] * cache.host_length for b in g["beam_idx"]]
            assert torch.equal(cache[1][0], g[call + ".keys"].index_select(0, g["beam_idx"]))
    with pytest.raises(RuntimeError):
        cache.reserve(cache[0], cap - cache.host_length + 1)                    # past the capacity: from the mirror
    with pytest.raises(RuntimeError):
        cache.advance(cap)
    with pytest.raises(ValueError):
        cache.reorder(torch.zeros(B + 1, dtype=torch.long))
    cache.advance_host(1)
    assert cache.host_length == int(cache.length) + 1                           # (a graph replay moved the device word)
    cache.reset()
    assert cache.host_length == 0 and int(cache.length) == 0 and cache.identity and cache[0][1].shape[2] == 0
    assert cache.src_row.tolist() == [[b] * cap for b in range(B)]
    with pytest.raises(ValueError):
        LlamaKVCache(0, 1, 1, 1)


def test_a_cache_handle_on_the_framework_route_keeps_the_cache_complete():
    """fp64 on the host: the handle's views are the past, the new keys and values go INTO the cache in framework ops and
    the handle comes back, so the caller's advance() counts the token whichever route the call took"""
    g = fixture("prefill_decode")
    m = module_of(g)
    cache = LlamaKVCache(2, 2, HEADS, 16, 128, F64, "cpu")
    cache.store.fill_(float("nan"))
    with torch.no_grad():
        for call in calls_of(g):
            out, _, present = m(g[call + ".hidden_states"], attention_mask=g[call + ".mask"],
                                position_ids=g[call + ".position_ids"], past_key_value=cache[1], use_cache=True)
            assert m.last_route == "framework" and m.last_reason == "host tensors" and present is cache[1]
            assert rel(out, g[call + ".out"]) <= BAR, call
            assert rel(present[0], g[call + ".keys"]) <= BAR and rel(present[1], g[call + ".values"]) <= BAR
            cache.advance()
            assert cache.host_length == g[call + ".keys"].shape[2] == int(cache.length)
        assert torch.isnan(cache.store[0]).all()
        # use_cache=False appends nothing and hands nothing back
        h = g["step2.hidden_states"]
        mask = torch.zeros(2, 1, 1, cache.host_length + 1, dtype=F64)
        out, _, present = m(h, attention_mask=mask, position_ids=g["step2.position_ids"], past_key_value=cache[1])
        assert present is None and cache[1].pending == 0
        # a cache that cannot take the rows raises: nothing is dropped in silence
        other = LlamaKVCache(1, 2, HEADS, 16, 128, torch.float32, "cpu")
        with pytest.raises(RuntimeError):
            m(g["prefill.hidden_states"], attention_mask=g["prefill.mask"], position_ids=g["prefill.position_ids"],
              past_key_value=other[0], use_cache=True)
        full = LlamaKVCache(1, 2, HEADS, 6, 128, F64, "cpu")
        with pytest.raises(RuntimeError):                                    # 7 tokens into 6 slots
            m(g["prefill.hidden_states"], attention_mask=g["prefill.mask"], position_ids=g["prefill.position_ids"],
              past_key_value=full[0], use_cache=True)


# ------------------------------------------------------------------ what keeps a call on the framework route
def test_routing_reasons_and_forced_routes():
    g = fixture("prefill_decode")
    m = module_of(g)
    h, mask, pos = (g["step0." + n] for n in ("hidden_states", "mask", "position_ids"))
    past = (g["prefill.keys"], g["prefill.values"])
    cache = LlamaKVCache(1, 2, HEADS, 16, 128, F64, "cpu")
    q = m.q_proj(h)
    assert m._kernel_reason(h, q, mask, past, False, True) == "no LlamaKVCache handle as past_key_value"
    assert m._kernel_reason(h, q, mask, None, False, True) == "no LlamaKVCache handle as past_key_value"
    assert m._kernel_reason(h, q, mask, cache[0], False, False) == "use_cache=False"
    assert m._kernel_reason(h, q, mask, cache[0], True, True) == "output_attentions"
    assert m._kernel_reason(h, q, mask, cache[0], False, True) == "host tensors"
    with torch.no_grad():
        out, _, present = m(h, attention_mask=mask, position_ids=pos, past_key_value=past, use_cache=False)
        assert present is None and m.last_route == "framework" and rel(out, g["step0.out"]) <= BAR
        assert m(h, attention_mask=mask, past_key_value=past)[0].shape == out.shape     # position_ids default to the past length on
        m.route = "kernels"
        for kw in (dict(past_key_value=past, use_cache=True), dict(past_key_value=cache[0], use_cache=True),
                   dict(past_key_value=cache[0], use_cache=True, output_attentions=True)):
            with pytest.raises(RuntimeError):
                m(h, attention_mask=mask, position_ids=pos, **kw)
        m.route = "triton"
        with pytest.raises(ValueError):
            m(h, attention_mask=mask, position_ids=pos, past_key_value=past)
        m.route = "framework"
        assert rel(m(h, attention_mask=mask, position_ids=pos, past_key_value=past)[0], g["step0.out"]) <= BAR
    with pytest.raises(ValueError):
        LlamaSelfAttention(types.SimpleNamespace(hidden_size=100, num_attention_heads=3, max_position_embeddings=8))
    from mmfs_amd.functions import llama_attn_decode, llama_attn_supported, llama_rope_append, rope_table
    from mmfs_amd import llama_attn
    assert mmfs_amd.LlamaSelfAttention is LlamaSelfAttention and mmfs_amd.LlamaKVCache is LlamaKVCache
    assert mmfs_amd.rope_table is rope_table and mmfs_amd.llama_attn_supported is llama_attn_supported
    assert mmfs_amd.llama_rope_append is llama_rope_append and mmfs_amd.llama_attn_decode is llama_attn_decode
    assert set(llama_attn.DEFAULT_ROUTE) == {"decode", "prefill"} and set(llama_attn.DEFAULT_ROUTE.values()) <= {"kernels", "framework"}
    assert not llama_attn_supported(torch.zeros(2, 1, 256, dtype=torch.bfloat16), 2, 16)             # host tensors


# ------------------------------------------------------------------ the C ABI without a GPU
from helpers import bound_library as _lib  # noqa: E402


def test_new_symbols_are_declared_and_exported_at_abi_14():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
        assert hasattr(lib, n), n
    assert lib.mmfs_msda_abi_version() == 14
    assert int(re.search(r"#define\s+MMFS_MSDA_ABI_VERSION\s+(\d+)", raw).group(1)) == 14
    assert "mmfs_llama_attn_supported" in raw[raw.index("#define MMFS_MSDA_ABI_VERSION"):raw.index("enum mmfs_dtype")]


def test_supported_query_answers_for_each_of_dtype_head_width_queries_and_capacity():
    f = _lib().mmfs_llama_attn_supported
    for dt in (1, 2):
        for Lq, cap in ((1, 1), (1, 77), (5, 77), (77, 77), (64, 2048), (1, 1 << 22)):
            assert f(dt, 128, Lq, cap) == 1, (dt, Lq, cap)
        for D in (0, 64, 127, 129, 256):
            assert f(dt, D, 1, 77) == 0, D
        for Lq in (-1, 0, 78, 1 << 33):
            assert f(dt, 128, Lq, 77) == 0, Lq
        for cap in (-1, 0, (1 << 22) + 1, 1 << 40):
            assert f(dt, 128, 1, cap) == 0, cap
    for dt in (0, 3, 9, -1):                                                         # fp32, fp64, unknown codes
        assert f(dt, 128, 1, 77) == 0, dt


def test_workspace_query():
    lib = _lib()
    f = lib.mmfs_llama_attn_decode_workspace_bytes
    per = (4 + 128) * 4                                     # a partial: m, l, two unused words, o[128], fp32
    wave, split = lib.mmfs_llama_attn_decode_keys(0), lib.mmfs_llama_attn_decode_keys(1)
    assert 4 <= wave <= 64 and split % wave == 0 and split >= wave and lib.mmfs_llama_attn_decode_keys(2) == -2
    from mmfs_amd.functions import llama_attn_func
    assert (llama_attn_func.WAVE_KEYS, llama_attn_func.SPLIT_KEYS) == (wave, split)
    assert f(2, 3, 1) == 6 * per and f(2, 3, split) == 6 * per and f(2, 3, split + 1) == 12 * per
    assert f(4, 32, 8 * split) == 128 * 8 * per
    assert f(0, 3, 5) == 0 and f(2, 0, 5) == 0
    for bad in ((-1, 3, 5), (2, -1, 5), (2, 3, 0), (2, 3, -4), (2, 3, (1 << 22) + 1), (1 << 21, 1, 5), (1 << 13, 1 << 13, 5)):
        assert f(*bad) == -2, bad


def test_argument_errors_return_before_any_launch():
    lib = _lib()
    fake = ctypes.c_void_p(4096)                                                     # never dereferenced on these paths
    odd = ctypes.c_void_p
    DTYPE, DIMS, NULLPTR, ALIGN, UNSUPPORTED = -1, -2, -3, -4, -5

    def append(dt=2, B=2, Lq=5, H=3, D=128, cap=77, max_pos=64, **named):
        p = dict.fromkeys(("q", "k", "v", "pos", "cos", "sin"), fake)
        tail = dict.fromkeys(("length", "q_rot", "kc", "vc", "src_row"), fake)
        p.update({n: named.pop(n) for n in list(named) if n in p})
        tail.update(named)
        return lib.mmfs_llama_attn_rope_append(dt, *p.values(), max_pos, *tail.values(), B, Lq, H, D, cap, None)

    def decode(dt=2, B=2, H=3, D=128, cap=77, bound=77, bias=fake, bias_dt=0, stride=20, blen=20, **named):
        p = dict.fromkeys(("q_rot", "kc", "vc", "src_row", "length"), fake)
        tail = dict.fromkeys(("context", "workspace"), fake)
        p.update({n: named.pop(n) for n in list(named) if n in p})
        tail.update(named)
        return lib.mmfs_llama_attn_decode(dt, *p.values(), bias, bias_dt, stride, blen, *tail.values(), B, H, D, cap, bound, None)

    for f in (append, decode):
        assert f(dt=9) == DTYPE and f(dt=-1) == DTYPE
        assert f(dt=0) == UNSUPPORTED and f(dt=3) == UNSUPPORTED                       # fp32 / fp64 storage: the framework's
        assert f(B=-1) == DIMS and f(H=-1) == DIMS and f(D=-1) == DIMS and f(cap=-1) == DIMS
        assert f(B=1 << 20, H=1 << 5) == DIMS and f(B=(1 << 20) + 1) == DIMS
        assert f(D=64) == UNSUPPORTED and f(D=127) == UNSUPPORTED and f(D=256) == UNSUPPORTED
        assert f(cap=0) == UNSUPPORTED and f(cap=(1 << 22) + 1) == UNSUPPORTED
        assert f(q_rot=None) == NULLPTR and f(kc=None) == NULLPTR and f(vc=None) == NULLPTR
        assert f(src_row=None) == NULLPTR and f(length=None) == NULLPTR
        assert f(q_rot=odd(4104)) == ALIGN and f(kc=odd(4104)) == ALIGN and f(vc=odd(4098)) == ALIGN
        assert f(src_row=odd(4098)) == ALIGN and f(length=odd(4097)) == ALIGN
    assert append(Lq=-1) == DIMS and append(Lq=0) == UNSUPPORTED and append(Lq=78) == UNSUPPORTED and append(max_pos=-1) == DIMS
    assert append(q=None) == NULLPTR and append(k=None) == NULLPTR and append(v=None) == NULLPTR and append(pos=None) == NULLPTR
    assert append(cos=None) == NULLPTR and append(sin=None) == NULLPTR
    assert append(q=odd(4104)) == ALIGN and append(v=odd(4104)) == ALIGN and append(pos=odd(4100)) == ALIGN
    assert append(cos=odd(4100)) == ALIGN and append(sin=odd(4104)) == ALIGN
    assert append(B=0, q=None, k=None, v=None, pos=None, q_rot=None) == 0              # nothing to do
    assert decode(bound=0) == DIMS and decode(bound=78) == DIMS and decode(bound=-3) == DIMS
    assert decode(context=None) == NULLPTR and decode(workspace=None) == NULLPTR
    assert decode(context=odd(4104)) == ALIGN and decode(workspace=odd(4100)) == ALIGN
    # the bias: fp32 or the storage type, nothing else; rows at least bias_len apart or one row for the batch
    assert decode(bias_dt=1) == DTYPE and decode(bias_dt=3) == DTYPE and decode(bias_dt=7) == DTYPE and decode(dt=1, bias_dt=2) == DTYPE
    assert decode(bias=None, bias_dt=7, q_rot=None) == NULLPTR                         # (no bias: its type is not looked at)
    assert decode(stride=5) == DIMS and decode(stride=-20) == DIMS and decode(blen=-1) == DIMS
    assert decode(bias=odd(4098)) == ALIGN and decode(bias=odd(4097), bias_dt=2) == ALIGN
    assert decode(stride=0, q_rot=None) == NULLPTR and decode(stride=32, q_rot=None) == NULLPTR    # (both strides pass the check)
    assert decode(B=0, q_rot=None, kc=None, vc=None, context=None, workspace=None) == 0
