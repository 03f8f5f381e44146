"""The Q-Former attention with per-head q/k LayerNorm (mmfs_amd/resampler.py, csrc/mmfs_attn.hip), host side: the
framework route in fp64 against the reference's fixtures (tests/golden/qk_attn_*.npz, made by
tests/golden/make_golden_qk_attn.py from the reference's patched class), the parameter names, the conditions that keep a
call on the framework route, the fp64 statement the GPU tests compare with (tests/qk_attn_refs.py) against the same
fixtures, and the C ABI's declarations and argument checks (every one returns before a launch, so they are safe without
a GPU)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from helpers import load_golden
from qk_attn_refs import attention64

import mmfs_amd
from mmfs_amd.resampler import QKNormAttention

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmfs_msda.h")
NAMES = ("mmfs_qk_attn_supported", "mmfs_qk_attn_forward", "mmfs_qk_attn_backward")
CASES = ("self_qknorm", "cross_qknorm_masked", "cross_plain_77", "cross_one_key_left")
BAR = 1e-12


def fixture(case):
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in load_golden("qk_attn_" + case).items()}
    for k, v in g.items():
        if v.dtype == torch.float32:
            g[k] = v.double()                                   # (stored as fp32 where that is lossless)
    return g


def config(norm, **more):
    return types.SimpleNamespace(hidden_size=128, num_attention_heads=2, encoder_hidden_size=40,
                                 attention_probs_dropout_prob=0.0, layer_norm_eps=1e-12, qk_normalization=norm, **more)


def module_of(g, dtype=torch.float64, **more):
    m = QKNormAttention(config(bool(g["qk_normalization"]), **more), is_cross_attention=bool(g["is_cross_attention"]))
    m.load_state_dict({k[len("param."):]: v for k, v in g.items() if k.startswith("param.")}, strict=True)
    return m.to(dtype).eval()


def call_of(g, m, hidden, enc=None, **kw):
    if bool(g["is_cross_attention"]):
        return m(hidden, encoder_hidden_states=enc, encoder_attention_mask=g.get("mask"), **kw)
    return m(hidden, attention_mask=g.get("mask"), **kw)


def rel(a, b, scale=None):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / (b.abs().max() if scale is None else scale).clamp_min(1e-300))


def norm_scale(g):
    """d(k_norm.bias) is 0 in exact arithmetic (a constant added to every key's score leaves the softmax alone): the
    fixture holds rounding noise there, so the LayerNorm gradients are compared on the scale of the largest of the four"""
    return max(g["grad." + n].abs().max() for n in ("q_norm.weight", "q_norm.bias", "k_norm.weight", "k_norm.bias"))


def grad_scale(g, name):
    """the scale a bias gradient is compared on: the largest column sum of |gradient of its layer's output|, the sum
    it is taken from (without k_norm, d(key.bias) is 0 in exact arithmetic for the same reason, and the fixture holds
    noise there); the LayerNorm gradients: ``norm_scale``"""
    layer = name.split(".")[0]
    if layer in ("q_norm", "k_norm"):
        return norm_scale(g)
    return g["grad." + {"query": "q", "key": "k", "value": "v"}[layer]].abs().sum((0, 1)).max()     # (a bias gradient sums rows)


# ------------------------------------------------------------------ the framework route against the fixtures, fp64
@pytest.mark.parametrize("case", CASES)
def test_framework_route_against_the_fixture(case):
    g = fixture(case)
    m = module_of(g)
    hidden = g["hidden_states"].clone().requires_grad_(True)
    enc = g["encoder_hidden_states"].clone().requires_grad_(True) if "encoder_hidden_states" in g else None
    kept = {}

    def keep(tag):
        def hook(_module, _inputs, output):
            output.retain_grad()
            kept[tag] = output
        return hook

    for layer, tag in (("query", "q"), ("key", "k"), ("value", "v")):
        getattr(m, layer).register_forward_hook(keep(tag))
    out = call_of(g, m, hidden, enc)
    assert m.last_route == "framework" and len(out) == 2 and len(out[1]) == 2
    assert out[0].dtype == torch.float64 and rel(out[0], g["context"]) <= BAR
    B, H, Nk = hidden.shape[0], 2, (enc if enc is not None else hidden).shape[1]
    assert out[1][0].shape == (B, H, Nk, 64) and out[1][1].shape == (B, H, Nk, 64)
    out[0].backward(g["upstream"])
    # the fixture holds the gradients of the Linear layers' outputs, of their biases and of the LayerNorm parameters
    for tag in ("q", "k", "v"):
        assert rel(kept[tag].grad, g["grad." + tag]) <= BAR, tag
    for name, p in m.named_parameters():
        if p.dim() == 1:
            assert rel(p.grad, g["grad." + name], grad_scale(g, name)) <= BAR, name
    assert hidden.grad.shape == hidden.shape and (enc is None or enc.grad.shape == enc.shape)


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_are_the_reference_class_s(case):
    g = fixture(case)
    want = {k[len("param."):] for k in g if k.startswith("param.")}
    m = QKNormAttention(config(bool(g["qk_normalization"])), is_cross_attention=bool(g["is_cross_attention"]))
    assert set(m.state_dict()) == want
    assert ("q_norm.weight" in want) == bool(g["qk_normalization"])
    for name, p in m.named_parameters():
        assert p.shape == g["param." + name].shape, name


def test_the_fixtures_hold_what_they_are_for():
    g = fixture("cross_qknorm_masked")
    assert g["mask"].shape == (2, 1, 1, 19) and float(g["mask"][0].abs().max()) == 0.0
    assert (g["mask"][1, 0, 0, 10:] == torch.finfo(torch.float32).min).all() and (g["mask"][1, 0, 0, :10] == 0).all()
    g = fixture("cross_one_key_left")
    assert int((g["mask"][1] == 0).sum()) == 1 and float(g["mask"][1, 0, 0, 4]) == 0.0
    g = fixture("cross_plain_77")
    assert g["hidden_states"].shape == (2, 77, 128) and not bool(g["qk_normalization"])
    assert "mask" not in fixture("self_qknorm")


# ------------------------------------------------------------------ the fp64 statement of the GPU tests
@pytest.mark.parametrize("case", CASES)
def test_the_written_out_fp64_statement_matches_the_fixture(case):
    """tests/qk_attn_refs.py (forward and hand-written backward on q, k, v) through the fixture's Linear layers"""
    g = fixture(case)
    P = {k[len("param."):]: v for k, v in g.items() if k.startswith("param.")}
    hidden = g["hidden_states"]
    src = g.get("encoder_hidden_states", hidden)
    q = hidden @ P["query.weight"].T + P["query.bias"]
    k = src @ P["key.weight"].T + P["key.bias"]
    v = src @ P["value.weight"].T + P["value.bias"]
    norm = tuple(P[n] for n in ("q_norm.weight", "q_norm.bias", "k_norm.weight", "k_norm.bias")) if "q_norm.weight" in P else None
    bias = g["mask"].reshape(2, -1) if "mask" in g else None
    r = attention64(q, k, v, 2, norm=norm, eps=1e-12, bias=bias, upstream=g["upstream"], dtype=torch.float64)
    assert rel(r["context"], g["context"]) <= BAR
    for tag in ("q", "k", "v"):
        assert rel(r["d" + tag], g["grad." + tag]) <= BAR, tag
    if norm is not None:
        for i, n in enumerate(("q_norm.weight", "q_norm.bias", "k_norm.weight", "k_norm.bias")):
            assert rel(r["dparams"][i], g["grad." + n], norm_scale(g)) <= BAR, n
    for name in ("context", "lse", "dq", "dk", "dv"):                   # in fp64 the bounds are the fp32 terms alone
        assert bool((r["E_" + name] >= 0).all()) and bool(torch.isfinite(r["E_" + name]).all())


# ------------------------------------------------------------------ what keeps a call on the framework route
def test_every_listed_condition_takes_the_framework_route_with_the_reference_s_tuple():
    g = fixture("cross_qknorm_masked")
    hidden, enc = g["hidden_states"], g["encoder_hidden_states"]
    m = module_of(g)
    assert m._fused_reason(None, None, False, True) is None
    assert m._fused_reason(torch.ones(2), None, False, True) == "head_mask"
    assert m._fused_reason(None, (enc, enc), False, False) == "past_key_value"
    assert m._fused_reason(None, None, True, True) == "output_attentions"
    m.save_attention = True
    assert m._fused_reason(None, None, False, True) == "save_attention"
    m.save_attention = False
    m.dropout.p = 0.1
    assert m._fused_reason(None, None, False, True) is None                          # eval mode
    m.train()
    assert m._fused_reason(None, None, False, True) == "dropout in training mode"
    m.eval()
    m.dropout.p = 0.0
    # the mask: one bias per key or the framework route
    ok, bias = m._key_bias(g["mask"], 2, 19)
    assert ok and bias.shape == (2, 19) and torch.equal(bias, g["mask"].reshape(2, 19))
    assert m._key_bias(None, 2, 19) == (True, None)
    assert m._key_bias(g["mask"][0:1], 2, 19)[1].shape == (2, 19)                    # a mask shared by the batch
    assert not m._key_bias(g["mask"].reshape(2, 1, 19), 2, 19)[0]                    # 3-D
    assert not m._key_bias(g["mask"].expand(2, 1, 5, 19), 2, 19)[0]                  # varies per query
    assert not m._key_bias(g["mask"].expand(2, 2, 1, 19), 2, 19)[0]                  # per head
    # the tuple shapes
    out = call_of(g, m, hidden, enc, output_attentions=True)
    assert len(out) == 3 and out[1].shape == (2, 2, 5, 19) and len(out[2]) == 2
    assert rel(out[1].sum(-1), torch.ones(2, 2, 5, dtype=torch.float64)) <= 1e-12
    out = call_of(g, m, hidden, enc, head_mask=torch.tensor([1.0, 0.0], dtype=torch.float64).view(1, 2, 1, 1))
    assert len(out) == 2 and float(out[0][..., 64:].detach().abs().max()) == 0.0 and rel(out[0][..., :64], g["context"][..., :64]) <= BAR
    m.save_attention = True
    call_of(g, m, hidden.clone().requires_grad_(True), enc)
    assert m.get_attention_map().shape == (2, 2, 5, 19)
    # a cached key / value pair is prepended (self-attention)
    gs = fixture("self_qknorm")
    ms = module_of(gs)
    first = ms(gs["hidden_states"])
    again = ms(gs["hidden_states"], past_key_value=first[1])
    assert again[1][0].shape == (2, 2, 10, 64) and rel(again[0], gs["context"]) <= BAR  # (the same keys twice: the same average)


def test_relative_position_embeddings_are_the_framework_route():
    g = fixture("self_qknorm")
    cfg = config(True, position_embedding_type="relative_key_query", max_position_embeddings=8)
    m = QKNormAttention(cfg).double().eval()
    assert m._fused_reason(None, None, False, False) == "relative position embeddings"
    assert "distance_embedding.weight" in m.state_dict()
    out = m(g["hidden_states"])
    assert m.last_route == "framework" and out[0].shape == (2, 5, 128)
    cfg = config(True, position_embedding_type="relative_key", max_position_embeddings=8)
    assert QKNormAttention(cfg).double().eval()(g["hidden_states"])[0].shape == (2, 5, 128)


def test_a_forced_kernel_route_that_does_not_apply_is_an_error_and_the_names_are_exported():
    g = fixture("self_qknorm")
    m = module_of(g)
    m.route = "kernels"
    with pytest.raises(RuntimeError):
        m(g["hidden_states"])                                                        # host tensors
    with pytest.raises(RuntimeError):
        m(g["hidden_states"], output_attentions=True)
    m.route = "triton"
    with pytest.raises(ValueError):
        m(g["hidden_states"])
    with pytest.raises(ValueError):
        QKNormAttention(types.SimpleNamespace(hidden_size=100, num_attention_heads=3, attention_probs_dropout_prob=0.0,
                                              layer_norm_eps=1e-12, qk_normalization=False))
    from mmfs_amd.functions import QKNormAttentionFunction, qk_attn_supported
    assert mmfs_amd.QKNormAttention is QKNormAttention and mmfs_amd.qk_attn_supported is qk_attn_supported
    assert mmfs_amd.QKNormAttentionFunction is QKNormAttentionFunction
    x = torch.zeros(2, 5, 128, dtype=torch.bfloat16)
    assert not qk_attn_supported(x, x, x, 2)                                         # host tensors


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
    assert "mmfs_qk_attn_supported" in raw[raw.index("#define MMFS_MSDA_ABI_VERSION"):raw.index("enum mmfs_dtype")]


def test_supported_query_answers_for_each_of_dtype_head_width_queries_and_keys():
    f = _lib().mmfs_qk_attn_supported
    for dt in (1, 2):
        for Nq in (1, 15, 64, 77, 128):
            for Nk in (1, 33, 257, 2048, 8192):
                assert f(dt, 64, Nq, Nk) == 1, (dt, Nq, Nk)
        for D in (0, 32, 63, 65, 128):
            assert f(dt, D, 64, 64) == 0, D
        for Nq in (-1, 0, 129, 1 << 33):
            assert f(dt, 64, Nq, 64) == 0, Nq
        for Nk in (-1, 0, 8193, 1 << 33):
            assert f(dt, 64, 64, Nk) == 0, Nk
    for dt in (0, 3, 9, -1):                                                         # fp32, fp64, unknown codes
        assert f(dt, 64, 64, 64) == 0, dt


def test_argument_errors_return_before_any_launch():
    lib = _lib()
    fake = ctypes.c_void_p(4096)                                                     # never dereferenced on these paths
    DTYPE, DIMS, NULLPTR, ALIGN, UNSUPPORTED = -1, -2, -3, -4, -5
    NORM = ("qw", "qb", "kw", "kb")

    def fwd(dt=2, B=2, H=3, D=64, Nq=5, Nk=19, norm_dt=0, bias=fake, bias_dt=0, stride=19, **named):
        p = dict.fromkeys(("q", "k", "v") + NORM, fake)
        p.update({n: named.pop(n) for n in list(named) if n in p})
        tail = dict.fromkeys(("context", "lse", "stats"), fake)
        tail.update(named)
        return lib.mmfs_qk_attn_forward(dt, *p.values(), norm_dt, 1e-5, bias, bias_dt, stride, *tail.values(), B, H, D, Nq, Nk, None)

    def bwd(dt=2, B=2, H=3, D=64, Nq=5, Nk=19, norm_dt=0, bias=fake, bias_dt=0, stride=19, **named):
        p = dict.fromkeys(("q", "k", "v") + NORM, fake)
        p.update({n: named.pop(n) for n in list(named) if n in p})
        tail = dict.fromkeys(("context", "grad_context", "stats", "dq", "dk", "dv", "partials", "dparams"), fake)
        tail.update(named)
        return lib.mmfs_qk_attn_backward(dt, *p.values(), norm_dt, 1e-5, bias, bias_dt, stride, *tail.values(), B, H, D, Nq, Nk, None)

    for f in (fwd, bwd):
        assert f(dt=9) == DTYPE and f(dt=-1) == DTYPE
        assert f(dt=0) == UNSUPPORTED and f(dt=3) == UNSUPPORTED                       # fp32 / fp64 storage: the framework's
        assert f(B=-1) == DIMS and f(H=-1) == DIMS and f(D=-1) == DIMS and f(Nq=-1) == DIMS and f(Nk=-1) == DIMS
        assert f(B=1 << 20, H=1 << 5) == DIMS and f(B=(1 << 20) + 1) == DIMS
        assert f(D=32) == UNSUPPORTED and f(Nq=0) == UNSUPPORTED and f(Nq=129) == UNSUPPORTED
        assert f(Nk=0) == UNSUPPORTED and f(Nk=8193) == UNSUPPORTED
        assert f(q=None) == NULLPTR and f(k=None) == NULLPTR and f(v=None) == NULLPTR and f(stats=None) == NULLPTR
        assert f(context=None) == NULLPTR
        assert f(qw=None) == NULLPTR and f(kb=None) == NULLPTR and f(qw=None, qb=None, kw=None) == NULLPTR    # some, not all
        assert f(q=ctypes.c_void_p(4104)) == ALIGN and f(v=ctypes.c_void_p(4098)) == ALIGN
        assert f(bias=ctypes.c_void_p(4098)) == ALIGN and f(stats=ctypes.c_void_p(4098)) == ALIGN
        assert f(kw=ctypes.c_void_p(4098)) == ALIGN and f(kw=ctypes.c_void_p(4097), norm_dt=2) == ALIGN
        # the small tensors: fp32 or the storage type, nothing else; the bias rows Nk apart or one row for the batch
        assert f(norm_dt=1) == DTYPE and f(norm_dt=3) == DTYPE and f(bias_dt=1) == DTYPE and f(bias_dt=7) == DTYPE
        assert f(dt=1, norm_dt=2) == DTYPE and f(dt=1, bias_dt=2) == DTYPE
        assert f(bias=None, bias_dt=7, q=None) == NULLPTR                              # (no bias: its type is not looked at)
        assert f(stride=5) == DIMS and f(stride=-19) == DIMS and f(bias=ctypes.c_void_p(4097), bias_dt=2) == ALIGN
        assert f(B=0, q=None, k=None, v=None, qw=None, qb=None, kw=None, kb=None) == 0   # nothing to do
    assert fwd(lse=None) == NULLPTR and fwd(lse=ctypes.c_void_p(4098)) == ALIGN
    assert bwd(grad_context=None) == NULLPTR and bwd(dq=None) == NULLPTR and bwd(dk=None) == NULLPTR and bwd(dv=None) == NULLPTR
    assert bwd(partials=None) == NULLPTR and bwd(dparams=None) == NULLPTR
    assert bwd(dk=ctypes.c_void_p(4104)) == ALIGN and bwd(grad_context=ctypes.c_void_p(4104)) == ALIGN
    assert bwd(partials=ctypes.c_void_p(4098)) == ALIGN
