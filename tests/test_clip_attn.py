"""The CLIP ViT's self-attention (csrc/mmfs_clip_attn.hip, include/mmfs_clip_attn.h, mmfs_amd.clip_attn), host side: the new
header against its signature table; the C ABI's argument checks, every one of which returns before a launch; the module's
surface, its state dict and its framework route; ``convert_clip_visual_attn``; and ``clip64``'s bounds and the tight row
measure as a yardstick at exactly the GPU tests' inputs (the framework's statement in T and a host model of the kernels'
roundings pass, four defective variants do not)."""
import ctypes
import os
import re
import types

import pytest
import torch
from torch import nn

from clip_attn_refs import FAMILIES, TIGHT_NAMES, bound_ratios, clip64, draw, family, row_error, tight_ratios
from helpers import bound_library as _lib

import mmfs_amd
from mmfs_amd import clip_attn
from mmfs_amd.clip_attn import CLIPSelfAttention, convert_clip_visual_attn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmfs_clip_attn.h")
DTYPE, DIMS, NULLPTR, ALIGN, UNSUPPORTED = -1, -2, -3, -4, -5
B_GPU, H_GPU = 2, 3                                     # tests/test_clip_attn_gpu.py's
HALVES = [torch.bfloat16, torch.float16]
ids = lambda d: str(d).split(".")[1]


# ------------------------------------------------------------------ the header, the table, the library
def header_prototypes():
    """[(name, return kind, argument kinds)] of every ``type mmfs_name(args);`` of the header, in its order (the parser of
    tests/test_capi.py)"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(HEADER).read(), flags=re.S)
    kinds = {"int": "i", "int64_t": "l", "unsigned": "u", "float": "f", "const char *": "s", "void": "v"}
    out = []
    for ret, name, args in re.findall(r"^(const char \*|\w+)\s*\b(mmfs_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        args = [" ".join(a.split()) for a in args.split(",")]
        out.append((name, kinds[ret], "".join("p" if "*" in a else kinds[a.rsplit(" ", 1)[0]] for a in args if a != "void")))
    return out


def test_the_second_table_is_the_second_header():
    import mmfs_abi
    protos = header_prototypes()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(p[0] for p in protos) == sorted(set(re.findall(r"\b(mmfs_[a-z0-9_]+)\s*\(", text)))
    table = mmfs_abi.CLIP_ATTN_SIGNATURES
    assert list(table) == [p[0] for p in protos] and len(table) == 5
    for name, ret, args in protos:
        assert table[name] == (ret, args), f"{name}: the table says {table[name]}, the header {(ret, args)}"
    assert not set(table) & set(mmfs_abi.SIGNATURES)
    assert '#include "mmfs_msda.h"' in open(HEADER).read()


def test_the_library_exports_the_entries_and_the_version_has_not_moved():
    import mmfs_abi
    lib = _lib()
    for name in mmfs_abi.CLIP_ATTN_SIGNATURES:
        assert hasattr(lib, name), name
    assert lib.mmfs_msda_abi_version() == 14

    class Without:                                      # a library from before the entries: the usual ImportError
        _name = "old.so"

        def __getattr__(self, name):
            if name.startswith("mmfs_clip_attn"):
                raise AttributeError(name)
            return types.SimpleNamespace()

    with pytest.raises(ImportError, match="mmfs_clip_attn_supported"):
        mmfs_abi.bind(Without())


def test_the_queries_are_host_only():
    lib = _lib()
    tiles = tuple(lib.mmfs_clip_attn_tiles(i) for i in range(5))
    Q, K, KB, QT, W = tiles
    assert min(tiles) > 0 and Q % W == 0 and Q % K == 0 and KB % QT == 0 and K % 16 == 0 and QT % 16 == 0
    assert lib.mmfs_clip_attn_tiles(5) == DIMS and lib.mmfs_clip_attn_tiles(-1) == DIMS
    sup = lib.mmfs_clip_attn_supported
    assert sup(2, 64, 1) == 1 and sup(1, 64, 1 << 22) == 1 and sup(2, 64, 257) == 1 and sup(1, 64, 1025) == 1
    assert sup(0, 64, 8) == 0 and sup(3, 64, 8) == 0 and sup(2, 128, 8) == 0 and sup(2, 64, 0) == 0 and sup(2, 64, (1 << 22) + 1) == 0
    ws = lib.mmfs_clip_attn_workspace_bytes
    assert ws(32, 16, 257) == 32 * 16 * 257 * 4 and ws(0, 3, 5) == 0 and ws(2, 3, 0) == 0
    assert ws(-1, 3, 5) == DIMS and ws(2, -3, 5) == DIMS and ws(2, 3, -5) == DIMS and ws(1 << 20, 1 << 5, 5) == DIMS


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: host-only checks, run where no GPU is visible")
def test_argument_errors_return_before_any_launch():
    lib = _lib()
    fake = ctypes.c_void_p(4096)                                            # never dereferenced on these paths
    odd = ctypes.c_void_p

    def fwd(dt=2, B=2, L=5, H=3, D=64, **named):
        p = dict.fromkeys(("q", "k", "v", "out", "lse"), fake)
        p.update(named)
        return lib.mmfs_clip_attn_forward(dt, *p.values(), B, L, H, D, None)

    def bwd(dt=2, B=2, L=5, H=3, D=64, ws_bytes=None, **named):
        p = dict.fromkeys(("q", "k", "v", "out", "dout", "lse", "dq", "dk", "dv", "workspace"), fake)
        p.update(named)
        have = B * H * L * 4 if ws_bytes is None else ws_bytes
        return lib.mmfs_clip_attn_backward(dt, *p.values(), have, B, L, H, D, None)

    pointers = {fwd: ("q", "k", "v", "out"), bwd: ("q", "k", "v", "out", "dout", "lse", "dq", "dk", "dv", "workspace")}
    for f, names in pointers.items():
        assert f(dt=9) == DTYPE and f(dt=-1) == DTYPE
        assert f(B=-1) == DIMS and f(H=-1) == DIMS and f(D=-1) == DIMS and f(L=-1) == DIMS
        assert f(B=1 << 20, H=1 << 5) == DIMS and f(B=(1 << 20) + 1) == DIMS
        assert f(dt=0) == UNSUPPORTED and f(dt=3) == UNSUPPORTED            # fp32 / fp64 storage: the framework's
        assert f(D=128) == UNSUPPORTED and f(D=63) == UNSUPPORTED and f(D=32) == UNSUPPORTED
        assert f(L=(1 << 22) + 1) == UNSUPPORTED
        assert f(D=128, B=0) == UNSUPPORTED                                 # (refused before it is found empty)
        # a grid of more than 2^31 - 1 workgroups is refused, never truncated: B H = 2^24, 129 query tiles
        assert f(B=1 << 12, H=1 << 12, L=128 * 128 + 1) == DIMS
        for name in names:
            assert f(**{name: None}) == NULLPTR, name
            step = 4 if name == "lse" else 16
            assert f(**{name: odd(4096 + step // 2)}) == ALIGN, name
        # empty problems: 0 without a launch, whatever the pointers
        for kw in (dict(B=0), dict(H=0), dict(L=0)):
            assert f(**kw) == 0, kw
            assert f(**kw, **{n: None for n in names}) == 0, kw
    assert fwd(lse=odd(4096 + 2)) == ALIGN                                  # lse may be NULL (a NULL one launches), not misaligned
    assert bwd(ws_bytes=2 * 3 * 5 * 4 - 1) == NULLPTR and bwd(ws_bytes=0) == NULLPTR and bwd(ws_bytes=-1) == NULLPTR


# ------------------------------------------------------------------ the module
def config(hidden=128, heads=2, dropout=0.0):
    return types.SimpleNamespace(hidden_size=hidden, num_attention_heads=heads, attention_dropout=dropout)


def hf_statement(m, h, attention_mask=None, causal_attention_mask=None):
    """independently written: Hugging Face's CLIPAttention as einsums over [B, H, L, D]"""
    B, L, _ = h.shape
    split = lambda x: x.view(B, L, m.num_heads, m.head_dim).permute(0, 2, 1, 3)
    q, k, v = split(m.q_proj(h)) * m.head_dim ** -0.5, split(m.k_proj(h)), split(m.v_proj(h))
    s = torch.einsum("bhjc,bhtc->bhjt", q, k)
    for mask in (causal_attention_mask, attention_mask):
        if mask is not None:
            s = s + mask
    p = s.softmax(-1)
    return m.out_proj(torch.einsum("bhjt,bhtc->bhjc", p, v).permute(0, 2, 1, 3).reshape(B, L, -1)), p


def test_the_surface_and_the_state_dict():
    assert mmfs_amd.CLIPSelfAttention is CLIPSelfAttention and mmfs_amd.convert_clip_visual_attn is convert_clip_visual_attn
    assert mmfs_amd.clip_attention is clip_attn.clip_attention
    assert set(clip_attn.DEFAULT_ROUTE) == {"L257", "long"} and set(clip_attn.DEFAULT_ROUTE.values()) <= {"kernels", "framework"}
    assert clip_attn.shape_class(257) == "L257" and clip_attn.shape_class(1025) == "long"
    from mmfs_amd.functions import clip_attn_func
    assert clip_attn_func.CLIP_TILES == tuple(_lib().mmfs_clip_attn_tiles(i) for i in range(5))
    assert set(clip_attn_func.launches) == {"forward", "backward"}
    for name in ("clip_attn_supported", "clip_forward", "clip_backward", "ClipAttentionFunction"):
        assert hasattr(clip_attn_func, name), name
    m = CLIPSelfAttention(config())
    assert (m.embed_dim, m.num_heads, m.head_dim, m.scale, m.dropout) == (128, 2, 64, 0.125, 0.0)
    assert (m.route, m.last_route, m.last_reason) == (None, None, None)
    assert set(m.state_dict()) == {f"{p}.{w}" for p in ("q_proj", "k_proj", "v_proj", "out_proj") for w in ("weight", "bias")}
    with pytest.raises(ValueError, match="divisible"):
        CLIPSelfAttention(config(hidden=130, heads=4))
    # a state dict in the shape of the reference's CLIPXAttention loads strictly
    torch.manual_seed(0)
    theirs = {f"{p}.{w}": torch.randn(128, 128) if w == "weight" else torch.randn(128)
              for p in ("k_proj", "v_proj", "q_proj", "out_proj") for w in ("weight", "bias")}
    m.load_state_dict(theirs, strict=True)
    assert torch.equal(m.q_proj.weight, theirs["q_proj.weight"]) and torch.equal(m.out_proj.bias, theirs["out_proj.bias"])


@torch.no_grad()
def test_the_framework_route_is_the_statement_and_says_why():
    torch.manual_seed(1)
    m = CLIPSelfAttention(config()).eval()
    h = torch.randn(2, 7, 128)
    out, weights = m(h)
    assert weights is None and (m.last_route, m.last_reason) == ("framework", "host tensors")
    want, p = hf_statement(m, h)
    assert float((out - want).abs().max()) < 1e-5
    out, weights = m(h, output_attentions=True)
    assert m.last_reason == "output_attentions" and weights.shape == (2, 2, 7, 7) and float((weights - p).abs().max()) < 1e-6
    causal = torch.zeros(7, 7).masked_fill(torch.ones(7, 7, dtype=torch.bool).triu(1), torch.finfo(torch.float32).min)[None, None].expand(2, 1, 7, 7)
    pad = torch.zeros(2, 1, 7, 7)
    pad[1, :, :, 5:] = torch.finfo(torch.float32).min
    for kw in (dict(causal_attention_mask=causal), dict(attention_mask=pad), dict(causal_attention_mask=causal, attention_mask=pad)):
        out, _ = m(h, **kw)
        assert (m.last_route, m.last_reason) == ("framework", "a mask")
        assert float((out - hf_statement(m, h, **kw)[0]).abs().max()) < 1e-5, list(kw)
    with pytest.raises(ValueError, match="should be of size"):
        m(h, attention_mask=torch.zeros(2, 1, 7, 6))
    # keyword arguments of later callers are accepted and ignored
    assert torch.equal(m(h, some_future_flag=True)[0], m(h)[0])
    # dropout acts in training only
    d = CLIPSelfAttention(config(dropout=0.5))
    d.load_state_dict(m.state_dict())
    assert torch.equal(d.eval()(h)[0], m(h)[0])
    d.train()
    torch.manual_seed(2)
    a = d(h)[0]
    assert d.last_reason == "dropout in training" and not torch.equal(a, m(h)[0])
    # the knob
    m.route = "kernels"
    with pytest.raises(RuntimeError, match="route='kernels'.*host tensors"):
        m(h)
    m.route = "both"
    with pytest.raises(ValueError):
        m(h)
    m.route = "framework"
    m(h)
    assert (m.last_route, m.last_reason) == ("framework", "host tensors")


class StubLayer(nn.Module):
    def __init__(self, attn):
        super().__init__()
        self.self_attn = attn


def test_convert_adopts_the_linear_layers():
    torch.manual_seed(3)
    attns = [CLIPSelfAttention(config()).double(), CLIPSelfAttention(config()).half()]
    attns[0].requires_grad_(False)
    attns[1].eval()
    model = nn.Module()
    model.vision_model = nn.Module()
    model.vision_model.encoder = nn.Module()
    model.vision_model.encoder.layers = nn.ModuleList(StubLayer(a) for a in attns)
    before = [{n: p for n, p in a.named_parameters()} for a in attns]
    assert convert_clip_visual_attn(model) is model
    for old, layer, params in zip(attns, model.vision_model.encoder.layers, before):
        new = layer.self_attn
        assert isinstance(new, CLIPSelfAttention) and new is not old and new.training == old.training
        for name in ("q_proj", "k_proj", "v_proj", "out_proj"):
            assert getattr(new, name) is getattr(old, name)
        now = dict(new.named_parameters())
        assert set(now) == set(params)
        for n in now:
            assert now[n] is params[n] and now[n].dtype == params[n].dtype and now[n].requires_grad == params[n].requires_grad


def test_convert_leaves_a_clip_vision_model_with_its_outputs():
    transformers = pytest.importorskip("transformers")
    cfg = transformers.CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                                        image_size=28, patch_size=14, attention_dropout=0.0)
    torch.manual_seed(4)
    model = transformers.CLIPVisionModel(cfg).eval()
    pixels = torch.randn(2, 3, 28, 28)
    with torch.no_grad():
        before = model(pixel_values=pixels).last_hidden_state
    names = [n for n, _ in model.named_parameters()]
    convert_clip_visual_attn(model)
    assert [n for n, _ in model.named_parameters()] == names
    try:
        with torch.no_grad():
            after = model(pixel_values=pixels).last_hidden_state
    except TypeError as e:                                                  # another version's layer passes what this forward does not take
        pytest.skip(f"this transformers version's layer call does not fit: {e}")
    layers = getattr(model, "vision_model", model).encoder.layers
    assert all(isinstance(l.self_attn, CLIPSelfAttention) and l.self_attn.last_route == "framework" for l in layers)
    assert float((after - before).abs().max()) < 1e-5


# ------------------------------------------------------------------ the bounds and the tight measure are a yardstick
def lengths():
    lib = _lib()
    Q, K, KB, QT, _ = (lib.mmfs_clip_attn_tiles(i) for i in range(5))
    return sorted({1, 2, K - 1, K, K + 1, Q - 1, Q, Q + 1, QT - 1, QT, QT + 1, KB - 1, KB, KB + 1, 2 * Q + K // 2 + 3, 257})


def split(x, heads):
    return x.unflatten(-1, (heads, 64)).transpose(1, 2)


def merge(x):
    return x.transpose(1, 2).flatten(2)


def statement(q, k, v, do, heads, scaled=True, zero_tail=0, drop_last=0, delta_sign=1.0):
    """The module's framework statement in q's type with its backward written out as autograd runs it (every product rounded
    to T; the softmax and its backward in T, as the statement has them) -> dict of context, dq, dk, dv.  The keyword arguments
    are the four defects: no 1 / 8; ``zero_tail`` keys of zeros behind L that score 0 instead of -Inf; dk without the last
    ``drop_last`` queries; delta with the wrong sign."""
    T = q.dtype
    qh, kh, vh, g = split(q, heads), split(k, heads), split(v, heads), split(do, heads)
    n = q.shape[1]
    if zero_tail:
        pad = torch.zeros(kh.shape[0], heads, zero_tail, 64, dtype=T)
        kh, vh = torch.cat((kh, pad), 2), torch.cat((vh, pad), 2)
    scale = 0.125 if scaled else 1.0
    qs = qh * scale
    p = (qs @ kh.transpose(-1, -2)).softmax(-1)
    ctx = p @ vh
    dv = p.transpose(-1, -2) @ g
    dp = g @ vh.transpose(-1, -2)
    ds = p * (dp - delta_sign * (p * dp).sum(-1, keepdim=True))
    dq = (ds @ kh) * scale
    live = n - drop_last
    dk = ds[:, :, :live].transpose(-1, -2) @ qs[:, :, :live]
    return dict(context=merge(ctx), dq=merge(dq), dk=merge(dk[:, :, :n]), dv=merge(dv[:, :, :n]))


def kernel_model(q, k, v, do, heads, dtype):
    """The kernels' rounding points on the host: fp64 arithmetic, P and dS rounded to T where they enter a product, delta
    from the stored context, every output rounded once."""
    rt = lambda x: x.to(dtype).double()
    qh, kh, vh, g = (split(t.double(), heads) for t in (q, k, v, do))
    p = (qh @ kh.transpose(-1, -2) * 0.125).softmax(-1)
    ctx = rt(rt(p) @ vh)
    ds = rt(p * (g @ vh.transpose(-1, -2) - (g * ctx).sum(-1, keepdim=True)))
    out = dict(context=ctx, dq=ds @ kh * 0.125, dk=ds.transpose(-1, -2) @ qh * 0.125, dv=rt(p).transpose(-1, -2) @ g)
    return {n: merge(t).to(dtype) for n, t in out.items()}


_refs = {}


def reference(L, dtype):
    if (L, dtype) not in _refs:
        x = draw(100 + L, L, dtype, B_GPU, H_GPU)
        _refs[L, dtype] = (x, clip64(*x[:3], H_GPU, dtype, upstream=x[3]))
    return _refs[L, dtype]


@pytest.mark.parametrize("dtype", HALVES, ids=ids)
@pytest.mark.parametrize("L", lengths())
def test_the_statement_and_a_model_of_the_kernels_hold_both_measures_at_the_gpu_tests_inputs(L, dtype):
    (q, k, v, do), ref = reference(L, dtype)
    for what, got in (("statement", statement(q, k, v, do, H_GPU)), ("model", kernel_model(q, k, v, do, H_GPU, dtype))):
        loose = bound_ratios(got, ref)
        tight = tight_ratios(got, ref, dtype) if L >= 2 else {}
        print(f"{what} L {L} {dtype}: per-element " + ", ".join(f"{n} {x:.3f}" for n, x in loose.items()) +
              "; row error " + ", ".join(f"{n} {x:.3f}" for n, x in tight.items()))
        assert max(loose.values()) <= 1.0, (what, loose)
        assert max(tight.values(), default=0.0) <= 1.0, (what, tight)
    if L == 1:                                                              # where the tight measure has nothing to measure
        assert not ref["dq"].any() and not ref["dk"].any()


@pytest.mark.parametrize("dtype", HALVES, ids=ids)
@pytest.mark.parametrize("name", FAMILIES)
def test_the_statement_and_the_model_hold_both_measures_at_the_score_families(name, dtype):
    L = lengths()[-1]
    q, k, v, do = family(name, 5, L, dtype, 1, 2)
    ref = clip64(q, k, v, 2, dtype, upstream=do)
    top = ref["p"].max(-1).values
    print(f"{name} L {L} {dtype}: lse {float(ref['lse'].min()):.1f} .. {float(ref['lse'].max()):.1f}, a row's largest weight "
          f"{float(top.min()):.3f} .. {float(top.max()):.3f}, median {float(top.median()):.3f}")
    assert float(top.median()) > 0.3                                        # (unit-normal rows: about 0.05)
    loose = bound_ratios(statement(q, k, v, do, 2), ref)
    model = kernel_model(q, k, v, do, 2, dtype)
    tight = tight_ratios(model, ref, dtype)
    print(f"{name} L {L} {dtype}: statement per-element " + ", ".join(f"{n} {x:.3f}" for n, x in loose.items()) +
          "; model row error " + ", ".join(f"{n} {x:.3f}" for n, x in tight.items()))
    assert max(loose.values()) <= 1.0 and max(bound_ratios(model, ref).values()) <= 1.0 and max(tight.values()) <= 1.0


@pytest.mark.parametrize("dtype", HALVES, ids=ids)
@pytest.mark.parametrize("L", [65, 257, lengths()[-1]])
def test_both_measures_together_refuse_four_defects(L, dtype):
    """Stated in fp64, so that nothing but the defect separates them from the reference: each misses a per-element bound or
    the tight measure; so do a gradient of zeros, the negated gradient and half the gradient."""
    (q, k, v, do), ref = reference(L, dtype)
    K, QT = _lib().mmfs_clip_attn_tiles(1), _lib().mmfs_clip_attn_tiles(3)
    args = tuple(t.double() for t in (q, k, v, do))
    clean = statement(*args, H_GPU)
    assert max(bound_ratios(clean, ref).values()) <= 1.0 and max(tight_ratios(clean, ref, dtype).values()) <= 1.0
    defects = (dict(scaled=False), dict(zero_tail=-L % K), dict(drop_last=L - (L - 1) // QT * QT), dict(delta_sign=-1.0))
    for defect in defects:
        got = statement(*args, H_GPU, **defect)
        loose, tight = bound_ratios(got, ref), tight_ratios(got, ref, dtype)
        print(f"defect {defect} L {L} {dtype}: per-element " + ", ".join(f"{n} {x:.3g}" for n, x in loose.items()) +
              "; row error " + ", ".join(f"{n} {x:.3g}" for n, x in tight.items()))
        assert max(max(loose.values()), max(tight.values())) > 1.0, (defect, loose, tight)
    for m in ("dq", "dk", "dv"):
        for what, wrong in (("zeros", torch.zeros_like(ref[m])), ("negated", -ref[m]), ("half", 0.5 * ref[m])):
            assert row_error(wrong, ref[m], dtype, ref.get("S_" + m)) > 1.0, (m, what)
