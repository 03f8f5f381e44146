"""The LLM's self-attention in training (csrc/mmfs_llama_train.hip, LlamaSelfAttention's training route), host side: the
module's training call against the fp64 statement ``train64``; ``train64``'s bounds as a yardstick (the framework's
statement in T lies within them, four defective variants of it do not); the tight row-wise check at the GPU tests' own
inputs (a host model of the kernels' roundings passes it, the defects do not); what must not have moved; the C ABI's argument
checks, every one of which returns before a launch."""
import ctypes
import types

import pytest
import torch
from torch import nn

from helpers import bound_library as _lib
from llama_train_refs import TIGHT_NAMES, draw, row_error, tight_ratios, train64, worst

import mmfs_amd
from mmfs_amd import llama_attn
from mmfs_amd.llama_attn import LlamaSelfAttention, rope_table, rotate_half

DTYPE, DIMS, NULLPTR, ALIGN, UNSUPPORTED = -1, -2, -3, -4, -5
B, H, L = 2, 2, 70                                      # (more than one key tile; the bounds do not depend on tiles)
MAX_POS = 256
GRADS = ("dq", "dk", "dv")


class Fixed(nn.Module):
    """a Linear layer's stand-in that returns a given tensor: the module's statement between its Linear layers"""

    def __init__(self, t):
        super().__init__()
        self.t = t

    def forward(self, x):
        return self.t


def bare_module(q, k, v, heads):
    """a training-mode LlamaSelfAttention whose projections hand out q, k, v and whose o_proj is the identity"""
    cfg = types.SimpleNamespace(hidden_size=heads * 128, num_attention_heads=heads, max_position_embeddings=MAX_POS)
    m = LlamaSelfAttention(cfg).train()
    m.q_proj, m.k_proj, m.v_proj, m.o_proj = Fixed(q), Fixed(k), Fixed(v), nn.Identity()
    return m


def inputs(dtype, seed=0, L=L, qk=1.0):
    gen = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(B, L, H * 128, generator=gen) for _ in range(4))
    q, k, v, do = ((q * qk).to(dtype), ((k * 1.5 + 0.25) * qk).to(dtype), v.to(dtype), do.to(dtype))
    pos = torch.stack([torch.arange(L) + 3 + 11 * b for b in range(B)])     # a per-row offset, not shared
    return q, k, v, do, pos


def run_module(q, k, v, do, pos, mask=None, **kw):
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    m = bare_module(q, k, v, H)
    if mask is None:
        mask = torch.ones(B, q.shape[1])
    out, weights, present = m(torch.zeros(B, q.shape[1], H * 128, dtype=q.dtype), attention_mask=mask, position_ids=pos, **kw)
    out.backward(do)
    return m, out, weights, present, (q.grad, k.grad, v.grad)


@pytest.fixture(scope="module")
def ref64():
    q, k, v, do, pos = inputs(torch.float64)
    cos, sin = rope_table(128, MAX_POS)
    return (q, k, v, do, pos), train64(q, k, v, pos, cos, sin, H, torch.float64, upstream=do)


def test_the_training_call_is_the_fp64_statement(ref64):
    (q, k, v, do, pos), ref = ref64
    m, out, weights, present, grads = run_module(q, k, v, do, pos)
    assert weights is None and present is None
    assert (m.last_route, m.last_reason, m.last_train) == ("framework", "host tensors", "framework ops")
    for name, got in zip(("context",) + GRADS, (out,) + grads):
        err = float((got.detach() - ref[name]).abs().max())
        assert err < 1e-12, (name, err)
    # the mask is not read: its contents change nothing
    for mask in (torch.zeros(B, L), torch.ones(B, L, dtype=torch.bool), torch.zeros(B, L, dtype=torch.long),
                 torch.full((B, L), float("nan"))):
        _, out2, _, _, grads2 = run_module(q, k, v, do, pos, mask=mask)
        assert torch.equal(out2, out) and all(torch.equal(a, b) for a, b in zip(grads2, grads))
    # use_cache is ignored, output_attentions warns
    _, out3, weights, present, _ = run_module(q, k, v, do, pos, use_cache=True)
    assert present is None and weights is None and torch.equal(out3, out)
    with pytest.warns(UserWarning, match="Output attentions"):
        _, out4, weights, _, _ = run_module(q, k, v, do, pos, output_attentions=True)
    assert weights is None and torch.equal(out4, out)
    # position_ids default to 0 .. L - 1
    _, out5, _, _, _ = run_module(q, k, v, do, None)
    _, out6, _, _, _ = run_module(q, k, v, do, torch.arange(L)[None].expand(B, -1))
    assert torch.equal(out5, out6)


# ------------------------------------------------------------------ the bounds are a yardstick
def statement(q, k, v, do, pos, cos, sin, shift=0, scaled=True, forward_sign=False, with_delta=True, heads=H):
    """The framework's statement in q's type with its backward written out as autograd runs it (every product rounded to T,
    the softmax and its backward in fp32) -> (context, dq, dk, dv).  The keyword arguments are the four defects."""
    T = q.dtype
    c, s = (torch.cat((t, t), dim=-1).to(T)[pos].unsqueeze(1) for t in (cos, sin))
    split = lambda x: x.unflatten(-1, (heads, 128)).transpose(1, 2)
    merge = lambda x: x.transpose(1, 2).flatten(2)
    qh, kh, vh, g = split(q), split(k), split(v), split(do)
    qr, kr = qh * c + rotate_half(qh) * s, kh * c + rotate_half(kh) * s
    scale = 128 ** -0.5 if scaled else 1.0
    qs = qr * scale
    n = q.shape[1]
    future = torch.ones(n, n, dtype=torch.bool).triu(1 + shift)
    scores = (qs @ kr.transpose(-1, -2)).masked_fill(future, float("-inf"))
    wide = torch.promote_types(T, torch.float32)
    p32 = scores.softmax(-1, dtype=wide)
    p = p32.to(T)
    ctx = p @ vh
    dv = p.transpose(-1, -2) @ g
    dp = (g @ vh.transpose(-1, -2)).to(wide)
    ds = p32 * (dp - (p32 * dp).sum(-1, keepdim=True)) if with_delta else p32 * dp
    ds = ds.to(T).masked_fill(future, 0.0)
    dqr, dkr = (ds @ kr) * scale, ds.transpose(-1, -2) @ qs
    # rotate_half's adjoint is its negative; the defect keeps the forward's sign
    back = (lambda x: x * c + rotate_half(x) * s) if forward_sign else (lambda x: x * c - rotate_half(x) * s)
    return tuple(merge(t) for t in (ctx, back(dqr), back(dkr), dv))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=lambda d: str(d).split(".")[1])
def test_the_bounds_hold_the_framework_statement_and_refuse_four_defects(dtype):
    # The width of the bound on p is about 5 u |q| . |k| / sqrt(128) (the roundings of q_rot, k_rot, of q / sqrt(128) and of
    # the score).  At unit-normal rows |q| . |k| / sqrt(128) is about 10 and bf16's u is 2^-8: the bound lets p move by a
    # fifth, ds by as much, and a defect of the size of a gradient itself passes under it.  A yardstick needs scores whose
    # bound is narrow, so q and k are a quarter of that here.  The GPU tests hold the kernels at unit-normal rows, where
    # the tight check (row_error) is what tells right from wrong: the test behind this one shows that it does.
    q, k, v, do, pos = inputs(dtype, seed=1, qk=0.25)
    cos, sin = rope_table(128, MAX_POS)
    ref = train64(q, k, v, pos, cos, sin, H, dtype, upstream=do)
    names = ("context",) + GRADS

    def ratios(got):
        return {n: worst(g, ref[n], ref["E_" + n]) for n, g in zip(names, got)}

    # the module's training call (autograd) and the written-out statement
    m, out, _, _, grads = run_module(q, k, v, do, pos)
    assert m.last_train == "framework ops"
    for what, got in (("module", (out,) + grads), ("statement", statement(q, k, v, do, pos, cos, sin))):
        r = ratios(got)
        print(f"{what} {dtype}: worst |got - ref| / bound " + ", ".join(f"{n} {x:.3f}" for n, x in r.items()))
        assert max(r.values()) <= 1.0, (what, r)
    for defect in (dict(shift=1), dict(scaled=False), dict(forward_sign=True), dict(with_delta=False)):
        r = ratios(statement(q, k, v, do, pos, cos, sin, **defect))
        print(f"defect {defect} {dtype}: " + ", ".join(f"{n} {x:.3g}" for n, x in r.items()))
        assert max(r.values()) > 1.0, (defect, r)


# ------------------------------------------------------------------ the tight check at the GPU tests' own inputs
def kernel_model(q, k, v, do, pos, cos, sin, dtype, heads=None):
    """The kernels' rounding points on the host: fp64 arithmetic, q_rot, k_rot, P and dS rounded to T where they enter a
    product, every output rounded once -> (context, dq, dk, dv) in T."""
    rt = lambda x: x.to(dtype).double()
    c, s = (torch.cat((t, t), dim=-1).double()[pos].unsqueeze(1) for t in (cos, sin))
    split = lambda x: x.double().unflatten(-1, (heads or H_GPU, 128)).transpose(1, 2)
    merge = lambda x: x.transpose(1, 2).flatten(2).to(dtype)
    qh, kh, vh, g = split(q), split(k), split(v), split(do)
    qr, kr = rt(qh * c + rotate_half(qh) * s), rt(kh * c + rotate_half(kh) * s)
    n = q.shape[1]
    future = torch.ones(n, n, dtype=torch.bool).triu(1)
    p = (qr @ kr.transpose(-1, -2) * 128 ** -0.5).masked_fill(future, float("-inf")).softmax(-1)
    ctx = rt(rt(p) @ vh)                                                    # (the context the backward reads is the stored one)
    ds = rt(p * (g @ vh.transpose(-1, -2) - (g * ctx).sum(-1, keepdim=True)))
    dqr, dkr = ds @ kr * 128 ** -0.5, ds.transpose(-1, -2) @ qr * 128 ** -0.5
    back = lambda x: x * c - rotate_half(x) * s
    return merge(ctx), merge(back(dqr)), merge(back(dkr)), merge(rt(p).transpose(-1, -2) @ g)


B_GPU, H_GPU = 2, 3                                     # tests/test_llama_train_gpu.py's
DEFECTS = (dict(shift=1), dict(scaled=False), dict(forward_sign=True), dict(with_delta=False))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("n", [64, 291])
def test_the_tight_check_refuses_the_defects_at_the_gpu_tests_inputs(n, dtype):
    """At exactly the inputs tests/test_llama_train_gpu.py draws (unit-normal rows, where the per-element bounds on dq and dk
    are wider than the gradients): ``row_error`` passes a host model of the kernels' roundings and refuses the four
    defects, stated in fp64 so that nothing but the defect separates them from the reference, as well as a gradient of
    zeros, the negated gradient and half the gradient."""
    q, k, v, do, pos = draw(100 + n, n, dtype, B_GPU, H_GPU)
    cos, sin = rope_table(128, 512)
    ref = train64(q, k, v, pos, cos, sin, H_GPU, dtype, upstream=do)
    model = dict(zip(TIGHT_NAMES, kernel_model(q, k, v, do, pos, cos, sin, dtype)))
    tight = tight_ratios(model, ref, dtype)
    loose = {m: worst(model[m], ref[m], ref["E_" + m]) for m in TIGHT_NAMES}
    print(f"model of the kernels' roundings, L {n} {dtype}: row error " + ", ".join(f"{m} {x:.3f}" for m, x in tight.items()) +
          "; per-element " + ", ".join(f"{m} {x:.3f}" for m, x in loose.items()))
    assert max(tight.values()) <= 1.0 and max(loose.values()) <= 1.0, (tight, loose)
    for defect in DEFECTS:
        got = dict(zip(TIGHT_NAMES, statement(q.double(), k.double(), v.double(), do.double(), pos, cos, sin, heads=H_GPU, **defect)))
        r = tight_ratios(got, ref, dtype)
        print(f"defect {defect} L {n} {dtype}: row error " + ", ".join(f"{m} {x:.3g}" for m, x in r.items()))
        assert r["dq"] > 1.0 and r["dk"] > 1.0, (defect, r)
    for m in ("dq", "dk", "dv"):
        for what, wrong in (("zeros", torch.zeros_like(ref[m])), ("negated", -ref[m]), ("half", 0.5 * ref[m])):
            assert row_error(wrong, ref[m], dtype, ref.get("S_" + m)) > 1.0, (m, what)


# ------------------------------------------------------------------ what has not moved
def plain_module(dtype=torch.float64):
    cfg = types.SimpleNamespace(hidden_size=256, num_attention_heads=2, max_position_embeddings=64)
    torch.manual_seed(3)
    return LlamaSelfAttention(cfg).to(dtype)


def test_calls_outside_the_training_route_are_what_they_were():
    m = plain_module()
    h = torch.randn(2, 5, 256, dtype=torch.float64)
    two_d = torch.ones(2, 5, dtype=torch.float64)
    m.eval()
    with pytest.raises(ValueError):                                         # eval mode: a 2-D mask is no mask of this module
        m(h, attention_mask=two_d)
    assert m.last_train is None
    m.train()
    past = (torch.zeros(2, 2, 3, 128, dtype=torch.float64), torch.zeros(2, 2, 3, 128, dtype=torch.float64))
    with pytest.raises(ValueError):                                         # a cache: not the training convention
        m(h, attention_mask=two_d, past_key_value=past)
    with pytest.raises(ValueError):                                         # not [B, q_len]
        m(h, attention_mask=torch.ones(2, 6, dtype=torch.float64))
    # HF's 4-D causal mask and no mask at all: the framework route, the reference's statement, in either mode
    causal = torch.zeros(5, 5, dtype=torch.float64).masked_fill(torch.ones(5, 5, dtype=torch.bool).triu(1),
                                                                torch.finfo(torch.float64).min)[None, None].expand(2, 1, 5, 5)
    results = {}
    for mode in ("train", "eval"):
        getattr(m, mode)()
        for name, mask in (("4d", causal), ("none", None)):
            out, _, _ = m(h, attention_mask=mask)
            assert (m.last_route, m.last_train) == ("framework", None)
            results[mode, name] = out
    for name in ("4d", "none"):
        assert torch.equal(results["train", name], results["eval", name])
    assert not torch.allclose(results["train", "4d"], results["train", "none"])     # None keeps its non-causal meaning
    # and the training route agrees with the 4-D causal mask's framework route
    m.train()
    out, _, _ = m(h, attention_mask=two_d)
    assert m.last_train == "framework ops"
    assert float((out - results["train", "4d"]).detach().abs().max()) < 1e-12


def test_the_route_knob_and_the_threshold():
    assert isinstance(llama_attn.TRAIN_KERNEL_MIN_TOKENS, int) and llama_attn.TRAIN_KERNEL_MIN_TOKENS >= 1
    assert set(llama_attn.DEFAULT_ROUTE) == {"decode", "prefill"}
    m = plain_module().train()
    h = torch.zeros(1, 3, 256, dtype=torch.float64)
    mask = torch.ones(1, 3)
    m.route = "kernels"
    with pytest.raises(RuntimeError, match="host tensors"):
        m(h, attention_mask=mask)
    m.route = "framework"
    m(h, attention_mask=mask)
    assert (m.last_route, m.last_train) == ("framework", "framework ops")
    m.route = "both"
    with pytest.raises(ValueError):
        m(h, attention_mask=mask)


# ------------------------------------------------------------------ the C ABI without a device
def test_the_queries_are_host_only():
    lib = _lib()
    from mmfs_amd.functions import llama_train_func
    tiles = tuple(lib.mmfs_llama_attn_train_tiles(i) for i in range(5))
    Q, K, KB, QT, W = tiles
    assert min(tiles) > 0 and Q % W == 0 and Q % K == 0 and KB % QT == 0 and K % 16 == 0 and QT % 16 == 0
    assert lib.mmfs_llama_attn_train_tiles(5) == DIMS and lib.mmfs_llama_attn_train_tiles(-1) == DIMS
    assert llama_train_func.TRAIN_TILES == tiles
    assert set(llama_train_func.launches) == {"rope", "forward", "backward"}
    assert mmfs_amd.llama_attn_train is llama_train_func.llama_attn_train
    sup = lib.mmfs_llama_attn_train_supported
    assert sup(2, 128, 1) == 1 and sup(1, 128, 1 << 22) == 1
    assert sup(0, 128, 8) == 0 and sup(3, 128, 8) == 0 and sup(2, 64, 8) == 0 and sup(2, 128, 0) == 0 and sup(2, 128, (1 << 22) + 1) == 0
    ws = lib.mmfs_llama_attn_train_workspace_bytes
    assert ws(4, 32, 2048) == 4 * 32 * 2048 * 4 and ws(0, 3, 5) == 0 and ws(2, 3, 0) == 0
    assert ws(-1, 3, 5) == DIMS and ws(2, -3, 5) == DIMS and ws(2, 3, -5) == DIMS and ws(1 << 20, 1 << 5, 5) == DIMS


def test_argument_errors_return_before_any_launch():
    lib = _lib()
    fake = ctypes.c_void_p(4096)                                            # never dereferenced on these paths
    odd = ctypes.c_void_p

    def rope(dt=2, B=2, L=5, H=3, D=128, max_pos=64, **named):
        p = dict.fromkeys(("q", "k", "pos", "cos", "sin"), fake)
        o = dict.fromkeys(("q_rot", "k_rot"), fake)
        p.update({n: x for n, x in named.items() if n in p})
        o.update({n: x for n, x in named.items() if n in o})
        return lib.mmfs_llama_attn_train_rope(dt, *p.values(), max_pos, *o.values(), B, L, H, D, None)

    def fwd(dt=2, B=2, L=5, H=3, D=128, **named):
        p = dict.fromkeys(("q_rot", "k_rot", "v", "context", "lse"), fake)
        p.update(named)
        return lib.mmfs_llama_attn_train_forward(dt, *p.values(), B, L, H, D, None)

    def bwd(dt=2, B=2, L=5, H=3, D=128, max_pos=64, **named):
        p = dict.fromkeys(("q_rot", "k_rot", "v", "context", "grad_context", "lse", "pos", "cos", "sin"), fake)
        o = dict.fromkeys(("grad_q", "grad_k", "grad_v", "workspace"), fake)
        p.update({n: x for n, x in named.items() if n in p})
        o.update({n: x for n, x in named.items() if n in o})
        return lib.mmfs_llama_attn_train_backward(dt, *p.values(), max_pos, *o.values(), B, L, H, D, None)

    pointers = {rope: ("q", "k", "pos", "cos", "sin", "q_rot", "k_rot"), fwd: ("q_rot", "k_rot", "v", "context", "lse"),
                bwd: ("q_rot", "k_rot", "v", "context", "grad_context", "lse", "pos", "cos", "sin", "grad_q", "grad_k", "grad_v",
                      "workspace")}
    for f, names in pointers.items():
        assert f(dt=9) == DTYPE and f(dt=-1) == DTYPE
        assert f(B=-1) == DIMS and f(H=-1) == DIMS and f(D=-1) == DIMS and f(L=-1) == DIMS
        assert f(B=1 << 20, H=1 << 5) == DIMS and f(B=(1 << 20) + 1) == DIMS
        assert f(dt=0) == UNSUPPORTED and f(dt=3) == UNSUPPORTED            # fp32 / fp64 storage: the framework's
        assert f(D=64) == UNSUPPORTED and f(D=127) == UNSUPPORTED and f(D=256) == UNSUPPORTED
        assert f(L=(1 << 22) + 1) == UNSUPPORTED
        assert f(D=64, B=0) == UNSUPPORTED                                  # (refused before it is found empty)
        for name in names:
            assert f(**{name: None}) == NULLPTR, name
            step = 4 if name == "lse" else 8 if name == "pos" else 16
            assert f(**{name: odd(4096 + step // 2)}) == ALIGN, name
        # empty problems: 0 without a launch, whatever the pointers
        for kw in (dict(B=0), dict(H=0), dict(L=0)):
            assert f(**kw) == 0, kw
            assert f(**kw, **{n: None for n in names}) == 0, kw
    assert rope(max_pos=-1) == DIMS and bwd(max_pos=-1) == DIMS
