"""The Q-Former attention kernels (csrc/mmfs_attn.hip) on the device, through mmfs_amd.functions.QKNormAttentionFunction
and mmfs_amd.QKNormAttention.

``context``, ``lse``, ``dq``, ``dk``, ``dv`` and the four LayerNorm parameter gradients are held element by element to
fp64 on the stored q, k, v under the bounds of the kernel file's header (tests/qk_attn_refs.py states them;
tests/test_qk_attn.py pins that statement to the reference's fixtures); the framework route's result in the storage
type on the same inputs is held to the SAME bounds, so a bound is one the reference statement itself meets.  Outputs
are poisoned before the kernels run: an element nobody wrote is NaN.

Worst bound ratios measured on an MI355X are kept in profiles/qk_attn.md."""
import types

import numpy as np
import pytest
import torch

from front_end_refs import worst
from helpers import load_golden, poison_allocations
from qk_attn_refs import attention64

from mmfs_amd.resampler import QKNormAttention

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.bfloat16, torch.float16]
EPS = 1e-12
NORM_NAMES = ("q_norm.weight", "q_norm.bias", "k_norm.weight", "k_norm.bias")
# (Nq, Nk, qk-norm, bias): every Nq of {1, 15, 16, 17, 64, 77, 128} and every Nk of {1, 31, 32, 33, 64, 257, 300}
SHAPES = [(1, 1, True, False), (15, 31, True, True), (16, 32, False, True), (17, 33, True, False), (64, 64, True, True),
          (77, 257, False, True), (128, 300, True, True), (64, 257, False, False)]


def func():
    from mmfs_amd.functions import qk_attn_func
    return qk_attn_func


def module(H, norm, dtype, params=None, dropout=0.0, **more):
    cfg = types.SimpleNamespace(hidden_size=H * 64, num_attention_heads=H, encoder_hidden_size=H * 64,
                                attention_probs_dropout_prob=dropout, layer_norm_eps=EPS, qk_normalization=norm, **more)
    m = QKNormAttention(cfg, is_cross_attention=True).to(DEV, dtype).eval()
    if params is not None:
        with torch.no_grad():
            for name, p in zip(NORM_NAMES, params):
                m.get_parameter(name).copy_(p)
    return m


def draw(gen, B, Nq, Nk, H, dtype, norm, bias):
    q = torch.randn(B, Nq, H * 64, generator=gen).to(DEV, dtype)
    k = (torch.randn(B, Nk, H * 64, generator=gen) * 1.5 + 0.25).to(DEV, dtype)
    v = torch.randn(B, Nk, H * 64, generator=gen).to(DEV, dtype)
    up = torch.randn(B, Nq, H * 64, generator=gen).to(DEV, dtype)
    params = None
    if norm:
        params = tuple((torch.randn(64, generator=gen) * 0.3 + (1.0 if i % 2 == 0 else 0.0)).to(DEV, dtype) for i in range(4))
    kb = (torch.randn(B, Nk, generator=gen) * 2).to(DEV, dtype).float() if bias else None
    return q, k, v, up, params, kb


def run_kernels(q, k, v, up, params, kb, H):
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    ps = [p.clone().requires_grad_(True) for p in params] if params else [None] * 4
    before = dict(func().launches)
    ctx, lse = func().QKNormAttentionFunction.apply(*leaves, *ps, EPS, kb, H)
    grads = torch.autograd.grad(ctx, leaves + (ps if params else []), up)
    took = (func().launches["forward"] - before["forward"], func().launches["backward"] - before["backward"])
    assert took == (1, 2 if params else 1), took
    out = {"context": ctx.detach(), "lse": lse, "dq": grads[0], "dk": grads[1], "dv": grads[2]}
    if params:
        out["dparams"] = torch.stack(grads[3:])
    return out


def run_framework(q, k, v, up, params, kb, H):
    m = module(H, params is not None, q.dtype, params)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    mask = None if kb is None else kb.to(q.dtype)[:, None, None, :]
    before = dict(func().launches)
    res = m._framework(None, *leaves, mask, None, True, None, False)
    ps = [m.get_parameter(n) for n in NORM_NAMES] if params else []
    grads = torch.autograd.grad(res[0], leaves + ps, up)
    assert func().launches == before and len(res) == 2
    out = {"context": res[0].detach(), "dq": grads[0], "dk": grads[1], "dv": grads[2]}
    if params:
        out["dparams"] = torch.stack(grads[3:])
    return out


def hold(tag, got, r, report):
    for name, t in got.items():
        ref, bound = r[name], r["E_" + name]
        w = worst(t.detach(), ref, bound)
        report.append((f"{tag} {name}", w[0]))
        assert w[0] <= 1.0, (f"{tag} {name}: |got - ref| / bound = {w[0]:.3g} at {w[1]}: got {w[2]!r}, ref {w[3]!r}, "
                             f"bound {w[4]:.3g}")


def show(report):
    by_kind = {}
    for what, ratio in report:
        by_kind[what] = max(by_kind.get(what, 0.0), ratio)
    print("worst |got - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(by_kind.items())))


def both_routes(q, k, v, up, params, kb, H, report):
    r = attention64(q, k, v, H, norm=params, eps=EPS, bias=kb, upstream=up, dtype=q.dtype)
    got = run_kernels(q, k, v, up, params, kb, H)
    for name in ("context", "dq", "dk", "dv"):
        assert got[name].dtype == q.dtype and got[name].shape == r[name].shape
    hold("kernels", got, r, report)
    hold("framework", run_framework(q, k, v, up, params, kb, H), r, report)
    return r, got


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}{'n' if s[2] else ''}{'b' if s[3] else ''}")
def test_both_routes_hold_the_bounds(shape, dtype, monkeypatch):
    """B = 2, H = 3: an odd head count catches a wrong head stride"""
    Nq, Nk, norm, bias = shape
    gen = torch.Generator().manual_seed(1000 * Nq + Nk)
    q, k, v, up, params, kb = draw(gen, 2, Nq, Nk, 3, dtype, norm, bias)
    poison_allocations(monkeypatch)
    report = []
    both_routes(q, k, v, up, params, kb, 3, report)
    show(report)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("dims", [(1, 3, 77, 40), (1, 1, 1, 5), (3, 1, 5, 19)], ids=lambda s: "x".join(map(str, s)))
def test_an_odd_number_of_rows_holds_the_bounds(dims, dtype, monkeypatch):
    """B H Nq odd: the per-row statistics (lse, then the pairs (m, l) in the same allocation) start on any 4-byte
    boundary; any B and H are served"""
    B, H, Nq, Nk = dims
    gen = torch.Generator().manual_seed(B * 1000 + H * 100 + Nq)
    q, k, v, up, params, kb = draw(gen, B, Nq, Nk, H, dtype, True, True)
    poison_allocations(monkeypatch)
    report = []
    both_routes(q, k, v, up, params, kb, H, report)
    m = module(H, True, dtype, params)                      # and through the module: the kernels, no error
    out = m(q, encoder_hidden_states=k)
    assert m.last_route == "kernels" and out[0].shape == (B, Nq, H * 64) and bool(torch.isfinite(out[0]).all())
    show(report)


# ------------------------------------------------------------------ masks
def masked_bias(kind, B, Nk, dtype):
    """Nk = 160 keys = tiles [0, 64), [64, 128), [128, 160); batch row 0 carries the mask, row 1 a shorter one"""
    low = torch.finfo(dtype).min
    kb = torch.zeros(B, Nk)
    if kind == "tail":
        kb[0, 140:] = low
        kb[1, 150:] = low
    elif kind == "middle_tile":
        kb[0, 64:128] = low
        kb[1, 70:100] = low
    elif kind == "first_tile":
        kb[0, :64] = low
        kb[1, :3] = low
    elif kind == "all_lowest":
        kb[0, :] = low
        kb[1, 1:] = low
    return kb.to(DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("kind", ["tail", "middle_tile", "first_tile", "all_lowest"])
def test_masked_keys(kind, dtype, monkeypatch):
    gen = torch.Generator().manual_seed(77)
    q, k, v, up, params, _ = draw(gen, 2, 21, 160, 3, dtype, True, False)
    kb = masked_bias(kind, 2, 160, dtype)
    poison_allocations(monkeypatch)
    report = []
    r, got = both_routes(q, k, v, up, params, kb, 3, report)
    if kind == "all_lowest":
        # every key at finfo(T).min: the uniform average of v, and one key left: that key's v
        want = v.double().mean(1, keepdim=True).expand(-1, 21, -1)
        assert float((r["context"][0] - want[0]).abs().max()) <= 1e-12
        assert float((got["context"][0].double() - want[0]).abs().max()) <= float(r["E_context"][0].max())
        assert torch.equal(got["context"][1], v[1, 0:1].expand(21, -1))
    show(report)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_keys_at_minus_infinity_are_nan_exactly_where_the_framework_route_has_nan(dtype, monkeypatch):
    gen = torch.Generator().manual_seed(78)
    q, k, v, up, params, _ = draw(gen, 2, 21, 160, 3, dtype, True, False)
    kb = torch.zeros(2, 160, device=DEV)
    kb[0, :] = -float("inf")                              # the whole row: NaN
    kb[1, :64] = -float("inf")                            # a whole first tile: must not poison the running pair
    kb[1, 100:] = -float("inf")
    poison_allocations(monkeypatch)
    with torch.no_grad():
        ctx, lse = func().QKNormAttentionFunction.apply(q, k, v, *params, EPS, kb, 3)
        fw = module(3, True, dtype, params)._framework(None, q, k, v, kb.to(dtype)[:, None, None, :], None, True, None, False)[0]
    assert torch.equal(torch.isnan(ctx), torch.isnan(fw))
    assert bool(torch.isnan(ctx[0]).all()) and not bool(torch.isnan(ctx[1]).any())
    r = attention64(q[1:], k[1:], v[1:], 3, norm=params, eps=EPS, bias=kb[1:], dtype=dtype)
    report = []
    hold("kernels", {"context": ctx[1:], "lse": lse[1:]}, r, report)
    hold("framework", {"context": fw[1:]}, r, report)
    show(report)


# ------------------------------------------------------------------ large scores
def large_bias(kind, B, Nk, dtype):
    """q and k are normalised, so a large part of a score can only come through the key bias: an fp32 row that rises or falls
    by 0.5 a key (a running maximum that rises at every key tile; tiles that underflow behind the first), or one key at +8;
    at values T holds, since the framework route casts the bias to T"""
    t = torch.arange(Nk, dtype=torch.float32)
    row = {"rise": 0.5 * t, "fall": -0.5 * t, "peak": torch.zeros(Nk).index_fill_(0, torch.tensor([Nk // 2]), 8.0)}[kind]
    return row.to(dtype).float()[None].expand(B, -1).contiguous().to(DEV)


LARGE = [SHAPES[4], max(SHAPES, key=lambda s: s[0] * s[1])]
assert LARGE[0][:2] == (64, 64)


def large_case(shape, kind, dtype):
    Nq, Nk, norm, _ = shape
    gen = torch.Generator().manual_seed(1000 * Nq + Nk + 7)
    q, k, v, up, params, _ = draw(gen, 2, Nq, Nk, 3, dtype, norm, False)
    return q, k, v, up, params, large_bias(kind, 2, Nk, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("kind", ["rise", "fall", "peak"])
@pytest.mark.parametrize("shape", LARGE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_kernels_hold_the_bounds_at_large_key_biases(shape, kind, dtype, monkeypatch):
    """Forward and backward against attention64; lse reaches 153 at the rising bias over 300 keys.  In bf16 at (128, 300) one
    key's bias lies 88.5 below the largest: its weights sit at 2^-126, where the hardware exp2 returns 0; qk_attn_bwd carries
    such a key's column of P and dS times a power of two (profiles/qk_attn.md: dv measured 2.86 and 3.09 before that)."""
    q, k, v, up, params, kb = large_case(shape, kind, dtype)
    r = attention64(q, k, v, 3, norm=params, eps=EPS, bias=kb, upstream=up, dtype=dtype)
    poison_allocations(monkeypatch)
    report = []
    hold("kernels", run_kernels(q, k, v, up, params, kb, 3), r, report)
    print(f"{kind} lse {float(r['lse'].min()):.1f} .. {float(r['lse'].max()):.1f}")
    show(report)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("kind", ["rise", "fall", "peak"])
@pytest.mark.parametrize("shape", LARGE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_framework_route_holds_the_bounds_at_large_key_biases(shape, kind, dtype, monkeypatch):
    """The framework route under the same bounds.  With a mask in 16-bit storage it adds the bias and takes the softmax in
    fp32 (a sum in T rounds score + 150 to a grid of 1 in bf16, which E_s = .. + 3 u |s0| does not count: the context measured
    up to 13.5 that way, profiles/qk_attn.md)."""
    q, k, v, up, params, kb = large_case(shape, kind, dtype)
    r = attention64(q, k, v, 3, norm=params, eps=EPS, bias=kb, upstream=up, dtype=dtype)
    poison_allocations(monkeypatch)
    report = []
    try:
        hold("framework", run_framework(q, k, v, up, params, kb, 3), r, report)
    finally:
        show(report)


# ------------------------------------------------------------------ the reference's fixtures
@pytest.mark.parametrize("case", ["self_qknorm", "cross_qknorm_masked", "cross_plain_77", "cross_one_key_left"])
def test_goldens_at_bf16(case, monkeypatch):
    """the fixture's inputs and parameters cast to bf16, q / k / v from its Linear layers on the device; both routes
    against fp64 on those q, k, v under the same bounds"""
    dtype = torch.bfloat16
    g = {n: torch.from_numpy(np.asarray(a)) for n, a in load_golden("qk_attn_" + case).items()}
    norm, cross = bool(g["qk_normalization"]), bool(g["is_cross_attention"])
    cfg = types.SimpleNamespace(hidden_size=128, num_attention_heads=2, encoder_hidden_size=40,
                                attention_probs_dropout_prob=0.0, layer_norm_eps=EPS, qk_normalization=norm)
    m = QKNormAttention(cfg, is_cross_attention=cross)
    m.load_state_dict({n[len("param."):]: a for n, a in g.items() if n.startswith("param.")}, strict=True)
    m = m.to(DEV, dtype).eval()
    hidden = g["hidden_states"].to(DEV, dtype)
    src = g["encoder_hidden_states"].to(DEV, dtype) if cross else hidden
    up = g["upstream"].to(DEV, dtype)
    with torch.no_grad():
        q, k, v = m.query(hidden), m.key(src), m.value(src)
    params = tuple(m.get_parameter(n).detach() for n in NORM_NAMES) if norm else None
    kb = None
    if "mask" in g:                                          # HF writes finfo(T).min where the fixture has finfo(float32).min
        kb = torch.where(g["mask"].reshape(2, -1) < 0, torch.finfo(dtype).min, 0.0).float().to(DEV)
    poison_allocations(monkeypatch)
    report = []
    both_routes(q, k, v, up, params, kb, 2, report)
    # and the module itself takes the kernels on this call, with the same context
    mask = None if kb is None else kb.to(dtype)[:, None, None, :]
    out = m(hidden, encoder_hidden_states=src, encoder_attention_mask=mask) if cross else m(hidden, attention_mask=mask)
    assert m.last_route == "kernels" and len(out) == 2 and out[1] is None
    with torch.no_grad():
        want, _ = func().QKNormAttentionFunction.apply(q, k, v, *(params or (None,) * 4), EPS, kb, 2)
    assert torch.equal(out[0], want)
    # not far from the fixture's own fp64 context either (bf16 inputs and parameters: a loose, absolute check)
    assert float((out[0].detach().double().cpu() - g["context"].double()).abs().max()) <= 0.05 * float(g["context"].abs().max())
    show(report)


# ------------------------------------------------------------------ reproducibility, graphs, routes
def test_two_runs_agree_bit_for_bit(monkeypatch):
    gen = torch.Generator().manual_seed(5)
    q, k, v, up, params, kb = draw(gen, 4, 77, 300, 3, torch.bfloat16, True, True)
    poison_allocations(monkeypatch)
    a = run_kernels(q, k, v, up, params, kb, 3)
    b = run_kernels(q, k, v, up, params, kb, 3)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_parameters_and_bias_of_either_type_and_a_shared_bias_give_the_same_bits():
    """the kernels read the LayerNorm parameters and the bias as fp32 or as T where they lie; one bias row may serve the batch"""
    gen = torch.Generator().manual_seed(8)
    q, k, v, up, params, kb = draw(gen, 2, 17, 70, 3, torch.float16, True, True)
    kb[1] = kb[0]
    a = run_kernels(q, k, v, up, params, kb, 3)
    b = run_kernels(q, k, v, up, tuple(p.float() for p in params), kb.to(q.dtype), 3)
    c = run_kernels(q, k, v, up, params, kb[0:1].expand(2, -1), 3)
    for name in a:
        assert torch.equal(a[name], b[name].to(a[name].dtype)) and torch.equal(a[name], c[name]), name
    assert b["dparams"].dtype == torch.float32 and a["dparams"].dtype == torch.float16


def test_forward_and_backward_captured_into_one_graph_replay_the_eager_bits():
    gen = torch.Generator().manual_seed(6)
    q, k, v, up, params, kb = draw(gen, 2, 64, 257, 3, torch.bfloat16, True, True)
    eager = run_kernels(q, k, v, up, params, kb, 3)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    ps = [p.clone().requires_grad_(True) for p in params]

    def step():
        ctx, lse = func().QKNormAttentionFunction.apply(*leaves, *ps, EPS, kb, 3)
        return (ctx.detach(), lse) + torch.autograd.grad(ctx, leaves + ps, up)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = {"context": outs[0], "lse": outs[1], "dq": outs[2], "dk": outs[3], "dv": outs[4], "dparams": torch.stack(outs[5:])}
        for name in eager:
            assert torch.equal(got[name], eager[name]), name


def test_the_module_takes_the_kernels_unless_the_call_asks_for_more():
    dtype, H = torch.bfloat16, 3
    gen = torch.Generator().manual_seed(9)
    m = module(H, True, dtype)
    hidden = torch.randn(2, 16, H * 64, generator=gen).to(DEV, dtype)
    enc = torch.randn(2, 40, H * 64, generator=gen).to(DEV, dtype)
    mask = torch.zeros(2, 1, 1, 40, device=DEV, dtype=dtype)
    mask[1, ..., 30:] = torch.finfo(dtype).min

    def took(**kw):
        before = dict(func().launches)
        out = m(hidden, encoder_hidden_states=enc, encoder_attention_mask=kw.pop("mask", mask), **kw)
        return m.last_route, func().launches["forward"] - before["forward"], out

    route, n, out = took()
    assert (route, n) == ("kernels", 1) and len(out) == 2 and out[1] is None and out[0].shape == (2, 16, H * 64)
    fused = out[0]
    for kw, length in ((dict(head_mask=torch.ones(1, H, 1, 1, device=DEV, dtype=dtype)), 2), (dict(output_attentions=True), 3),
                       (dict(mask=mask.expand(2, 1, 16, 40)), 2)):
        route, n, out = took(**kw)
        assert (route, n) == ("framework", 0) and len(out) == length and len(out[-1]) == 2, kw
        assert float((out[0].detach().float() - fused.detach().float()).abs().max()) <= 0.05                 # (the same mathematics)
    route, n, out = took(mask=torch.zeros(H, 16, 40, device=DEV, dtype=dtype))             # a 3-D mask
    assert (route, n) == ("framework", 0) and len(out) == 2 and len(out[-1]) == 2
    m.save_attention = True
    assert took()[:2] == ("framework", 0)
    m.save_attention = False
    m.dropout.p = 0.1
    assert took()[:2] == ("kernels", 1)                              # eval mode: dropout is the identity
    m.train()
    assert took()[:2] == ("framework", 0)
    m.eval()
    with torch.autocast("cuda", dtype=dtype):
        assert took()[:2] == ("framework", 0)
    # self-attention with a cached pair, and fp32 storage
    ms = module(H, True, dtype)
    first = ms(hidden)
    assert ms.last_route == "kernels" and first[1] is None
    ms.route = "framework"
    pair = ms(hidden)[1]
    ms.route = None
    ms(hidden, past_key_value=pair)
    assert ms.last_route == "framework"
    m32 = module(H, True, torch.float32)
    m32(hidden.float(), encoder_hidden_states=enc.float())
    assert m32.last_route == "framework"
    m.route = "kernels"
    with pytest.raises(RuntimeError):
        m(hidden, encoder_hidden_states=enc, output_attentions=True)
