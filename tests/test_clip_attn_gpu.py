"""The CLIP ViT's self-attention on the device (csrc/mmfs_clip_attn.hip), through the C ABI's entries
(mmfs_amd.functions.clip_attn_func.clip_forward / clip_backward), the autograd.Function and CLIPSelfAttention's kernel route.

``context``, ``lse``, ``dq``, ``dk``, ``dv`` are held element by element to fp64 on the stored inputs under the bounds of the
kernel file's header (tests/clip_attn_refs.py states them; tests/test_clip_attn.py shows that the framework's statement meets
them and four defective ones do not), and the context and the three gradients row by row to a tight relative measure
(``row_error``; the same file shows, at exactly these inputs, the defects it refuses).  Outputs are poisoned before the kernels
run: an element nobody wrote is NaN.

Worst ratios of both measured on an MI355X are kept in profiles/clip_attn.md."""
import types

import pytest
import torch
from torch.utils.checkpoint import checkpoint

from clip_attn_refs import FAMILIES, NAMES, bound_ratios, clip64, draw as refs_draw, family, tight_ratios
from helpers import poison_allocations

import MultiScaleDeformableAttention as MSDA
import mmfs_amd
from mmfs_amd.clip_attn import CLIPSelfAttention
from mmfs_amd.functions import clip_attn_func as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.bfloat16, torch.float16]
B, H = 2, 3
ids = lambda d: str(d).split(".")[1]


def lengths():
    Q, K, KB, QT, _ = F.CLIP_TILES
    return sorted({1, 2, K - 1, K, K + 1, Q - 1, Q, Q + 1, QT - 1, QT, QT + 1, KB - 1, KB, KB + 1, 2 * Q + K // 2 + 3, 257})


def long_length():
    Q, K = F.CLIP_TILES[:2]
    return 2 * Q + K // 2 + 3


def pytest_generate_tests(metafunc):
    if "L" in metafunc.fixturenames:                                        # (the tile sizes come from the library)
        metafunc.parametrize("L", lengths())


def draw(seed, L, dtype, B=B, H=H):
    return refs_draw(seed, L, dtype, B, H, device=DEV)


def run_abi(q, k, v, up, heads=H):
    """the two entries one after the other, as the Function calls them"""
    ctx, lse = F.clip_forward(q, k, v, heads)
    dq, dk, dv = F.clip_backward(q, k, v, ctx, up, lse, heads)
    torch.cuda.synchronize()
    return dict(zip(NAMES, (ctx, lse, dq, dk, dv)))


def run_function(q, k, v, up, heads=H):
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    ctx = mmfs_amd.clip_attention(*leaves, heads)
    grads = torch.autograd.grad(ctx, leaves, up)
    torch.cuda.synchronize()
    return dict(zip(("context", "dq", "dk", "dv"), (ctx.detach(),) + grads))


def hold_both_measures(what, x, heads, dtype, monkeypatch, tight=True):
    q, k, v, up = x
    ref = clip64(q, k, v, heads, dtype, upstream=up)
    poison_allocations(monkeypatch)
    abi = run_abi(q, k, v, up, heads)
    fn = run_function(q, k, v, up, heads)
    ratios = bound_ratios(abi, ref)
    print(f"{what} {dtype}: worst |got - ref| / bound " + ", ".join(f"{n} {r:.3f}" for n, r in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    if tight:
        rows = tight_ratios(abi, ref, dtype)
        print(f"{what} {dtype}: worst row error / (8 u (|row| + share + floor)) " + ", ".join(f"{n} {r:.3f}" for n, r in rows.items()))
        assert max(rows.values()) <= 1.0, rows
    for n in fn:                                                            # the Function is the two entries
        assert torch.equal(fn[n], abi[n]), n


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_every_output_holds_its_bound(L, dtype, monkeypatch):
    hold_both_measures(f"L {L}", draw(100 + L, L, dtype), H, dtype, monkeypatch, tight=L >= 2)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", FAMILIES)
def test_peaked_and_sink_rows_hold_both_measures(name, dtype, monkeypatch):
    hold_both_measures(name, family(name, 5, long_length(), dtype, 1, 2, device=DEV), 2, dtype, monkeypatch)


def test_the_forward_without_lse_is_the_forward(monkeypatch):
    q, k, v, up = draw(3, long_length(), torch.bfloat16)
    poison_allocations(monkeypatch)
    with_lse, lse = F.clip_forward(q, k, v, H)
    without, none = F.clip_forward(q, k, v, H, want_lse=False)
    assert none is None and torch.equal(with_lse, without) and bool(torch.isfinite(lse).all())
    before = dict(F.launches)
    with torch.no_grad():
        assert torch.equal(mmfs_amd.clip_attention(q, k, v, H), with_lse)
    assert {n: F.launches[n] - before[n] for n in before} == {"forward": 1, "backward": 0}


# ------------------------------------------------------------------ the module
def module(dtype, heads=H, dropout=0.0, seed=0):
    torch.manual_seed(seed)
    cfg = types.SimpleNamespace(hidden_size=heads * 64, num_attention_heads=heads, attention_dropout=dropout)
    return CLIPSelfAttention(cfg).to(DEV, dtype)


def hidden(seed, L, dtype, heads=H, rows=B):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(rows, L, heads * 64, generator=gen).to(DEV, dtype)


def test_the_module_route_is_the_function_bit_for_bit():
    dtype, L = torch.bfloat16, long_length()
    m = module(dtype)
    h, up = hidden(7, L, dtype).requires_grad_(True), hidden(8, L, dtype)
    before = dict(F.launches)
    out, weights = m(h)
    (dh,) = torch.autograd.grad(out, h, up)
    assert weights is None and (m.last_route, m.last_reason) == ("kernels", None)
    assert {n: F.launches[n] - before[n] for n in before} == {"forward": 1, "backward": 2}
    h2 = h.detach().clone().requires_grad_(True)
    want = m.out_proj(F.ClipAttentionFunction.apply(m.q_proj(h2), m.k_proj(h2), m.v_proj(h2), H))
    (dh2,) = torch.autograd.grad(want, h2, up)
    assert torch.equal(out, want) and torch.equal(dh, dh2)
    # without gradients: the kernels all the same
    with torch.no_grad():
        again, _ = m(h)
    assert m.last_route == "kernels" and torch.equal(again, out)
    # forced to the framework's statement: no launch, the same numbers to the rounding of T
    before = dict(F.launches)
    m.route = "framework"
    with torch.no_grad():
        fw, _ = m(h)
    assert (m.last_route, m.last_reason) == ("framework", None) and F.launches == before
    assert float((fw.float() - again.float()).abs().max()) <= 2.0 ** -5 * float(again.float().abs().max())


def test_routing_refusals_name_their_reason():
    dtype, L = torch.bfloat16, 9
    m = module(dtype).train()
    h = hidden(9, L, dtype)
    m(h)
    assert (m.last_route, m.last_reason) == ("kernels", None)               # training mode, dropout 0
    m.float()
    m(h.float())
    assert (m.last_route, m.last_reason) == ("framework", "tensors the kernels do not serve")
    m.to(dtype)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        m(h)
    assert (m.last_route, m.last_reason) == ("framework", "autocast")
    mask = torch.zeros(B, 1, L, L, device=DEV, dtype=dtype)
    m(h, attention_mask=mask)
    assert (m.last_route, m.last_reason) == ("framework", "a mask")
    m(h, causal_attention_mask=mask)
    assert (m.last_route, m.last_reason) == ("framework", "a mask")
    _, weights = m(h, output_attentions=True)
    assert (m.last_route, m.last_reason) == ("framework", "output_attentions") and weights.shape == (B, H, L, L)
    d = module(dtype, dropout=0.1).train()
    d(h)
    assert (d.last_route, d.last_reason) == ("framework", "dropout in training")
    d.eval()
    d(h)
    assert d.last_route == "kernels"
    wide = module(dtype, heads=1)
    wide.num_heads, wide.head_dim = 2, 32                                   # heads of 32 channels
    wide(hidden(10, L, dtype, heads=1))
    assert (wide.last_route, wide.last_reason) == ("framework", "tensors the kernels do not serve")
    # a forced kernel route that does not apply raises with the reason
    m.route = "kernels"
    for kw, why in ((dict(attention_mask=mask), "a mask"), (dict(output_attentions=True), "output_attentions")):
        with pytest.raises(RuntimeError, match=f"route='kernels'.*{why}"):
            m(h, **kw)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(RuntimeError, match="route='kernels'.*autocast"):
            m(h)
    d.train()
    d.route = "kernels"
    with pytest.raises(RuntimeError, match="route='kernels'.*dropout in training"):
        d(h)


def test_a_checkpointed_encoder_layer_with_frozen_weights_gives_the_same_gradients():
    dtype, L = torch.bfloat16, long_length()
    m = module(dtype).requires_grad_(False)
    up = hidden(12, L, dtype)

    def run(wrap):
        h = hidden(11, L, dtype).requires_grad_(True)
        call = lambda x: m(x)[0]
        out = call(h) if wrap is None else wrap(call, h)
        out.backward(up)                                                    # (a reentrant checkpoint takes no autograd.grad)
        assert m.last_route == "kernels" and all(p.grad is None for p in m.parameters())
        return out.detach(), h.grad

    plain = run(None)
    for reentrant in (False, True):
        again = run(lambda call, x: checkpoint(call, x, use_reentrant=reentrant))
        assert torch.equal(plain[0], again[0]) and torch.equal(plain[1], again[1]), reentrant


# ------------------------------------------------------------------ partial tiles, isolation, reproducibility
GUARD = 64                                              # elements of T before and behind an output (128 bytes: 16-byte aligned)


def guarded(shape, dtype):
    """-> (buffer of a bit pattern, the output inside it, GUARD elements from either end)"""
    n = 1
    for s in shape:
        n *= s
    guard = GUARD * 2 // torch.empty((), dtype=dtype).element_size()
    buf = torch.empty(n + 2 * guard, dtype=dtype, device=DEV)
    buf.view(torch.uint8).fill_(0xA5)
    return buf, buf[guard:guard + n].view(shape), guard


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_partial_tiles_write_their_rows_and_nothing_else(dtype):
    for L in (F.CLIP_TILES[0] + 1, 1):
        q, k, v, up = draw(31 + L, L, dtype)
        want = run_abi(q, k, v, up)
        outs = {n: guarded((B, H, L) if n in ("lse", "ws") else (B, L, H * 64), torch.float32 if n in ("lse", "ws") else dtype)
                for n in NAMES + ("ws",)}
        ptr = lambda n: outs[n][1].data_ptr()
        code = MSDA._DTYPE_CODE[dtype]
        MSDA._call("clip_attn_fwd", "mmfs_clip_attn_forward", DEV, code, q.data_ptr(), k.data_ptr(), v.data_ptr(), ptr("context"),
                   ptr("lse"), B, L, H, 64)
        MSDA._call("clip_attn_bwd", "mmfs_clip_attn_backward", DEV, code, q.data_ptr(), k.data_ptr(), v.data_ptr(), ptr("context"),
                   up.data_ptr(), ptr("lse"), ptr("dq"), ptr("dk"), ptr("dv"), ptr("ws"), B * H * L * 4, B, L, H, 64)
        torch.cuda.synchronize()
        for n, (buf, out, guard) in outs.items():
            raw = buf.view(torch.uint8)
            edge = guard * buf.element_size()
            assert bool((raw[:edge] == 0xA5).all()) and bool((raw[-edge:] == 0xA5).all()), (n, L)
            if n != "ws":
                assert torch.equal(out, want[n]), (n, L)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_a_nan_in_one_key_stays_in_its_head(dtype, monkeypatch):
    Q, K = F.CLIP_TILES[:2]
    L = long_length()
    q, k, v, up = draw(37, L, dtype)
    poison_allocations(monkeypatch)
    clean = run_abi(q, k, v, up)
    assert all(bool(torch.isfinite(clean[n]).all()) for n in NAMES)
    per_head = lambda n, t, b, h: t[b, h] if n == "lse" else t[b, :, 64 * h:64 * h + 64]
    for t, (b0, h0) in ((0, (0, 0)), (K + 5, (1, 2)), (L - 1, (0, 1))):     # the first tile, inside a tile, the one-key tail
        k2 = k.clone()
        k2[b0, t, 64 * h0 + 7] = float("nan")
        got = run_abi(q, k2, v, up)
        for b in range(B):
            for h in range(H):
                for n in NAMES:
                    a, c = per_head(n, got[n], b, h), per_head(n, clean[n], b, h)
                    if (b, h) == (b0, h0):
                        assert bool(torch.isnan(a).all()), (n, t, b, h)
                    else:
                        assert torch.equal(a, c), (n, t, b, h)


def test_two_runs_and_a_row_alone_agree_bit_for_bit(monkeypatch):
    dtype, L = torch.bfloat16, long_length()
    q, k, v, up = draw(13, L, dtype)
    poison_allocations(monkeypatch)
    a, b = run_abi(q, k, v, up), run_abi(q, k, v, up)
    for n in NAMES:
        assert torch.equal(a[n], b[n]), n
    for row in range(B):
        alone = run_abi(*(t[row:row + 1].contiguous() for t in (q, k, v, up)))
        for n in NAMES:
            assert torch.equal(alone[n][0], a[n][row]), (n, row)


def test_forward_and_backward_captured_into_one_graph_replay_the_eager_bits():
    dtype, L = torch.bfloat16, long_length()
    q, k, v, up = draw(17, L, dtype)
    eager = run_function(q, k, v, up)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]

    def step():
        ctx = mmfs_amd.clip_attention(*leaves, H)
        return (ctx.detach(),) + torch.autograd.grad(ctx, leaves, up)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(3):
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for n, t in zip(("context", "dq", "dk", "dv"), outs):
            assert torch.equal(t, eager[n]), n


def test_no_tensor_of_size_l_squared():
    """B = 1, H = 2, L = 2048, bf16: the two heads' scores in T are 16 MiB; q, k, v, dO and the context, dq, dk, dv are 512 KiB
    each, lse and delta 16 KiB each.  The kernel route's rise above the inputs stays under its own tensors -- the context, dq, dk,
    dv, autograd's sums of the three gradients (q, k and v are one leaf here), lse and delta -- plus a fixed 1 MiB; the framework
    statement's does not stay under the scores."""
    dtype, L, heads = torch.bfloat16, 2048, 2
    q, k, v, up = draw(19, L, dtype, B=1, H=heads)
    one = q.numel() * q.element_size()
    small = heads * L * 4
    scores = heads * L * L * 2
    budget = 7 * one + 2 * small + (1 << 20)
    m = module(dtype, heads=heads)
    m.q_proj, m.k_proj, m.v_proj, m.out_proj = (torch.nn.Identity() for _ in range(4))

    def rise(route):
        leaf = q.clone().requires_grad_(True)
        m.route = route
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out, _ = m(leaf)
        torch.autograd.grad(out, leaf, up)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    rise("kernels")                                                         # (the library's first call)
    kernels, framework = rise("kernels"), rise("framework")
    print(f"peak rise: kernels {kernels / 2 ** 20:.2f} MiB (budget {budget / 2 ** 20:.2f}), framework ops {framework / 2 ** 20:.1f} MiB, "
          f"scores {scores / 2 ** 20:.0f} MiB")
    assert kernels <= budget < scores < framework


def test_the_backward_is_linear_in_the_upstream_gradient_and_the_forward_in_v(monkeypatch):
    """bf16: backward(2^k dO) is 2^k backward(dO) and the context of 2^k v is 2^k times the context, bit for bit, for k = -20 and
    +20 (a power of two moves no significand, and bf16's exponent range is fp32's)."""
    dtype = torch.bfloat16
    q, k, v, up = draw(41, long_length(), dtype)
    poison_allocations(monkeypatch)
    clean = run_abi(q, k, v, up)
    for e in (-20, 20):
        scaled = lambda t: (t.float() * 2.0 ** e).to(dtype)
        got = run_abi(q, k, v, scaled(up))
        for n in ("dq", "dk", "dv"):
            assert bool(torch.isfinite(got[n]).all()) and torch.equal(got[n], scaled(clean[n])), (n, e)
        assert torch.equal(got["context"], clean["context"]) and torch.equal(got["lse"], clean["lse"]), e
        wide = run_abi(q, k, scaled(v), up)
        assert torch.equal(wide["context"], scaled(clean["context"])) and torch.equal(wide["lse"], clean["lse"]), e
