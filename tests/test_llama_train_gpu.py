"""The LLM's self-attention in training on the device (csrc/mmfs_llama_train.hip), through the C ABI's entries
(mmfs_amd.functions.llama_train_func.train_rope / train_forward / train_backward), the autograd.Function and
LlamaSelfAttention's training route.

``q_rot``, ``k_rot``, ``context``, ``lse``, ``dq``, ``dk``, ``dv`` are held element by element to fp64 on the stored
inputs under the bounds of the kernel file's header (tests/llama_train_refs.py states them; tests/test_llama_train.py shows
that the framework's statement meets them and four defective ones do not), and the context and the three gradients row
by row to a tight relative measure (``row_error``; the same file shows, at exactly these inputs, the defects it refuses).  Outputs are poisoned before the kernels run:
an element nobody wrote is NaN.

Peaked, drifting and sink score rows (tests/attn_score_families.py; tests/test_attn_families.py shows on the host what they
catch that unit-normal rows let pass), a walk over nine query tiles, positions outside the rotary table and the backward's
linearity in dO follow the unit-normal tests.

Worst bound ratios measured on an MI355X are kept in profiles/llama_attn.md, "Training"."""
import types

import pytest
import torch
from torch import nn
from torch.utils.checkpoint import checkpoint

from attn_score_families import TRAIN_FAMILIES, WALK_FAMILY, train_inputs
from helpers import poison_allocations
from llama_train_refs import draw as refs_draw, tight_ratios, train64, worst

import mmfs_amd
from mmfs_amd.llama_attn import LlamaSelfAttention, rope_table

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.bfloat16, torch.float16]
B, H = 2, 3
MAX_POS = 512
NAMES = ("q_rot", "k_rot", "context", "lse", "dq", "dk", "dv")


def func():
    from mmfs_amd.functions import llama_train_func
    return llama_train_func


def lengths():
    Q, K = func().TRAIN_TILES[:2]
    return [1, 2, K - 1, K, K + 1, Q - 1, Q, Q + 1, 2 * Q + K // 2 + 3]


def pytest_generate_tests(metafunc):
    if "L" in metafunc.fixturenames:                                        # (the tile sizes come from the library)
        metafunc.parametrize("L", lengths())


def draw(seed, L, dtype, B=B, H=H, first=5):
    # every position inside the table (the framework's statement indexes it unchecked)
    q, k, v, up, pos = refs_draw(seed, L, dtype, B, H, first=first, device=DEV)
    assert int(pos.max()) < max(MAX_POS, L)
    return q, k, v, up, pos


_tables = {}


def tables(max_pos=MAX_POS):
    if max_pos not in _tables:
        _tables[max_pos] = rope_table(128, max_pos, device=DEV)
    return _tables[max_pos]


def run_abi(q, k, v, up, pos, heads=H, max_pos=MAX_POS):
    """the three entries one after the other, as the Function calls them"""
    f = func()
    cos, sin = tables(max_pos)
    q_rot, k_rot = f.train_rope(q, k, pos, cos, sin, heads)
    ctx, lse = f.train_forward(q_rot, k_rot, v, heads)
    dq, dk, dv = f.train_backward(q_rot, k_rot, v, ctx, up, lse, pos, cos, sin, heads)
    torch.cuda.synchronize()
    return dict(zip(NAMES, (q_rot, k_rot, ctx, lse, dq, dk, dv)))


def run_function(q, k, v, up, pos, heads=H, max_pos=MAX_POS):
    cos, sin = tables(max_pos)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    ctx = mmfs_amd.llama_attn_train(*leaves, pos, cos, sin, heads)
    grads = torch.autograd.grad(ctx, leaves, up)
    torch.cuda.synchronize()
    return dict(zip(("context", "dq", "dk", "dv"), (ctx.detach(),) + grads))


class Fixed(nn.Module):
    def __init__(self, t):
        super().__init__()
        self.t = t

    def forward(self, x):
        return self.t


def bare_module(leaves, heads=H):
    """a training-mode LlamaSelfAttention whose projections hand out q, k, v and whose o_proj is the identity"""
    cfg = types.SimpleNamespace(hidden_size=heads * 128, num_attention_heads=heads, max_position_embeddings=MAX_POS)
    m = LlamaSelfAttention(cfg).train()
    m.q_proj, m.k_proj, m.v_proj, m.o_proj = Fixed(leaves[0]), Fixed(leaves[1]), Fixed(leaves[2]), nn.Identity()
    return m


def run_module(q, k, v, up, pos, route=None, heads=H, wrap=None):
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    m = bare_module(leaves, heads)
    m.route = route
    hidden = torch.zeros_like(q).requires_grad_(True)                       # (a checkpoint wants an input that requires grad)
    mask = torch.ones(q.shape[:2], device=DEV)
    call = lambda h: m(h, attention_mask=mask, position_ids=pos)[0]
    ctx = call(hidden) if wrap is None else wrap(call, hidden)
    grads = torch.autograd.grad(ctx, leaves, up)
    torch.cuda.synchronize()
    return m, dict(zip(("context", "dq", "dk", "dv"), (ctx.detach(),) + grads))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_every_output_holds_its_bound(L, dtype, monkeypatch):
    q, k, v, up, pos = draw(100 + L, L, dtype)
    cos, sin = tables()
    ref = train64(q, k, v, pos, cos.cpu(), sin.cpu(), H, dtype, upstream=up)
    poison_allocations(monkeypatch)
    abi = run_abi(q, k, v, up, pos)
    fn = run_function(q, k, v, up, pos)
    ratios = {n: worst(abi[n], ref[n], ref["E_" + n]) for n in NAMES}
    print(f"L {L} {dtype}: worst |got - ref| / bound " + ", ".join(f"{n} {x:.3f}" for n, x in ratios.items()))
    tight = tight_ratios(abi, ref, dtype)
    print(f"L {L} {dtype}: worst row error / (8 u (|row| + share + floor)) " + ", ".join(f"{n} {x:.3f}" for n, x in tight.items()))
    assert max(ratios.values()) <= 1.0, ratios
    assert max(tight.values()) <= 1.0, tight
    for n in fn:                                                            # the Function is the three entries
        assert torch.equal(fn[n], abi[n]), n


def test_the_module_route_is_the_function_bit_for_bit():
    dtype, L = torch.bfloat16, lengths()[-1]
    q, k, v, up, pos = draw(7, L, dtype)
    fn = run_function(q, k, v, up, pos)
    before = dict(func().launches)
    m, got = run_module(q, k, v, up, pos)
    assert (m.last_route, m.last_reason, m.last_train) == ("kernels", None, "kernel")
    assert {n: func().launches[n] - before[n] for n in before} == {"rope": 1, "forward": 1, "backward": 2}
    for n in fn:
        assert torch.equal(got[n], fn[n]), n
    # forced to the framework's statement: no launch, the same numbers to the bounds
    before = dict(func().launches)
    m, fw = run_module(q, k, v, up, pos, route="framework")
    assert (m.last_route, m.last_train) == ("framework", "framework ops") and func().launches == before
    cos, sin = tables()
    ref = train64(q, k, v, pos, cos.cpu(), sin.cpu(), H, dtype, upstream=up)
    for n in fw:
        assert worst(fw[n], ref[n], ref["E_" + n]) <= 1.0, n
    # forced to the kernels where they do not apply
    with pytest.raises(RuntimeError, match="route='kernels'"):
        run_module(q.float(), k.float(), v.float(), up.float(), pos, route="kernels")
    m, _ = run_module(q.float(), k.float(), v.float(), up.float(), pos)
    assert (m.last_route, m.last_reason, m.last_train) == ("framework", "tensors the kernels do not serve", "framework ops")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        m, _ = run_module(q, k, v, up, pos)
    assert (m.last_route, m.last_reason) == ("framework", "autocast")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_causality_by_poison(dtype):
    Q, K = func().TRAIN_TILES[:2]
    L = 2 * Q + K // 2 + 3
    q, k, v, up, pos = draw(11, L, dtype)
    clean = run_abi(q, k, v, up, pos)
    for t in (K, Q, K + 5, Q + K + 17, 1, L - 1):                           # on a tile's edge, inside a tile, the ends
        # a NaN in token t's k and v reaches no earlier query
        k2, v2 = k.clone(), v.clone()
        k2[:, t] = float("nan")
        v2[:, t] = float("nan")
        got = run_abi(q, k2, v2, up, pos)
        assert torch.equal(got["context"][:, :t], clean["context"][:, :t]), t
        assert torch.equal(got["lse"][:, :, :t], clean["lse"][:, :, :t]), t
        assert bool(torch.isnan(got["context"][:, t:]).all()), t
        # a NaN in query j's upstream gradient reaches no later key
        j = t - 1 if t == L - 1 else t
        up2 = up.clone()
        up2[:, j] = float("nan")
        got = run_abi(q, k, v, up2, pos)
        for n in ("dk", "dv"):
            assert torch.equal(got[n][:, j + 1:], clean[n][:, j + 1:]), (n, j)
            assert bool(torch.isnan(got[n][:, :j + 1]).all()), (n, j)
        assert torch.equal(torch.cat((got["dq"][:, :j], got["dq"][:, j + 1:]), 1),
                           torch.cat((clean["dq"][:, :j], clean["dq"][:, j + 1:]), 1)), j


def test_two_runs_and_a_row_alone_agree_bit_for_bit(monkeypatch):
    dtype, L = torch.bfloat16, lengths()[-1]
    q, k, v, up, pos = draw(13, L, dtype)
    poison_allocations(monkeypatch)
    a, b = run_abi(q, k, v, up, pos), run_abi(q, k, v, up, pos)
    for n in NAMES:
        assert torch.equal(a[n], b[n]), n
    for row in range(B):
        alone = run_abi(*(t[row:row + 1].contiguous() for t in (q, k, v, up, pos)))
        for n in NAMES:
            assert torch.equal(alone[n][0], a[n][row]), (n, row)


def test_rope_forward_and_backward_captured_into_one_graph_replay_the_eager_bits():
    dtype, L = torch.bfloat16, lengths()[-1]
    q, k, v, up, pos = draw(17, L, dtype)
    cos, sin = tables()
    eager = run_function(q, k, v, up, pos)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]

    def step():
        ctx = mmfs_amd.llama_attn_train(*leaves, pos, cos, sin, H)
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
    """B = 1, H = 1, L = 4096, bf16: one score tensor in T is 32 MiB; the route's own tensors are 1 MiB each"""
    dtype, L = torch.bfloat16, 4096
    q, k, v, up, pos = draw(19, L, dtype, B=1, H=1, first=0)
    line = L * L * 2

    def rise(route):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        run_module(q, k, v, up, pos, route=route, heads=1)
        return torch.cuda.max_memory_allocated() - before

    rise(None)                                                              # (the rotary table and the library's first call)
    kernels, framework = rise(None), rise("framework")
    print(f"peak rise: kernels {kernels / 2 ** 20:.1f} MiB, framework ops {framework / 2 ** 20:.1f} MiB, line {line / 2 ** 20:.0f} MiB")
    assert kernels < line < framework


def test_a_checkpointed_call_gives_the_same_gradients():
    dtype, L = torch.bfloat16, lengths()[-1]
    q, k, v, up, pos = draw(23, L, dtype)
    _, plain = run_module(q, k, v, up, pos)
    m, again = run_module(q, k, v, up, pos, wrap=lambda call, h: checkpoint(call, h, use_reentrant=False))
    assert m.last_train == "kernel"
    for n in plain:
        assert torch.equal(plain[n], again[n]), n


# ------------------------------------------------------------------ peaked, drifting and sink rows; the long walk
FB, FH, FSEED = 1, 2, 5                                 # tests/test_attn_families.py's: the host model is held at these very inputs
WALK_MAX_POS = 2048


def family_length():
    Q, K = func().TRAIN_TILES[:2]
    return 2 * Q + K // 2 + 3


def walk_length():
    Q, K = func().TRAIN_TILES[:2]
    return 8 * Q + K + 5


def hold_both_measures(name, L, dtype, monkeypatch, max_pos=MAX_POS):
    q, k, v, up, pos = train_inputs(name, FSEED, L, dtype, FB, FH, device=DEV)
    assert 0 <= int(pos.min()) and int(pos.max()) < max_pos
    cos, sin = tables(max_pos)
    ref = train64(q, k, v, pos, cos.cpu(), sin.cpu(), FH, dtype, upstream=up)
    poison_allocations(monkeypatch)
    abi = run_abi(q, k, v, up, pos, FH, max_pos)
    fn = run_function(q, k, v, up, pos, FH, max_pos)
    ratios = {n: worst(abi[n], ref[n], ref["E_" + n]) for n in NAMES}
    tight = tight_ratios(abi, ref, dtype)
    print(f"{name} L {L} {dtype}: lse {float(ref['lse'].min()):.1f} .. {float(ref['lse'].max()):.1f}; worst |got - ref| / bound " +
          ", ".join(f"{n} {x:.3f}" for n, x in ratios.items()))
    print(f"{name} L {L} {dtype}: worst row error / (8 u (|row| + share + floor)) " + ", ".join(f"{n} {x:.3f}" for n, x in tight.items()))
    assert max(ratios.values()) <= 1.0, ratios
    assert max(tight.values()) <= 1.0, tight
    for n in fn:                                                            # the Function is the three entries
        assert torch.equal(fn[n], abi[n]), n


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("name", TRAIN_FAMILIES, ids=lambda n: n.replace(" ", "_"))
def test_peaked_drifting_and_sink_rows_hold_both_measures(name, dtype, monkeypatch):
    """every position 0, where the rotation is exact: a running maximum that rises by 19 or more a key tile and
    scores above 88.7 (``rising``), whole key tiles that underflow behind an early maximum (``falling``), one key with most of
    a row's weight (``sink``); lse reaches 105, so the backward's exp((K q^T - lse sqrt(128)) / sqrt(128)) starts its
    accumulators near -1190"""
    hold_both_measures(name, family_length(), dtype, monkeypatch)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("name", [WALK_FAMILY, "plain"], ids=lambda n: n.replace(" ", "_"))
def test_a_walk_over_nine_query_tiles_holds_both_measures(name, dtype, monkeypatch):
    """L = 8 Q + K + 5: the rising family at position 0 and the plain draw at real positions 5 .. L + 4"""
    hold_both_measures(name, walk_length(), dtype, monkeypatch, WALK_MAX_POS)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_a_position_outside_the_table_is_nan_from_that_token_on_and_nowhere_else(dtype, monkeypatch):
    """One token t of batch row 0 at position -1, MAX_POS or 2^40.  The expectation is the kernels' contract, not train64's:
    its matrix products turn 0 x NaN into NaN where the kernels select."""
    Q, K = func().TRAIN_TILES[:2]
    L = family_length()
    q, k, v, up, pos = draw(29, L, dtype, B=2, H=FH)
    poison_allocations(monkeypatch)
    clean = run_abi(q, k, v, up, pos, FH)
    assert all(bool(torch.isfinite(clean[n]).all()) for n in NAMES)
    for t in (0, K + 5, L - 1):
        for bad in (-1, MAX_POS, 1 << 40):
            pos2 = pos.clone()
            pos2[0, t] = bad
            got = run_abi(q, k, v, up, pos2, FH)
            where = (t, bad)
            for n in NAMES:                                                 # the other batch row
                assert torch.equal(got[n][1], clean[n][1]), (n, where)
            others = torch.arange(L, device=DEV) != t
            for n in ("q_rot", "k_rot"):
                assert bool(torch.isnan(got[n][0, t]).all()), (n, where)
                assert torch.equal(got[n][0, others], clean[n][0, others]), (n, where)
            for n in ("context", "dq"):
                assert torch.equal(got[n][0, :t], clean[n][0, :t]), (n, where)
                assert bool(torch.isnan(got[n][0, t:]).all()), (n, where)
            assert torch.equal(got["lse"][0, :, :t], clean["lse"][0, :, :t]), where
            for n in ("dk", "dv"):
                assert bool(torch.isnan(got[n][0]).all()), (n, where)


@pytest.mark.parametrize("name", ["plain", TRAIN_FAMILIES[0]], ids=lambda n: n.replace(" ", "_"))
def test_the_backward_is_linear_in_the_upstream_gradient_and_the_forward_in_v(name, monkeypatch):
    """bf16: backward(2^k dO) is 2^k backward(dO) and the context of 2^k v is 2^k times the context, bit for bit, for k = -20 and
    +20 (a power of two moves no significand, and bf16's exponent range is fp32's).  Not in fp16: at dO 2^-10 dS is subnormal
    there, and a host model of the kernels' roundings misses dk by 1.35 of the tight measure."""
    dtype = torch.bfloat16
    q, k, v, up, pos = train_inputs(name, FSEED, family_length(), dtype, FB, FH, device=DEV)
    poison_allocations(monkeypatch)
    clean = run_abi(q, k, v, up, pos, FH)
    for e in (-20, 20):
        scaled = lambda t: (t.float() * 2.0 ** e).to(dtype)
        got = run_abi(q, k, v, scaled(up), pos, FH)
        for n in ("dq", "dk", "dv"):
            assert bool(torch.isfinite(got[n]).all()) and torch.equal(got[n], scaled(clean[n])), (n, e)
        assert torch.equal(got["context"], clean["context"]) and torch.equal(got["lse"], clean["lse"]), e
        wide = run_abi(q, k, scaled(v), up, pos, FH)
        assert torch.equal(wide["context"], scaled(clean["context"])) and torch.equal(wide["lse"], clean["lse"]), e
