"""The LLM's self-attention in training on the device (csrc/mmfs_llama_train.hip), through the C ABI's entries
(mmfs_amd.functions.llama_train_func.train_rope / train_forward / train_backward), the autograd.Function and
LlamaSelfAttention's training route.

``q_rot``, ``k_rot``, ``context``, ``lse``, ``dq``, ``dk``, ``dv`` are held element by element to fp64 on the stored
inputs under the bounds of the kernel file's header (tests/llama_train_refs.py states them; tests/test_llama_train.py shows
that the framework's statement meets them and four defective ones do not), and the context and the three gradients row
by row to a tight relative measure (``row_error``; the same file shows, at exactly these inputs, the defects it refuses).  Outputs are poisoned before the kernels run:
an element nobody wrote is NaN.

Worst bound ratios measured on an MI355X are kept in profiles/llama_attn.md, "Training"."""
import types

import pytest
import torch
from torch import nn
from torch.utils.checkpoint import checkpoint

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


def tables():
    if "t" not in _tables:
        _tables["t"] = rope_table(128, MAX_POS, device=DEV)
    return _tables["t"]


def run_abi(q, k, v, up, pos, heads=H):
    """the three entries one after the other, as the Function calls them"""
    f = func()
    cos, sin = tables()
    q_rot, k_rot = f.train_rope(q, k, pos, cos, sin, heads)
    ctx, lse = f.train_forward(q_rot, k_rot, v, heads)
    dq, dk, dv = f.train_backward(q_rot, k_rot, v, ctx, up, lse, pos, cos, sin, heads)
    torch.cuda.synchronize()
    return dict(zip(NAMES, (q_rot, k_rot, ctx, lse, dq, dk, dv)))


def run_function(q, k, v, up, pos, heads=H):
    cos, sin = tables()
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
