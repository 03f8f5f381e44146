"""The inference-only fp8 value bank on the device (include/mmfs_msda.h "fp8 bank"): the quantiser kernel is bit-identical to
the torch rule and deterministic, the row-gather forward and the fused sampler on an e4m3 bank with its scales stay within
the per-element fp64 bound of the dequantised bank, the shared-bank maps are bit-exact, and the modules / graphs that keep
projections take the opt-in."""
import contextlib
import io
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mm-interleaved_amd"), os.path.join(ROOT, "tests")]

import MultiScaleDeformableAttention as MSDA  # noqa: E402
from helpers import assert_within_bounds, level_tables  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def codes(q):
    return q.view(torch.uint8)


def edge_bank(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * torch.logspace(-5, 1, shape[-3]).view(-1, 1, 1)
    x[..., 0, :, 3] = 0.0                                   # zero columns
    x[..., 1, 0, 5] = -0.0
    x[..., 2, 0, 6] = 3.0e3                                 # a column maximum
    x[..., 4, 0, 6] = -3.0e3 * (1 - 2 ** -9)
    x.view(-1)[7::97] = float("nan")                        # non-finite elements
    x.view(-1)[11::131] = float("inf")
    x.view(-1)[13::151] = float("-inf")
    return x.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 37, 4, 32), (1, 5, 8, 64), (3, 300, 2, 128), (13, 2, 21, 1, 96)])
def test_quantizer_is_the_torch_rule_bit_for_bit(dtype, shape):
    for seed, x in enumerate((torch.randn(*shape).to(dtype), edge_bank(shape, dtype, 5))):
        want_q, want_s = MSDA.quantize_bank_fp8_reference(x)
        xd = x.to(DEV)
        q, s = MSDA.quantize_bank_fp8(xd)
        assert q.dtype == F8 and s.dtype == torch.float32 and q.shape == x.shape
        assert torch.equal(s.cpu(), want_s), (dtype, shape, seed)
        assert torch.equal(codes(q).cpu(), codes(want_q)), (dtype, shape, seed)
        q2, s2 = MSDA.quantize_bank_fp8(xd)
        assert torch.equal(codes(q2), codes(q)) and torch.equal(s2, s)


def test_thirteen_banks_in_one_launch_are_each_bank_alone():
    x = torch.randn(13, 2, 84, 4, 32, device=DEV, dtype=torch.bfloat16) * 3
    MSDA._event_log = []
    try:
        q, s = MSDA.quantize_bank_fp8(x)
        launches = [n for n, _, _ in MSDA._event_log]
    finally:
        MSDA._event_log = None
    assert launches == ["bank_quantize_fp8"]
    for k in (0, 6, 12):
        qk, sk = MSDA.quantize_bank_fp8(x[k].clone())
        assert torch.equal(codes(q[k]), codes(qk)) and torch.equal(s[k], sk)


# ---------------------------------------------------------------- the op forward on an fp8 bank
def op_case(B, H, D, Nq, P, shapes, n, dtype, seed, zero_frac=0.2, nan=False):
    g = torch.Generator().manual_seed(seed)
    sh, start = level_tables(shapes * n)
    S, L = int(sh.prod(1).sum()), sh.shape[0]
    x = torch.randn(B, S, H, D, generator=g) * torch.rand(1, 1, H, D, generator=g) * 4
    if nan:
        x.view(-1)[17::1009] = float("nan")
    q, s = MSDA.quantize_bank_fp8(x.to(DEV))
    loc = torch.rand(B, Nq, H, L, P, 2, generator=g) * 1.3 - 0.15              # samples out of range too
    attn = torch.rand(B, Nq, H, L, P, generator=g) + 1e-5
    attn = attn / attn.sum((-1, -2), keepdim=True)
    if zero_frac:
        attn[torch.rand(attn.shape, generator=g) < zero_frac] = 0.0            # zero weights
        attn[0, :3] = 0.0                                                      # whole outputs with A = 0
    rt = lambda t: t.to(dtype).double()
    xin = dict(value=MSDA.dequantize_bank_fp8(q, s, torch.float64).cpu(), shapes=sh, start=start, loc=rt(loc),
               attn=rt(attn), grad=torch.zeros(B, Nq, H * D, dtype=torch.float64))
    dev = dict(q=q, s=s, shapes=sh.to(DEV), start=start.to(DEV), loc=loc.to(DEV, dtype), attn=attn.to(DEV, dtype))
    return xin, dev


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("P", [4, 8])
def test_op_forward_fp8_within_the_bound_of_the_dequantised_bank(dtype, D, P):
    shapes, n = ([(16, 16), (8, 8), (4, 4), (2, 2)], 1) if D != 64 else ([(8, 8), (4, 4)], 2)
    x, d = op_case(2, 4, D, 70, P, shapes, n, dtype, seed=D + P)
    out = MSDA.ms_deform_attn_forward(d["q"], d["shapes"], d["start"], d["loc"], d["attn"], 1, value_scale=d["s"])
    assert out.dtype == dtype and out.shape == (2, 70, 4 * D)
    assert_within_bounds([out.double().cpu(), None, None, None], x, dtype, f"fp8 {dtype} D={D} P={P}", outputs=("out",))
    assert (out[0, :3] == 0).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_op_forward_fp8_nan_exactly_where_the_oracle_is_not_finite(dtype):
    from oracle import msda_oracle
    x, d = op_case(2, 4, 64, 96, 4, [(16, 16), (8, 8), (4, 4)], 1, dtype, seed=3, zero_frac=0.0, nan=True)
    out = MSDA.ms_deform_attn_forward(d["q"], d["shapes"], d["start"], d["loc"], d["attn"], 1, value_scale=d["s"])
    ref = np.asarray(msda_oracle.forward(x["value"], x["shapes"], x["start"], x["loc"], x["attn"])).reshape(out.shape)
    bad = ~np.isfinite(ref)
    assert bad.any() and not bad.all()
    assert np.array_equal(torch.isnan(out).cpu().numpy(), bad)
    assert_within_bounds([out.double().cpu(), None, None, None], x, dtype, "fp8 nan", outputs=("out",))


def test_op_forward_fp8_refused_head_width_takes_the_dequantised_path():
    x, d = op_case(1, 2, 48, 33, 4, [(8, 8), (4, 4)], 1, torch.bfloat16, seed=9)
    out = MSDA.ms_deform_attn_forward(d["q"], d["shapes"], d["start"], d["loc"], d["attn"], 1, value_scale=d["s"])
    want = MSDA.ms_deform_attn_forward(MSDA.dequantize_bank_fp8(d["q"], d["s"], torch.bfloat16), d["shapes"], d["start"],
                                       d["loc"], d["attn"], 1)
    assert torch.equal(out, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Bv,g,lay", [(1, 2, "tile"), (3, 2, "interleave"), (2, 5, "interleave"), (3, 5, "tile")])
def test_shared_map_on_an_fp8_bank_equals_the_expanded_bank(dtype, Bv, g, lay):
    x, d = op_case(Bv, 4, 64, 40, 8, [(8, 8), (4, 4), (2, 2)], 2, dtype, seed=Bv * 10 + g)
    gen = torch.Generator().manual_seed(g)
    B = Bv * g
    loc = (torch.rand(B, 40, 4, 6, 8, 2, generator=gen) * 1.2 - 0.1).to(DEV, dtype)
    attn = (torch.rand(B, 40, 4, 6, 8, generator=gen) / 48).to(DEV, dtype)
    exp = (lambda t: torch.cat([t] * g)) if lay == "tile" else (lambda t: t.repeat_interleave(g, 0))
    got = MSDA.ms_deform_attn_forward(d["q"], d["shapes"], d["start"], loc, attn, 1, value_repeat=lay, value_scale=d["s"])
    want = MSDA.ms_deform_attn_forward(exp(codes(d["q"])).view(F8), d["shapes"], d["start"], loc, attn, 1,
                                       value_scale=exp(d["s"]))
    assert torch.equal(got, want)


def test_gradients_through_an_fp8_bank_raise():
    from mmfs_amd.functions import MSDeformAttnFunction
    _, d = op_case(1, 2, 32, 8, 4, [(4, 4)], 1, torch.float32, seed=1)
    loc = d["loc"].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        MSDeformAttnFunction.apply(d["q"], d["shapes"], d["start"], loc, d["attn"], 1, False, None, d["s"])
    with torch.no_grad():
        out = MSDeformAttnFunction.apply(d["q"], d["shapes"], d["start"], loc, d["attn"], 1, False, None, d["s"])
    assert out.dtype == torch.float32


# ---------------------------------------------------------------- the fused sampler (MMFS module)
def _mmfs(dtype):
    from mmfs_amd.modules import MMFS
    torch.manual_seed(0)
    m = MMFS(d_model=128, d_query=64, d_value=96, n_levels=3, n_heads=4, n_points=4,
             spatial_shapes=[8, 4, 2], base_spatial_shape=4, max_num_image_per_seq=8)
    with torch.no_grad():
        m.sampling_offsets.weight.normal_(0, 0.05)
        m.attention_weights.weight.normal_(0, 0.05)
        m.ignore_token.normal_(0, 0.1)
    return m.to(DEV, dtype).eval()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Lq", [37, 1])
@pytest.mark.parametrize("lay", [None, "interleave"])
def test_fused_sampler_fp8_equals_plan_plus_op(dtype, Lq, lay):
    from mmfs_amd.functions.mmfs_plan_func import sample_forward_groups
    from mmfs_amd.levels import make_level_tables
    m = _mmfs(dtype)
    n, hw, Bv = 2, 84, 2
    g = 3 if lay else 1
    sh, start, _ = make_level_tables([(8, 8), (4, 4), (2, 2)], n, DEV)
    gen = torch.Generator(device=DEV).manual_seed(Lq)
    q = torch.randn(Bv * g, Lq, 64, generator=gen, device=DEV).to(dtype)
    ref = torch.rand(Bv * g, Lq, 1, 2, generator=gen, device=DEV)
    feats = torch.randn(Bv, n, hw, 96, generator=gen, device=DEV).to(dtype)
    mask = torch.ones(Bv * g, n, device=DEV)
    mask[-1, 1] = 0
    with torch.no_grad():
        v8, sc = MSDA.quantize_bank_fp8(m.value_proj(feats).view(Bv, n * hw, 1, 128))
        v8 = v8.view(Bv, n, hw, 128)
        m.fused_sampler = True
        got = m(q, ref, feats, sh, start, attention_mask=mask, value=v8, value_scale=sc, bank_repeat=lay)
        m.fused_sampler = False
        want = m(q, ref, feats, sh, start, attention_mask=mask, value=v8, value_scale=sc, bank_repeat=lay)
    assert got.dtype == dtype
    groups = sample_forward_groups(F8, Lq, 32, 3 * n, 4)
    if groups == 1:
        assert torch.equal(got, want)
    else:
        assert Lq == 1 and groups > 1
        u = {torch.float32: 2 ** -23, torch.float16: 2 ** -10, torch.bfloat16: 2 ** -7}[dtype]
        # the pre-projection output differs by one rounding; the output projection spreads it over d_model columns
        tol = 8 * u * float(want.abs().max())
        assert float((got.float() - want.float()).abs().max()) <= tol


# ---------------------------------------------------------------- modules and graphs
def _net(dtype):
    from mmfs_amd.blocks import MMFSNet
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        net = MMFSNet(input_channel=64, block_out_channels=[32, 64], layers_per_block=1, downsample_factor=2,
                      n_levels=3, n_points=8, gradient_checkpointing=True, spatial_shapes=[16, 8, 4])
    with torch.no_grad():
        for blk in net._blocks():
            blk.conv.weight.normal_(0, 0.02)
            blk.mmfs.sampling_offsets.weight.normal_(0, 0.01)
            blk.feat_norm.weight.uniform_(0.5, 1.5)
    return net.to(DEV, dtype).eval()


def _net_inputs(B, Bv, dtype):
    chans, sides = [32, 32, 32, 64], [8, 8, 8, 4]
    gen = torch.Generator(device=DEV).manual_seed(1)
    res = [torch.randn(B, c, s, s, generator=gen, device=DEV).to(dtype) for c, s in zip(chans, sides)]
    mid = torch.randn(B, 64, 4, 4, generator=gen, device=DEV).to(dtype)
    feats = [torch.randn(Bv, 1, 64, s, s, generator=gen, device=DEV).to(dtype) for s in (16, 8, 4)]
    return mid, res, feats, torch.ones(B, 1, device=DEV, dtype=torch.long)


def _flat(o):
    return (o[0],) + tuple(o[1])


def test_mmfs_net_keeps_an_fp8_bank_and_graphs_it():
    from mmfs_amd.graphs import GraphedMMFSNet
    dtype = torch.bfloat16
    net = _net(dtype)
    Bv, B = 2, 4
    mid, res, feats, mask = _net_inputs(B, Bv, dtype)
    with torch.no_grad():
        want = net(mid, res, feats, mask, bank_repeat="tile")
        base = net.__dict__["_projected"]
        assert base.scales is None
        net.kept_bank_dtype = F8
        got = net(mid, res, feats, mask, bank_repeat="tile")
        proj = net.__dict__["_projected"]
        assert proj.scales is not None and len(proj.scales) == len(proj.values) == 5
        assert all(v.dtype == F8 and v.element_size() == 1 and v.shape[0] == Bv for v in proj.values)
        # each kept bank is the rule applied to the 16-bit projection
        for v, s, v16 in zip(proj.values, proj.scales, base.values):
            rq, rs = MSDA.quantize_bank_fp8_reference(v16.reshape(Bv, -1, 1, v16.shape[-1]).cpu())
            assert torch.equal(s.cpu(), rs) and torch.equal(codes(v).reshape(rq.shape).cpu(), codes(rq))
        again = net(mid, res, feats, mask, bank_repeat="tile")
        assert net.__dict__["_projected"] is proj
        graphed = GraphedMMFSNet(net, mid, res, feats, mask, bank_repeat="tile")
        assert graphed._proj.scales is not None
        replay = graphed(mid, res)
    for x, x2, y in zip(_flat(got), _flat(again), _flat(replay)):
        assert torch.equal(x, x2) and torch.equal(x, y)
    # against the 16-bit bank: each block adds its sampled term to its input; the term moves by at most the bank's
    # quantisation error (2^-4 relative) carried through the output projection and the 1x1 convolution
    for x, y, r in zip(_flat(got), _flat(want), (mid,) + tuple(res)):
        term = (y.float() - r.float()).abs().max()
        assert float((x.float() - y.float()).abs().max()) <= 2 ** -3 * float(term) + 2 ** -7 * float(y.abs().max())
    net.kept_bank_dtype = None


def test_mmfs_net_never_quantises_under_gradients():
    net = _net(torch.float32)
    net.kept_bank_dtype = F8
    mid, res, feats, mask = _net_inputs(2, 2, torch.float32)
    with torch.no_grad():
        proj = net.project_features(feats, bank_dtype=F8)
    assert all(v.dtype == F8 for v in proj.values)
    feats = [f.requires_grad_(True) for f in feats]
    out = net(mid, res, feats, mask)                       # eval but grad mode: no cache, no fp8
    assert "_projected" not in net.__dict__
    out[0].sum().backward()
    assert feats[0].grad is not None
    with pytest.raises(RuntimeError, match="inference only"):
        net.project_features(feats, bank_dtype=F8)


@pytest.mark.parametrize("Lq", [1, 17])
def test_llama_schedule_fp8_interleave_with_five_beams_and_its_graph(Lq):
    from mmfs_amd.blocks import LlamaMMFSAttention, LlamaMMFSSchedule
    from mmfs_amd.graphs import GraphedLlamaMMFSStack
    cfg = types.SimpleNamespace(hidden_size=512, num_attention_heads=8, rms_norm_eps=1e-6,
                                max_position_embeddings=64, image_embed_dim=128, spatial_shapes=[8, 4, 2])
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        layers = [LlamaMMFSAttention(cfg, 4 * i).to(DEV, torch.bfloat16).eval() for i in range(3)]
    with torch.no_grad():
        for l in layers:
            l.gate.fill_(0.7)
            l.attn.sampling_offsets.weight.normal_(0, 0.02)
            l.norm2.weight.uniform_(0.5, 1.5)
    Bv, g, n, hw = 2, 5, 2, 64 + 16 + 4
    hidden = torch.randn(Bv * g, Lq, 512, device=DEV, dtype=torch.bfloat16)
    feats = torch.randn(Bv, n, hw, 128, device=DEV, dtype=torch.bfloat16)
    mask = torch.ones(Bv * g, Lq, n, device=DEV)
    mask[3, :, 1] = 0
    with torch.no_grad():
        sched = LlamaMMFSSchedule(layers)
        b16 = sched.project(feats, bank_repeat="interleave")
        sched.kept_bank_dtype = F8
        b8 = sched.project(feats, bank_repeat="interleave")
        assert b8 is not b16 and b8.scales is not None and sched.project(feats, bank_repeat="interleave") is b8
        assert all(v.dtype == F8 and v.element_size() == 1 and v.shape[0] == Bv for v in b8.values)
        h8 = h16 = hidden
        for k, l in enumerate(layers):
            h8 = l(h8, feats, mask, value=b8.values[k], value_scale=b8.scales[k], bank_repeat="interleave", residual=h8)
            h16 = l(h16, feats, mask, value=b16.values[k], bank_repeat="interleave", residual=h16)
        # expanded fp8 bank: the same bits
        hx = hidden
        for k, l in enumerate(layers):
            hx = l(hx, feats.repeat_interleave(g, 0), mask, value=b8.values[k].repeat_interleave(g, 0),
                   value_scale=b8.scales[k].repeat_interleave(g, 0), residual=hx)
        graphed = GraphedLlamaMMFSStack(layers, hidden, b8, mask)
        replay = graphed(hidden)
    assert torch.equal(h8, hx)
    assert torch.equal(replay, h8)
    delta = (h16.float() - hidden.float()).abs().max()
    assert float((h8.float() - h16.float()).abs().max()) <= 2 ** -3 * float(delta) + 2 ** -7 * float(h16.abs().max())
