"""A shared value bank on the device (include/mmfs_msda.h MMFS_BANK_*): one bank of Bv rows serves B = g * Bv query rows --
classifier-free guidance's ``torch.cat([bank] * 2)`` ("tile"), beam search's ``repeat_interleave(num_beams, 0)``
("interleave").  The per-query arithmetic does not change, only the slab a query row reads from, so every comparison is
BIT-EXACT against the same formulation fed the expanded bank."""
import contextlib
import io
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mm-interleaved_amd")]

import MultiScaleDeformableAttention as MSDA  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (H, D, P, levels per image, images) of BASELINE's geometries, scaled down in B / Nq by the tests
GEOMS = {
    "north_star": (8, 128, 4, [(64, 64), (32, 32), (16, 16), (8, 8)], 1),
    "cfg2_sd_real": (16, 64, 8, [(64, 64), (32, 32), (16, 16), (8, 8)], 1),
    "cfg5_llm_n4": (16, 64, 8, [(32, 32), (16, 16), (8, 8)], 4),
}
MAPS = [(Bv, g, lay) for Bv in (1, 3) for g in (2, 5) for lay in ("tile", "interleave")]


def expand(t, g, lay):
    return torch.cat([t] * g) if lay == "tile" else t.repeat_interleave(g, 0)


def op_inputs(geom, Bv, B, Nq, dtype, seed=0):
    H, D, P, shapes, n = GEOMS[geom]
    gen = torch.Generator(device=DEV).manual_seed(seed)
    sh = torch.tensor(shapes * n, dtype=torch.long, device=DEV)
    start = torch.cat((sh.new_zeros(1), sh.prod(1).cumsum(0)[:-1]))
    S, L = int(sh.prod(1).sum()), sh.shape[0]
    value = torch.rand(Bv, S, H, D, generator=gen, device=DEV).to(dtype)
    loc = (torch.rand(B, Nq, H, L, P, 2, generator=gen, device=DEV) * 1.2 - 0.1).to(dtype)
    attn = torch.rand(B, Nq, H, L, P, generator=gen, device=DEV) + 1e-5
    attn = (attn / attn.sum((-1, -2), keepdim=True)).to(dtype)
    return value, sh, start, loc, attn


@pytest.fixture()
def fwd_algo():
    yield
    MSDA._fwd_algo = "auto"


@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.float64])
@pytest.mark.parametrize("algo", ["auto", "gather", "lds", "slices", "waves"])
def test_op_forward_equals_the_expanded_bank(geom, dtype, algo, fwd_algo):
    if dtype == torch.float64 and algo != "gather":
        pytest.skip("fp64 has the row gather only")
    MSDA._fwd_algo = algo
    ran = 0
    for Bv, g, lay in MAPS:
        value, sh, start, loc, attn = op_inputs(geom, Bv, Bv * g, 96, dtype, seed=Bv * 10 + g)
        try:
            want = MSDA.ms_deform_attn_forward(expand(value, g, lay), sh, start, loc, attn, 1)
        except RuntimeError as e:
            assert "unsupported" in str(e), e
            continue
        got = MSDA.ms_deform_attn_forward(value, sh, start, loc, attn, 1, value_repeat=lay)
        assert torch.equal(got, want), (geom, dtype, algo, Bv, g, lay)
        # the identity map through the new entry is today's call
        if g == 2 and lay == "tile":
            full = expand(value, g, lay)
            assert torch.equal(MSDA.ms_deform_attn_forward(full, sh, start, loc, attn, 1, value_repeat="interleave"), want)
        ran += 1
    if algo in ("auto", "gather") or (dtype in (torch.float16, torch.bfloat16) and algo != "waves") or \
            (algo == "waves" and dtype != torch.float32 and geom == "north_star"):
        assert ran == len(MAPS), f"{algo} refused a shape it supports"


def _mmfs(dtype, n_points=4, n_levels=3, d_model=128, n_heads=4):
    from mmfs_amd.modules import MMFS
    torch.manual_seed(0)
    m = MMFS(d_model=d_model, d_query=64, d_value=96, n_levels=n_levels, n_heads=n_heads, n_points=n_points,
             spatial_shapes=[8, 4, 2][:n_levels], base_spatial_shape=4, max_num_image_per_seq=8)
    with torch.no_grad():
        m.sampling_offsets.weight.normal_(0, 0.05)
        m.attention_weights.weight.normal_(0, 0.05)
        m.ignore_token.normal_(0, 0.1)
    return m.to(DEV, dtype).eval()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("Lq", [37, 1])          # Lq = 1: a decode step, the mmfs_sample_decode kernel
def test_fused_sampler_equals_the_expanded_bank(dtype, Lq):
    from mmfs_amd.levels import make_level_tables
    m = _mmfs(dtype)
    n = 2
    sh, start, _ = make_level_tables([(8, 8), (4, 4), (2, 2)], n, DEV)
    hw = 84
    for Bv, g, lay in MAPS:
        B = Bv * g
        gen = torch.Generator(device=DEV).manual_seed(B)
        q = torch.randn(B, Lq, 64, generator=gen, device=DEV).to(dtype)
        ref = torch.rand(B, Lq, 1, 2, generator=gen, device=DEV)
        feats = torch.randn(Bv, n, hw, 96, generator=gen, device=DEV).to(dtype)
        mask = torch.ones(B, n, device=DEV)
        mask[-1, 1] = 0
        with torch.no_grad():
            value = m.value_proj(feats)         # (one projection for both: fewer rows may take another GEMM kernel)
            got = m(q, ref, feats, sh, start, attention_mask=mask, value=value, bank_repeat=lay)
            want = m(q, ref, expand(feats, g, lay), sh, start, attention_mask=mask, value=expand(value, g, lay))
        assert torch.equal(got, want), (dtype, Lq, Bv, g, lay)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("lay", ["tile", "interleave"])
def test_unfused_module_path_equals_the_expanded_bank(dtype, lay):
    m = _mmfs(dtype)
    m.fused_sampler = False
    from mmfs_amd.levels import make_level_tables
    sh, start, _ = make_level_tables([(8, 8), (4, 4), (2, 2)], 1, DEV)
    Bv, g = 2, 3
    q = torch.randn(Bv * g, 20, 64, device=DEV).to(dtype)
    ref = torch.rand(1, 20, 1, 2, device=DEV)
    feats = torch.randn(Bv, 1, 84, 96, device=DEV).to(dtype)
    with torch.no_grad():
        value = m.value_proj(feats)
        got = m(q, ref, feats, sh, start, attention_mask=torch.ones(Bv * g, 1, device=DEV), value=value, bank_repeat=lay)
        want = m(q, ref, expand(feats, g, lay), sh, start, attention_mask=torch.ones(Bv * g, 1, device=DEV),
                 value=expand(value, g, lay))
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Bv,g,lay", [(1, 2, "tile"), (3, 2, "interleave"), (2, 5, "tile"), (1, 5, "interleave")])
def test_backward_equals_autograd_through_expand(dtype, Bv, g, lay):
    from mmfs_amd.functions import MSDeformAttnFunction
    value, sh, start, loc, attn = op_inputs("cfg2_sd_real", Bv, Bv * g, 64, dtype, seed=g)
    cot = torch.randn(Bv * g, 64, value.shape[2] * value.shape[3], device=DEV).to(dtype)

    def run(shared):
        v = value.clone().requires_grad_(True)
        lo = loc.clone().requires_grad_(True)
        a = attn.clone().requires_grad_(True)
        if shared:
            out = MSDeformAttnFunction.apply(v, sh, start, lo, a, 1, False, lay)
        else:
            ve = v[None].expand(g, *v.shape) if lay == "tile" else v[:, None].expand(v.shape[0], g, *v.shape[1:])
            out = MSDeformAttnFunction.apply(ve.reshape(Bv * g, *v.shape[1:]).contiguous(), sh, start, lo, a, 1)
        out.backward(cot)
        return out, v.grad, lo.grad, a.grad

    for x, y, name in zip(run(True), run(False), ("out", "grad_value", "grad_loc", "grad_attn")):
        assert torch.equal(x, y), name


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


def _net_inputs(net, B, Bv, dtype):
    # residuals: conv_in, one per layer of stage 0 + its downsampler, stage 1's layer (sd_shapes [8, 4, 2])
    chans = [32, 32, 32, 64]
    sides = [8, 8, 8, 4]
    gen = torch.Generator(device=DEV).manual_seed(1)
    res = [torch.randn(B, c, s, s, generator=gen, device=DEV).to(dtype) for c, s in zip(chans, sides)]
    mid = torch.randn(B, 64, 4, 4, generator=gen, device=DEV).to(dtype)
    feats = [torch.randn(Bv, 1, 64, s, s, generator=gen, device=DEV).to(dtype) for s in (16, 8, 4)]
    return mid, res, feats, torch.ones(B, 1, device=DEV, dtype=torch.long)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mmfs_net_with_cfg_shares_the_bank(dtype):
    from mmfs_amd.blocks.sd_mmfs import ProjectedFeatures
    net = _net(dtype)
    Bv, B = 2, 4
    mid, res, feats, mask = _net_inputs(net, B, Bv, dtype)
    with torch.no_grad():
        proj = net.project_features(feats)
        assert all(v.shape[0] == Bv for v in proj.values)
        got = net(mid, res, proj, mask, bank_repeat="tile")
        doubled = ProjectedFeatures([torch.cat([v] * 2) for v in proj.values], torch.cat([proj.bank] * 2), proj.shapes)
        want = net(mid, res, doubled, mask)
    for x, y in zip((got[0],) + tuple(got[1]), (want[0],) + tuple(want[1])):
        assert torch.equal(x, y)


def test_mmfs_net_dedupes_a_doubled_bank_on_request():
    dtype = torch.float32
    net = _net(dtype)
    Bv, B = 2, 4
    mid, res, feats, mask = _net_inputs(net, B, Bv, dtype)
    doubled = [torch.cat([f] * 2) for f in feats]
    with torch.no_grad():
        want = net(mid, res, doubled, mask)
        assert all(v.shape[0] == B for v in net.__dict__["_projected"].values)      # off by default: all rows projected
        net.clear_feature_cache()
        net.dedupe_repeated_bank = True
        got = net(mid, res, doubled, mask)
        proj = net.__dict__["_projected"]
        assert proj.bank_repeat == "tile" and all(v.shape[0] == Bv for v in proj.values)
        again = net(mid, res, doubled, mask)                                         # the kept projections, no new check
        assert net.__dict__["_projected"] is proj
        # halves that differ are projected whole
        net.clear_feature_cache()
        other = [torch.cat([f, f.flip(0)]) for f in feats]
        net(mid, res, other, mask)
        assert net.__dict__["_projected"].bank_repeat is None
    scale = max(float(y.abs().max()) for y in (want[0],) + tuple(want[1]))
    for x, x2, y in zip((got[0],) + tuple(got[1]), (again[0],) + tuple(again[1]), (want[0],) + tuple(want[1])):
        assert float((x - y).abs().max()) <= 2e-5 * scale
        assert torch.equal(x, x2)


@pytest.mark.parametrize("Lq", [1, 17])
def test_llama_schedule_with_beams_shares_the_bank(Lq):
    from mmfs_amd.blocks import LlamaMMFSAttention, LlamaMMFSSchedule
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
        bank = LlamaMMFSSchedule(layers).project(feats, bank_repeat="interleave")
        assert bank.bank_repeat == "interleave" and all(v.shape[0] == Bv for v in bank.values)
        h1 = h2 = hidden
        for k, l in enumerate(layers):
            h1 = h1 + l(h1, feats, mask, value=bank.values[k], bank_repeat=bank.bank_repeat)
            h2 = h2 + l(h2, feats.repeat_interleave(g, 0), mask, value=bank.values[k].repeat_interleave(g, 0))
    assert torch.equal(h1, h2)


def test_stress_shared_forward_at_north_star_size():
    """50 back-to-back shared-bank forwards at the full north-star size (Bv = 4 serving B = 8, "tile"): every run equal
    to the first bit for bit, and the first equal to the expanded bank's call (tests/test_stress_gpu.py's scan)."""
    H, D, P, shapes, n = GEOMS["north_star"]
    value, sh, start, loc, attn = op_inputs("north_star", 4, 8, 4096, torch.bfloat16, seed=7)
    first = MSDA.ms_deform_attn_forward(value, sh, start, loc, attn, 1, value_repeat="tile")
    bad = 0
    for _ in range(49):
        bad += not torch.equal(MSDA.ms_deform_attn_forward(value, sh, start, loc, attn, 1, value_repeat="tile"), first)
    assert bad == 0, f"{bad} of 49 runs differ from the first"
    assert torch.equal(first, MSDA.ms_deform_attn_forward(torch.cat([value] * 2), sh, start, loc, attn, 1))
