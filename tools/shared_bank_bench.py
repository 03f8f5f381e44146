#!/usr/bin/env python3
"""Shared value bank (include/mmfs_msda.h MMFS_BANK_*) against the copied bank the reference's generation modes make:
  sd   BASELINE config 4's denoising step with classifier-free guidance: MMFSNet, B = 8 images -> 16 query rows, bf16, eval,
       no grad, replayed as a HIP graph (mmfs_amd.graphs.GraphedMMFSNet); doubled bank (torch.cat([bank] * 2)) vs the
       8-row bank with bank_repeat="tile": ms per step, bytes of the kept projections, one-time projection ms;
  llm  a decode step of 8 LLM MMFS layers (Vicuna-7B widths, one 32/16/8 image per sequence), B = 4 sequences x
       num_beams = 5: bank repeated per beam vs the 4-row bank with "interleave" -- the same three figures (the step
       replayed as one HIP graph, and eager);
(mmfs_sample_fwd with the g copies of a bank row launched next to each other was measured with an earlier revision of this
tool: no faster, not kept -- DESIGN.md 4.9, profiles/shared_bank_r07.md.)
Every pair is checked bit-equal (the doubled run is fed the shared run's projections, copied).  Prints one JSON line.
    python tools/shared_bank_bench.py [sd] [llm]
Not the contract benchmark (bench.py)."""
import contextlib
import io
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mm-interleaved_amd")]
import torch  # noqa: E402
import MultiScaleDeformableAttention as MSDA  # noqa: E402
from mmfs_amd.blocks import LlamaMMFSAttention, LlamaMMFSSchedule, MMFSNet  # noqa: E402
from mmfs_amd.blocks.sd_mmfs import ProjectedFeatures  # noqa: E402
from mmfs_amd.graphs import GraphedMMFSNet  # noqa: E402

dev, dt = "cuda", torch.bfloat16
what = sys.argv[1:] or ["sd", "llm"]
result = {}


def ms(fn, iters, rounds=1):
    """median over ``rounds`` of the mean ms per call of ``iters`` calls"""
    outs = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        outs.append((time.perf_counter() - t) / iters * 1e3)
    return statistics.median(outs)


def interleaved(fns, iters, rounds=7):
    """{name: median ms per call}, the candidates' rounds alternating (clock / thermal drift falls on both)"""
    for f in fns.values():
        ms(f, 3)
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            got[k].append(ms(f, iters))
    return {k: round(statistics.median(v), 4) for k, v in got.items()}


def nbytes(ts):
    return sum(t.numel() * t.element_size() for t in ts)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def sd_net():
    with contextlib.redirect_stdout(io.StringIO()):
        net = MMFSNet(input_channel=1024, block_out_channels=[320, 640, 1280, 1280], layers_per_block=2,
                      n_levels=4, n_points=8, gradient_checkpointing=True, spatial_shapes=[64, 32, 16, 8]).to(dev, dt)
    torch.manual_seed(0)
    with torch.no_grad():
        for blk in net._blocks():
            blk.conv.weight.normal_(0, 0.02)
            blk.mmfs.sampling_offsets.weight.normal_(0, 0.01)
            blk.feat_norm.weight.uniform_(0.5, 1.5)
            blk.feat_norm.bias.normal_(0, 0.1)
    net.eval()
    Bv, B = 8, 16
    geom = list(zip([320] * 4 + [640] * 3 + [1280] * 5, [64] * 3 + [32] * 3 + [16] * 3 + [8] * 3))
    res = [torch.randn(B, c, s, s, device=dev, dtype=dt) for c, s in geom]
    mid = torch.randn(B, 1280, 8, 8, device=dev, dtype=dt)
    feats = [torch.randn(Bv, 1, 1024, s, s, device=dev, dtype=dt) for s in (64, 32, 16, 8)]
    mask = torch.ones(B, 1, device=dev, dtype=torch.long)
    return net, mid, res, feats, mask


if "sd" in what:
    net, mid, res, feats, mask = sd_net()
    doubled = [torch.cat([f] * 2) for f in feats]
    with torch.no_grad():
        t_proj = interleaved({"doubled": lambda: net.project_features(doubled), "shared": lambda: net.project_features(feats)},
                             iters=3, rounds=5)
        proj_s = net.project_features(feats)
        proj_d = ProjectedFeatures([torch.cat([v] * 2) for v in proj_s.values], torch.cat([proj_s.bank] * 2), proj_s.shapes)

    g_d = GraphedMMFSNet(net, mid, res, proj_d, mask)
    g_s = GraphedMMFSNet(net, mid, res, proj_s, mask, bank_repeat="tile")
    out_d, out_s = g_d(mid, res), g_s(mid, res)
    bit_equal = same((out_d[0],) + tuple(out_d[1]), (out_s[0],) + tuple(out_s[1]))
    t_step = interleaved({"doubled": lambda: g_d(mid, res), "shared": lambda: g_s(mid, res)}, iters=20)
    result["sd_cfg4_cfg"] = dict(B_images=8, query_rows=16, step_ms=t_step, projection_ms=t_proj,
                                 projection_bytes=dict(doubled=nbytes(proj_d.values), shared=nbytes(proj_s.values)),
                                 bit_equal=bit_equal)
    del g_d, g_s, out_d, out_s
    del net, proj_s, proj_d
    torch.cuda.empty_cache()

if "llm" in what:
    cfg = types.SimpleNamespace(hidden_size=4096, num_attention_heads=32, rms_norm_eps=1e-6, max_position_embeddings=2048,
                                image_embed_dim=1024, spatial_shapes=[32, 16, 8])
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        layers = [LlamaMMFSAttention(cfg, 4 * i).to(dev, dt).eval() for i in range(8)]
    with torch.no_grad():
        for l in layers:
            l.gate.fill_(0.5)
            l.attn.sampling_offsets.weight.normal_(0, 0.01)
    Bv, beams = 4, 5
    B = Bv * beams
    feats = torch.randn(Bv, 1, 32 * 32 + 16 * 16 + 8 * 8, 1024, device=dev, dtype=dt)
    feats_x = feats.repeat_interleave(beams, 0)
    hidden = torch.randn(B, 1, 4096, device=dev, dtype=dt)
    mask = torch.ones(B, 1, 1, device=dev)
    sched = LlamaMMFSSchedule(layers)
    sched.cache_projected_bank = False
    with torch.no_grad():
        t_proj = interleaved({"expanded": lambda: sched.project(feats_x), "shared": lambda: sched.project(feats, "interleave")},
                             iters=3, rounds=5)
        bank_s = sched.project(feats, bank_repeat="interleave")
        vals_x = [v.repeat_interleave(beams, 0) for v in bank_s.values]

        def step_x():
            h = hidden
            for k, l in enumerate(layers):
                h = h + l(h, feats_x, mask, value=vals_x[k])
            return h

        def step_s():
            h = hidden
            for k, l in enumerate(layers):
                h = h + l(h, feats, mask, value=bank_s.values[k], bank_repeat="interleave")
            return h

        bit_equal = torch.equal(step_x(), step_s())
        t_eager = interleaved({"expanded": step_x, "shared": step_s}, iters=50)

        def graphed(fn):                     # the decode step as the project replays it: one HIP graph
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    fn()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = fn()
            return graph, out
        gx, ox = graphed(step_x)
        gs, os_ = graphed(step_s)
        gx.replay(), gs.replay()
        bit_equal = bit_equal and torch.equal(ox, os_)
        t_step = interleaved({"expanded": gx.replay, "shared": gs.replay}, iters=100)
    result["llm_decode_beams5"] = dict(sequences=Bv, num_beams=beams, layers=8, step_ms=t_step, eager_step_ms=t_eager,
                                       projection_ms=t_proj,
                                       projection_bytes=dict(expanded=nbytes(vals_x), shared=nbytes(bank_s.values)),
                                       bit_equal=bit_equal)

print(json.dumps(result))
