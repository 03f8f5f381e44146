#!/usr/bin/env python3
"""The fp8 value bank (include/mmfs_msda.h "fp8 bank") against the bf16 kept bank, in the two generation
loops that reuse one projected bank:
  sd   BASELINE config 4's denoising step with classifier-free guidance: MMFSNet, B = 8 images -> 16 query rows over the
       shared 8-row bank ("tile"), bf16, eval, no grad, replayed as a HIP graph (GraphedMMFSNet);
  llm  a decode step of 8 LLM MMFS layers (Vicuna-7B widths, one 32/16/8 image per sequence), B = 4 sequences x
       num_beams = 5 over the shared 4-row bank ("interleave"), replayed as one HIP graph (GraphedLlamaMMFSStack);
each with the bank kept in bf16 and in fp8: ms per step (interleaved rounds, medians), kept bytes (+ the scales), the
one-time project (+ quantise) ms, and the largest per-element |dequantised fp8 - bf16| of the kept bank as a fraction of
the quantisation bound 2^-4 |x| + 2^-10 scale.  Prints one JSON line.
    python tools/fp8_bank_bench.py [sd] [llm]
    python tools/fp8_bank_bench.py prof [sd] [llm]    # only replays both graphs (for rocprofv3 --kernel-trace --stats)
Not the contract benchmark (bench.py)."""
import contextlib
import io
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mm-interleaved_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import MultiScaleDeformableAttention as MSDA  # noqa: E402
from mmfs_amd.blocks import LlamaMMFSAttention, LlamaMMFSSchedule  # noqa: E402
from mmfs_amd.graphs import GraphedLlamaMMFSStack, GraphedMMFSNet  # noqa: E402

args = sys.argv[1:]
prof = "prof" in args
what = [a for a in args if a != "prof"] or ["sd", "llm"]
dev, dt, F8 = "cuda", torch.bfloat16, torch.float8_e4m3fn
result = {}

with contextlib.redirect_stdout(io.StringIO()):            # (the helpers of the shared-bank tool; its own run is skipped)
    sys.argv = [sys.argv[0], "none"]
    import shared_bank_bench as sbb                            # noqa: E402


def kept_bytes(values, scales):
    return dict(bank=sbb.nbytes(values), scales=sbb.nbytes(scales or []))


def error_fraction(v16, v8, s8):
    """max over the kept elements of |dequant(fp8) - bf16| / (2^-4 |bf16| + 2^-10 scale)"""
    worst = 0.0
    for a, q, s in zip(v16, v8, s8):
        x = a.reshape(s.shape[0], -1, s.shape[1]).float()
        d = q.reshape(x.shape).float() * s[:, None, :]
        bound = 2 ** -4 * x.abs() + 2 ** -10 * s[:, None, :]
        worst = max(worst, float(((d - x).abs() / bound.clamp_min(1e-30)).max()))
    return round(worst, 4)


if "sd" in what:
    net, mid, res, feats, mask = sbb.sd_net()
    res, mid, mask = res, mid, mask
    with torch.no_grad():
        t_proj = sbb.interleaved({"bf16": lambda: net.project_features(feats),
                                  "fp8": lambda: net.project_features(feats, bank_dtype=F8)}, iters=3, rounds=5)
        p16 = net.project_features(feats)
        p8 = net.project_features(feats, bank_dtype=F8)
    g16 = GraphedMMFSNet(net, mid, res, p16, mask, bank_repeat="tile")
    g8 = GraphedMMFSNet(net, mid, res, p8, mask, bank_repeat="tile")
    if prof:
        for _ in range(50):
            g16(mid, res)
            g8(mid, res)
        torch.cuda.synchronize()
    else:
        o16, o8 = g16(mid, res), g8(mid, res)
        diff = max(float((a.float() - b.float()).abs().max()) for a, b in zip((o16[0],) + tuple(o16[1]), (o8[0],) + tuple(o8[1])))
        t_step = sbb.interleaved({"bf16": lambda: g16(mid, res), "fp8": lambda: g8(mid, res)}, iters=20)
        result["sd_cfg4_cfg"] = dict(B_images=8, query_rows=16, step_ms=t_step, project_ms=t_proj,
                                     kept_bytes=dict(bf16=kept_bytes(p16.values, None), fp8=kept_bytes(p8.values, p8.scales)),
                                     kept_error_over_bound=error_fraction(p16.values, p8.values, p8.scales),
                                     max_abs_output_diff=diff)
    del g16, g8, net, p16, p8
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
    feats = torch.randn(Bv, 1, 32 * 32 + 16 * 16 + 8 * 8, 1024, device=dev, dtype=dt)
    hidden = torch.randn(Bv * beams, 1, 4096, device=dev, dtype=dt)
    mask = torch.ones(Bv * beams, 1, 1, device=dev)
    s16, s8 = LlamaMMFSSchedule(layers), LlamaMMFSSchedule(layers)
    s16.cache_projected_bank = s8.cache_projected_bank = False
    s8.kept_bank_dtype = F8
    with torch.no_grad():
        # (cache off: every call projects; the fp8 schedule then quantises -- it keeps only with the cache on, so the
        # quantising call is timed through _project)
        t_proj = sbb.interleaved({"bf16": lambda: s16.project(feats, "interleave"),
                                  "fp8": lambda: s8._project(feats, F8)}, iters=3, rounds=5)
        s16.cache_projected_bank = s8.cache_projected_bank = True
        b16 = s16.project(feats, bank_repeat="interleave")
        b8 = s8.project(feats, bank_repeat="interleave")
    assert b8.scales is not None
    g16 = GraphedLlamaMMFSStack(layers, hidden, b16, mask)
    g8 = GraphedLlamaMMFSStack(layers, hidden, b8, mask)
    if prof:
        for _ in range(200):
            g16(hidden)
            g8(hidden)
        torch.cuda.synchronize()
    else:
        diff = float((g16(hidden).float() - g8(hidden).float()).abs().max())
        t_step = sbb.interleaved({"bf16": lambda: g16(hidden), "fp8": lambda: g8(hidden)}, iters=100)
        result["llm_decode_beams5"] = dict(sequences=Bv, num_beams=beams, layers=8, step_ms=t_step, project_ms=t_proj,
                                           kept_bytes=dict(bf16=kept_bytes(b16.values, None), fp8=kept_bytes(b8.values, b8.scales)),
                                           kept_error_over_bound=error_fraction(b16.values, b8.values, b8.scales),
                                           max_abs_output_diff=diff)

print(json.dumps(result))
