#!/usr/bin/env python3
"""The LLM's self-attention at decode per layer-step at Vicuna-7B geometry (H = 32, D = 128, bf16),
between the three Linear layers' outputs and the context (the Linear layers are GEMVs on every route and are left out),
for B in {4, 20 (4 x 5 beams)} and T in {128, 512, 2048} keys after the step:
  framework   the statement this library had before the kernels: mmfs_amd.LlamaSelfAttention's framework route -- the
              reference's rope, ``torch.cat`` onto a tuple cache, matmul / clamp / fp32 softmax / matmul -- and, with
              beams, the reference's ``index_select`` of the layer's new keys and values (``_reorder_cache``).  Its rope
              indexes the table once where the reference repeats and gathers it twice: the cheaper of the two.
  kernels     csrc/mmfs_llama_attn.hip on a LlamaKVCache: append, decode, merge; with beams ``cache.reorder`` once per
              step, spread over the layers the step walks.
A step walks ``layers`` layers with their own keys and values (at least 1 GiB of them together, at most 32), so that no
layer's cache is still in the chip's memory-side cache when its turn comes again -- as in a model of 32 layers.  Device
events around ``iters`` synchronised steps (a window of at least ~0.1 s), the two routes in alternating rounds of one
process, the median of 5 rounds with their spread; per layer-step = step / layers.  Algorithmic bytes are one read of the
layer's keys and values, 2 B H T D e; their rate is set against the 6.3 TB/s a streaming kernel reaches on an MI355X.
``graph`` columns: the same step of either route captured once with ``torch.cuda.graph`` and replayed -- the device's
share of the time, without the host's gaps between launches.
``prefill`` lines: a prompt of Lq = 128, 512 and 2048 tokens into an empty cache, B = 4, causal mask -- the framework route's
rope and attention on the new keys as they lie, against the kernel route's: ``llama_rope_append`` and then the same
attention in framework ops on the cache's views (strided in the key axis: the capacity is Lq + 64).
Prints one JSON line; ``--md PATH`` also writes the tables.
    python tools/llama_attn_bench.py [--md profiles/llama_attn_table.md]
Not the contract benchmark (bench.py)."""
import argparse
import json
import math
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mm-interleaved_amd")]
import torch  # noqa: E402

import mmfs_amd  # noqa: E402
from mmfs_amd.llama_attn import LlamaKVCache, LlamaSelfAttention  # noqa: E402
# the entries LlamaSelfAttention calls (the public llama_rope_append / llama_attn_decode check their arguments on the host first)
from mmfs_amd.functions.llama_attn_func import _attn_decode as attn_decode, _rope_append as rope_append  # noqa: E402

dev = torch.device("cuda:0")
DT = torch.bfloat16
H, D = 32, 128
STREAM_TBS = 6.3
SHAPES = [(B, T) for B in (4, 20) for T in (128, 512, 2048)]


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def interleaved(fns, rounds=5, window_ms=100.0):
    iters = {}
    for k, f in fns.items():
        timed(f, 3)
        iters[k] = max(3, min(400, int(window_ms / max(timed(f, 3), 1e-3))))
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            got[k].append(timed(f, iters[k]))
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in got.items()}


def graphed(fn):
    """``fn`` captured once (after a warm-up on a side stream) -> its replay"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md")
    args = ap.parse_args()
    cfg = types.SimpleNamespace(hidden_size=H * D, num_attention_heads=H, max_position_embeddings=2048)
    m = LlamaSelfAttention(cfg)                        # (its four Linear layers stay on the host: they are not timed)
    cos, sin = m.rope(dev)
    rows = []
    for B, T in SHAPES:
        beams = B > 4
        layer_bytes = 2 * B * H * T * D * 2
        layers = max(2, min(32, math.ceil(2 ** 30 / layer_bytes)))
        gen = torch.Generator(device=dev).manual_seed(0)
        draw = lambda *s: torch.empty(s, dtype=DT, device=dev).normal_(0.0, 1.0, generator=gen)
        cache = LlamaKVCache(layers, B, H, T, D, DT, dev)
        cache.store[:, :, :, :, :T - 1].normal_(0.0, 1.0, generator=gen)
        cache.set_length(T - 1)
        past = [(cache.store[i, 0, :, :, :T - 1].clone(), cache.store[i, 1, :, :, :T - 1].clone()) for i in range(layers)]
        q, k, v = draw(B, 1, H * D), draw(B, 1, H * D), draw(B, 1, H * D)
        pos = torch.full((B, 1), T - 1, device=dev)
        keep = torch.arange(T, device=dev)[None, :] >= torch.arange(B, device=dev)[:, None] % 4      # left padding of 0 .. 3
        mask = torch.where(keep, 0.0, torch.finfo(DT).min).to(DT)[:, None, None, :]                  # HF's extended mask
        bias = mask.reshape(B, T)
        beam_idx = torch.arange(B, device=dev).roll(1)
        last = {}

        def framework():
            with torch.no_grad():
                for i in range(layers):
                    hq, hk, hv = (t.view(B, 1, H, D).transpose(1, 2) for t in (q, k, v))
                    c = torch.cat((cos, cos), dim=-1)[:T].to(DT)[pos].unsqueeze(1)
                    s = torch.cat((sin, sin), dim=-1)[:T].to(DT)[pos].unsqueeze(1)
                    hq = (hq * c) + (mmfs_amd.llama_attn.rotate_half(hq) * s)
                    hk = (hk * c) + (mmfs_amd.llama_attn.rotate_half(hk) * s)
                    keys, values = torch.cat([past[i][0], hk], dim=2), torch.cat([past[i][1], hv], dim=2)
                    last["framework"] = m._attend(hq, keys, values, mask, False)[0]
                    if beams:
                        last["present"] = (keys.index_select(0, beam_idx), values.index_select(0, beam_idx))

        def kernels():
            for i in range(layers):
                layer = cache[i]
                q_rot = rope_append(q, k, v, pos, cos, sin, layer.keys, layer.values, cache.length, cache.src_row)
                last["kernels"] = attn_decode(q_rot, layer.keys, layer.values, cache.length, cache.src_row, bias, T)
            if beams:
                cache.reorder(beam_idx)

        # faster and different is not faster: the last layer's context of both routes on these very inputs
        framework()
        kernels()
        torch.cuda.synchronize()
        gap = float((last["framework"].double() - last["kernels"].double()).abs().max())
        scale = float(last["framework"].double().abs().max())
        cache.reset()
        cache.set_length(T - 1)
        t = interleaved({"framework": framework, "kernels": kernels, "framework_graph": graphed(framework),
                         "kernels_graph": graphed(kernels)})
        fw, kn, fwg, kng = (t[name][0] / layers * 1e3 for name in ("framework", "kernels", "framework_graph", "kernels_graph"))
        rows.append(dict(B=B, T=T, beams=beams, layers=layers, framework_us=round(fw, 2), kernels_us=round(kn, 2),
                         framework_spread_us=round(t["framework"][1] / layers * 1e3, 2),
                         kernels_spread_us=round(t["kernels"][1] / layers * 1e3, 2), speedup=round(fw / kn, 2),
                         framework_graph_us=round(fwg, 2), kernels_graph_us=round(kng, 2),
                         kernels_graph_share_of_stream=round(layer_bytes / (kng * 1e-6) / (STREAM_TBS * 1e12), 3),
                         algorithmic_MB=round(layer_bytes / 1e6, 2),
                         kernels_share_of_stream=round(layer_bytes / (kn * 1e-6) / (STREAM_TBS * 1e12), 3),
                         framework_share_of_stream=round(layer_bytes / (fw * 1e-6) / (STREAM_TBS * 1e12), 3),
                         agree_max_abs=gap, context_scale=scale))
        del cache, past, last
        torch.cuda.empty_cache()
    prefill = []
    for Lq in (128, 512, 2048):
        B = 4
        gen = torch.Generator(device=dev).manual_seed(1)
        draw = lambda *s: torch.empty(s, dtype=DT, device=dev).normal_(0.0, 1.0, generator=gen)
        q, k, v = draw(B, Lq, H * D), draw(B, Lq, H * D), draw(B, Lq, H * D)
        pos = torch.arange(Lq, device=dev)[None].expand(B, -1).contiguous()
        mask = torch.full((Lq, Lq), torch.finfo(DT).min, dtype=DT, device=dev).triu(1)[None, None].expand(B, 1, Lq, Lq)
        cache = LlamaKVCache(1, B, H, Lq + 64, D, DT, dev)
        last = {}

        def framework():
            with torch.no_grad():
                c = torch.cat((cos, cos), dim=-1).to(DT)[pos].unsqueeze(1)
                s = torch.cat((sin, sin), dim=-1).to(DT)[pos].unsqueeze(1)
                hq, hk, hv = m._split(q), m._split(k), m._split(v)
                hq = hq * c + mmfs_amd.llama_attn.rotate_half(hq) * s
                hk = hk * c + mmfs_amd.llama_attn.rotate_half(hk) * s
                last["framework"] = m._attend(hq, hk, hv, mask, False)[0]

        def kernels():
            with torch.no_grad():
                layer = cache[0]
                q_rot = rope_append(q, k, v, pos, cos, sin, layer.keys, layer.values, cache.length, cache.src_row)
                last["kernels"] = m._attend(m._split(q_rot), layer.keys[:, :, :Lq], layer.values[:, :, :Lq], mask, False)[0]

        framework()
        kernels()
        torch.cuda.synchronize()
        gap = float((last["framework"].double() - last["kernels"].double()).abs().max())
        t = interleaved({"framework": framework, "kernels": kernels})
        prefill.append(dict(B=B, Lq=Lq, framework_us=round(t["framework"][0] * 1e3, 1), kernels_us=round(t["kernels"][0] * 1e3, 1),
                            framework_spread_us=round(t["framework"][1] * 1e3, 1), kernels_spread_us=round(t["kernels"][1] * 1e3, 1),
                            agree_max_abs=gap))
        del cache, last
        torch.cuda.empty_cache()
    print(json.dumps({"decode": rows, "prefill": prefill}))
    if args.md:
        lines = ["| B | T | beams | layers walked | framework us | kernels us | speed-up | algorithmic MB | kernels: share of 6.3 TB/s "
                 "| framework: share | graph: framework us | graph: kernels us | graph: kernels' share | max abs difference "
                 "(context scale) |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['B']} | {r['T']} | {'yes' if r['beams'] else 'no'} | {r['layers']} | {r['framework_us']} +- "
                         f"{r['framework_spread_us']} | {r['kernels_us']} +- {r['kernels_spread_us']} | {r['speedup']} | "
                         f"{r['algorithmic_MB']} | {r['kernels_share_of_stream']} | {r['framework_share_of_stream']} | "
                         f"{r['framework_graph_us']} | {r['kernels_graph_us']} | {r['kernels_graph_share_of_stream']} | "
                         f"{r['agree_max_abs']:.3g} ({r['context_scale']:.3g}) |")
        lines += ["", "| B | prompt Lq | framework us | kernels us | max abs difference |", "|---|---|---|---|---|"]
        for r in prefill:
            lines.append(f"| {r['B']} | {r['Lq']} | {r['framework_us']} +- {r['framework_spread_us']} | {r['kernels_us']} +- "
                         f"{r['kernels_spread_us']} | {r['agree_max_abs']:.3g} |")
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
