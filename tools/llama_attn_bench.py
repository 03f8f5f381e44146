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
``prefill`` lines: a prompt of Lq = 2, 16, 128, 512 and 2048 tokens into an empty cache and one chunk of 512 onto 1536 held
tokens, B = 4, HF's mask as the reference builds it (left padding of 0 .. 3 + causal, in bf16) -- the framework route's
rope and attention on the new keys as they lie, against the kernel route's two forms, alternating in one process:
``llama_rope_append`` and then the same attention in framework ops on the cache's views (strided in the key axis: the
capacity is 64 more than the keys; what ``prefill_kernel = False`` selects), and ``llama_rope_append`` and then the prefill
kernel (csrc/mmfs_llama_prefill.hip), once on that mask as it lies and once on the padding row with the causal flag.
Algorithmic FLOPs are 4 B H D (Lq held + Lq (Lq + 1) / 2): the causal half of the two products, over the median time.
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
from mmfs_amd.functions.llama_attn_func import (_attn_decode as attn_decode, _attn_prefill as attn_prefill,  # noqa: E402
                                                _rope_append as rope_append)

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
    ap.add_argument("--only", choices=("decode", "prefill"), help="one half of the lines (the table then has that half alone)")
    args = ap.parse_args()
    cfg = types.SimpleNamespace(hidden_size=H * D, num_attention_heads=H, max_position_embeddings=2048)
    m = LlamaSelfAttention(cfg)                        # (its four Linear layers stay on the host: they are not timed)
    cos, sin = m.rope(dev)
    rows = []
    for B, T in () if args.only == "prefill" else SHAPES:
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
    for held, Lq in () if args.only == "decode" else ((0, 2), (0, 16), (0, 128), (0, 512), (0, 2048), (1536, 512)):
        B, n = 4, held + Lq
        gen = torch.Generator(device=dev).manual_seed(1)
        draw = lambda *s: torch.empty(s, dtype=DT, device=dev).normal_(0.0, 1.0, generator=gen)
        q, k, v = draw(B, Lq, H * D), draw(B, Lq, H * D), draw(B, Lq, H * D)
        pos = torch.arange(held, n, device=dev)[None].expand(B, -1).contiguous()
        # HF's mask as the reference builds it: _expand_mask (left padding of 0 .. 3) + _make_causal_mask, in T
        low = torch.finfo(DT).min
        keep = torch.arange(n, device=dev)[None, :] >= torch.arange(B, device=dev)[:, None] % 4
        row = torch.where(keep, 0.0, low).to(DT)[:, None, None, :]                                   # [B, 1, 1, n]
        causal = torch.cat((torch.zeros(Lq, held, dtype=DT, device=dev), torch.full((Lq, Lq), low, dtype=DT, device=dev).triu(1)), -1)
        mask = row.expand(B, 1, Lq, n) + causal[None, None]
        cache = LlamaKVCache(1, B, H, n + 64, D, DT, dev)
        cache.store[:, :, :, :, :held].normal_(0.0, 1.0, generator=gen)
        cache.set_length(held)
        past = (cache.store[0, 0, :, :, :held].clone(), cache.store[0, 1, :, :, :held].clone())
        last = {}

        def framework():
            with torch.no_grad():
                c = torch.cat((cos, cos), dim=-1).to(DT)[pos].unsqueeze(1)
                s = torch.cat((sin, sin), dim=-1).to(DT)[pos].unsqueeze(1)
                hq, hk, hv = m._split(q), m._split(k), m._split(v)
                hq = hq * c + mmfs_amd.llama_attn.rotate_half(hq) * s
                hk = hk * c + mmfs_amd.llama_attn.rotate_half(hk) * s
                if held:
                    hk, hv = torch.cat((past[0], hk), dim=2), torch.cat((past[1], hv), dim=2)
                last["framework"] = m._attend(hq, hk, hv, mask, False)[0]

        def append():
            layer = cache[0]
            return layer, rope_append(q, k, v, pos, cos, sin, layer.keys, layer.values, cache.length, cache.src_row)

        def kernels():                                 # append + framework ops on the cache's views (prefill_kernel = False)
            with torch.no_grad():
                layer, q_rot = append()
                last["kernels"] = m._attend(m._split(q_rot), layer.keys[:, :, :n], layer.values[:, :, :n], mask, False)[0]

        def prefill_hf():                              # append + the prefill kernel on HF's mask as it lies
            layer, q_rot = append()
            last["prefill_hf"] = attn_prefill(q_rot, layer.keys, layer.values, cache.length, cache.src_row, mask)

        def prefill_flag():                            # append + the prefill kernel: the padding row and the causal flag
            layer, q_rot = append()
            last["prefill_flag"] = attn_prefill(q_rot, layer.keys, layer.values, cache.length, cache.src_row, row, True)

        fns = {"framework": framework, "kernels": kernels, "prefill_hf": prefill_hf, "prefill_flag": prefill_flag}
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        gap = {name: float((last["framework"].double() - last[name].double()).abs().max()) for name in fns if name != "framework"}
        scale = float(last["framework"].double().abs().max())
        last.clear()
        t = interleaved(fns)
        flops = 4 * B * H * D * (Lq * held + Lq * (Lq + 1) // 2)
        r = dict(B=B, held=held, Lq=Lq, context_scale=scale, algorithmic_GFLOP=round(flops / 1e9, 2))
        for name in fns:
            r[name + "_us"], r[name + "_spread_us"] = round(t[name][0] * 1e3, 1), round(t[name][1] * 1e3, 1)
            if name != "framework":
                r[name + "_max_abs_to_framework"] = gap[name]
        for name in ("prefill_hf", "prefill_flag"):
            r[name + "_algorithmic_TFLOPs"] = round(flops / (t[name][0] * 1e-3) / 1e12, 1)
            # the kernel is the default on a line only where its median gain over append + framework ops exceeds both spreads
            r[name + "_gain_exceeds_spreads"] = t["kernels"][0] - t[name][0] > max(t["kernels"][1], t[name][1])
        prefill.append(r)
        del cache, last, past, mask
        torch.cuda.empty_cache()
    print(json.dumps({"decode": rows, "prefill": prefill}))
    if args.md:
        lines = [] if args.only == "prefill" else ["| B | T | beams | layers walked | framework us | kernels us | speed-up | algorithmic MB | kernels: share of 6.3 TB/s "
                 "| framework: share | graph: framework us | graph: kernels us | graph: kernels' share | max abs difference "
                 "(context scale) |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['B']} | {r['T']} | {'yes' if r['beams'] else 'no'} | {r['layers']} | {r['framework_us']} +- "
                         f"{r['framework_spread_us']} | {r['kernels_us']} +- {r['kernels_spread_us']} | {r['speedup']} | "
                         f"{r['algorithmic_MB']} | {r['kernels_share_of_stream']} | {r['framework_share_of_stream']} | "
                         f"{r['framework_graph_us']} | {r['kernels_graph_us']} | {r['kernels_graph_share_of_stream']} | "
                         f"{r['agree_max_abs']:.3g} ({r['context_scale']:.3g}) |")
        lines += [] if args.only == "decode" else ["", "| B | held | prompt Lq | framework us | append + framework ops us | append + prefill kernel, HF mask us | "
                  "append + prefill kernel, padding row + causal flag us | algorithmic GFLOP | algorithmic TFLOP/s (HF mask / flag) | "
                  "gain over append + framework ops exceeds both spreads (HF mask / flag) | max abs difference to framework "
                  "(ops / HF mask / flag; context scale) |", "|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in prefill:
            pm = lambda name: f"{r[name + '_us']} +- {r[name + '_spread_us']}"
            lines.append(f"| {r['B']} | {r['held']} | {r['Lq']} | {pm('framework')} | {pm('kernels')} | {pm('prefill_hf')} | "
                         f"{pm('prefill_flag')} | {r['algorithmic_GFLOP']} | {r['prefill_hf_algorithmic_TFLOPs']} / "
                         f"{r['prefill_flag_algorithmic_TFLOPs']} | {'yes' if r['prefill_hf_gain_exceeds_spreads'] else 'no'} / "
                         f"{'yes' if r['prefill_flag_gain_exceeds_spreads'] else 'no'} | {r['kernels_max_abs_to_framework']:.3g} / "
                         f"{r['prefill_hf_max_abs_to_framework']:.3g} / {r['prefill_flag_max_abs_to_framework']:.3g} "
                         f"({r['context_scale']:.3g}) |")
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
