#!/usr/bin/env python3
"""The Q-Former attention at the pipeline's three shapes, bf16, between the Linear layers' outputs and
the context (the Linear layers are GEMMs on every route and are left out):
  tokenizer_self     B = 32, Nq = Nk = 64, H = 12, qk-norm
  tokenizer_cross    B = 32, Nq = 64, Nk = 257, H = 12, qk-norm
  decoder_cross      B = 8, Nq = 77, Nk = 2048, H = 16, no qk-norm, a mask that cuts every row to another length
Candidates, in the same interleaved rounds of one process:
  framework          mmfs_amd.QKNormAttention's framework route (the reference's statement)
  sdpa               the same LayerNorms in front of F.scaled_dot_product_attention
  kernels            csrc/mmfs_attn.hip
Per candidate and mode (forward + backward; the forward under no_grad): device ms per call (events around a synchronised
batch of ``--iters`` calls, so host-bound gaps count; 500 calls make a window of 15 .. 300 ms: a window of a few
milliseconds measures the clock and the scheduler), the median of 7 rounds with the rounds' spread max - min, and the peak of allocated
memory above the resident tensors in one call.  Prints one JSON line; ``--md PATH`` also writes the table.
    python tools/qk_attn_bench.py [--md profiles/qk_attn_table.md] [--iters 500]
Not the contract benchmark (bench.py)."""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mm-interleaved_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mmfs_amd.functions.qk_attn_func import QKNormAttentionFunction  # noqa: E402
from mmfs_amd.resampler import QKNormAttention  # noqa: E402

dev = "cuda"
DT = torch.bfloat16
SHAPES = {"tokenizer_self": dict(B=32, Nq=64, Nk=64, H=12, norm=True, mask=False),
          "tokenizer_cross": dict(B=32, Nq=64, Nk=257, H=12, norm=True, mask=False),
          "decoder_cross": dict(B=8, Nq=77, Nk=2048, H=16, norm=False, mask=True)}


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def interleaved(fns, iters, rounds=7):
    for f in fns.values():
        timed(f, 50)
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            got[k].append(timed(f, iters))
    return {k: dict(device_ms=round(statistics.median(v), 4), spread=round(max(v) - min(v), 4)) for k, v in got.items()}


def peak_above_resident(fn):
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md")
    ap.add_argument("--iters", type=int, default=500)
    args = ap.parse_args()
    result = {}
    for name, c in SHAPES.items():
        B, Nq, Nk, H = c["B"], c["Nq"], c["Nk"], c["H"]
        gen = torch.Generator(device=dev).manual_seed(0)
        draw = lambda *s: torch.empty(s, dtype=DT, device=dev).normal_(0.0, 1.0, generator=gen)
        q, k, v = (draw(B, n, H * 64).requires_grad_(True) for n in (Nq, Nk, Nk))
        up = draw(B, Nq, H * 64)
        cfg = types.SimpleNamespace(hidden_size=H * 64, num_attention_heads=H, encoder_hidden_size=H * 64,
                                    attention_probs_dropout_prob=0.0, layer_norm_eps=1e-12, qk_normalization=c["norm"])
        m = QKNormAttention(cfg, is_cross_attention=True).to(dev, DT).eval()
        bias = mask = None
        if c["mask"]:
            lengths = torch.linspace(Nk // 4, Nk, B, device=dev).long()
            keep = torch.arange(Nk, device=dev)[None, :] < lengths[:, None]
            mask = torch.where(keep, 0.0, torch.finfo(DT).min).to(DT)[:, None, None, :]     # HF's extended mask
            bias = mask.reshape(B, Nk)
        params = [m.q_norm.weight, m.q_norm.bias, m.k_norm.weight, m.k_norm.bias] if c["norm"] else [None] * 4
        leaves = [q, k, v] + [p for p in params if p is not None]

        def framework():
            return m._framework(None, q, k, v, mask, None, True, None, False)[0]

        def sdpa():
            heads = lambda x: x.unflatten(-1, (H, 64)).transpose(1, 2)
            out = F.scaled_dot_product_attention(m.q_norm(heads(q)), m.k_norm(heads(k)), heads(v), attn_mask=mask)
            return out.transpose(1, 2).flatten(2)

        def kernels():
            return QKNormAttentionFunction.apply(q, k, v, *params, 1e-12, bias, H)[0]

        last = {}

        def both(f):
            def run():
                last["grads"] = torch.autograd.grad(f(), leaves, up)
            return run

        def forward(f):
            def run():
                with torch.no_grad():
                    last["out"] = f()
            return run

        cands = {"framework": framework, "sdpa": sdpa, "kernels": kernels}
        # faster and different is not faster: the candidates' results on these very inputs
        forward(framework)()
        want = last["out"].double()
        agree = {}
        for kname, f in cands.items():
            forward(f)()
            agree[kname] = float((last["out"].double() - want).abs().max())
        entry = dict(agree_max_abs=agree, context_scale=float(want.abs().max()))
        for mode, wrap in (("fwd_bwd", both), ("fwd_nograd", forward)):
            fns = {kname: wrap(f) for kname, f in cands.items()}
            rows = interleaved(fns, args.iters)
            for kname, f in fns.items():
                last.clear()
                rows[kname]["peak_MB"] = round(peak_above_resident(f) / 1e6, 2)
            last.clear()
            entry[mode] = rows
        result[name] = entry
        del q, k, v
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if args.md:
        lines = ["| shape | mode | candidate | device ms | spread | peak MB above resident |", "|---|---|---|---|---|---|"]
        for key, r in result.items():
            for mode in ("fwd_bwd", "fwd_nograd"):
                for kname, x in r[mode].items():
                    lines.append(f"| {key} | {mode} | {kname} | {x['device_ms']} | {x['spread']} | {x['peak_MB']} |")
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
