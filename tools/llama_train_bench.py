"""Forward + backward of the LLM's self-attention in training, the Linear layers excluded, on one MI355X: H = 32, D = 128, bf16,
B = 4, L in {128, 512, 2048}.  Three lines, interleaved in one process (the median of 5 rounds and their spread):

  kernels     csrc/mmfs_llama_train.hip through ``mmfs_amd.llama_attn_train``: rope, forward, dq, dkdv
  framework   the module's framework statement with HF's 4-D causal mask -- what a training call ran before the training
              route existed: rotate, [B, H, L, L] scores in T and fp32, autograd
  sdpa        for information: torch.nn.functional.scaled_dot_product_attention(is_causal=True) on the rotated tensors, if
              this torch build serves it on the device

and the time of each entry of the C ABI by device events (rope, forward, backward = dq + dkdv) with the algorithmic
matrix-core FLOPs over it: 4 / 6 / 8 B H D L (L + 1) / 2 for forward / dq / dkdv (2, 3 and 4 products over the causal half)
against the chip's 2.5 PFLOP/s bf16 rate (MI355X_MICROARCH.md).  ``--trace L`` runs the kernels alone a few times at one
length: the program to put behind ``rocprofv3 --kernel-trace --stats --`` for the split of the backward into its two kernels.

    python tools/llama_train_bench.py [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mm-interleaved_amd")]
import torch  # noqa: E402

import mmfs_amd  # noqa: E402
from mmfs_amd.functions import llama_train_func as F  # noqa: E402
from mmfs_amd.llama_attn import LlamaSelfAttention, rope_table, rotate_half  # noqa: E402

dev = torch.device("cuda:0")
DT = torch.bfloat16
B, H, D = 4, 32, 128
LENGTHS = (128, 512, 2048)
PEAK_TFLOPS = 2500.0


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def interleaved(fns, rounds=5, window_ms=200.0):
    iters = {}
    for k, f in fns.items():
        timed(f, 3)
        iters[k] = max(3, min(400, int(window_ms / max(timed(f, 3), 1e-3))))
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            got[k].append(timed(f, iters[k]))
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in got.items()}


def problem(L):
    gen = torch.Generator().manual_seed(L)
    q, k, v, up = (torch.randn(B, L, H * D, generator=gen).to(dev, DT) for _ in range(4))
    pos = torch.arange(L, device=dev)[None].expand(B, -1).contiguous()
    cos, sin = rope_table(D, max(L, 2048), device=dev)
    return q, k, v, up, pos, cos, sin


def lines(L):
    q, k, v, up, pos, cos, sin = problem(L)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    cfg = types.SimpleNamespace(hidden_size=H * D, num_attention_heads=H, max_position_embeddings=2048)
    m = LlamaSelfAttention(cfg)                                              # (for _attend and _split: no Linear layer runs)
    causal = torch.full((L, L), torch.finfo(DT).min, dtype=DT, device=dev).triu(1)[None, None].expand(B, 1, L, L)
    c2, s2 = (torch.cat((t, t), dim=-1).to(DT)[pos].unsqueeze(1) for t in (cos, sin))

    def rotated():
        query, keys = m._split(leaves[0]), m._split(leaves[1])
        return query * c2 + rotate_half(query) * s2, keys * c2 + rotate_half(keys) * s2

    def kernels():
        ctx = mmfs_amd.llama_attn_train(*leaves, pos, cos, sin, H)
        return torch.autograd.grad(ctx, leaves, up)

    def framework():
        query, keys = rotated()
        ctx, _ = m._attend(query, keys, m._split(leaves[2]), causal, False)
        return torch.autograd.grad(ctx, leaves, up)

    def sdpa():
        query, keys = rotated()
        ctx = torch.nn.functional.scaled_dot_product_attention(query, keys, m._split(leaves[2]), is_causal=True)
        return torch.autograd.grad(ctx.transpose(1, 2).flatten(2), leaves, up)

    fns = {"kernels": kernels, "framework": framework}
    try:
        sdpa()
        torch.cuda.synchronize()
        fns["sdpa"] = sdpa
    except Exception as e:                                                   # not served by this build: the line is left out
        print(f"sdpa not served at L {L}: {type(e).__name__}: {e}", file=sys.stderr)
    # the lines compute the same thing
    a, b = kernels(), framework()
    diff = max(float((x.float() - y.float()).abs().max()) for x, y in zip(a, b))
    t = interleaved(fns)
    r = {"L": L, "kernels_max_abs_to_framework": diff}
    for name, (med, spread) in t.items():
        r[name + "_us"], r[name + "_spread_us"] = round(med * 1e3, 1), round(spread * 1e3, 1)
    r["kernels_gain_exceeds_spreads"] = t["framework"][0] - t["kernels"][0] > max(t["framework"][1], t["kernels"][1])
    # each entry of the C ABI on its own
    qd, kd, vd = (x.detach() for x in leaves)
    q_rot, k_rot = F.train_rope(qd, kd, pos, cos, sin, H)
    ctx, lse = F.train_forward(q_rot, k_rot, vd, H)
    e = interleaved({"rope": lambda: F.train_rope(qd, kd, pos, cos, sin, H),
                     "forward": lambda: F.train_forward(q_rot, k_rot, vd, H),
                     "backward": lambda: F.train_backward(q_rot, k_rot, vd, ctx, up, lse, pos, cos, sin, H)})
    pairs = B * H * D * L * (L + 1) / 2
    for name, products in (("rope", 0), ("forward", 2), ("backward", 7)):
        r[name + "_entry_us"], r[name + "_entry_spread_us"] = round(e[name][0] * 1e3, 1), round(e[name][1] * 1e3, 1)
        if products:
            tf = 2 * products * pairs / (e[name][0] * 1e-3) / 1e12
            r[name + "_mfma_TFLOPs"], r[name + "_share_of_bf16_rate"] = round(tf, 1), round(tf / PEAK_TFLOPS, 4)
    return r


def trace(L, n=5):
    q, k, v, up, pos, cos, sin = problem(L)
    for _ in range(n):
        q_rot, k_rot = F.train_rope(q, k, pos, cos, sin, H)
        ctx, lse = F.train_forward(q_rot, k_rot, v, H)
        F.train_backward(q_rot, k_rot, v, ctx, up, lse, pos, cos, sin, H)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--trace", type=int, default=0, help="run the kernels alone at this length (for rocprofv3)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("llama_train_bench: needs the GPU")
    if args.trace:
        trace(args.trace)
        return
    rows = [lines(L) for L in LENGTHS]
    for r in rows:
        print(json.dumps(r))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
