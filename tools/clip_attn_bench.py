"""The CLIP ViT's self-attention, the Linear layers excluded, on one MI355X: H = 16, D = 64, bf16, at
(B, L) = (32, 257) -- a batch of 224 px images -- and (8, 1025) -- 448 px.  Forward alone and forward + backward, three
lines each, interleaved in one process (the median of 5 rounds and their spread):

  kernels     csrc/mmfs_clip_attn.hip through ``mmfs_amd.clip_attention``: forward; dq, dkdv
  framework   the module's framework statement (CLIPSelfAttention._framework): q / 8, bmm, softmax in T, bmm -- [B H, L, L]
              scores, autograd
  sdpa        for information: torch.nn.functional.scaled_dot_product_attention on the split heads, if this torch build
              serves it on the device

and the time of each entry of the C ABI by device events (forward; backward = dq + dkdv) with the algorithmic matrix-core
FLOPs over it: 4 / 6 / 8 B H L^2 64 for forward / dq / dkdv (2, 3 and 4 products), 14 for the backward entry, against the
chip's 2.5 PFLOP/s bf16 rate (MI355X_MICROARCH.md).  ``--trace B,L`` runs the kernels alone a few times at one shape: the
program to put behind ``rocprofv3 --kernel-trace --stats --`` for the split of the backward into its two kernels.

    python tools/clip_attn_bench.py [--json out.json]
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
from mmfs_amd.clip_attn import CLIPSelfAttention, shape_class  # noqa: E402
from mmfs_amd.functions import clip_attn_func as F  # noqa: E402

dev = torch.device("cuda:0")
DT = torch.bfloat16
H, D = 16, 64
SHAPES = ((32, 257), (8, 1025))
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


def problem(B, L):
    gen = torch.Generator().manual_seed(L)
    return tuple(torch.randn(B, L, H * D, generator=gen).to(dev, DT) for _ in range(4))


def lines(B, L):
    q, k, v, up = problem(B, L)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    cfg = types.SimpleNamespace(hidden_size=H * D, num_attention_heads=H, attention_dropout=0.0)
    with torch.device("meta"):
        m = CLIPSelfAttention(cfg).eval()                                    # (for _framework: no Linear layer runs)
    split = lambda x: x.unflatten(-1, (H, D)).transpose(1, 2)

    def framework_ctx(a, b, c):
        return m._framework(a, b, c, None, None, False)[0]

    def sdpa_ctx(a, b, c):
        return torch.nn.functional.scaled_dot_product_attention(split(a), split(b), split(c)).transpose(1, 2).flatten(2)

    routes = {"kernels": lambda a, b, c: mmfs_amd.clip_attention(a, b, c, H), "framework": framework_ctx}
    try:
        torch.autograd.grad(sdpa_ctx(*leaves), leaves, up)
        torch.cuda.synchronize()
        routes["sdpa"] = sdpa_ctx
    except Exception as e:                                                   # not served by this build: the line is left out
        print(f"sdpa not served at L {L}: {type(e).__name__}: {e}", file=sys.stderr)

    def forward_of(f):
        def run():
            with torch.no_grad():
                return f(q, k, v)
        return run

    def both_of(f):
        return lambda: torch.autograd.grad(f(*leaves), leaves, up)

    # the lines compute the same thing
    a, b = both_of(routes["kernels"])(), both_of(routes["framework"])()
    diff = max(float((x.float() - y.float()).abs().max()) for x, y in zip(a, b))
    r = {"B": B, "L": L, "class": shape_class(L), "kernels_max_abs_to_framework": diff}
    for what, wrap in (("fwd", forward_of), ("fwdbwd", both_of)):
        t = interleaved({name: wrap(f) for name, f in routes.items()})
        for name, (med, spread) in t.items():
            r[f"{what}_{name}_us"], r[f"{what}_{name}_spread_us"] = round(med * 1e3, 1), round(spread * 1e3, 1)
        r[f"{what}_kernels_gain_exceeds_spreads"] = t["framework"][0] - t["kernels"][0] > max(t["framework"][1], t["kernels"][1])
    # each entry of the C ABI on its own
    ctx, lse = F.clip_forward(q, k, v, H)
    e = interleaved({"forward": lambda: F.clip_forward(q, k, v, H),
                     "backward": lambda: F.clip_backward(q, k, v, ctx, up, lse, H)})
    pairs = B * H * L * L * D
    for name, products in (("forward", 2), ("backward", 7)):
        r[name + "_entry_us"], r[name + "_entry_spread_us"] = round(e[name][0] * 1e3, 1), round(e[name][1] * 1e3, 1)
        tf = 2 * products * pairs / (e[name][0] * 1e-3) / 1e12
        r[name + "_mfma_TFLOPs"], r[name + "_share_of_bf16_rate"] = round(tf, 1), round(tf / PEAK_TFLOPS, 4)
    return r


def trace(B, L, n=5):
    q, k, v, up = problem(B, L)
    for _ in range(n):
        ctx, lse = F.clip_forward(q, k, v, H)
        F.clip_backward(q, k, v, ctx, up, lse, H)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--trace", default="", help="B,L: run the kernels alone at this shape (for rocprofv3)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("clip_attn_bench: needs the GPU")
    if args.trace:
        trace(*(int(x) for x in args.trace.split(",")))
        return
    rows = [lines(B, L) for B, L in SHAPES]
    for r in rows:
        print(json.dumps(r))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
