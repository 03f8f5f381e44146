#!/usr/bin/env python3
"""The text loss at the training step's shapes -- logits [2, 2048, 32003] and [8, 512, 32003], bf16 and
f32, L - 1 labels of which one in ten is ignored -- forward + backward, in the same interleaved rounds of one process:
  reference        the reference's four lines on the same logits: "b n c -> b c n", .float(), the slice made contiguous,
                   F.cross_entropy (restated here, in this project's own words)
  framework        mmfs_amd.text_loss with route="framework" (the logits stay where they are, the labels grow to [B, L])
  kernels          the kernels of csrc/mmfs_text_loss.hip
Per candidate: device ms per call (events around a synchronised batch), the median of 7 rounds with the rounds' spread
max - min; GB/s against the three-pass byte count (valid rows read twice, every row written once, in the storage type);
the peak of allocated memory above the resident tensors in one call.  Prints one JSON line; ``--md PATH`` also writes the
table.
    python tools/text_loss_bench.py [--md profiles/text_loss_table.md] [--iters 5]
Not the contract benchmark (bench.py)."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mm-interleaved_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

tl = importlib.import_module("mmfs_amd.text_loss")

dev = "cuda"
SHAPES = [(2, 2048, 32003), (8, 512, 32003)]
DTYPES = [("bf16", torch.bfloat16), ("f32", torch.float32)]


def timed(fn, iters):
    """device ms per call of a synchronised batch"""
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
        timed(f, 2)
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            got[k].append(timed(f, iters))
    return {k: dict(device_ms=round(statistics.median(v), 4), spread=round(max(v) - min(v), 4)) for k, v in got.items()}


def peak_above_resident(fn):
    """bytes of the allocation peak of one call above what was resident before it"""
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
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    result = {}
    for B, L, V in SHAPES:
        for tag, dt in DTYPES:
            gen = torch.Generator(device=dev).manual_seed(0)
            x = torch.empty((B, L, V), dtype=dt, device=dev).normal_(0.0, 3.0, generator=gen).requires_grad_(True)
            labels = torch.randint(0, V, (B, L - 1), device=dev, generator=gen)
            labels[torch.rand((B, L - 1), device=dev, generator=gen) < 0.1] = -100
            valid = int((labels != -100).sum())
            passes = (2 * valid + B * L) * V * x.element_size()
            last = {}

            def step(loss_of):
                def run():
                    loss = loss_of()
                    (grad,) = torch.autograd.grad(loss, x)
                    last["loss"], last["grad"] = loss.detach(), grad
                return run

            def reference():
                logits = x.permute(0, 2, 1).float()
                return F.cross_entropy(logits[..., :-1].contiguous(), labels.contiguous())

            framework = lambda: tl.text_loss(x, labels, route="framework")
            kernels = lambda: tl.text_loss(x, labels, route="kernels")
            fns = {"reference": step(reference), "framework": step(framework), "kernels": step(kernels)}
            # faster and different is not faster: the candidates' results on these very inputs
            fns["reference"]()
            want = last["loss"].double(), last["grad"].double()
            agree = {}
            for k in ("framework", "kernels"):
                fns[k]()
                agree[k] = dict(loss_rel=float((last["loss"].double() - want[0]).abs() / want[0].abs()),
                                grad_max_abs=float((last["grad"].double() - want[1]).abs().max()),
                                grad_scale=float(want[1].abs().max()))
            last.clear()
            rows = interleaved(fns, args.iters)
            for k, f in fns.items():
                last.clear()
                rows[k]["peak_MB"] = round(peak_above_resident(f) / 1e6, 1)
                rows[k]["GBps_three_pass"] = round(passes / rows[k]["device_ms"] / 1e6, 1)
            last.clear()
            result[f"{B}x{L}x{V}_{tag}"] = dict(valid_rows=valid, three_pass_MB=round(passes / 1e6, 1), agree=agree, rows=rows)
            del x
            torch.cuda.empty_cache()
    print(json.dumps(result))
    if args.md:
        lines = ["| logits | candidate | device ms | spread | GB/s of three passes | peak MB above resident |", "|---|---|---|---|---|---|"]
        for key, r in result.items():
            for name, v in r["rows"].items():
                lines.append(f"| {key} | {name} | {v['device_ms']} | {v['spread']} | {v['GBps_three_pass']} | {v['peak_MB']} |")
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
