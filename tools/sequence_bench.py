#!/usr/bin/env python3
"""The interleaved sequence at the LLM's shape -- B = 4, L = 2048, C = 4096, bf16, with 32 and with 4
images, max_len 1024 and 77 -- four ways in the same interleaved rounds of one process:
  loop           a plain per-image loop over nonzero() results with a host-built sin-cos table per call: what a caller
                 that has not changed pays (restated here, in this project's own words)
  framework      mmfs_amd.sequence with route="framework" (loop-free, sync-free framework ops)
  project_first  the kernels, projection over the B L tokens and then the gather
  gather_first   the kernels, gather and then the projection over the n_images max_len rows
and the embeddings (assemble_mm_embeds) three ways: loop-free reference statements with nonzero(), framework, kernels.
Per candidate: wall ms per call (host clock around a synchronised batch -- where the syncs show) and device ms per call
(events), medians of 7 rounds with the rounds' spread max - min.  Prints one JSON line; ``--md PATH`` also writes the
table.
    python tools/sequence_bench.py [--md profiles/sequence.md] [--iters 5]
Not the contract benchmark (bench.py)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mm-interleaved_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from mmfs_amd import sequence as seq  # noqa: E402

dev, dt = "cuda", torch.bfloat16
B, L, C, SEQ_LEN = 4, 2048, 4096, 2048
BOS, SOI, IMAGE, TOKENS_PER_IMAGE = 1, 5, 4, 64


def timed(fn, iters):
    """(wall ms, device ms) per call of a synchronised batch"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - w0) * 1e3 / iters, t0.elapsed_time(t1) / iters


def interleaved(fns, iters, rounds=7):
    """{name: wall / device medians and spreads (max - min over the rounds)}, the candidates' rounds alternating"""
    for f in fns.values():
        timed(f, 2)
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            got[k].append(timed(f, iters))
    out = {}
    for k, v in got.items():
        wall, device = [a for a, _ in v], [b for _, b in v]
        out[k] = dict(wall_ms=round(statistics.median(wall), 4), wall_spread=round(max(wall) - min(wall), 4),
                      device_ms=round(statistics.median(device), 4), device_spread=round(max(device) - min(device), 4))
    return out


def layout(n_images, max_len):
    """<soi> tokens evenly over the rows, each followed by image tokens; <bos> of an image so that the longest context
    is max_len"""
    gen = torch.Generator().manual_seed(0)
    ids = torch.randint(10, 1000, (B, L), generator=gen)
    per_row = n_images // B
    cols = [(k + 1) * (L // per_row) - 1 - TOKENS_PER_IMAGE for k in range(per_row)]
    for r in range(B):
        for c in cols:
            ids[r, c] = SOI
            ids[r, c + 1:c + 1 + TOKENS_PER_IMAGE] = IMAGE
    bos = torch.tensor([max(0, c + 1 - max_len) for _ in range(B) for c in cols])
    return ids.to(dev), bos.to(dev)


def loop_context(context, ids, bos, proj):
    """per image: slice with device scalars, flip, copy into a zero-filled buffer; project every padded row; add a table
    made on the host"""
    rows, cols = (ids == SOI).nonzero(as_tuple=True)
    lengths = cols - bos + 1
    longest = int(max(lengths))
    n = cols.shape[0]
    feats = torch.zeros((n, longest, C), dtype=context.dtype, device=context.device)
    mask = torch.zeros((n, longest), dtype=torch.long, device=context.device)
    for i in range(n):
        piece = context[rows[i], bos[i]:cols[i] + 1].flip(0)
        feats[i, :lengths[i]] = piece
        mask[i, :lengths[i]] = 1
    freq = 1.0 / 10000 ** (np.arange(C // 2, dtype=np.float32) / (C / 2.0))
    angle = np.arange(SEQ_LEN, dtype=np.float32)[:, None] * freq[None, :]
    table = torch.from_numpy(np.concatenate([np.sin(angle), np.cos(angle)], axis=1)).to(context)
    return proj(feats) + table[None, :longest], mask


def loop_embeds(text, ids, vis, soi):
    flat = text.reshape(B * L, C).to(vis.dtype)
    r, c = (ids == IMAGE).nonzero(as_tuple=True)
    at = (r * L + c)[:, None].expand(-1, C)
    assert at.shape[0] == vis.shape[0]
    out = torch.scatter(flat, 0, at, vis)
    r, c = (ids == SOI).nonzero(as_tuple=True)
    at = (r * L + c)[:, None].expand(-1, C)
    return torch.scatter_add(out, 0, at, soi.repeat(at.shape[0], 1)).view(B, L, C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md")
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    torch.manual_seed(0)
    proj = torch.nn.Linear(C, C).to(dev, dt)
    context = torch.randn(B, L, C, device=dev, dtype=dt)
    text = torch.randn(B, L, C, device=dev, dtype=dt)
    soi = torch.randn(1, C, device=dev, dtype=dt)
    result = dict(shape=dict(B=B, L=L, C=C, dtype="bf16", seq_len=SEQ_LEN), context={}, embeds={})
    with torch.no_grad():
        for n_images in (32, 4):
            for max_len in (1024, 77):
                ids, bos = layout(n_images, max_len)

                def ours(route, order):
                    return lambda: seq.prepare_context_features_for_image_decoder(
                        context, ids, proj, soi_token_id=SOI, n_images=n_images, seq_len=SEQ_LEN, nearest_bos_idxs=bos,
                        max_len=max_len, order=order, route=route)
                fns = {"loop": lambda: loop_context(context, ids, bos, proj),
                       "framework_project_first": ours("framework", "project_first"),
                       "framework_gather_first": ours("framework", "gather_first"),
                       "kernels_project_first": ours("kernels", "project_first"),
                       "kernels_gather_first": ours("kernels", "gather_first")}
                a, b = fns["loop"](), fns["kernels_project_first"]()
                assert a[0].shape == b[0].shape and torch.equal(a[1], b[1])
                key = f"images{n_images}_maxlen{max_len}"
                result["context"][key] = interleaved(fns, args.iters)
                result["context"][key]["auto_takes"] = "project_first" if B * L <= n_images * max_len else "gather_first"
            vis = torch.randn(n_images * TOKENS_PER_IMAGE, C, device=dev, dtype=dt)

            def embeds(route):
                return lambda: seq.assemble_mm_embeds(text, ids, vis, soi, image_token_id=IMAGE, soi_token_id=SOI, route=route)
            fns = {"loop": lambda: loop_embeds(text, ids, vis, soi), "framework": embeds("framework"), "kernels": embeds("kernels")}
            assert torch.equal(fns["loop"](), fns["kernels"]())
            result["embeds"][f"images{n_images}"] = interleaved(fns, args.iters)
    print(json.dumps(result))
    if args.md:
        lines = ["| call | candidate | wall ms | spread | device ms | spread |", "|---|---|---|---|---|---|"]
        for group in ("context", "embeds"):
            for key, rows in result[group].items():
                for name, v in rows.items():
                    if isinstance(v, dict):
                        lines.append(f"| {group} {key} | {name} | {v['wall_ms']} | {v['wall_spread']} | {v['device_ms']} | "
                                     f"{v['device_spread']} |")
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
