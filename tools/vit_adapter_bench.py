#!/usr/bin/env python3
"""The image encoder's MSDeformAttn front end: framework ops (``fused_front_end`` off, the code path
before the switch existed) against the fused plan kernels, and plan + op against the fused sampler for calls without
gradients, at the ViT-Adapter's shapes in bf16 -- d_model 1024, 16 heads, D = 32, P = 4, B = 32:
  injector   256 queries over the 32^2 / 16^2 / 8^2 pyramid
  extractor  1344 queries over the 16^2 map
for the module alone and for a whole ``InteractionBlockWithCls`` (identity ``blocks``, one extractor with its ConvFFN):
ms for forward + backward, ms for the no-grad forward (medians of interleaved rounds, with the rounds' spread
max - min), and kernel launches per call.  Prints one JSON line.
    python tools/vit_adapter_bench.py
    python tools/vit_adapter_bench.py prof off|on [framework|kernel]   # only runs the block (for rocprofv3 --kernel-trace --stats)
    python tools/vit_adapter_bench.py dwconv          # ConvFFN's depthwise convolution: the framework
                                                      # statement (``DWConv.token_kernel`` off, the only path before the
                                                      # switch existed) against the token kernel, for ``ConvFFN`` alone
                                                      # and for the block, in the same interleaved rounds
    python tools/vit_adapter_bench.py pyramid [nhwc]  # the output pyramid: the framework statement
                                                      # (``AdapterPyramidHead.token_kernel`` off) against the token
                                                      # kernels, all four levels and without the 64^2 level, c1 in NCHW
                                                      # (or channels_last), in the same interleaved rounds; + the
                                                      # kernels' algorithmic bytes
    python tools/vit_adapter_bench.py prof pyramid framework|kernel [all|no1] [nhwc]   # only runs the head
Not the contract benchmark (bench.py)."""
import json
import os
import statistics
import sys
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mm-interleaved_amd")]
import torch  # noqa: E402
from mmfs_amd.blocks import AdapterPyramidHead, ConvFFN, DWConv, InteractionBlockWithCls, deform_inputs  # noqa: E402
from mmfs_amd.modules import MSDeformAttn  # noqa: E402

dev, dt = "cuda", torch.bfloat16
DIM, HEADS, P, B, IMAGE = 1024, 16, 4, 32, 256
Hidden = namedtuple("Hidden", "last_hidden_state")
SETTINGS = {"off": (False, False), "on": (True, False), "on_sampler": (True, True)}   # fused_front_end, fused_sampler


def ms(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def interleaved(fns, iters, rounds=7):
    """{name: (median ms per call, max - min over the rounds)}, the candidates' rounds alternating"""
    for f in fns.values():
        ms(f, 3)
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            got[k].append(ms(f, iters))
    return {k: dict(ms=round(statistics.median(v), 4), spread=round(max(v) - min(v), 4)) for k, v in got.items()}


def launches(fn):
    """Kernels one call launches (the profiler's device events), or None where the profiler gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:
        return None


def set_route(module, setting):
    fused, sampler = SETTINGS[setting]
    for m in module.modules():
        if isinstance(m, MSDeformAttn):
            m.fused_front_end, m.fused_sampler = fused, sampler


def set_dwconv_route(module, setting):
    """"framework" | "kernel" for every DWConv of the module; the attention modules on their defaults"""
    set_route(module, "on_sampler")
    for m in module.modules():
        if isinstance(m, DWConv):
            m.token_kernel = setting == "kernel"


def randomise(module):
    torch.manual_seed(0)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, MSDeformAttn):
                m.sampling_offsets.weight.normal_(0, 0.01)
                m.attention_weights.weight.normal_(0, 0.02)
        for n, p in module.named_parameters():
            if n.endswith("gamma"):
                p.fill_(0.5)


def candidates(module, call, inputs, set_route=set_route):
    """fwd+bwd / no-grad closures per setting; the module's route is switched inside the closure (an attribute write)."""
    grads = [t for t in inputs if t.requires_grad] + list(module.parameters())

    def train(setting):
        def f():
            set_route(module, setting)
            module.train()
            out = call(module)
            outs = out if isinstance(out, tuple) else (out,)
            torch.autograd.grad([o for o in outs], grads, [torch.ones_like(o) for o in outs], allow_unused=True)
        return f

    def infer(setting):
        def f():
            set_route(module, setting)
            module.eval()
            with torch.no_grad():
                call(module)
        return f

    return train, infer


def measure(module, call, inputs, iters):
    train, infer = candidates(module, call, inputs)
    t = interleaved({s: train(s) for s in ("off", "on")}, iters)
    i = interleaved({s: infer(s) for s in SETTINGS}, iters)
    return dict(fwd_bwd=t, nograd_fwd=i,
                launches=dict(fwd_bwd={s: launches(train(s)) for s in ("off", "on")},
                              nograd_fwd={s: launches(infer(s)) for s in SETTINGS}))


def measure_dwconv(module, call, inputs, iters):
    train, infer = candidates(module, call, inputs, set_dwconv_route)
    routes = ("framework", "kernel")
    return dict(fwd_bwd=interleaved({s: train(s) for s in routes}, iters),
                nograd_fwd=interleaved({s: infer(s) for s in routes}, iters),
                launches=dict(fwd_bwd={s: launches(train(s)) for s in routes},
                              nograd_fwd={s: launches(infer(s)) for s in routes}))


def pyramid_bytes(Bn, H, W, C, mask, nhwc, tables=True, e=2):
    """Algorithmic bytes of the pyramid head's kernels from the shapes: every input read once, every output written
    once, position tables (fp32) once per call; the backward's level-1 rows are read by each kernel that needs them.
    The forward's framework ops in front of level 1 (the copy of c2 and the GEMM) are listed too."""
    px = [16 * H * W, 4 * H * W, H * W, H * W // 4]
    on = [(mask >> l) & 1 for l in range(4)]
    row = C * e * Bn
    tab = [C * 4 * n if tables else 0 for n in px]
    lvl1 = (3 * px[0] + px[2]) * row + tab[0]                                  # up, c1, out + x1
    rows = sum((2 * px[l] + px[2]) * row + tab[l] for l in (1, 2, 3) if on[l])   # c_l, out + x_l
    out = {"pyramid_fwd_rows": rows + (lvl1 if on[0] and nhwc else 0)}
    if on[0] and not nhwc:
        out["pyramid_fwd_c1_nchw"] = lvl1
    back = sum((px[l] + px[2]) * row for l in (1, 2, 3) if on[l])              # g_l read, g_x_l written
    if on[0]:
        back += (2 * px[0] + px[0] + px[2]) * row + (px[0] * row if nhwc else 0)   # g_1 -> g_up (+ g_c1); g_1 -> g_x1
        if not nhwc:
            out["pyramid_bwd_c1_nchw"] = 2 * px[0] * row
    out["pyramid_bwd_rows"] = back
    if on[0]:       # the framework ops in front of level 1: c2 gathered out of c (a copy for B > 1), then the GEMM
        out["adapter_up_c2_copy"] = 2 * px[1] * row
        out["adapter_up_gemm"] = (px[1] + px[0]) * row + 4 * C * C * e
    return out


def pyramid_setup(nhwc):
    torch.manual_seed(2)
    H = W = IMAGE // 16
    head = AdapterPyramidHead(DIM).to(dev, dt)
    rn = lambda *s: torch.randn(*s, device=dev, dtype=dt).requires_grad_(True)     # noqa: E731
    c = rn(B, 21 * H * W // 4, DIM)
    xs = [rn(B, H * W, DIM) for _ in range(4)]
    c1 = torch.randn(B, DIM, 4 * H, 4 * W, device=dev, dtype=dt)
    if nhwc:
        c1 = c1.contiguous(memory_format=torch.channels_last)
    c1.requires_grad_(True)
    pos = torch.randn(1 + 16 * 16, DIM, device=dev)              # the reference's table: a 16 x 16 grid behind a class-token row
    return head, c, xs, c1, pos, H, W


def set_pyramid_route(module, setting):
    module.token_kernel = setting == "kernel"


def main_pyramid(args):
    nhwc = "nhwc" in args
    head, c, xs, c1, pos, H, W = pyramid_setup(nhwc)
    masks = {"all": (0, 1, 2, 3), "no1": (1, 2, 3)}
    if args[:1] == ["prof"]:
        levels = masks["no1" if "no1" in args else "all"]
        train, infer = candidates(head, lambda m: m(c, xs, c1, H, W, pos_embed=pos, levels=levels), [c, c1] + xs,
                                  set_pyramid_route)
        f, g = train(args[2]), infer(args[2])
        for _ in range(30):
            f()
            g()
        torch.cuda.synchronize()
        return
    routes = ("framework", "kernel")
    result = dict(shape=dict(C=DIM, H=H, W=W, B=B, dtype="bf16", c1="channels_last" if nhwc else "nchw", tables=True))
    for name, levels in masks.items():
        train, infer = candidates(head, lambda m: m(c, xs, c1, H, W, pos_embed=pos, levels=levels), [c, c1] + xs,
                                  set_pyramid_route)
        result[name] = dict(fwd_bwd=interleaved({s: train(s) for s in routes}, 10),
                            nograd_fwd=interleaved({s: infer(s) for s in routes}, 10),
                            launches=dict(fwd_bwd={s: launches(train(s)) for s in routes},
                                          nograd_fwd={s: launches(infer(s)) for s in routes}),
                            kernel_bytes=pyramid_bytes(B, H, W, DIM, sum(1 << l for l in levels), nhwc))
    print(json.dumps(result))


def main():
    args = sys.argv[1:]
    if args[:1] == ["pyramid"] or args[:2] == ["prof", "pyramid"]:
        return main_pyramid(args[1:] if args[0] == "pyramid" else args)
    image = torch.zeros(1, 3, IMAGE, IMAGE, device=dev)
    d1, d2 = deform_inputs(image)
    hw = IMAGE // 16
    n_vit, n_pyr = hw * hw, int(d1[1].prod(1).sum())
    x = torch.randn(B, n_vit, DIM, device=dev, dtype=dt).requires_grad_(True)
    c = torch.randn(B, n_pyr, DIM, device=dev, dtype=dt).requires_grad_(True)
    cls = torch.randn(B, 1, DIM, device=dev, dtype=dt).requires_grad_(True)
    block = InteractionBlockWithCls(dim=DIM, num_heads=HEADS, n_points=P, cffn_ratio=0.25, deform_ratio=0.5).to(dev, dt)
    randomise(block)
    call_block = lambda m: m(x, c, cls, lambda t: Hidden(t), d1, d2, hw, hw)     # noqa: E731
    if args[:1] == ["prof"]:
        train, infer = candidates(block, call_block, [x, c, cls])
        f, g = train(args[1]), infer(args[1])
        if args[2:]:                                   # the depthwise convolution's route, set once: the closures leave it alone
            set_dwconv_route(block, args[2])
        for _ in range(30):
            f()
            g()
        torch.cuda.synchronize()
        return
    if args[:1] == ["dwconv"]:
        torch.manual_seed(1)
        ffn = ConvFFN(DIM, int(DIM * 0.25)).to(dev, dt)
        result = dict(shape=dict(d_model=DIM, hidden=int(DIM * 0.25), B=B, tokens=n_pyr, dtype="bf16"))
        result["conv_ffn"] = measure_dwconv(ffn, lambda m: m(c, hw, hw), [c], 20)
        result["interaction_block_cls"] = measure_dwconv(block, call_block, [x, c, cls], 10)
        print(json.dumps(result))
        return
    inj = MSDeformAttn(d_model=DIM, n_levels=3, n_heads=HEADS, n_points=P, ratio=0.5).to(dev, dt)
    ext = MSDeformAttn(d_model=DIM, n_levels=1, n_heads=HEADS, n_points=P, ratio=0.5).to(dev, dt)
    randomise(inj)
    randomise(ext)
    result = dict(shape=dict(d_model=DIM, heads=HEADS, D=DIM // 2 // HEADS, P=P, B=B, dtype="bf16", injector_queries=n_vit,
                             extractor_queries=n_pyr))
    result["module_injector"] = measure(inj, lambda m: m(x, d1[0], c, d1[1], d1[2]), [x, c], 20)
    result["module_extractor"] = measure(ext, lambda m: m(c, d2[0], x, d2[1], d2[2]), [x, c], 20)
    result["interaction_block_cls"] = measure(block, call_block, [x, c, cls], 10)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
