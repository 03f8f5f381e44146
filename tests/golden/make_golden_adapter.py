#!/usr/bin/env python3
"""tests/golden/make_golden_adapter.py -- golden vectors of the ViT-Adapter's interaction blocks.

Runs ONLY in the build container, where the reference is mounted read-only (``REF`` of make_golden.py, whose
helpers this script reuses).  It imports the reference's
``encoders/vit_adapter/adapter_modules.py`` through a package shell (nothing is copied), with
  * the module's ``MSDeformAttnFunction`` bound to the reference's own ``ms_deform_attn_core_pytorch`` (the native
    extension cannot be built here), and
  * a stub ``timm.models.layers.DropPath`` (``timm`` is not installed; no fixture uses drop_path > 0),
feeds the blocks seeded inputs in fp64 and stores inputs, parameters, outputs, one upstream gradient per output,
input gradients and parameter gradients as ``.npz`` data:

    adapter_injector          Injector  (ViT tokens query the 3-level pyramid)
    adapter_extractor         Extractor with its ConvFFN  (pyramid tokens query the ViT map)
    adapter_interaction_cls   InteractionBlockWithCls, extra_extractor=True, ``blocks`` = t -> t + tanh(t @ Wb)

Geometry: dim 128, 2 heads, deform_ratio 0.5 (D = 32 as in the adapter), P = 4, cffn_ratio 0.25, a 128-px image
(pyramid 16^2 / 8^2 / 4^2 = 336 tokens, ViT map 8^2 = 64 tokens), B = 2.  ``gamma`` is randomised with the other
parameters (it initialises to 0, which would hide the injector).

Each fixture also holds the reference's OWN low-precision error: the same block run by the reference in bf16 and
fp16 on the CPU against its fp64 run, per output, relative to the largest fp64 entry (``ref_err.<dtype>.<output>``)
-- the yardstick of the 16-bit GPU tests.

A fixture larger than the repository's limit for one file is written in parts, ``<name>.npz`` and
``<name>.p<k>.npz``; tests read them back as one dictionary.

Usage:  python tests/golden/make_golden_adapter.py     (rewrites the adapter_*.npz files)
"""
import glob
import importlib
import os
import sys
import types
from collections import namedtuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, randomise  # noqa: E402

PART_BYTES = 900 * 1024          # per committed file (the repository's limit is 1 MiB)
GEOM = dict(dim=128, num_heads=2, n_points=4, deform_ratio=0.5, cffn_ratio=0.25)
IMAGE, B = 128, 2


def import_reference_adapter():
    """adapter_modules.py inside a shell of its package (its __init__ imports the CLIP ViT and more)."""
    if "timm" not in sys.modules:
        class DropPath(torch.nn.Module):         # never applied: every fixture has drop_path = 0
            def __init__(self, drop_prob=0.0):
                super().__init__()
                self.drop_prob = drop_prob

            def forward(self, x):
                assert self.drop_prob == 0.0 or not self.training
                return x

        for name in ("timm", "timm.models", "timm.models.layers"):
            sys.modules[name] = types.ModuleType(name)
        sys.modules["timm.models.layers"].DropPath = DropPath
    name = "ref_vit_adapter"
    if name not in sys.modules:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, "mm_interleaved/models/encoders/vit_adapter")]
        sys.modules[name] = m
    funcs = importlib.import_module(name + ".ops.functions.ms_deform_attn_func")
    attn = importlib.import_module(name + ".ops.modules.ms_deform_attn")

    class CoreAsFunction:
        @staticmethod
        def apply(value, shapes, start, loc, attn_w, im2col_step):
            return funcs.ms_deform_attn_core_pytorch(value, shapes, loc, attn_w)

    attn.MSDeformAttnFunction = CoreAsFunction
    return importlib.import_module(name + ".adapter_modules")


def save_parts(name, arrays):
    for old in glob.glob(os.path.join(OUT, name + ".npz")) + glob.glob(os.path.join(OUT, name + ".p*.npz")):
        os.remove(old)
    conv = {}
    for k, v in arrays.items():
        v = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
        if v.dtype == np.float64 and np.array_equal(v.astype(np.float32).astype(np.float64), v):
            v = v.astype(np.float32)             # lossless: inputs / parameters are drawn in fp32
        conv[k] = v
    parts, size = [{}], 0
    for k, v in conv.items():
        if size and size + v.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += v.nbytes
    for i, part in enumerate(parts):
        path = os.path.join(OUT, name + (".npz" if i == 0 else f".p{i}.npz"))
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < (1 << 20), path
        print(f"{os.path.basename(path)}  {os.path.getsize(path) / 1024:.0f} KiB")


def rel_err(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


def run_case(make, inputs, call, out_names, grads_out, dtype):
    """Build the reference module, load ``make.params`` if given, run forward (+ backward in fp64)."""
    m = make.build().to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in make.params.items()})
    xs = {k: v.to(dtype).requires_grad_(dtype == torch.float64) for k, v in inputs.items()}
    outs = call(m, xs, dtype)
    outs = dict(zip(out_names, outs if isinstance(outs, tuple) else (outs,)))
    if dtype == torch.float64:
        torch.autograd.backward([outs[n] for n in out_names], [grads_out[n] for n in out_names])
    return m, xs, outs


Case = namedtuple("Case", "build params")


def adapter_case(name, build, cfg, inputs, call, out_names, seed, extra=None):
    gen = torch.Generator().manual_seed(seed)
    ref = build().double()
    randomise(ref, gen)
    make = Case(build, {k: v.detach().clone() for k, v in ref.state_dict().items()})
    inputs = {k: torch.randn(shape, generator=gen).double() for k, shape in inputs.items()}
    extra = {k: (torch.randn(shape, generator=gen) * scale).double() for k, (shape, scale) in (extra or {}).items()}
    call_x = lambda m, xs, dt: call(m, xs, {k: v.to(dt) for k, v in extra.items()})     # noqa: E731
    _, _, probe = run_case(make, inputs, call_x, out_names, None, torch.float32)
    grads_out = {n: torch.randn(probe[n].shape, generator=gen).double() for n in out_names}
    m, xs, outs = run_case(make, inputs, call_x, out_names, grads_out, torch.float64)
    arrays = {"cfg": np.array(repr(cfg))}
    arrays.update({"in." + k: v for k, v in inputs.items()})
    arrays.update({"extra." + k: v for k, v in extra.items()})
    arrays.update({"param." + k: v for k, v in make.params.items()})
    arrays.update({"out." + n: outs[n] for n in out_names})
    arrays.update({"grad_out." + n: grads_out[n] for n in out_names})
    arrays.update({"grad_in." + k: v.grad for k, v in xs.items()})
    arrays.update({"grad." + k: p.grad for k, p in m.named_parameters()})
    # the reference's own 16-bit error, per output
    for dt, tag in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        with torch.no_grad():
            _, _, lp = run_case(make, inputs, call_x, out_names, None, dt)
        for n in out_names:
            arrays[f"ref_err.{tag}.{n}"] = np.float64(rel_err(lp[n], outs[n].detach()))
    with torch.no_grad():
        _, _, f32 = run_case(make, inputs, call_x, out_names, None, torch.float32)
    for n in out_names:
        arrays[f"ref_err.fp32.{n}"] = np.float64(rel_err(f32[n], outs[n].detach()))
    print(name, {k: float(v) for k, v in arrays.items() if k.startswith("ref_err.")})
    return arrays


def main():
    am = import_reference_adapter()
    dim = GEOM["dim"]
    image = torch.zeros(B, 3, IMAGE, IMAGE)
    di1, di2 = am.deform_inputs(image)
    hw = IMAGE // 16
    n_vit, n_pyr = hw * hw, int(di1[1].prod(1).sum())
    deform = {"di1.reference_points": di1[0], "di1.spatial_shapes": di1[1], "di1.level_start_index": di1[2],
              "di2.reference_points": di2[0], "di2.spatial_shapes": di2[1], "di2.level_start_index": di2[2],
              "image_hw": np.array([IMAGE, IMAGE])}
    ref_of = lambda di, dt: [di[0].to(dt), di[1], di[2]]     # noqa: E731

    cfg = dict(dim=dim, num_heads=GEOM["num_heads"], n_points=GEOM["n_points"], n_levels=3,
               deform_ratio=GEOM["deform_ratio"], init_values=0.0)
    arrays = adapter_case(
        "adapter_injector", lambda: am.Injector(**cfg), cfg, {"query": (B, n_vit, dim), "feat": (B, n_pyr, dim)},
        lambda m, xs, ex: m(xs["query"], di1[0].to(xs["query"].dtype), xs["feat"], di1[1], di1[2]), ("out",), seed=60)
    save_parts("adapter_injector", {**arrays, **deform})

    cfg = dict(dim=dim, num_heads=GEOM["num_heads"], n_points=GEOM["n_points"], n_levels=1,
               deform_ratio=GEOM["deform_ratio"], with_cffn=True, cffn_ratio=GEOM["cffn_ratio"])
    arrays = adapter_case(
        "adapter_extractor", lambda: am.Extractor(**cfg), cfg, {"query": (B, n_pyr, dim), "feat": (B, n_vit, dim)},
        lambda m, xs, ex: m(xs["query"], di2[0].to(xs["query"].dtype), xs["feat"], di2[1], di2[2], hw, hw), ("out",),
        seed=61)
    save_parts("adapter_extractor", {**arrays, **deform})

    cfg = dict(dim=dim, num_heads=GEOM["num_heads"], n_points=GEOM["n_points"], cffn_ratio=GEOM["cffn_ratio"],
               init_values=0.0, deform_ratio=GEOM["deform_ratio"], extra_extractor=True)
    Hidden = namedtuple("Hidden", "last_hidden_state")

    def call_block(m, xs, ex):
        dt = xs["x"].dtype
        blocks = lambda t: Hidden(t + torch.tanh(t @ ex["Wb"]))     # noqa: E731
        return m(xs["x"], xs["c"], xs["cls"], blocks, ref_of(di1, dt), ref_of(di2, dt), hw, hw)

    arrays = adapter_case(
        "adapter_interaction_cls", lambda: am.InteractionBlockWithCls(**cfg), cfg,
        {"x": (B, n_vit, dim), "c": (B, n_pyr, dim), "cls": (B, 1, dim)}, call_block, ("x", "c", "cls"), seed=62,
        extra={"Wb": ((dim, dim), 1.0 / dim ** 0.5)})
    save_parts("adapter_interaction_cls", {**arrays, **deform})


if __name__ == "__main__":
    main()
