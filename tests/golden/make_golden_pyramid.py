#!/usr/bin/env python3
"""tests/golden/make_golden_pyramid.py -- golden vectors of the ViT-Adapter's output pyramid.

Runs ONLY in the build container, where the reference is mounted read-only (``REF`` of make_golden.py; the helpers of
make_golden.py and make_golden_adapter.py are reused as they are).  Nothing is copied: the reference's own statements
run in fp64,
  * ``SpatialPriorModule`` (adapter_modules.py, through make_golden_adapter's package shell) on a seeded image gives
    c1 [B, C, 4H, 4W] and the tokens c2 | c3 | c4;
  * the tail of ``CLIPVisionTransformerAdapter.forward`` (encoders/vit_adapter/vit_adapter_hf.py) from "Split & Reshape"
    to ``multiscale_features`` is compiled out of the file's AST and executed on those, on seeded ViT tokens x1..x4 and
    on a randomised ``adapter_up``;
  * the position step of ``VisualTokenizer.forward`` (encoders/visual_tokenizer.py: the loop over
    ``multiscale_features``) is compiled out of its AST the same way and run with the reference's
    ``get_2d_sincos_pos_embed`` / ``get_abs_pos`` (models/utils/pos_embed.py).

Stored as ``adapter_pyramid*.npz`` (parts as make_golden_adapter.save_parts writes them): the inputs (c, c1, x1..x4),
the ``adapter_up`` parameters, the sin-cos table and the four resized tables, the four outputs without and with the
tables (``out.l<k>`` / ``out_pos.l<k>``), one upstream gradient per level, all input and parameter gradients (the
tables are constants: the gradients are those of either run), and the reference's OWN error in fp32 / fp16 / bf16 per
output against its fp64 run, relative to the largest fp64 entry (``ref_err.<dtype>.l<k>`` without tables,
``ref_err_pos.<dtype>.l<k>`` with) -- the yardstick of the 16-bit GPU tests.

Geometry: a 96-px image (ViT map H = W = 6, pyramid 24^2 / 12^2 / 6^2 / 3^2 = 765 tokens), dim 64, B = 2, sin-cos grid 16.

Usage:  python tests/golden/make_golden_pyramid.py     (rewrites the adapter_pyramid*.npz files)
"""
import ast
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from einops import rearrange

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, randomise  # noqa: E402
from make_golden_adapter import import_reference_adapter, rel_err, save_parts  # noqa: E402

IMAGE, B, DIM, INPLANES, GRID = 96, 2, 64, 16, 16
ENC = os.path.join(REF, "mm_interleaved/models/encoders")


def statements_of(path, cls, func, first, last, args, result, ns):
    """The statements of ``cls.func`` in ``path`` from the first one ``first(node)`` accepts to the first one
    ``last(node)`` accepts, compiled from the file's AST as a function ``(args) -> result``."""
    tree = ast.parse(open(path).read())
    klass = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    fn = next(n for n in klass.body if isinstance(n, ast.FunctionDef) and n.name == func)
    lo = next(i for i, n in enumerate(fn.body) if first(n))
    hi = next(i for i, n in enumerate(fn.body) if i >= lo and last(n))
    shell = ast.parse(f"def run({', '.join(args)}):\n    pass\n    return {result}\n")
    shell.body[0].body[0:1] = fn.body[lo:hi + 1]
    ast.fix_missing_locations(shell)
    scope = dict(ns)
    exec(compile(shell, path, "exec"), scope)
    return scope["run"]


def assigns(name):
    def test(node):
        return isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets)
    return test


def reference_tail():
    """c2 = c[:, 0:c2.size(1), :] ... multiscale_features = [c1, c2, c3, c4]"""
    return statements_of(os.path.join(ENC, "vit_adapter/vit_adapter_hf.py"), "CLIPVisionTransformerAdapter", "forward",
                         assigns("c2"), assigns("multiscale_features"),
                         ("self", "c", "c1", "c2", "c3", "c4", "outs", "bs", "dim", "H", "W"), "multiscale_features",
                         {"torch": torch, "F": F})


def reference_pos_step(pos_mod):
    """multiscale_features_n = [] ; for ms_feat in multiscale_features: ... ; multiscale_features = multiscale_features_n"""
    return statements_of(os.path.join(ENC, "visual_tokenizer.py"), "VisualTokenizer", "forward",
                         assigns("multiscale_features_n"), assigns("multiscale_features"),
                         ("self", "multiscale_features"), "multiscale_features",
                         {"torch": torch, "rearrange": rearrange, "get_abs_pos": pos_mod.get_abs_pos})


def main():
    am = import_reference_adapter()
    spec = importlib.util.spec_from_file_location("ref_pos_embed", os.path.join(REF, "mm_interleaved/models/utils/pos_embed.py"))
    pos_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pos_mod)
    tail, pos_step = reference_tail(), reference_pos_step(pos_mod)

    gen = torch.Generator().manual_seed(70)
    H = W = IMAGE // 16
    spm = am.SpatialPriorModule(inplanes=INPLANES, embed_dim=DIM, with_cp=False).double()
    randomise(spm, gen)
    up = torch.nn.ConvTranspose2d(DIM, DIM, 2, 2).double()
    randomise(up, gen)
    params = {"adapter_up." + k: v.detach().clone() for k, v in up.state_dict().items()}
    with torch.no_grad():
        c1, c2, c3, c4 = spm(torch.randn(B, 3, IMAGE, IMAGE, generator=gen).double())
    sizes = (int(c2.shape[1]), int(c3.shape[1]), int(c4.shape[1]))
    assert tuple(c1.shape) == (B, DIM, 4 * H, 4 * W) and sizes == (4 * H * W, H * W, H * W // 4)
    # inputs are drawn / rounded in fp32 so that the fixture stores them losslessly
    inputs = {"c": torch.cat((c2, c3, c4), 1).float().double(), "c1": c1.float().double()}
    for k in range(1, 5):
        inputs[f"x{k}"] = torch.randn(B, H * W, DIM, generator=gen).double()
    pos_embed = torch.from_numpy(pos_mod.get_2d_sincos_pos_embed(DIM, GRID, cls_token=True)).float()
    grads_out = {l: torch.randn(B, DIM, s, s, generator=gen).double() for l, s in enumerate((4 * H, 2 * H, H, H // 2))}

    def run(dtype, with_pos, grad):
        holder = types.SimpleNamespace(adapter_up=torch.nn.ConvTranspose2d(DIM, DIM, 2, 2).to(dtype),
                                       pos_embed=pos_embed if dtype == torch.float64 else pos_embed.to(dtype))
        holder.adapter_up.load_state_dict({k: v.to(dtype) for k, v in up.state_dict().items()})
        xs = {k: v.to(dtype).requires_grad_(grad) for k, v in inputs.items()}
        c = xs["c"]
        parts = (c[:, :sizes[0]], c[:, sizes[0]:sizes[0] + sizes[1]], c[:, sizes[0] + sizes[1]:])
        outs = [xs[f"x{k}"].transpose(1, 2).view(B, DIM, H, W).contiguous() for k in range(1, 5)]
        feats = tail(holder, c, xs["c1"], *parts, outs, B, DIM, H, W)
        if with_pos:
            feats = pos_step(holder, feats)
        if grad:
            torch.autograd.backward(list(feats), [grads_out[l] for l in range(4)])
        return holder, xs, feats

    holder, xs, plain = run(torch.float64, False, True)
    with torch.no_grad():
        _, _, with_pos = run(torch.float64, True, False)
    arrays = {"image_hw": np.array([IMAGE, IMAGE]), "pos_embed": pos_embed}
    arrays.update({"in." + k: v for k, v in inputs.items()})
    arrays.update({"param." + k: v for k, v in params.items()})
    for l in range(4):
        side = int(plain[l].shape[-1])
        arrays[f"pos.l{l}"] = pos_mod.get_abs_pos(pos_embed[1:], side * side)
        arrays[f"out.l{l}"] = plain[l]
        arrays[f"out_pos.l{l}"] = with_pos[l]
        arrays[f"grad_out.l{l}"] = grads_out[l]
    arrays.update({"grad_in." + k: v.grad for k, v in xs.items()})
    arrays.update({"grad.adapter_up." + k: p.grad for k, p in holder.adapter_up.named_parameters()})
    for dt, tag in ((torch.float32, "fp32"), (torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        for key, flag, want in (("ref_err", False, plain), ("ref_err_pos", True, with_pos)):
            with torch.no_grad():
                _, _, low = run(dt, flag, False)
            for l in range(4):
                arrays[f"{key}.{tag}.l{l}"] = np.float64(rel_err(low[l], want[l].detach()))
    print({k: float(v) for k, v in arrays.items() if k.startswith("ref_err")})
    save_parts("adapter_pyramid", arrays)


if __name__ == "__main__":
    main()
