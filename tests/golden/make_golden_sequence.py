#!/usr/bin/env python3
"""tests/golden/make_golden_sequence.py -- golden vectors of the interleaved sequence (mmfs_amd/sequence.py).

Runs ONLY in the build container, where the reference is mounted read-only (``REF`` of make_golden.py).  Nothing is
copied: ``MMInterleaved._prepare_mm_embeds`` and ``MMInterleaved._prepare_context_features_for_image_decoder``
(mm_interleaved/models/mm_interleaved.py) are compiled out of the file's AST and run in fp64 against a stub ``self``
that holds what the two methods touch -- ``special_token_dict``, ``seq_len``, a seeded square ``context_feat_proj``, a
seeded ``soi_token``, a tokenizer that returns seeded ``vis_embed``, ``get_input_embeddings`` over a seeded table -- with
the reference's own ``get_1d_sincos_pos_embed_from_grid`` (models/utils/pos_embed.py).

Layout (B = 3, L = 24, C = 16, seq_len = 32):
    row 0   <bos> at 0, <soi> at 5 + two image tokens, <bos> at 12, <soi> at 20 + two image tokens
    row 1   no image
    row 2   <soi> at 1 + two image tokens, <soi> at 23 (the last column)
``sequence_bos.npz``:   nearest_bos_idxs = [0, 12, 0, 0]: lengths [6, 9, 2, 24], L_max = 24 -- a document boundary, two
                        images sharing context in one row, a context of two tokens, one of full length (no padding).
``sequence_start.npz``: nearest_bos_idxs = None and image_start_token_idx = [7, 22, 3, 23] (the last image token of each
                        image): lengths [8, 23, 4, 24].
Each file stores the inputs, the fp32 sin-cos table, mm_embeds, the features and the int64 mask, one upstream gradient
per output and the fp64 gradients of text_embeds, vis_embed, soi_token, context_features, the weight and the bias.

Usage:  python tests/golden/make_golden_sequence.py     (rewrites tests/golden/sequence_*.npz)
"""
import ast
import importlib.util
import os
import sys
import types
import typing

import numpy as np
import torch
from einops import rearrange

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, save  # noqa: E402

B, L, C, SEQ_LEN, VOCAB = 3, 24, 16, 32, 64
BOS, SOI, IMAGE = 1, 60, 61
MODEL = os.path.join(REF, "mm_interleaved/models/mm_interleaved.py")
POS = os.path.join(REF, "mm_interleaved/models/utils/pos_embed.py")


def reference_methods(names):
    """The named methods of ``MMInterleaved``, compiled from the file's AST as plain functions of (self, ...)."""
    spec = importlib.util.spec_from_file_location("ref_pos_embed", POS)
    pos_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pos_mod)
    tree = ast.parse(open(MODEL).read())
    klass = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "MMInterleaved")
    scope = {"torch": torch, "np": np, "rearrange": rearrange, "Optional": typing.Optional, "Union": typing.Union,
             "List": typing.List, "get_1d_sincos_pos_embed_from_grid": pos_mod.get_1d_sincos_pos_embed_from_grid}
    for node in klass.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), MODEL, "exec"), scope)
    return [scope[n] for n in names], pos_mod


def text_ids():
    gen = torch.Generator().manual_seed(140)
    ids = torch.randint(2, 50, (B, L), generator=gen)
    ids[:, 0] = BOS
    ids[0, 5], ids[0, 6], ids[0, 7] = SOI, IMAGE, IMAGE
    ids[0, 12] = BOS
    ids[0, 20], ids[0, 21], ids[0, 22] = SOI, IMAGE, IMAGE
    ids[2, 1], ids[2, 2], ids[2, 3] = SOI, IMAGE, IMAGE
    ids[2, 23] = SOI
    return ids


def main():
    (embeds, context), pos_mod = reference_methods(["_prepare_mm_embeds", "_prepare_context_features_for_image_decoder"])
    gen = torch.Generator().manual_seed(141)
    draw = lambda *shape: torch.randn(*shape, generator=gen).double()        # (fp32 draws: stored losslessly)
    ids = text_ids()
    table, vis = draw(VOCAB, C), draw(3, 2, C)
    proj = torch.nn.Linear(C, C).double()
    with torch.no_grad():
        proj.weight.copy_(draw(C, C) * 0.3)
        proj.bias.copy_(draw(C))
    ctx_in = draw(B, L, C)
    grad_embeds = draw(B, L, C)
    holder = types.SimpleNamespace(
        special_token_dict={"bos_token_id": BOS, "soi_token_id": SOI, "image_token_id": IMAGE}, seq_len=SEQ_LEN,
        context_feat_proj=proj, soi_token=torch.nn.Parameter(draw(1, C)),
        visual_tokenizer=lambda images: {"vis_embed": holder.vis, "multiscale_features": []},
        _prepare_mmfs_features_for_mm_decoder=lambda *a, **k: {})

    def lookup(which):
        holder.text_embeds = table[which].requires_grad_(True)
        return holder.text_embeds
    holder.mm_decoder = types.SimpleNamespace(get_input_embeddings=lambda: lookup)
    holder.vis = vis.clone().requires_grad_(True)
    mm = embeds(holder, ids, image_tensors=torch.zeros(3, 1), num_image_per_seq=torch.tensor([2, 0, 1]))["mm_embeds"]
    mm.backward(grad_embeds)
    common = {"text_ids": ids, "special_ids": np.array([BOS, SOI, IMAGE]), "seq_len": np.array(SEQ_LEN),
              "text_embeds": holder.text_embeds, "vis_embed": vis, "soi_token": holder.soi_token, "mm_embeds": mm,
              "grad_out.mm_embeds": grad_embeds, "grad.text_embeds": holder.text_embeds.grad, "grad.vis_embed": holder.vis.grad,
              "grad.soi_token": holder.soi_token.grad, "context_features": ctx_in, "weight": proj.weight, "bias": proj.bias,
              "pos_table": pos_mod.get_1d_sincos_pos_embed_from_grid(C, np.arange(SEQ_LEN, dtype=np.float32))}
    assert common["pos_table"].dtype == np.float32

    cases = {"sequence_bos": dict(nearest_bos_idxs=torch.tensor([0, 12, 0, 0])),
             "sequence_start": dict(image_start_token_idx=torch.tensor([7, 22, 3, 23]))}
    for name, kw in cases.items():
        x = ctx_in.clone().requires_grad_(True)
        proj.zero_grad()
        feats, mask = context(holder, x, ids, **kw)
        assert mask.dtype == torch.long and feats.shape[0] == 4
        grad_out = draw(*feats.shape)
        feats.backward(grad_out)
        arrays = dict(common)
        arrays.update({k: v for k, v in kw.items()})
        arrays.update({"features": feats, "mask": mask, "grad_out.features": grad_out, "grad.context_features": x.grad,
                       "grad.weight": proj.weight.grad.clone(), "grad.bias": proj.bias.grad.clone()})
        print(name, "lengths", mask.sum(1).tolist(), "L_max", feats.shape[1])
        save(name, **arrays)


if __name__ == "__main__":
    main()
