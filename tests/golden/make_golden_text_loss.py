#!/usr/bin/env python3
"""tests/golden/make_golden_text_loss.py -- golden vectors of the text loss (mmfs_amd/text_loss.py).

Runs ONLY in the build container, where the reference is mounted read-only (``REF`` of make_golden.py).  Nothing is
copied: ``MMInterleaved._prepare_gt_text_ids`` (mm_interleaved/models/mm_interleaved.py) is compiled out of the file's AST
and run against a stub ``self`` that holds what the method touches -- ``special_token_dict`` and
``dataset_to_ignore_noimage_cond_loss``.  The loss is the statement that ends ``MMInterleaved.forward``, in fp64:
F.cross_entropy on the logits permuted to [B, V, L], cut to L - 1 columns and made contiguous.

Layout (B = 4, L = 24, V = 40; <bos> 1, <soi> 37, image 38, pad 39):
    row 0   two documents: <bos> at 0 with no image, <bos> at 10, <soi> at 13 + two image tokens
    row 1   no <bos>: <soi> at 4 + two image tokens
    row 2   <bos> at 0, <soi> directly behind it + two image tokens, padding from column 18
    row 3   <bos> at 0, <soi> at 6 + two image tokens, attention-mask zeros at columns 11 .. 14
``text_loss_<case>.npz``, cases: ``plain`` (offset 0), ``noimage`` (ignore_noimage_cond_loss), ``offset_int`` (3),
``offset_list`` ([0, 5, 2, 30] as a list), ``offset_tensor`` (the same as a tensor, with noimage), ``given`` (a given
gt_text_ids).  Each file stores the ids, the mask, the special ids, the offset, the flags, the labels, the logits (fp32
draws, scored in fp64), the fp64 loss and its fp64 gradient.

Usage:  python tests/golden/make_golden_text_loss.py     (rewrites tests/golden/text_loss_*.npz)
"""
import ast
import os
import sys
import types
import typing

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, save  # noqa: E402

B, L, V = 4, 24, 40
BOS, SOI, IMAGE, PAD = 1, 37, 38, 39
MODEL = os.path.join(REF, "mm_interleaved/models/mm_interleaved.py")
DATASET = "noimage_cond_dataset"


def reference_method(name):
    """The named method of ``MMInterleaved``, compiled from the file's AST as a plain function of (self, ...)."""
    tree = ast.parse(open(MODEL).read())
    klass = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "MMInterleaved")
    scope = {"torch": torch, "np": np, "Optional": typing.Optional, "Union": typing.Union, "List": typing.List}
    node = next(n for n in klass.body if isinstance(n, ast.FunctionDef) and n.name == name)
    exec(compile(ast.Module(body=[node], type_ignores=[]), MODEL, "exec"), scope)
    return scope[name]


def inputs():
    gen = torch.Generator().manual_seed(150)
    ids = torch.randint(2, 37, (B, L), generator=gen)
    mask = torch.ones(B, L, dtype=torch.long)
    ids[0, 0], ids[0, 10] = BOS, BOS
    ids[0, 13], ids[0, 14], ids[0, 15] = SOI, IMAGE, IMAGE
    ids[1, 4], ids[1, 5], ids[1, 6] = SOI, IMAGE, IMAGE
    ids[2, 0], ids[2, 1], ids[2, 2], ids[2, 3] = BOS, SOI, IMAGE, IMAGE
    ids[2, 18:] = PAD
    mask[2, 18:] = 0
    ids[3, 0] = BOS
    ids[3, 6], ids[3, 7], ids[3, 8] = SOI, IMAGE, IMAGE
    mask[3, 11:15] = 0
    return ids, mask


def main():
    labels_of = reference_method("_prepare_gt_text_ids")
    holder = types.SimpleNamespace(
        special_token_dict={"bos_token_id": BOS, "soi_token_id": SOI, "image_token_id": IMAGE, "pad_token_id": PAD},
        dataset_to_ignore_noimage_cond_loss=[DATASET])
    ids, mask = inputs()
    gen = torch.Generator().manual_seed(151)
    given = torch.randint(0, V, (B, L), generator=gen)
    given[1, 3:9] = -100
    offsets = [0, 5, 2, 30]
    cases = {"plain": dict(offset=0, noimage=False),
             "noimage": dict(offset=0, noimage=True),
             "offset_int": dict(offset=3, noimage=False),
             "offset_list": dict(offset=offsets, noimage=False),
             "offset_tensor": dict(offset=torch.tensor(offsets), noimage=True),
             "given": dict(offset=0, noimage=False, gt=given)}
    for name, c in cases.items():
        labels = labels_of(holder, ids, attention_mask=mask, ignore_prompt_token_offset=c["offset"],
                           gt_text_ids=c.get("gt"), meta={"dataset_name": DATASET if c["noimage"] else "other"})
        logits = (torch.randn(B, L, V, generator=gen) * 3).double().requires_grad_(True)      # (fp32 draws: stored losslessly)
        text_logits = logits.permute(0, 2, 1)
        loss = F.cross_entropy(text_logits[..., :-1].contiguous(), labels.contiguous())
        loss.backward()
        arrays = {"text_ids": ids, "attention_mask": mask, "special_ids": np.array([BOS, SOI, IMAGE, PAD]),
                  "offset": np.asarray(c["offset"]), "noimage": np.array(c["noimage"]), "labels": labels.contiguous(),
                  "logits": logits.detach().float(), "loss": loss.detach(), "grad.logits": logits.grad}
        if "gt" in c:
            arrays["gt_text_ids"] = c["gt"]
        assert torch.equal(arrays["logits"].double(), logits.detach())
        print(name, "scored", int((labels != -100).sum()), "of", labels.numel(), "loss", float(loss))
        save("text_loss_" + name, **arrays)


if __name__ == "__main__":
    main()
