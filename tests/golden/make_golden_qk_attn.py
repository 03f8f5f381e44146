#!/usr/bin/env python3
"""tests/golden/make_golden_qk_attn.py -- golden vectors of the Q-Former attention with per-head q/k LayerNorm
(mmfs_amd/resampler.py).

Runs ONLY in the build container, where the reference is mounted read-only (``REF`` of make_golden.py).  Nothing is
copied: the reference's patched ``Blip2QFormerMultiHeadAttention``
(mm_interleaved/models/utils/monkey_patch/blip2_qknorm_monkey_patch.py) is imported from its file and run in fp64 on a
``SimpleNamespace`` config, parameters randomised (a LayerNorm starts as the identity, which pins nothing).

``qk_attn_<case>.npz`` (2 heads of 64, hidden 128, encoder width 40, B = 2):
    self_qknorm           self-attention, 5 tokens, qk-norm, no mask
    cross_qknorm_masked   5 queries over 19 keys, qk-norm; batch row 1 masks its last 9 keys with finfo(float32).min
    cross_plain_77        77 queries over 40 keys, no qk-norm; row 0 masks its last 7 keys, row 1 its first 10
    cross_one_key_left    5 queries over 19 keys, qk-norm; batch row 1 keeps key 4 alone
Each file stores the inputs, the extended mask [B, 1, 1, Nk] (when there is one), the parameters (``param.<name>``), the
upstream gradient, the context, and the gradients (``grad.<name>``) of the three Linear layers' OUTPUTS (``q``, ``k``, ``v``:
what the attention itself hands back), of their biases and of the LayerNorm parameters.  The gradients of the inputs and of
the Linear weights are products of those with the stored inputs and weights and are left out: they were most of a file.

Usage:  python tests/golden/make_golden_qk_attn.py     (rewrites tests/golden/qk_attn_*.npz)
"""
import contextlib
import importlib.util
import io
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, save  # noqa: E402

PATCH = os.path.join(REF, "mm_interleaved/models/utils/monkey_patch/blip2_qknorm_monkey_patch.py")
B, HEADS, HIDDEN, ENCODER = 2, 2, 128, 40
MIN = torch.finfo(torch.float32).min

CASES = {
    "self_qknorm": dict(cross=False, Nq=5, Nk=5, norm=True, masked={}),
    "cross_qknorm_masked": dict(cross=True, Nq=5, Nk=19, norm=True, masked={1: range(10, 19)}),
    "cross_plain_77": dict(cross=True, Nq=77, Nk=40, norm=False, masked={0: range(33, 40), 1: range(0, 10)}),
    "cross_one_key_left": dict(cross=True, Nq=5, Nk=19, norm=True, masked={1: [k for k in range(19) if k != 4]}),
}


def reference_class():
    spec = importlib.util.spec_from_file_location("ref_blip2_qknorm", PATCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Blip2QFormerMultiHeadAttention


def config(norm):
    return types.SimpleNamespace(hidden_size=HIDDEN, num_attention_heads=HEADS, encoder_hidden_size=ENCODER,
                                 attention_probs_dropout_prob=0.0, layer_norm_eps=1e-12, qk_normalization=norm)


def main():
    klass = reference_class()
    for seed, (name, c) in enumerate(CASES.items()):
        gen = torch.Generator().manual_seed(160 + seed)
        with contextlib.redirect_stdout(io.StringIO()):
            m = klass(config(c["norm"]), is_cross_attention=c["cross"])
        with torch.no_grad():
            for pname, p in m.named_parameters():
                scale = 0.3 if p.dim() == 2 else 0.2
                p.copy_(torch.randn(p.shape, generator=gen) * scale + (1.0 if pname.endswith("norm.weight") else 0.0))
        m = m.double().eval()
        hidden = torch.randn(B, c["Nq"], HIDDEN, generator=gen).double().requires_grad_(True)
        arrays, kwargs, leaves = {}, {}, {"hidden_states": hidden}
        if c["cross"]:
            enc = torch.randn(B, c["Nk"], ENCODER, generator=gen).double().requires_grad_(True)
            leaves["encoder_hidden_states"] = enc
            kwargs["encoder_hidden_states"] = enc
        if c["masked"]:
            mask = torch.zeros(B, 1, 1, c["Nk"], dtype=torch.float64)
            for row, keys in c["masked"].items():
                mask[row, 0, 0, list(keys)] = MIN
            kwargs["encoder_attention_mask" if c["cross"] else "attention_mask"] = mask
            arrays["mask"] = mask
        upstream = torch.randn(B, c["Nq"], HIDDEN, generator=gen).double()
        linear_out = {}

        def keep(tag):
            def hook(_module, _inputs, output):
                output.retain_grad()
                linear_out[tag] = output
            return hook

        handles = [getattr(m, layer).register_forward_hook(keep(tag)) for layer, tag in (("query", "q"), ("key", "k"), ("value", "v"))]
        out = m(hidden, **kwargs)
        for h in handles:
            h.remove()
        context = out[0]
        assert len(out) == 2 and context.shape == (B, c["Nq"], HIDDEN)
        context.backward(upstream)
        arrays.update({k: v.detach() for k, v in leaves.items()})
        arrays.update({"upstream": upstream, "context": context.detach(), "qk_normalization": torch.tensor(c["norm"]),
                       "is_cross_attention": torch.tensor(c["cross"])})
        arrays.update({"grad." + tag: t.grad for tag, t in linear_out.items()})
        for pname, p in m.named_parameters():
            arrays["param." + pname] = p.detach()
            if p.dim() == 1:
                arrays["grad." + pname] = p.grad
        print(name, "context", tuple(context.shape), "keys of the state dict:", sorted(m.state_dict()))
        save("qk_attn_" + name, **arrays)


if __name__ == "__main__":
    main()
