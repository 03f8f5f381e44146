#!/usr/bin/env python3
"""tests/golden/make_golden_llama_attn.py -- golden vectors of the LLM's self-attention in text generation
(mmfs_amd/llama_attn.py).

Runs ONLY in the build container, where the reference is mounted read-only (``REF`` of make_golden.py).  Nothing is
copied: the reference's ``LlamaAttention``, ``_expand_mask`` and ``_make_causal_mask``
(mm_interleaved/models/decoders/modeling_llama_mmfs.py) are imported through ``make_golden.import_reference_blocks()``
and run in fp64 on the CPU with the reference's tuple cache.  ``.double()`` leaves the rotary table at the values the
class computed in fp32, which is what ``mmfs_amd.rope_table`` must reproduce.  The masks are built in fp32 and cast
(``_make_causal_mask`` overflows when asked for fp64 under the default dtype), as ``LlamaModel`` builds them (:599-620):
causal + padding for the prompt, the padding mask [B, 1, 1, kv_len] alone for a single new token.
The class's ``softmax(.., dtype=torch.float32)`` is an UPCAST for the 16-bit types it was written for; on fp64 scores it
would round the probabilities to fp32 (6e-8) and the goldens with them, so while the class runs here that one call keeps
the scores' own type (``fp64_softmax``): the goldens are fp64 throughout.

2 heads of 128, hidden 256.  Weights are multiples of 1/1024 and inputs multiples of 1/64 with at most 7 significant
bits: both are exact in bf16 and in fp16, so a test that casts them loses nothing (and they are stored as fp16).

``llama_attn_<case>.npz``:
    prefill_decode    B = 2, a prompt of 7 tokens, row 1 left-padded by 3, then 3 single-token steps
    all_masked_row    B = 2, a prompt of 5, then one step whose row 1 masks every key: the uniform average of its values
    decode_beams      B = 3, a prompt of 5, one step, the reference's ``index_select([2, 2, 0])`` on its tuples
                      (``_reorder_cache``, :913-917), then two more steps
Each file stores the parameters (``param.<name>``), and per call ``<call>.hidden_states``, ``.mask`` ([B, 1, q_len,
kv_len]), ``.position_ids``, ``.out`` (the module's output), ``.keys`` / ``.values`` (the present, [B, H, kv_len, 128]);
calls are ``prefill``, ``step0``, ``step1``, ...; ``beam_idx`` and ``reorder_after`` (the call it follows) where there is one.

Checked here: the class runs on the CPU with a tuple cache, and the last step of ``prefill_decode`` equals the last row of
one prefill over all 10 tokens (printed; asserted to 1e-13 of the largest output).

Usage:  python tests/golden/make_golden_llama_attn.py     (rewrites tests/golden/llama_attn_*.npz)
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference_blocks, save  # noqa: E402

HEADS, HIDDEN, MAX_POS = 2, 256, 64


def config():
    return types.SimpleNamespace(hidden_size=HIDDEN, num_attention_heads=HEADS, max_position_embeddings=MAX_POS)


def grid_values(shape, step, gen):
    """multiples of ``step`` with |k| <= 127: exact in bf16 and fp16"""
    return torch.randint(-127, 128, shape, generator=gen).double() * step


@contextlib.contextmanager
def fp64_softmax(llama):
    """softmax(x, dtype=float32) of an fp64 x stays in fp64 while the reference's class runs"""
    functional = llama.nn.functional
    plain = functional.softmax

    def softmax(x, dim=None, dtype=None, **kw):
        return plain(x, dim=dim, dtype=None if x.dtype == torch.float64 else dtype, **kw)

    functional.softmax = softmax
    try:
        yield
    finally:
        functional.softmax = plain


def masks_of(llama, mask2d, q_len):
    """LlamaModel._prepare_decoder_attention_mask (:599-620) in fp32, cast: [B, 1, q_len, kv_len]"""
    B, kv = mask2d.shape
    combined = None
    if q_len > 1:
        combined = llama._make_causal_mask((B, q_len), torch.float32, device=mask2d.device, past_key_values_length=kv - q_len)
    expanded = llama._expand_mask(mask2d, torch.float32, tgt_len=q_len)
    combined = expanded if combined is None else expanded + combined
    return combined.double()


def positions_of(mask2d, q_len):
    """HF's position_ids of a left-padded batch: cumsum(mask) - 1, 1 at padding; the last q_len columns"""
    pos = mask2d.long().cumsum(-1) - 1
    pos.masked_fill_(mask2d == 0, 1)
    return pos[:, -q_len:].contiguous()


def run_case(llama, name, seed, B, prompt, pad, steps, mask_all_row=None, beam_idx=None, reorder_after=None, check_full=False):
    gen = torch.Generator().manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        m = llama.LlamaAttention(config())
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(grid_values(p.shape, 1.0 / 1024, gen))
    m = m.double().eval()
    arrays = {"param." + n: p.detach().numpy().astype(np.float16) for n, p in m.named_parameters()}
    assert sorted(m.state_dict()) == ["k_proj.weight", "o_proj.weight", "q_proj.weight", "v_proj.weight"]
    mask2d = torch.ones(B, prompt)
    for row, n in pad.items():
        mask2d[row, :n] = 0
    past, hiddens, outs = None, [], []
    calls = ["prefill"] + [f"step{i}" for i in range(steps)]
    with torch.no_grad(), fp64_softmax(llama):
        for call in calls:
            q_len = prompt if call == "prefill" else 1
            if call != "prefill":
                mask2d = torch.cat((mask2d, torch.ones(B, 1)), dim=1)
            hidden = grid_values((B, q_len, HIDDEN), 1.0 / 64, gen)
            mask = masks_of(llama, mask2d, q_len)
            if mask_all_row is not None and call != "prefill":
                mask[mask_all_row] = float(torch.finfo(torch.float32).min)
            pos = positions_of(mask2d, q_len)
            out, weights, past = m(hidden, attention_mask=mask, position_ids=pos, past_key_value=past, use_cache=True)
            assert weights is None and past[0].shape == (B, HEADS, mask2d.shape[1], HIDDEN // HEADS)
            arrays.update({call + ".hidden_states": hidden.numpy().astype(np.float16), call + ".mask": mask,
                           call + ".position_ids": pos, call + ".out": out, call + ".keys": past[0], call + ".values": past[1]})
            hiddens.append(hidden)
            outs.append(out)
            if call == reorder_after:
                idx = torch.tensor(beam_idx)
                past = tuple(t.index_select(0, idx) for t in past)             # LlamaForCausalLM._reorder_cache
                arrays["beam_idx"] = idx
                arrays["reorder_after"] = np.array(calls.index(call))
        if check_full:
            full_mask2d = mask2d
            hidden = torch.cat(hiddens, dim=1)
            n = hidden.shape[1]
            out, _, _ = m(hidden, attention_mask=masks_of(llama, full_mask2d, n), position_ids=positions_of(full_mask2d, n),
                          use_cache=True)
            gap = float((out[:, -1:] - outs[-1]).abs().max() / outs[-1].abs().max())
            print(f"{name}: the last step against the last row of one prefill over {n} tokens: {gap:.1e}")
            assert gap <= 1e-13
    if mask_all_row is not None:
        # every key masked: the uniform average of the row's values through o_proj
        want = past[1][mask_all_row].mean(1).reshape(1, HIDDEN) @ m.o_proj.weight.T
        assert float((outs[-1][mask_all_row] - want).abs().max()) <= 1e-13
    save("llama_attn_" + name, **arrays)


def main():
    _, llama = import_reference_blocks()
    run_case(llama, "prefill_decode", 170, B=2, prompt=7, pad={1: 3}, steps=3, check_full=True)
    run_case(llama, "all_masked_row", 171, B=2, prompt=5, pad={}, steps=1, mask_all_row=1)
    run_case(llama, "decode_beams", 172, B=3, prompt=5, pad={}, steps=3, beam_idx=[2, 2, 0], reorder_after="step0")


if __name__ == "__main__":
    main()
