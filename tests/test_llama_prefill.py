"""The LLM's self-attention over a prompt (csrc/mmfs_llama_prefill.hip), host side: the C ABI's argument checks (every
one returns before a launch, so they are safe without a GPU), the library's tile sizes, the module's knob, and a host
model of the kernel's tile walk (tests/llama_prefill_refs.py): with its skip rule it is bit-equal to itself without, and
both are under ``attend64``'s bounds on masks built as HF builds them, -Inf entries included."""
import ctypes
import os
import types

import pytest
import torch

from front_end_refs import worst
from llama_attn_refs import attend64
from llama_prefill_refs import clamped, hf_mask, left_padded, padding_row, tile_walk

import mmfs_amd
from mmfs_amd import llama_attn
from mmfs_amd.llama_attn import LlamaSelfAttention

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPE, DIMS, NULLPTR, ALIGN, UNSUPPORTED = -1, -2, -3, -4, -5
CAUSAL, VISIT_ALL = 1, 2


from helpers import bound_library as _lib  # noqa: E402


def test_the_tile_sizes_are_positive_and_the_package_reads_them_from_the_library():
    lib = _lib()
    W, G, K = (lib.mmfs_llama_attn_prefill_tiles(i) for i in range(3))
    assert W > 0 and G > 0 and K > 0 and G % W == 0
    assert lib.mmfs_llama_attn_prefill_tiles(3) == DIMS and lib.mmfs_llama_attn_prefill_tiles(-1) == DIMS
    from mmfs_amd.functions import llama_attn_func
    assert llama_attn_func.PREFILL_TILES == (W, G, K)
    assert (llama_attn_func.PREFILL_CAUSAL, llama_attn_func.PREFILL_VISIT_ALL) == (CAUSAL, VISIT_ALL)
    assert set(llama_attn_func.launches) >= {"append", "decode", "prefill"}
    assert mmfs_amd.llama_attn_prefill is llama_attn_func.llama_attn_prefill
    header = open(os.path.join(ROOT, "include", "mmfs_msda.h")).read()
    assert "#define MMFS_LLAMA_PREFILL_CAUSAL 1u" in header and "#define MMFS_LLAMA_PREFILL_VISIT_ALL 2u" in header


def test_argument_errors_return_before_any_launch():
    lib = _lib()
    fake = ctypes.c_void_p(4096)                                            # never dereferenced on these paths
    odd = ctypes.c_void_p

    def f(dt=2, B=2, Lq=5, H=3, D=128, cap=77, bias=fake, bias_dt=0, bstride=5 * 20, qstride=20, blen=20, flags=0, context=fake,
          **named):
        p = dict.fromkeys(("q_rot", "kc", "vc", "src_row", "length"), fake)
        p.update(named)
        return lib.mmfs_llama_attn_prefill(dt, *p.values(), bias, bias_dt, bstride, qstride, blen, flags, context, B, Lq, H, D, cap, None)

    assert f(dt=9) == DTYPE and f(dt=-1) == DTYPE
    assert f(dt=0) == UNSUPPORTED and f(dt=3) == UNSUPPORTED                # fp32 / fp64 storage: the framework's
    assert f(B=-1) == DIMS and f(H=-1) == DIMS and f(D=-1) == DIMS and f(cap=-1) == DIMS and f(Lq=-1) == DIMS
    assert f(B=1 << 20, H=1 << 5) == DIMS and f(B=(1 << 20) + 1) == DIMS
    assert f(D=64) == UNSUPPORTED and f(D=127) == UNSUPPORTED and f(D=256) == UNSUPPORTED
    assert f(cap=0) == UNSUPPORTED and f(cap=(1 << 22) + 1) == UNSUPPORTED and f(Lq=0) == UNSUPPORTED and f(Lq=78) == UNSUPPORTED
    assert f(q_rot=None) == NULLPTR and f(kc=None) == NULLPTR and f(vc=None) == NULLPTR and f(context=None) == NULLPTR
    assert f(src_row=None) == NULLPTR and f(length=None) == NULLPTR
    assert f(q_rot=odd(4104)) == ALIGN and f(kc=odd(4104)) == ALIGN and f(vc=odd(4098)) == ALIGN and f(context=odd(4104)) == ALIGN
    assert f(src_row=odd(4098)) == ALIGN and f(length=odd(4097)) == ALIGN
    # the bias: its type, its strides, its alignment (its element size alone)
    assert f(bias_dt=1) == DTYPE and f(bias_dt=3) == DTYPE and f(bias_dt=9) == DTYPE
    assert f(B=0, bias=None, bias_dt=9, qstride=-3, bstride=7, blen=-1) == 0                 # no bias: nothing of it is checked
    assert f(blen=-1) == DIMS and f(blen=(1 << 22) + 1) == DIMS
    assert f(qstride=19) == DIMS and f(qstride=-20) == DIMS and f(qstride=1) == DIMS
    assert f(bstride=99) == DIMS and f(bstride=-100) == DIMS and f(bstride=20) == DIMS       # 4 * 20 + 20 = 100 spans a batch row
    assert f(qstride=0, bstride=19) == DIMS and f(qstride=0, bstride=-1) == DIMS
    assert f(flags=4) == DIMS and f(flags=1 << 31) == DIMS and f(flags=7) == DIMS
    assert f(bias=odd(4098)) == ALIGN and f(bias=odd(4097), bias_dt=2) == ALIGN
    # what passes every check, and is empty: no launch, 0
    for kw in (dict(B=0), dict(H=0), dict(B=0, flags=3), dict(B=0, qstride=0, bstride=0), dict(B=0, bias=odd(4098), bias_dt=2),
               dict(B=0, qstride=21, bstride=4 * 21 + 20), dict(B=0, qstride=0, bstride=20), dict(B=0, bias=None)):
        assert f(**kw) == 0, kw
    assert f(B=0, q_rot=None, context=None) == 0


def test_the_knob_takes_none_true_and_false_alone():
    cfg = types.SimpleNamespace(hidden_size=256, num_attention_heads=2, max_position_embeddings=16)
    m = LlamaSelfAttention(cfg).double().eval()
    assert m.prefill_kernel is None and m.last_prefill is None
    assert isinstance(llama_attn.PREFILL_KERNEL_MIN_TOKENS, int) and llama_attn.PREFILL_KERNEL_MIN_TOKENS >= 2
    assert set(llama_attn.DEFAULT_ROUTE) == {"decode", "prefill"}
    h = torch.zeros(1, 3, 256, dtype=torch.float64)
    for ok in (None, True, False):                      # host tensors take the framework route whatever the knob says
        m.prefill_kernel = ok
        with torch.no_grad():
            m(h)
        assert m.last_route == "framework" and m.last_prefill is None
    for bad in (1, 0, "kernel", "yes", 2.0):
        m.prefill_kernel = bad
        with pytest.raises(ValueError):
            m(h)


# ------------------------------------------------------------------ the tile walk on the host
B, H = 2, 3
CASES = [(0, 2), (0, 65), (3, 33), (63, 130), (65, 257)]


def pads_of(n):
    return min(n - 1, n // 3 + 1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("held,Lq", CASES)
def test_the_tile_walk_skips_without_moving_a_bit_and_holds_the_bounds(held, Lq, dtype):
    from mmfs_amd.functions.llama_attn_func import PREFILL_TILES
    n = held + Lq
    gen = torch.Generator().manual_seed(1000 * held + Lq)
    q_rot = torch.randn(B, Lq, H * 128, generator=gen).to(dtype)
    keys = (torch.randn(B, H, n, 128, generator=gen) * 1.5 + 0.25).to(dtype)
    values = torch.randn(B, H, n, 128, generator=gen).to(dtype)
    attention = left_padded(B, n, pads_of(n))
    mask = hf_mask(attention, Lq, dtype)
    row = padding_row(attention, dtype)
    if pads_of(n) > held + 1:                           # a padded key that is a future key of query 0: finfo.min twice
        assert bool(torch.isinf(mask[1]).any()) and not bool(torch.isinf(mask[0]).any())
    ref = attend64(q_rot, keys, values, H, mask=clamped(mask, dtype), dtype=dtype)
    assert bool(torch.isfinite(ref["context"]).all())
    worst_ratio = 0.0
    results = []
    for kw in (dict(mask=mask), dict(mask=row, causal=True)):
        full, all_tiles = tile_walk(q_rot, keys, values, H, held, dtype=dtype, tiles=PREFILL_TILES, skip=False, **kw)
        cut, some_tiles = tile_walk(q_rot, keys, values, H, held, dtype=dtype, tiles=PREFILL_TILES, skip=True, **kw)
        assert torch.equal(full.view(torch.int16), cut.view(torch.int16))
        assert some_tiles <= all_tiles
        if n > 2 * PREFILL_TILES[2]:
            assert some_tiles < all_tiles                                   # (the rule does skip: the test is not vacuous)
        w = worst(cut, ref["context"], ref["E_context"])
        assert w[0] <= 1.0, f"|got - ref| / bound = {w[0]:.3g} at {w[1]}: got {w[2]!r}, ref {w[3]!r}, bound {w[4]:.3g}"
        worst_ratio = max(worst_ratio, w[0])
        results.append(cut)
    assert torch.equal(results[0].view(torch.int16), results[1].view(torch.int16))     # the flag IS the materialised mask
    # a padded query row: the mean of all n value rows
    want = values[1].double().mean(1)                                       # [H, 128]
    got = results[0][1, 0].double().reshape(H, 128)
    assert bool(((got - want).abs() <= ref["E_context"][1, 0].reshape(H, 128)).all())
    print(f"worst |got - ref| / bound: {worst_ratio:.3f}")
