"""GPU: the one-pass feature-bank kernel (csrc/mmfs_bank.hip) against the framework-op
statement of the same steps (gather over images, "c (h w) -> (h w) c", concatenation over levels, zero
slots -- mm_interleaved.py:223-250).  A copy: the bar is bit-equality; the backward sums in fp32."""
import pytest
import torch

from helpers import (OUTPUT_GUARD, STORAGE_T, STORAGE_U, assert_bit_equal, assert_guards_intact, assert_no_poison,
                     assert_payload_unchanged, placed, poison)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def torch_bank(levels, src):
    packed = torch.cat([f.flatten(2).transpose(1, 2) for f in levels], dim=1)
    valid = (src >= 0) & (src < packed.shape[0])
    rows = packed.index_select(0, src.clamp(0, packed.shape[0] - 1))
    return rows * valid[:, None, None].to(rows.dtype)


CASES = [
    # n_img, C, level shapes, slot indices
    (5, 64, [(32, 32), (16, 16), (8, 8)], [0, 1, -1, 4, 2, 3, -1, -1]),            # LLM bank, padded slots
    (3, 1024, [(64, 64), (32, 32), (16, 16), (8, 8)], [2, 0, 1]),                  # SD pack, real widths
    (4, 24, [(14, 14), (7, 7)], [3, 3, 0, 7, -5, 1]),                              # odd sizes: scalar paths; repeats; out of range
    (2, 72, [(5, 9), (1, 1), (3, 70)], [1, 0, 1]),                                 # ragged tiles in both directions
    (1, 8, [(1, 1)], [0]),
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("case", CASES, ids=[f"img{c[0]}C{c[1]}L{len(c[2])}" for c in CASES])
def test_bank_gather_is_a_bit_exact_copy(case, dtype):
    from mmfs_amd.functions import BankGatherFunction, bank_gather_supported
    n_img, C, shapes, slots = case
    g = torch.Generator().manual_seed(7)
    levels = [torch.randn(n_img, C, h, w, generator=g).to(DEV, dtype) for h, w in shapes]
    src = torch.tensor(slots, device=DEV)
    assert bank_gather_supported(levels, src.numel())
    got = BankGatherFunction.apply(src, *levels)
    want = torch_bank(levels, src)
    assert got.shape == want.shape and torch.equal(got, want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("case", CASES[:4], ids=[f"img{c[0]}C{c[1]}L{len(c[2])}" for c in CASES[:4]])
def test_bank_scatter_is_the_adjoint(case, dtype):
    from mmfs_amd.functions import BankGatherFunction
    n_img, C, shapes, slots = case
    g = torch.Generator().manual_seed(9)
    base = [torch.randn(n_img, C, h, w, generator=g).to(DEV, dtype) for h, w in shapes]
    src = torch.tensor(slots, device=DEV)
    lv_a = [f.clone().requires_grad_(True) for f in base]
    lv_b = [f.clone().double().requires_grad_(True) for f in base]
    out = BankGatherFunction.apply(src, *lv_a)
    grad = torch.randn(out.shape, generator=g).to(DEV, dtype)
    out.backward(grad)
    torch_bank(lv_b, src).backward(grad.double())
    repeats = len(set(s for s in slots if 0 <= s < n_img)) < sum(0 <= s < n_img for s in slots)
    for a, b in zip(lv_a, lv_b):
        want = b.grad.to(dtype)                     # fp64 sum rounded once == fp32 sum rounded once for <= a few terms
        if not repeats:
            assert torch.equal(a.grad, want)
        else:
            tol = 1e-6 if dtype == torch.float32 else 8e-3
            assert float((a.grad.double() - b.grad).abs().max()) <= tol * max(1.0, float(b.grad.abs().max()))
        shown = torch.zeros(n_img, dtype=torch.bool)
        for s in slots:
            if 0 <= s < n_img:
                shown[s] = True
        assert float(a.grad[~shown.to(DEV)].abs().sum()) == 0.0      # images nobody shows: exact zeros


def test_builders_use_the_kernel_and_match_the_framework_ops():
    """prepare_mmfs_features_for_mm_decoder / pack_image_levels / MMFSNet._pack on device tensors go
    through BankGatherFunction and give the bank the host statement gives."""
    import MultiScaleDeformableAttention as MSDA
    from mmfs_amd import bank
    from mmfs_amd.blocks import MMFSNet
    g = torch.Generator().manual_seed(3)
    num = torch.tensor([2, 0, 3])
    levels = [torch.randn(5, 32, s, s, generator=g).to(torch.bfloat16) for s in (16, 8, 4)]
    want = bank.llm_feature_bank_from_levels(levels, num, 3)                       # host tensors: framework ops
    MSDA._event_log = log = []
    try:
        got = bank.llm_feature_bank_from_levels([f.to(DEV) for f in levels], num.to(DEV), 3)
        packed = bank.pack_image_levels([f.to(DEV) for f in levels])
        net_bank = MMFSNet._pack([f.to(DEV)[:4].reshape(2, 2, 32, f.shape[-1], f.shape[-1]) for f in levels])
    finally:
        MSDA._event_log = None
    assert [n for n, _, _ in log] == ["mmfs_bank_gather"] * 3
    assert torch.equal(got.cpu(), want)
    assert torch.equal(packed.cpu(), bank.pack_image_levels(levels))
    assert torch.equal(net_bank.cpu(), MMFSNet._pack([f[:4].reshape(2, 2, 32, f.shape[-1], f.shape[-1]) for f in levels]))


# ---------------------------------------------------------------------------------------------------------------------
# Placement and slot counts.  Every tensor above comes from torch's allocator (512-byte aligned) and no case has more
# than 8 slots: the scalar paths taken for a pointer off 16 bytes (csrc/mmfs_bank.hip: ``hw % VEC == 0 && ptr % 16 == 0``
# on the level side, ``C % VEC == 0 && ptr % 16 == 0`` on the bank side, in both kernels) and the scatter's ballots of
# waves 1..3 and its second 256-slot step never ran.
# ---------------------------------------------------------------------------------------------------------------------

DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def exact_bank(levels, src):
    """``torch_bank`` with a dead slot's rows +0 in every bit (its ``rows * 0`` is -0 under a negative entry; the kernel writes
    the zero rows the header promises)."""
    packed = torch.cat([f.flatten(2).transpose(1, 2) for f in levels], dim=1)
    valid = (src >= 0) & (src < packed.shape[0])
    rows = packed.index_select(0, src.clamp(0, packed.shape[0] - 1))
    return torch.where(valid[:, None, None], rows, torch.zeros_like(rows))

# hw = 16 and 8, C = 24: multiples of the 16-byte vector for 2-byte and 4-byte elements alike, so a side goes scalar for its
# pointer alone; two token tiles' worth of neither (a ragged tile on both axes)
OFF_SHAPES, OFF_C, OFF_IMG, OFF_SLOTS = [(4, 4), (2, 4)], 24, 3, [2, 0, -1, 1, 2, 2]


def _c_tables(tensors, shapes):
    import ctypes
    ptrs = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    hw = (ctypes.c_int64 * len(shapes))(*[h * w for h, w in shapes])
    return ptrs, hw


def _code(dtype):
    import MultiScaleDeformableAttention as MSDA
    return MSDA._FLOAT_CODE[dtype]


@pytest.mark.parametrize("off", ["levels", "bank", "both"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_bank_gather_with_pointers_one_element_off_16_bytes(dtype, off):
    """mmfs_bank_gather (the C entry: the wrapper's own bank is always aligned) with the level maps, the bank, or both
    starting one element past a 16-byte boundary, sizes at which that side is vectorised otherwise: a bit-exact copy, no
    byte outside the bank, the maps untouched."""
    import MultiScaleDeformableAttention as MSDA
    es = torch.empty((), dtype=dtype).element_size()
    g = torch.Generator().manual_seed(17)
    levels = [torch.randn(OFF_IMG, OFF_C, h, w, generator=g).to(dtype) for h, w in OFF_SHAPES]
    src = torch.tensor(OFF_SLOTS, device=DEV)
    lead_lv, lead_bank = (es if off in ("levels", "both") else 0), (es if off in ("bank", "both") else 0)
    hl = [placed(f, lead_lv, device=DEV, name=f"level {i}") for i, f in enumerate(levels)]
    S = sum(h * w for h, w in OFF_SHAPES)
    hb = placed(torch.zeros(len(OFF_SLOTS), S, OFF_C, dtype=dtype), lead_bank, OUTPUT_GUARD, DEV, name="bank")
    poison(hb.t)
    assert all(h.t.data_ptr() % 16 == lead_lv for h in hl) and hb.t.data_ptr() % 16 == lead_bank
    ptrs, hw = _c_tables([h.t for h in hl], OFF_SHAPES)
    MSDA._call("mmfs_bank_gather", "mmfs_bank_gather", torch.device(DEV, 0), _code(dtype), len(hl), ptrs, hw, src.data_ptr(),
               hb.t.data_ptr(), OFF_IMG, OFF_C, len(OFF_SLOTS))
    torch.cuda.synchronize()
    assert_guards_intact(hb, *hl)
    assert_payload_unchanged(*hl)
    assert_no_poison(hb.t, "bank")
    want = exact_bank([f.to(DEV) for f in levels], src)
    assert torch.equal(want, torch_bank([f.to(DEV) for f in levels], src))
    assert_bit_equal(hb.t, want, "bank")
    # the wrapper forwards a contiguous level's pointer as it is: the same through it
    if off == "levels":
        assert_bit_equal(BankGather(src, [h.t for h in hl]), hb.t, "bank through BankGatherFunction")


def BankGather(src, levels):
    from mmfs_amd.functions import BankGatherFunction
    return BankGatherFunction.apply(src, *levels)


def scatter_reference(grad_bank, src, n_img, C, shapes, dtype):
    """-> per level (fp64 sum [n_img, C, h, w], bound of the same shape): the kernel adds the slots that show an image in
    ascending order in fp32 and rounds once to the storage type, so |got - sum| <= (n - 1) 2^-24 sum|terms| (an fp32 sum
    of n terms) + the rounding of that sum (u_s relative; half a subnormal spacing below the normal range); n == 0 or
    all-zero terms: exactly 0."""
    g, s = grad_bank.double().cpu(), src.cpu()
    res, tok = [], 0
    for h, w in shapes:
        rows = g[:, tok:tok + h * w]                                     # [n_slots, hw, C]
        tok += h * w
        total, mag, n = (torch.zeros(n_img, C, h, w, dtype=torch.float64) for _ in range(3))
        for i in range(n_img):
            shown = (s == i)
            total[i] = rows[shown].sum(0).t().reshape(C, h, w)
            mag[i] = rows[shown].abs().sum(0).t().reshape(C, h, w)
            n[i] = float(shown.sum())
        fp32_err = (n - 1).clamp(min=0) * 2.0 ** -24 * mag
        bound = fp32_err + STORAGE_U[dtype] * (total.abs() + fp32_err) + STORAGE_T[dtype] * (mag > 0)
        res.append((total, bound))
    return res


def assert_scatter_within_bound(grads, grad_bank, src, n_img, C, shapes, dtype, what):
    worst = 0.0
    for l, (got, (want, bound)) in enumerate(zip(grads, scatter_reference(grad_bank, src, n_img, C, shapes, dtype))):
        err = (got.double().cpu() - want).abs()
        assert bool(torch.isfinite(got).all()), f"{what} level {l}: non-finite entries"
        over = err > bound
        assert not bool(over.any()), (f"{what} level {l}: {int(over.sum())} element(s) over the bound, the first at "
                                      f"{tuple(over.nonzero()[0].tolist())}: err {float(err[over][0]):.3e} > {float(bound[over][0]):.3e}")
        worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
    print(f"BOUND bank scatter {what}: worst ratio {worst:.3g}")
    return worst


@pytest.mark.parametrize("off", ["levels", "bank", "both"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_bank_scatter_with_pointers_one_element_off_16_bytes(dtype, off):
    """mmfs_bank_scatter with grad_bank (``vec_in``), the gradient maps (``vec_out``) or both one element off 16 bytes: the
    fp64 sum within the kernel's own bound, no byte outside the maps, grad_bank untouched."""
    import MultiScaleDeformableAttention as MSDA
    es = torch.empty((), dtype=dtype).element_size()
    g = torch.Generator().manual_seed(19)
    S = sum(h * w for h, w in OFF_SHAPES)
    grad_bank = torch.randn(len(OFF_SLOTS), S, OFF_C, generator=g).to(dtype)
    src = torch.tensor(OFF_SLOTS, device=DEV)
    lead_lv, lead_bank = (es if off in ("levels", "both") else 0), (es if off in ("bank", "both") else 0)
    hb = placed(grad_bank, lead_bank, device=DEV, name="grad_bank")
    hl = [placed(torch.zeros(OFF_IMG, OFF_C, h, w, dtype=dtype), lead_lv, OUTPUT_GUARD, DEV, name=f"grad level {i}")
          for i, (h, w) in enumerate(OFF_SHAPES)]
    for h in hl:
        poison(h.t)
    ptrs, hw = _c_tables([h.t for h in hl], OFF_SHAPES)
    MSDA._call("mmfs_bank_scatter", "mmfs_bank_scatter", torch.device(DEV, 0), _code(dtype), len(hl), ptrs, hw, src.data_ptr(),
               hb.t.data_ptr(), OFF_IMG, OFF_C, len(OFF_SLOTS))
    torch.cuda.synchronize()
    assert_guards_intact(hb, *hl)
    assert_payload_unchanged(hb)
    for i, h in enumerate(hl):
        assert_no_poison(h.t, f"grad level {i}")
    assert_scatter_within_bound([h.t for h in hl], grad_bank, src, OFF_IMG, OFF_C, OFF_SHAPES, dtype, f"{off} off")
    # alignment changes how the operands are loaded and stored, not the order of the sum: the aligned call's bits
    aligned = [torch.empty(OFF_IMG, OFF_C, h, w, dtype=dtype, device=DEV) for h, w in OFF_SHAPES]
    ptrs, hw = _c_tables(aligned, OFF_SHAPES)
    gb = grad_bank.to(DEV)
    MSDA._call("mmfs_bank_scatter", "mmfs_bank_scatter", torch.device(DEV, 0), _code(dtype), len(hl), ptrs, hw, src.data_ptr(),
               gb.data_ptr(), OFF_IMG, OFF_C, len(OFF_SLOTS))
    for i, (h, a) in enumerate(zip(hl, aligned)):
        assert_bit_equal(h.t, a, f"grad level {i} ({off} off vs aligned)")


MANY_SHAPES, MANY_C, MANY_IMG = [(7, 7), (1, 1)], 24, 3


@pytest.mark.parametrize("n_slots", [65, 256, 257, 600])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_bank_scatter_over_many_slots(dtype, n_slots):
    """More slots than one wave tests (65), exactly one 256-slot step, one more (257: the second step has a single slot)
    and a third step (600), three images shown again and again with padding slots between: matches in every wave's ballot
    and in every step, summed in ascending slot order."""
    g = torch.Generator().manual_seed(100 + n_slots)
    src = torch.randint(-1, MANY_IMG, (n_slots,), generator=g)
    src[-1] = 1                                                          # (the last slot of the last step counts)
    assert all(int((src == i).sum()) > n_slots // 8 for i in range(MANY_IMG))
    levels = [torch.randn(MANY_IMG, MANY_C, h, w, generator=g).to(DEV, dtype).requires_grad_(True) for h, w in MANY_SHAPES]
    out = BankGather(src.to(DEV), levels)
    assert torch.equal(out.detach(), torch_bank([f.detach() for f in levels], src.to(DEV)))
    grad = torch.randn(out.shape, generator=g).to(dtype)
    out.backward(grad.to(DEV))
    torch.cuda.synchronize()
    assert_scatter_within_bound([f.grad for f in levels], grad, src, MANY_IMG, MANY_C, MANY_SHAPES, dtype, f"{n_slots} slots")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_bank_scatter_of_an_image_no_slot_shows_among_300(dtype):
    g = torch.Generator().manual_seed(23)
    src = torch.randint(-1, 2, (300,), generator=g) * 2                  # -2 (padding), 0, 2: image 1 is never shown
    levels = [torch.randn(MANY_IMG, MANY_C, h, w, generator=g).to(DEV, dtype).requires_grad_(True) for h, w in MANY_SHAPES]
    out = BankGather(src.to(DEV), levels)
    grad = torch.randn(out.shape, generator=g).to(dtype)
    out.backward(grad.to(DEV))
    torch.cuda.synchronize()
    assert_scatter_within_bound([f.grad for f in levels], grad, src, MANY_IMG, MANY_C, MANY_SHAPES, dtype, "image 1 unseen")
    for f in levels:
        assert_bit_equal(f.grad[1], torch.zeros_like(f.grad[1]), "the gradient of the image nobody shows (+0, every bit)")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_bank_scatter_without_slots_gives_exact_zeros(dtype):
    """n_slots == 0 with three images, through the C entry (the wrapper's ``bank_gather_supported`` refuses no slots): no
    slot table and no grad_bank to read, every gradient element written, +0."""
    import MultiScaleDeformableAttention as MSDA
    hl = [placed(torch.zeros(MANY_IMG, MANY_C, h, w, dtype=dtype), 0, OUTPUT_GUARD, DEV, name=f"grad level {i}")
          for i, (h, w) in enumerate(MANY_SHAPES)]
    for h in hl:
        poison(h.t)
    ptrs, hw = _c_tables([h.t for h in hl], MANY_SHAPES)
    MSDA._call("mmfs_bank_scatter", "mmfs_bank_scatter", torch.device(DEV, 0), _code(dtype), len(hl), ptrs, hw, None, None,
               MANY_IMG, MANY_C, 0)
    torch.cuda.synchronize()
    assert_guards_intact(*hl)
    for i, h in enumerate(hl):
        assert_bit_equal(h.t, torch.zeros_like(h.t), f"grad level {i}")
