"""CPU-side checks of the inference-only fp8 value bank (include/mmfs_msda.h "fp8 bank"): the C ABI declares and exports its
three entries at ABI 14, refuses bad arguments before any launch (null pointers throughout: nothing reaches a device), and
the torch statement of the quantiser rule behaves as documented on its edge cases."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mm-interleaved_amd")]
HEADER = os.path.join(ROOT, "include", "mmfs_msda.h")
E_DTYPE, E_DIMS, E_NULLPTR, E_UNSUPPORTED = -1, -2, -3, -5
ENTRIES = ("mmfs_bank_quantize_fp8", "mmfs_msda_forward_fp8", "mmfs_sample_forward_heads_fp8")


from helpers import bound_library as _lib  # noqa: E402


def test_header_declares_and_library_exports_the_fp8_entries_at_abi_14():
    lib = _lib()
    text = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(lib, name)
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert int(re.search(r"#define\s+MMFS_MSDA_ABI_VERSION\s+(\d+)", text).group(1)) == 14
    assert "14 (additive)" in text
    assert lib.mmfs_msda_abi_version() == 14


@pytest.mark.parametrize("dtype,nb,Bv,R,C,want", [
    (3, 1, 2, 64, 256, E_DTYPE), (4, 1, 2, 64, 256, E_DTYPE), (-1, 1, 2, 64, 256, E_DTYPE),
    (2, -1, 2, 64, 256, E_DIMS), (2, 1, -2, 64, 256, E_DIMS), (2, 1, 2, -1, 256, E_DIMS),
    (2, 1, 2, 64, 40, E_UNSUPPORTED), (0, 13, 2, 64, 24, E_UNSUPPORTED),
    (2, 1, 2, 64, 256, E_NULLPTR), (0, 13, 2, 64, 512, E_NULLPTR), (1, 1, 1, 0, 64, E_NULLPTR)])
def test_quantize_refuses_bad_arguments_before_any_launch(dtype, nb, Bv, R, C, want):
    assert _lib().mmfs_bank_quantize_fp8(dtype, None, nb, Bv, R, C, None, None, None) == want


def _fwd(dtype=2, B=8, Bv=8, layout=0, S=64, H=8, D=128, L=4, Nq=16, P=4):
    return _lib().mmfs_msda_forward_fp8(dtype, None, None, None, None, None, None, None, B, Bv, layout, S, H, D, L, Nq, P, None)


def test_forward_fp8_refuses_bad_arguments_before_any_launch():
    assert _fwd(dtype=3) == E_DTYPE                       # fp64 output: no fp8 route
    assert _fwd(dtype=7) == E_DTYPE
    assert _fwd(Bv=0) == E_DIMS and _fwd(Bv=3) == E_DIMS and _fwd(B=-1) == E_DIMS
    assert _fwd(Bv=4, layout=2) == E_UNSUPPORTED
    for D in (8, 24, 40, 48, 100, 512):                   # D = 16 * 2^k, k <= 4 only
        assert _fwd(D=D) == E_UNSUPPORTED, D
    for D in (16, 32, 64, 128, 256):
        assert _fwd(D=D) == E_NULLPTR, D
    assert _fwd(Bv=4, layout=1) == E_NULLPTR and _fwd(Bv=2, layout=0) == E_NULLPTR


def _sample(dtype=2, N=6, Nv=6, layout=0, S=84, Lq=16, H=4, D=64, L=3, P=4, n=1, M=5, Lr=1, Nr=1):
    return _lib().mmfs_sample_forward_heads_fp8(dtype, None, None, None, None, None, None, 0, 0, None, None, None, None, None,
                                                None, None, None, N, Nv, layout, S, Lq, H, D, L, P, n, M, Lr, Nr, None)


def test_sampler_fp8_refuses_bad_arguments_before_any_launch():
    assert _sample(dtype=3) == E_DTYPE
    assert _sample(Nv=0) == E_DIMS and _sample(Nv=4, layout=1) == E_DIMS
    assert _sample(Nv=3, layout=5) == E_UNSUPPORTED
    for D in (8, 24, 48, 512):
        assert _sample(D=D) == E_UNSUPPORTED, D
    assert _sample(P=16) == E_UNSUPPORTED
    for D in (16, 32, 64, 128, 256):
        assert _sample(D=D) == E_NULLPTR, D
    assert _sample(Nv=3, layout=1) == E_NULLPTR


def test_existing_entries_still_refuse_other_dtypes():
    lib = _lib()
    assert lib.mmfs_msda_forward_shared(4, None, None, None, None, None, None, 8, 8, 0, 64, 8, 128, 4, 16, 4, 0, None) == E_DTYPE


# ---------------------------------------------------------------- the quantiser rule (torch statement)
def _codes(q):
    return q.view(torch.uint8)


def _rule():
    import MultiScaleDeformableAttention as MSDA
    return MSDA


def test_rule_zero_columns_are_zero_scale_and_plus_zero():
    MSDA = _rule()
    x = torch.randn(2, 9, 2, 16)
    x[:, :, 1, 3] = 0.0
    x[1, :, 0, 5] = -0.0
    q, s = MSDA.quantize_bank_fp8(x)
    assert s.shape == (2, 32) and s.dtype == torch.float32
    assert (s[:, 16 + 3] == 0).all() and s[1, 5] == 0
    assert (_codes(q)[:, :, 1, 3] == 0).all() and (_codes(q)[1, :, 0, 5] == 0).all()


def test_rule_column_maximum_maps_to_448():
    MSDA = _rule()
    x = torch.randn(3, 11, 1, 32)
    x[1, 4, 0, 7] = 100.0
    x[2, 6, 0, 9] = -250.0
    q, s = MSDA.quantize_bank_fp8(x)
    assert s[1, 7] == torch.tensor(100.0) / 448 and s[2, 9] == torch.tensor(250.0) / 448
    assert q[1, 4, 0, 7].float() == 448.0 and q[2, 6, 0, 9].float() == -448.0
    # every column's largest element is +-448, nothing exceeds it
    assert (q.float().abs().amax(1) == 448.0).all()
    d = MSDA.dequantize_bank_fp8(q, s)
    assert d[1, 4, 0, 7] == pytest.approx(100.0, rel=2 ** -20)


def test_rule_subnormal_range_and_the_error_bound():
    MSDA = _rule()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 2, 16, generator=g) * torch.logspace(-6, 0, 64).view(1, 64, 1, 1)
    x[:, 0] = 1.0                                              # amax 1 per column: scale 1/448
    q, s = MSDA.quantize_bank_fp8(x)
    y = x / s.view(2, 1, 2, 16)
    small = y.abs() < 2 ** -6                                  # below e4m3's smallest normal
    assert small.any()
    # subnormal codes are multiples of 2^-9 of the scale, rounded to nearest
    qs = q.float()[small]
    assert torch.equal(qs, torch.round(qs * 512) / 512)
    assert ((qs - y[small]).abs() <= 2 ** -10 + 1e-12).all()
    d = MSDA.dequantize_bank_fp8(q, s)
    bound = 2 ** -4 * x.abs() + 2 ** -10 * s.view(2, 1, 2, 16)
    assert ((d - x).abs() <= bound).all()


def test_rule_non_finite_elements_are_nan_codes_and_leave_the_scale():
    MSDA = _rule()
    x = torch.randn(2, 8, 1, 16)
    x[0, 2, 0, 4] = x[1, 5, 0, 4] = x[1, 6, 0, 11] = 0.0       # (not a column's maximum)
    ref_q, ref_s = MSDA.quantize_bank_fp8(x)
    x2 = x.clone()
    x2[0, 2, 0, 4] = float("nan")
    x2[1, 5, 0, 4] = float("inf")
    x2[1, 6, 0, 11] = float("-inf")
    q, s = MSDA.quantize_bank_fp8(x2)
    assert torch.equal(s, ref_s)                               # the scales ignore them
    codes = _codes(q)
    assert codes[0, 2, 0, 4] == 0x7f and codes[1, 5, 0, 4] == 0x7f and codes[1, 6, 0, 11] == 0x7f
    assert torch.isnan(q.float()[0, 2, 0, 4]) and torch.isnan(q.float()[1, 6, 0, 11])
    keep = torch.isfinite(x2)
    assert torch.equal(_codes(q)[keep], _codes(ref_q)[keep])   # no other element moves


def test_rule_batch_of_banks_is_each_bank_alone():
    MSDA = _rule()
    x = torch.randn(3, 2, 10, 2, 16)
    q, s = MSDA.quantize_bank_fp8(x)
    assert q.shape == x.shape and s.shape == (3, 2, 32)
    for k in range(3):
        qk, sk = MSDA.quantize_bank_fp8(x[k])
        assert torch.equal(_codes(q[k]), _codes(qk)) and torch.equal(s[k], sk)


def test_module_defaults_are_off():
    from mmfs_amd.blocks.llama_mmfs import LlamaMMFSSchedule
    from mmfs_amd.blocks.sd_mmfs import MMFSNet, ProjectedFeatures
    assert MMFSNet.kept_bank_dtype is None and LlamaMMFSSchedule.kept_bank_dtype is None
    assert ProjectedFeatures([], None, []).scales is None


def test_shim_refuses_a_bank_without_its_scale_on_the_cpu():
    MSDA = _rule()
    with pytest.raises(RuntimeError):
        MSDA.ms_deform_attn_forward(torch.zeros(1, 4, 1, 16, dtype=torch.float8_e4m3fn), None, None, None, None, 1)
