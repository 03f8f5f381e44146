"""CPU-side checks of the shared value bank (one bank of Bv rows serving B = g * Bv query rows, include/mmfs_msda.h
MMFS_BANK_*): the C ABI exports its two entries and refuses bad maps without touching a GPU, the host-side row map is the
index order of ``torch.cat([x] * g)`` / ``x.repeat_interleave(g, 0)``, and the shim's argument checks."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mm-interleaved_amd")]
HEADER = os.path.join(ROOT, "include", "mmfs_msda.h")
E_DIMS, E_UNSUPPORTED = -2, -5


from helpers import bound_library as _lib  # noqa: E402


def test_library_exports_the_shared_entries_at_abi_14():
    lib = _lib()
    for name in ("mmfs_msda_forward_shared", "mmfs_sample_forward_heads_shared"):
        assert hasattr(lib, name)
    text = open(HEADER).read()
    assert int(re.search(r"#define\s+MMFS_MSDA_ABI_VERSION\s+(\d+)", text).group(1)) == 14
    assert re.search(r"#define\s+MMFS_BANK_TILE\s+0\b", text) and re.search(r"#define\s+MMFS_BANK_INTERLEAVE\s+1\b", text)
    assert lib.mmfs_msda_abi_version() == 14


@pytest.mark.parametrize("B,Bv,layout,want", [(8, 0, 0, E_DIMS), (8, -2, 0, E_DIMS), (8, 3, 0, E_DIMS), (8, 3, 1, E_DIMS),
                                              (8, 4, 2, E_UNSUPPORTED), (8, 4, -1, E_UNSUPPORTED)])
def test_forward_shared_refuses_bad_maps_before_any_launch(B, Bv, layout, want):
    # (null pointers throughout: the checks come first, nothing reaches a device)
    assert _lib().mmfs_msda_forward_shared(2, None, None, None, None, None, None, B, Bv, layout, 64, 8, 128, 4, 16, 4,
                                           0, None) == want


@pytest.mark.parametrize("N,Nv,layout,want", [(6, 0, 0, E_DIMS), (6, 4, 1, E_DIMS), (6, 3, 5, E_UNSUPPORTED)])
def test_sampler_shared_refuses_bad_maps_before_any_launch(N, Nv, layout, want):
    # dims: S, Lq, H, D, L, P, n, M, Lr, Nr
    assert _lib().mmfs_sample_forward_heads_shared(2, None, None, None, None, None, 0, 0, None, None, None, None, None, None,
                                                   None, None, N, Nv, layout, 84, 16, 4, 64, 3, 4, 1, 5, 1, 1, None) == want


@pytest.mark.parametrize("Bv,g", [(1, 1), (1, 2), (3, 2), (1, 5), (3, 5), (4, 2), (2, 3)])
def test_row_map_is_the_index_order_of_the_expanded_bank(Bv, g):
    import MultiScaleDeformableAttention as MSDA
    rows = torch.arange(Bv)
    assert MSDA.value_row_map(g * Bv, Bv, "tile") == torch.cat([rows] * g).tolist()
    assert MSDA.value_row_map(g * Bv, Bv, "interleave") == rows.repeat_interleave(g, 0).tolist()
    if g == 1:
        assert MSDA.value_row_map(Bv, Bv, "tile") == MSDA.value_row_map(Bv, Bv, "interleave") == list(range(Bv))


def _args(Bv, B, H=2, D=8, Nq=5, P=4, shapes=((4, 4), (2, 2))):
    sh = torch.tensor(shapes, dtype=torch.long)
    start = torch.cat((sh.new_zeros(1), sh.prod(1).cumsum(0)[:-1]))
    S, L = int(sh.prod(1).sum()), len(shapes)
    return (torch.zeros(Bv, S, H, D), sh, start, torch.zeros(B, Nq, H, L, P, 2), torch.zeros(B, Nq, H, L, P))


def test_shim_checks():
    import MultiScaleDeformableAttention as MSDA
    # a shared bank: the query batch comes from the locations
    assert MSDA._dims_shared(*_args(3, 6), "tile") == (6, 20, 2, 8, 2, 5, 4, 3)
    assert MSDA._dims_shared(*_args(2, 10), "interleave")[0::7] == (10, 2)
    with pytest.raises(RuntimeError, match=r"bank's batch \(4\) must divide the query batch \(6\)"):
        MSDA._dims_shared(*_args(4, 6), "tile")
    with pytest.raises(RuntimeError, match=r"bank's batch \(0\) must divide"):
        MSDA._dims_shared(*_args(0, 6), "interleave")
    with pytest.raises(RuntimeError, match="value_repeat must be None, 'tile' or 'interleave'"):
        MSDA._dims_shared(*_args(3, 6), "repeat")
    with pytest.raises(RuntimeError, match="value_repeat must be None"):
        MSDA.value_row_map(6, 3, "cat")
    # no sharing asked: mismatched batches keep today's refusal, word for word
    with pytest.raises(RuntimeError, match=re.escape("sampling_loc shape (6, 5, 2, 2, 4, 2) != (3, 5, 2, 2, 4, 2)")):
        MSDA._dims(*_args(3, 6))
    # CPU tensors are refused first, as before, whatever the map
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        MSDA.ms_deform_attn_forward(*_args(3, 6), 1, value_repeat="tile")


def test_module_refuses_a_bank_that_does_not_divide_the_queries():
    from mmfs_amd.modules import MMFS
    m = MMFS(d_model=32, n_levels=2, n_heads=2, n_points=4, spatial_shapes=[4, 2], base_spatial_shape=4)
    q = torch.zeros(6, 5, 32)
    ref = torch.full((1, 5, 1, 2), 0.5)
    sh, start = _args(1, 1)[1:3]
    with pytest.raises(ValueError, match="bank_repeat='tile'"):
        m(q, ref, torch.zeros(4, 1, 20, 32), sh, start, attention_mask=torch.ones(6, 1), bank_repeat="tile")
    with pytest.raises(ValueError, match="bank_repeat='beams'"):
        m(q, ref, torch.zeros(3, 1, 20, 32), sh, start, attention_mask=torch.ones(6, 1), bank_repeat="beams")
