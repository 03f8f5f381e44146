"""GPU parity of the matrix-core grad_value reduce where two neighbouring whole 4x4 blocks are ONE work item of 4 x 8 pixels
(csrc/msda_bwd_tile.hip, ``tile_pair`` in csrc/msda_bwd_block.h; knob MMFS_TILE_PAIR): grad_value against the CPU oracle
per element, and against the same library with MMFS_TILE_PAIR=0 -- both runs lie within the element's bound of the
oracle, so they differ by at most twice that bound, and where the bound is 0 both are exactly 0.

Shapes are the smallest at which the pairing can go wrong: widths 8 (one pair), 4 (no pair), 12 (a pair and an odd last
block), 5 (a pair whose second block is one column), 1; heights 1, 3, 9 (a last block row shorter than 4, the border row of
cells); samples on pixel centres, on the seam column between the two blocks of a pair and outside the map; lists that are
empty in one or both blocks; a hot cell that cuts one block of a pair (no pair); a pair whose merged list is exactly
``tile_chunk`` records (still a pair) and one over (no pair)."""
import numpy as np
import pytest
import torch

import helpers
from helpers import assert_within_bounds, error_bounds, make_inputs
from test_op_gpu import run_hip

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
WIDTHS = [32, 64, 128]


# csrc/msda_bwd_block.h: tile_chunk, the records of a work item, for launches of fewer than 8 M record visits
TILE_CHUNK = {128: 768, 64: 768, 32: 3072}


def both_ways(x, dtype, what, monkeypatch, **kw):
    """grad_value with pairs and without, each within the per-element bound of the oracle; -> the two arrays."""
    import MultiScaleDeformableAttention as MSDA
    helpers.poison_allocations(monkeypatch)             # (a pixel row nobody writes is NaN, not the previous call's answer)
    log = []
    monkeypatch.setattr(MSDA, "_event_log", log)
    got = run_hip(x, dtype, use_autograd=False, **kw)
    if kw.get("register"):          # (a table the host knows: one entry per kernel; else the library's one checked call)
        assert "msda_bwd_value_reduce" in [n for n, _, _ in log], log
    with monkeypatch.context() as m:
        m.setenv("MMFS_TILE_PAIR", "0")
        alone = run_hip(x, dtype, use_autograd=False, **kw)
    monkeypatch.setattr(MSDA, "_event_log", None)
    res = assert_within_bounds(got, x, dtype, what + " pairs", outputs=("grad_value",))
    res0 = assert_within_bounds(alone, x, dtype, what + " MMFS_TILE_PAIR=0", outputs=("grad_value",))
    bound = error_bounds(x, dtype)[0]["grad_value"]
    diff = np.abs(got[1] - alone[1]).reshape(bound.shape)
    over = diff - 2.0 * bound
    print(f"TILE-PAIR {str(dtype)[6:]} {what}: worst ratio to the bound {res['grad_value'][0]:.3g} (pairs) "
          f"{res0['grad_value'][0]:.3g} (none); largest difference between the two {float(diff.max()):.3g}")
    assert float(over.max()) <= 0.0, f"{what}: the two runs differ by {float(over.max()):.3e} more than twice the bound"
    return got[1], alone[1]


GEOMETRY = [(9, 8), (3, 12), (1, 5), (9, 4), (3, 1), (1, 8), (9, 12), (4, 5)]


def geometry_inputs(B, H, D, dtype):
    """Uniform samples over and around every level; half of them moved onto pixel centres and onto the half-way points
    between two pixel columns / rows (x = 3.5: the seam between the two blocks of a pair), from one pixel outside the map
    to one pixel outside on the other side."""
    Nq, P = 48, 4
    x = make_inputs(B, H, D, Nq, P, GEOMETRY, seed=31, loc_range=(-0.15, 1.15), dtype=dtype)
    g = torch.Generator().manual_seed(32)
    for l, (Hl, Wl) in enumerate(GEOMETRY):
        ys = (torch.randint(-2, 2 * Hl + 2, (B, Nq, H, P), generator=g).double() * 0.5 + 0.5) / Hl
        xs = (torch.randint(-2, 2 * Wl + 2, (B, Nq, H, P), generator=g).double() * 0.5 + 0.5) / Wl
        move = torch.rand(B, Nq, H, P, generator=g) < 0.5
        x["loc"][:, :, :, l, :, 0] = torch.where(move, xs, x["loc"][:, :, :, l, :, 0])
        x["loc"][:, :, :, l, :, 1] = torch.where(move, ys, x["loc"][:, :, :, l, :, 1])
    x["loc"] = x["loc"].to(dtype).double()
    return x


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("register", [False, True], ids=["device-checked", "registered"])
def test_pairs_on_every_block_geometry(register, dtype, D, monkeypatch):
    """``registered``: the host knows the level table and the reduce's grid is the exact block count; else the grid is the
    bound and the table is checked on the device."""
    B, H = 2, 2
    both_ways(geometry_inputs(B, H, D, dtype), dtype, f"geometry D{D}", monkeypatch, register=register)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["left", "right", "nowhere"])
def test_pairs_with_empty_lists(where, dtype, D, monkeypatch):
    """One 4 x 8 level = one pair.  All samples over the left block's first columns (the right block's list is empty), over
    the right block's last columns, or outside the map (both lists empty: the pair's 32 rows are zeros, and written)."""
    B, H, Nq, P = 1, 2, 24, 4
    x = make_inputs(B, H, D, Nq, P, [(4, 8)], seed=41, dtype=dtype)
    lo, hi = {"left": (0.07, 0.30), "right": (0.70, 0.93), "nowhere": (1.2, 1.5)}[where]
    x["loc"][..., 0] = (x["loc"][..., 0] * (hi - lo) + lo).to(dtype).double()
    paired, _ = both_ways(x, dtype, f"empty {where} D{D}", monkeypatch, register=True)
    cols = paired.reshape(B, 4, 8, H, D)
    if where == "left":
        assert np.all(cols[:, :, 4:] == 0.0) and np.any(cols[:, :, :4] != 0.0)
    elif where == "right":
        assert np.all(cols[:, :, :4] == 0.0) and np.any(cols[:, :, 4:] != 0.0)
    else:
        assert np.all(cols == 0.0)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_cut_block_is_not_paired(dtype, D, monkeypatch):
    """A hot cell in the left block of a 4 x 8 level: its list is longer than ``tile_chunk`` and is cut into items with
    partial tiles, so the two blocks are walked on their own; a second level keeps pairs in the same launch."""
    B, H, P, shapes = 1, 2, 4, [(4, 8), (8, 8)]
    Nq = TILE_CHUNK[D] * 3 // 2 // P
    x = make_inputs(B, H, D, Nq, P, shapes, seed=51, dtype=dtype)
    hot = Nq * 5 // 6                                        # these queries' samples of level 0 fall around pixel (1.5, 1.5)
    x["loc"][:, :hot, :, 0] = ((x["loc"][:, :hot, :, 0] * 0.1 + torch.tensor([0.2, 0.45])).to(dtype)).double()
    both_ways(x, dtype, f"hot cell D{D}", monkeypatch, register=True)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("over", [0, 1])
def test_merged_list_at_and_over_tile_chunk(over, dtype, D, monkeypatch):
    """One 4 x 8 level whose samples all lie inside the map: the pair's merged list is every sample of the (b, h) slice,
    Nq * P records.  Exactly ``tile_chunk`` of them is still one item; four more and the blocks (each about half of them,
    whole) are walked on their own."""
    B, H, P = 2, 2, 4
    Nq = TILE_CHUNK[D] // P + over
    x = make_inputs(B, H, D, Nq, P, [(4, 8)], seed=61 + over, loc_range=(0.02, 0.98), dtype=dtype)
    both_ways(x, dtype, f"merged list of tile_chunk + {4 * over} D{D}", monkeypatch, register=True)


def test_pairs_on_the_sorted_records_route(monkeypatch):
    """The opt-in route whose records carry query * P + point (``a.qshift``) shares the reduce: a paired shape once."""
    import MultiScaleDeformableAttention as MSDA
    dtype = torch.bfloat16
    B, H, D, Nq, P, shapes = 2, 2, 128, 40, 4, [(8, 8), (4, 12), (3, 5)]
    monkeypatch.setattr(MSDA, "_taps_algo", "sorted")
    x = make_inputs(B, H, D, Nq, P, shapes, seed=71, loc_range=(-0.15, 1.15), dtype=dtype)
    both_ways(x, dtype, "sorted records", monkeypatch, register=True)
