"""CPU test of ``tile_pair`` (csrc/msda_bwd_block.h), the rule by which the matrix-core grad_value reduce takes two
neighbouring whole 4x4 blocks as one work item, through the library's host-only self-check (as tests/test_plan_cpu.py):
for a block row of every width 1-17 (one block; an even and an odd number of blocks; a last block of 1-4 columns, so every
(bx, nbx4) parity and run boundary), every ordered couple of its blocks merges exactly when the first is even, the second
its right neighbour and the merged list fits the chunk (one below, at, one above); the merged runs are the cells
4 bx .. 4 bx + 8 with the shared cell once; a cut partner, another block row or another level refuse."""
import pytest

from helpers import bound_library


@pytest.mark.parametrize("width", range(1, 18))
def test_pair_rule_on_every_block_row(width):
    selfcheck = bound_library().mmfs_msda_plan_selfcheck
    for height in (1, 3, 4, 9):
        assert selfcheck(height, width, 1) == 0, (height, width)
