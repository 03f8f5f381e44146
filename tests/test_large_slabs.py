"""CPU side of tests/test_large_slabs_gpu.py: what that file relies on, and that its check would see the faults it is
there for.

  * ``helpers.head_subset``: the oracle on the reduced problem IS the oracle's result at those heads, bit for bit -- the
    ground the GPU file stands on when it holds 8 of 256 heads of a 4 GiB tensor to the fp64 bound.
  * ``helpers.worst_ratio`` (the bound applied where the output lives) gives ``helpers.bound_ratios``' verdicts.
  * Planted faults.  The kernels' 32-bit arithmetic on byte offsets is restated in fp64 with a word of k bits and a row
    pitch scaled down to match, at NQ = 40 queries, and each fault the large-slab paths could have must break the
    per-element bound:
      - a contribution of one query dropped (a byte offset equal to the "no row" mark, 2^(k-1));
      - grad_out rows read from index (q * pitch mod 2^k) / pitch (the product wraps);
      - a buffer descriptor whose length was truncated to k bits (rows past it read as zeros).
    The bar the op's tests used before the per-element bound, TOL * max|ref| (tests/test_op_gpu.py), lets the dropped
    contribution through: asserted below, it is why the GPU file compares element by element."""
import numpy as np
import pytest
import torch

import helpers
from helpers import OUTPUTS, bound_ratios, error_bounds, head_subset, head_subset_outputs, make_inputs, worst_ratio

TOL_BF16 = 8e-3                      # tests/test_op_gpu.py TOL[torch.bfloat16]


def _oracle(x):
    return helpers._oracle(x)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("heads", [(0,), (4, 0, 2), (0, 1, 2, 3, 4), (3, 3)])
def test_head_subset_commutes_with_the_oracle(dtype, heads):
    B, H, D, Nq, P = 2, 5, 8, 7, 2
    x = make_inputs(B, H, D, Nq, P, [(3, 4), (0, 2), (2, 2)], seed=3, loc_range=(-0.2, 1.2), dtype=dtype)
    x["loc"][0, 1, 0, 0, 0, 0] = float("nan")
    x["attn"][1, 2, 4] = 0.0
    full = _oracle(x)
    sub = head_subset(x, heads)
    assert sub["value"].shape == (B, 16, len(heads), D) and sub["grad"].shape == (B, Nq, len(heads) * D)
    assert sub["shapes"] is x["shapes"] and sub["start"] is x["start"]
    want = head_subset_outputs([torch.as_tensor(t) for t in full], heads, H)
    for name, got, ref in zip(OUTPUTS, _oracle(sub), want):
        assert np.array_equal(got, ref.numpy().reshape(got.shape), equal_nan=True), name


def test_worst_ratio_is_bound_ratios():
    dtype = torch.bfloat16
    x = make_inputs(1, 2, 8, 9, 2, [(4, 5), (2, 2)], seed=5, loc_range=(-0.2, 1.2), dtype=dtype)
    bounds, ref = error_bounds(x, dtype)
    skip = torch.as_tensor(np.ascontiguousarray(helpers.near_crossing(x)))
    g = torch.Generator().manual_seed(1)
    for trial in ("clean", "noise", "stray", "nan"):
        got = {n: torch.as_tensor(ref[n]).clone() for n in OUTPUTS}
        if trial == "noise":
            got = {n: t * (1 + 2.0 ** -10 * torch.randn(t.shape, generator=g, dtype=torch.float64)) for n, t in got.items()}
        if trial == "stray":           # an element whose bound is 0 (an untouched pixel) gets something
            k = int(np.flatnonzero(np.broadcast_to(bounds["grad_value"], ref["grad_value"].shape).reshape(-1) == 0)[0])
            got["grad_value"].reshape(-1)[k] = 1e-30
        if trial == "nan":
            got["out"].reshape(-1)[3] = float("nan")
        want = bound_ratios([got[n].numpy() for n in OUTPUTS], x, dtype, bounds=bounds)
        for n in OUTPUTS:
            r = worst_ratio(got[n], torch.as_tensor(ref[n]), torch.as_tensor(np.broadcast_to(bounds[n], ref[n].shape).copy()),
                            skip if n == "grad_loc" else None)
            assert r[0] == want[n][0] or abs(r[0] - want[n][0]) <= 1e-12 * want[n][0], (trial, n, r, want[n])
        if trial == "stray":
            assert want["grad_value"][0] == float("inf")
        if trial == "nan":
            assert want["out"][0] == float("inf")


# --------------------------------------------------------------------------------------------------------------------
# fp64 restatement of the two gathers whose addresses the large-slab paths compute: grad_value reads grad_out row
# row_of(q); the forward reads value row pix unless reads(pix) says the descriptor answers zeros.
# --------------------------------------------------------------------------------------------------------------------
NQ, H, D, P = 40, 2, 8, 2
SHAPES = [(6, 6), (2, 3)]


def restate(x, row_of=lambda q: q, reads=lambda pix: True):
    value, loc, attn = x["value"].numpy(), x["loc"].numpy(), x["attn"].numpy()
    B, S = value.shape[:2]
    grad = x["grad"].numpy().reshape(B, NQ, H, D)
    out, gv = np.zeros((B, NQ, H, D)), np.zeros_like(value)
    for b in range(B):
        for q in range(NQ):
            r = row_of(q)
            for h in range(H):
                for l, ((Hl, Wl), s0) in enumerate(zip(x["shapes"].tolist(), x["start"].tolist())):
                    for p in range(P):
                        px, py = loc[b, q, h, l, p, 0] * Wl - 0.5, loc[b, q, h, l, p, 1] * Hl - 0.5
                        if not (py > -1 and px > -1 and py < Hl and px < Wl):
                            continue
                        x0, y0 = int(np.floor(px)), int(np.floor(py))
                        fx, fy = px - x0, py - y0
                        for dy, dx, w in ((0, 0, (1 - fy) * (1 - fx)), (0, 1, (1 - fy) * fx), (1, 0, fy * (1 - fx)), (1, 1, fy * fx)):
                            yy, xx = y0 + dy, x0 + dx
                            if 0 <= yy < Hl and 0 <= xx < Wl:
                                pix = s0 + yy * Wl + xx
                                if reads(pix):
                                    out[b, q, h] += w * attn[b, q, h, l, p] * value[b, pix, h]
                                if r is not None:
                                    gv[b, pix, h] += w * attn[b, q, h, l, p] * grad[b, r, h]
    return out.reshape(B, NQ, H * D), gv


def planted_case(q_alone):
    """NQ queries on a 6 x 6 and a 2 x 3 map; the first level's samples of every query but ``q_alone`` stay in columns
    >= 3, ``q_alone``'s sit on pixel (1, 1): its rows are all that pixel gets.  All of ``q_alone``'s attention weights are
    2^-10 (a query that attends elsewhere), so what it adds anywhere is small against the largest entry."""
    dtype = torch.bfloat16
    x = make_inputs(1, H, D, NQ, P, SHAPES, seed=11, loc_range=(0.0, 1.0), dtype=dtype)
    x["loc"][:, :, :, 0, :, 0] = (x["loc"][:, :, :, 0, :, 0] * 0.5 + 0.6).to(dtype).double()
    x["loc"][:, q_alone, :, 0] = 0.25                       # (1.5 / 6: pixel (1, 1), weights 1, 0, 0, 0)
    x["attn"][:, q_alone] = 2.0 ** -10
    return x, dtype


def test_restatement_is_the_oracle():
    x, dtype = planted_case(16)
    ref = _oracle(x)
    out, gv = restate(x)
    assert np.abs(out - ref[0]).max() <= 1e-13 and np.abs(gv - ref[1]).max() <= 1e-13
    res = bound_ratios([out, gv, None, None], x, dtype, ("out", "grad_value"))
    assert res["out"][0] <= 1e-6 and res["grad_value"][0] <= 1e-6


K_BITS, PITCH = 12, 128              # a 12-bit word for the kernels' 32, rows of 128 bytes for 65536: the same ratios


def test_a_dropped_contribution_breaks_the_bound_and_passes_the_old_bar():
    """The query whose byte offset q * pitch equals the "no row" mark 2^(k-1) is dropped (csrc/msda_bwd_value.hip before
    its flat path fetched records with a pitch of 1).  Its rows are all that pixel (1, 1) gets, so the element that should
    hold them is exactly 0: the per-element bound is broken by orders of magnitude, while the error is far below
    TOL * max|ref| -- the old bar lets the fault through."""
    mark = 1 << (K_BITS - 1)
    q_drop = mark // PITCH
    assert q_drop * PITCH == mark and q_drop < NQ
    x, dtype = planted_case(q_drop)
    ref = _oracle(x)[1]
    _, gv = restate(x, row_of=lambda q: None if q * PITCH == mark else q)
    err = np.abs(gv - ref)
    assert 0 < err.max() <= 0.5 * TOL_BF16 * np.abs(ref).max(), (err.max(), np.abs(ref).max())     # the old bar passes it
    res = bound_ratios([None, gv, None, None], x, dtype, ("grad_value",))["grad_value"]
    assert res[0] > 100 and "y=1 x=1" in res[1], res
    pix = x["start"][0] + 1 * SHAPES[0][1] + 1
    assert not gv[0, pix].any() and ref[0, pix].all()


def test_wrapped_row_offsets_break_the_bound():
    """grad_out rows read from (q * pitch mod 2^k) / pitch: queries from 2^k / pitch on read the rows of others."""
    x, dtype = planted_case(16)
    wrap = lambda q: (q * PITCH % (1 << K_BITS)) // PITCH
    assert wrap(NQ - 1) != NQ - 1 and wrap(5) == 5
    _, gv = restate(x, row_of=wrap)
    res = bound_ratios([None, gv, None, None], x, dtype, ("grad_value",))["grad_value"]
    assert res[0] > 100, res


def test_a_truncated_descriptor_length_breaks_the_bound():
    """A descriptor over S rows of ``pitch`` bytes whose length keeps k bits: rows from (S * pitch mod 2^k) / pitch on
    read as zeros (at S * pitch == 2^k, every row)."""
    x, dtype = planted_case(16)
    S = x["value"].shape[1]
    length = S * PITCH % (1 << K_BITS)
    assert 0 < length < S * PITCH
    out, _ = restate(x, reads=lambda pix: pix * PITCH < length)
    res = bound_ratios([out, None, None, None], x, dtype, ("out",))["out"]
    assert res[0] > 100, res
