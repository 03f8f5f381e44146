"""The per-element error bound of tests/helpers.py (used by check() in test_op_gpu.py, by fuzz_op.py and by
test_op_exact_scatter_gpu.py) has teeth and no false alarms -- on the CPU, with the oracle's own outputs standing in
for a kernel: results that a correct kernel could return pass, results with one contribution lost, moved or added
fail.  Also writes down the gap the bound closes: the old rule (TOL * max|ref| on out / grad_value) accepts a
dropped sample in bf16."""
import numpy as np
import pytest
import torch

import helpers as Hp
from helpers import make_inputs
from oracle import msda_oracle

TOL = {torch.float64: 1e-12, torch.float32: 1e-5, torch.float16: 1e-3, torch.bfloat16: 8e-3}     # check()'s old bars

NORTH_STAR = (2, 8, 128, 33, 4, [(16, 16), (8, 8), (4, 4), (2, 2)])
LLM = (1, 16, 64, 40, 8, [(8, 8), (4, 4), (2, 2)] * 4)
WIDE = (1, 8, 32, 4097, 4, [(16, 13), (40, 6)])          # levels 40 pixels wide: the bilinear weights' fp32 error shows


def inputs(case, dtype, seed=7):
    B, H, D, Nq, P, shapes = case
    return make_inputs(B, H, D, Nq, P, shapes, seed=seed, loc_range=(-0.15, 1.15), dtype=dtype)


def rounded(arrs, dtype):
    return [torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dtype).double().numpy() for a in arrs]


def old_rule_accepts(got, ref, dtype):
    ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(ref.shape) - ref).max()
    return err <= TOL[dtype] * max(1.0, float(np.abs(ref).max()))


def worst(res):
    return {n: r[0] for n, r in res.items()}


# ------------------------------------------------------------------------------------------------ the sums themselves
@pytest.mark.parametrize("case", [NORTH_STAR, LLM, (1, 2, 16, 30, 3, [(1, 7), (6, 1), (1, 1), (5, 3)])],
                         ids=["north_star", "llm", "degenerate"])
def test_term_sums_match_the_oracle_on_absolute_inputs(case):
    """The fp64 helper's A (bilinear weights kept) is the oracle's output on |inputs|: same edge semantics."""
    x = inputs(case, torch.float32)
    x["loc"][0, 0, 0, 0, 0, 0] = float("nan")
    x["loc"][0, 1, 0, -1, 0, 1] = float("inf")
    out, gv, _, ga = Hp.term_sums(x)
    v, sh, st, loc, at, gr = (x[k] for k in ("value", "shapes", "start", "loc", "attn", "grad"))
    a_out = msda_oracle.forward(v.abs(), sh, st, loc, at.abs())
    a_gv, _, a_ga = msda_oracle.backward(v.abs(), sh, st, loc, at.abs(), gr.abs())
    for got, want in ((out, a_out), (gv, a_gv), (ga, a_ga)):
        assert np.allclose(got, want, rtol=1e-12, atol=0.0)


def test_grad_loc_sum_follows_the_kernels_edges():
    """grad_loc's sum against a scalar restatement of msda_ref_body.inc: strict range test, corners off the map
    skipped, |attn| * extent * sum_c |g_c| * sum of |v| over the corners on the map; and it bounds the oracle's
    grad_loc (derivative weights lie in [0, 1])."""
    sh_list = [(3, 5), (1, 4), (2, 1)]
    x = make_inputs(1, 2, 3, 7, 3, sh_list, seed=3, loc_range=(-0.4, 1.4), dtype=torch.float64)
    x["loc"][0, 0, 0, 0, 0] = torch.tensor([0.1, 0.5 / 3])          # a pixel centre: both fractions 0
    x["loc"][0, 1, 1, 1, 2] = torch.tensor([-0.125, 0.5])          # x = -1: outside (strict test)
    _, _, gl, _ = Hp.term_sums(x)
    v, loc, at, g = x["value"].numpy(), x["loc"].numpy(), x["attn"].numpy(), x["grad"].numpy().reshape(1, 7, 2, 3)
    start = x["start"].tolist()
    want = np.zeros_like(gl)
    for q in range(7):
        for h in range(2):
            for l, (Hl, Wl) in enumerate(sh_list):
                for p in range(3):
                    px, py = loc[0, q, h, l, p, 0] * Wl - 0.5, loc[0, q, h, l, p, 1] * Hl - 0.5
                    if not (py > -1 and px > -1 and py < Hl and px < Wl):
                        continue
                    y0, x0 = int(np.floor(py)), int(np.floor(px))
                    s = 0.0
                    for yy in (y0, y0 + 1):
                        for xx in (x0, x0 + 1):
                            if 0 <= yy < Hl and 0 <= xx < Wl:
                                s += float(np.abs(g[0, q, h]) @ np.abs(v[0, start[l] + yy * Wl + xx, h]))
                    want[0, q, h, l, p] = abs(at[0, q, h, l, p]) * s * np.array([Wl, Hl])
    assert np.allclose(gl, want, rtol=1e-12, atol=0.0)
    _, ref_gl, _ = msda_oracle.backward(x["value"], x["shapes"], x["start"], x["loc"], x["attn"], x["grad"])
    assert (np.abs(ref_gl) <= gl * (1 + 1e-12)).all()


# ------------------------------------------------------------------------------------------------ accepted
@pytest.mark.parametrize("case", [NORTH_STAR, LLM, WIDE], ids=["north_star", "llm", "wide"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_accepts_the_reference_rounded_to_the_storage_type(case, dtype):
    x = inputs(case, dtype)
    ref = Hp._oracle(x)
    res = Hp.bound_ratios(rounded(ref, dtype), x, dtype)
    assert max(worst(res).values()) <= 1.0, res


@pytest.mark.parametrize("case", [NORTH_STAR, LLM, WIDE, (1, 4, 64, 6, 2, [(3, 3)] * 90)],
                         ids=["north_star", "llm", "wide", "L90"])
def test_accepts_the_oracles_fp32_evaluation_and_needs_lam_for_it(case):
    """An honest fp32 kernel: the oracle's own fp32 arithmetic (bilinear weights from loc * extent - 0.5 in fp32,
    sequential fp32 sums) meets the fp32 bound.  Without the lam term it would not, on 40-pixel-wide levels."""
    x = inputs(case, torch.float32)
    v, sh, st, loc, at, gr = (x[k] for k in ("value", "shapes", "start", "loc", "attn", "grad"))
    got = [msda_oracle.forward(v, sh, st, loc, at, dtype=np.float32),
           *msda_oracle.backward(v, sh, st, loc, at, gr, dtype=np.float32)]
    res = Hp.bound_ratios(got, x, torch.float32)
    assert max(worst(res).values()) <= 0.5, res
    if case is WIDE:
        ref = Hp._oracle(x)[0]
        a_out = msda_oracle.forward(v.abs(), sh, st, loc, at.abs())
        no_lam = Hp.STORAGE_U[torch.float32] * np.abs(ref) + Hp.GAMMA[torch.float32] * a_out
        err = np.abs(got[0] - ref)
        assert float((err[no_lam > 0] / no_lam[no_lam > 0]).max()) > 4.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_accepts_terms_perturbed_by_two_to_the_minus_16(dtype):
    """Weights carried as hi + lo 16-bit parts: every term off by 2^-16 relative (through the attention weight; grad
    entries perturbed too, so grad_attn's terms move as well) stays inside the bound."""
    x = inputs(LLM, dtype, seed=5)
    g = torch.Generator().manual_seed(1)
    sign = lambda t: torch.randint(0, 2, t.shape, generator=g).double() * 2 - 1
    y = dict(x, attn=x["attn"] * (1 + sign(x["attn"]) * 2.0 ** -16), grad=x["grad"] * (1 + sign(x["grad"]) * 2.0 ** -16))
    res = Hp.bound_ratios(Hp._oracle(y), x, dtype)
    assert max(worst(res).values()) <= 1.0, res


# ------------------------------------------------------------------------------------------------ rejected
def _contributing_samples(x, n, seed):
    """(b, q, h, l, p) of ``n`` random samples that contribute something (inside the map, nonzero weight)."""
    _, _, gl, _ = Hp.term_sums(x)
    ok = gl[..., 0] > 0
    idx = np.argwhere(ok)
    rng = np.random.default_rng(seed)
    return [tuple(int(i) for i in idx[k]) for k in rng.choice(len(idx), size=n, replace=False)]


@pytest.mark.parametrize("case,dtype", [(LLM, torch.bfloat16), (NORTH_STAR, torch.bfloat16), (NORTH_STAR, torch.float16),
                                        (NORTH_STAR, torch.float32)], ids=["llm-bf16", "north_star-bf16", "north_star-f16",
                                                                           "north_star-f32"])
def test_rejects_a_dropped_sample(case, dtype):
    """A lost record / atomic / off-by-one at a seam: one sample's attention weight zeroed.  grad_value (one product per
    touched entry, next to few others) must show it every time.  For bf16 the old rule misses some of the same drops."""
    x = inputs(case, dtype)
    bounds, _ = Hp.error_bounds(x, dtype)
    ref = Hp._oracle(x)
    old_missed = 0
    samples = _contributing_samples(x, 24, seed=0)
    for s in samples:
        y = dict(x, attn=x["attn"].clone())
        y["attn"][s] = 0.0
        got = rounded(Hp._oracle(y), dtype)
        res = Hp.bound_ratios(got, x, dtype, outputs=("grad_value",), bounds=bounds)
        assert res["grad_value"][0] > 1.0, (s, res)
        old_missed += old_rule_accepts(got[1], ref[1], dtype)
    if case is LLM:
        assert old_missed > 0, "the old rule caught every drop: the case no longer shows the gap"


def test_rejects_a_contribution_moved_to_the_neighbouring_pixel():
    x = inputs(NORTH_STAR, torch.bfloat16)
    bounds, _ = Hp.error_bounds(x, torch.bfloat16)
    ref = Hp._oracle(x)
    for s in _contributing_samples(x, 6, seed=1):
        only = torch.zeros_like(x["attn"])
        only[s] = x["attn"][s]
        gv_s = msda_oracle.backward(x["value"], x["shapes"], x["start"], x["loc"], only, x["grad"])[0]
        b, _, h = s[0], s[1], s[2]
        pix = np.flatnonzero(np.abs(gv_s[b, :, h]).sum(-1) > 0)
        p = int(pix[np.argmax(np.abs(gv_s[b, pix, h]).sum(-1))])        # the sample's heaviest corner
        shapes, start = x["shapes"].tolist(), x["start"].tolist()
        l = max(i for i in range(len(start)) if start[i] <= p)
        Wl = shapes[l][1]
        nb = p + 1 if (p - start[l]) % Wl < Wl - 1 else p - 1        # its neighbour in the same row of the level
        gv = np.array(ref[1])
        gv[b, nb, h] += gv_s[b, p, h]
        gv[b, p, h] -= gv_s[b, p, h]
        got = rounded([ref[0], gv, ref[2], ref[3]], torch.bfloat16)
        res = Hp.bound_ratios(got, x, torch.bfloat16, outputs=("grad_value",), bounds=bounds)
        assert res["grad_value"][0] > 1.0, (s, res)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_rejects_a_stray_write_into_an_untouched_entry(dtype):
    x = inputs(NORTH_STAR, dtype)
    x["loc"][:, :, :, 0] = x["loc"][:, :, :, 0] * 0.5           # the right half of level 0 is never sampled
    bounds, ref = Hp.error_bounds(x, dtype)
    untouched = np.argwhere(bounds["grad_value"] == 0)
    assert len(untouched) > 0
    gv = np.array(ref["grad_value"])
    gv[tuple(untouched[len(untouched) // 2])] = 2.0 ** -20
    got = [ref["out"], gv, ref["grad_loc"], ref["grad_attn"]]
    res = Hp.bound_ratios(rounded(got, dtype), x, dtype, bounds=bounds)
    assert res["grad_value"][0] == float("inf") and "level 0" in res["grad_value"][1], res
    assert max(r[0] for n, r in res.items() if n != "grad_value") <= 1.0, res


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_rejects_a_dropped_bilinear_corner_in_out(dtype):
    """One corner of one sample left out of the forward's sum (a corner test off by one)."""
    x = inputs(NORTH_STAR, dtype)
    bounds, ref = Hp.error_bounds(x, dtype)
    at, loc = x["attn"].numpy(), x["loc"].numpy()
    shapes, start = x["shapes"].tolist(), x["start"].tolist()
    rejected = 0
    for (b, q, h, l, p) in _contributing_samples(x, 6, seed=2):
        Hl, Wl = shapes[l]
        px, py = loc[b, q, h, l, p, 0] * Wl - 0.5, loc[b, q, h, l, p, 1] * Hl - 0.5
        x0, y0 = int(np.floor(px)), int(np.floor(py))
        fx, fy = px - x0, py - y0
        corners = [(w, yy, xx) for w, yy, xx in (((1 - fy) * (1 - fx), y0, x0), ((1 - fy) * fx, y0, x0 + 1),
                                                 (fy * (1 - fx), y0 + 1, x0), (fy * fx, y0 + 1, x0 + 1))
                   if 0 <= yy < Hl and 0 <= xx < Wl]
        w, yy, xx = max(corners)
        out = np.array(ref["out"]).reshape(at.shape[0], at.shape[1], at.shape[2], -1)
        out[b, q, h] -= at[b, q, h, l, p] * w * x["value"][b, start[l] + yy * Wl + xx, h].numpy()
        got = [out.reshape(ref["out"].shape), ref["grad_value"], ref["grad_loc"], ref["grad_attn"]]
        res = Hp.bound_ratios(rounded(got, dtype), x, dtype, outputs=("out",), bounds=bounds)
        rejected += res["out"][0] > 1.0
    assert rejected == 6


def test_poisoned_allocation_of_an_unwritten_output_breaks_the_bound(monkeypatch):
    """helpers.poison_allocations: under it, an output nobody writes fails assert_within_bounds -- the caching allocator
    can no longer hand a kernel that skips elements the block holding the previous identical call's answer.  The one
    level with H * W == 0 is where that bites: its samples' gradients must be written as exact zeros."""
    x = make_inputs(1, 2, 8, 5, 4, [(4, 4), (0, 3), (2, 2)], seed=2, loc_range=(-0.1, 1.1), dtype=torch.bfloat16)
    ref = [np.asarray(r) for r in Hp._oracle(x)]
    Hp.assert_within_bounds(ref, x, torch.bfloat16, "oracle")
    Hp.poison_allocations(monkeypatch)
    for k, name in enumerate(Hp.OUTPUTS):
        got = list(ref)
        got[k] = torch.empty(np.asarray(ref[k]).shape, dtype=torch.bfloat16).double().numpy()     # never written
        assert np.isnan(got[k]).all()
        with pytest.raises(AssertionError, match=name):
            Hp.assert_within_bounds(got, x, torch.bfloat16, "unwritten")
    # only the empty level's grad_loc / grad_attn left unwritten (what the sorted backward did): caught too
    for k in (2, 3):
        got = list(ref)
        part = torch.from_numpy(np.asarray(ref[k]).copy()).reshape(x["loc"].shape[:5] + ((2,) if k == 2 else ()))
        part[:, :, :, 1] = torch.empty_like(part[:, :, :, 1])
        got[k] = part.numpy()
        with pytest.raises(AssertionError, match="level=1"):
            Hp.assert_within_bounds(got, x, torch.bfloat16, "empty level unwritten")
    # the other types: uint8 workspaces 0xA5, integers a non-zero pattern, bool True
    assert (torch.empty(7, dtype=torch.uint8) == 0xA5).all()
    assert (torch.empty_like(torch.zeros(3, dtype=torch.int32)) == 0x5A5A5A5A).all()
    assert (torch.empty(2, 2, dtype=torch.int64) != 0).all() and torch.empty(3, dtype=torch.bool).all()
    assert torch.isnan(torch.empty(4, requires_grad=True)).all()
