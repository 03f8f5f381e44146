"""Inputs on which every grad_value contribution has one destination, through every route of the op.

Per (b, h, level) the samples sit on DISTINCT pixel centres (loc = (i + 0.5) / extent, exact in 16-bit storage for
power-of-two extents up to 128; the border rows and columns first), the rest wholly outside the map: every touched
grad_value entry is then a single product attn * grad, and a misrouted, dropped or duplicated record shows at its own
element against the per-element bound of tests/helpers.py.  The hot variant adds thousands of samples on one cell of
the largest level (the LLM distribution: overflow queues, cut items), next to which the sparse entries must still meet
their own bounds.  grad_loc sits on its discontinuity at pixel centres and is left out."""
import numpy as np
import pytest
import torch

from helpers import assert_within_bounds, level_tables
from test_op_gpu import run_hip

pytestmark = pytest.mark.gpu

SHAPES = [(16, 32), (8, 8), (1, 16), (4, 1), (2, 2), (1, 1)]       # powers of two, 1-wide and 1-tall levels
B, H, D, P = 2, 4, 128, 4


def exact_scatter_inputs(dtype, Nq, hot, seed=3):
    g = torch.Generator().manual_seed(seed)
    sh, start = level_tables(SHAPES)
    S = int(sh.prod(1).sum())
    loc = torch.full((B, Nq, H, len(SHAPES), P, 2), -1.0, dtype=torch.float64)        # wholly outside by default
    for b in range(B):
        for h in range(H):
            for l, (Hl, Wl) in enumerate(SHAPES):
                ys, xs = torch.meshgrid(torch.arange(Hl), torch.arange(Wl), indexing="ij")
                ys, xs = ys.reshape(-1), xs.reshape(-1)
                border = (ys == 0) | (ys == Hl - 1) | (xs == 0) | (xs == Wl - 1)
                order = torch.cat([torch.nonzero(m).reshape(-1)[torch.randperm(int(m.sum()), generator=g)]
                                   for m in (border, ~border)])
                n = min(len(order), Nq * P)
                slots = torch.randperm(Nq * P, generator=g)[:n]                        # which (q, p) get a pixel
                q, p = slots // P, slots % P
                loc[b, q, h, l, p, 0] = (xs[order[:n]].double() + 0.5) / Wl
                loc[b, q, h, l, p, 1] = (ys[order[:n]].double() + 0.5) / Hl
                if hot and l == 0:                                                     # every other sample of level 0 on one cell
                    rest = torch.ones(Nq * P, dtype=torch.bool)
                    rest[slots] = False
                    q, p = torch.nonzero(rest).reshape(-1) // P, torch.nonzero(rest).reshape(-1) % P
                    loc[b, q, h, l, p, 0] = 5.5 / Wl
                    loc[b, q, h, l, p, 1] = 9.5 / Hl
    rt = lambda t: t.to(dtype).to(torch.float64)
    attn = torch.rand(B, Nq, H, len(SHAPES), P, generator=g) + 1e-5
    attn = attn / attn.sum((-1, -2), keepdim=True)
    x = dict(value=rt(torch.rand(B, S, H, D, generator=g) - 0.3), shapes=sh, start=start, loc=rt(loc), attn=rt(attn),
             grad=rt(torch.randn(B, Nq, H * D, generator=g)))
    assert torch.equal(x["loc"], loc)                      # the centres are exact in the storage type
    return x


ROUTES = {
    # name: (forward formulation, MMFS_* knobs, module attributes, register the table)
    "default":          ("auto", {}, {}, True),
    "fresh_table":      ("auto", {}, {}, False),
    "fwd_gather":       ("gather", {}, {}, True),
    "fwd_lds":          ("lds", {}, {}, True),
    "fwd_slices":       ("slices", {}, {}, True),
    "fwd_waves":        ("waves", {}, {}, True),
    "value_block":      ("auto", {"MMFS_VALUE_ALGO": "block"}, {}, True),
    "value_pixel":      ("auto", {"MMFS_VALUE_ALGO": "pixel"}, {}, True),
    "taps_sorted":      ("auto", {}, {"_taps_prefer_sorted": True}, True),
    "atomic":           ("auto", {}, {"_bwd_algo": "atomic"}, True),
    "hybrid_off":       ("auto", {}, {"_hybrid": False}, True),
    "hybrid_on":        ("auto", {}, {"_hybrid": True}, True),
    "sort_seams":       ("auto", {"MMFS_NT_MIN": "3"}, {}, True),
    "sort_window":      ("auto", {"MMFS_SORT_WINDOW_KB": "21"}, {}, True),
}
SIXTEEN_BIT_ONLY = {"fwd_lds", "fwd_slices", "fwd_waves"}      # the matrix-core forwards take 16-bit storage only
CASES = [(r, d) for r in ROUTES for d in (torch.bfloat16, torch.float16, torch.float32)
         if not (r in SIXTEEN_BIT_ONLY and d == torch.float32)]


@pytest.mark.parametrize("hot", [False, True], ids=["sparse", "hot"])
@pytest.mark.parametrize("route,dtype", CASES, ids=[f"{r}-{str(d)[6:]}" for r, d in CASES])
def test_every_contribution_lands_on_its_own_element(route, dtype, hot, monkeypatch):
    import MultiScaleDeformableAttention as MSDA
    fwd, env, attrs, register = ROUTES[route]
    monkeypatch.setattr(MSDA, "_ws_cache", {})                 # (the workspace's tile bound depends on MMFS_NT_MIN)
    for k in ("MMFS_VALUE_ALGO", "MMFS_NT_MIN", "MMFS_SORT_WINDOW_KB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(MSDA, "_fwd_algo", fwd)
    for k, v in attrs.items():
        monkeypatch.setattr(MSDA, k, v)
    took = MSDA.route_counts["sorted"]
    x = exact_scatter_inputs(dtype, Nq=1500 if hot else 300, hot=hot)
    try:
        got = run_hip(x, dtype, use_autograd=False, register=register)
    finally:
        MSDA._ws_cache.clear()
    if route == "taps_sorted" and dtype != torch.float32:
        assert MSDA.route_counts["sorted"] > took
    touched = np.count_nonzero(np.abs(got[1]).sum(-1))
    assert touched > 0.5 * B * H * int(np.prod(SHAPES, 1).sum())      # (most pixels hold exactly one product)
    res = assert_within_bounds(got, x, dtype, f"{route} {'hot' if hot else 'sparse'}",
                               outputs=("out", "grad_value", "grad_attn"))
    print(f"BOUND {str(dtype)[6:]} scatter {route} {'hot' if hot else 'sparse'}: "
          + " ".join(f"{n}={r[0]:.3g}" for n, r in res.items()))
