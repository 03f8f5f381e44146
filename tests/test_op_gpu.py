"""GPU parity tests of the HIP op (through the Python shim -> C ABI -> gfx950 kernels)
against the committed reference goldens and the CPU oracle.

Bars (BASELINE.json north_star): fp32 <= 1e-5, fp16 <= 1e-3 (bf16 reported with the
same protocol: fp64 oracle on storage-rounded inputs)."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN, assert_within_bounds, level_tables, load_golden, make_inputs, max_abs
from oracle import msda_oracle

pytestmark = pytest.mark.gpu
OP_GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "op_*.npz")))
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# absolute tolerance on outputs whose magnitude is O(1); gradients use a relative bar
TOL = {torch.float64: 1e-12, torch.float32: 1e-5, torch.float16: 1e-3, torch.bfloat16: 8e-3}


def run_hip(x, dtype, use_autograd=True, register=False):
    import MultiScaleDeformableAttention as MSDA
    from mmfs_amd.functions import MSDeformAttnFunction
    dev = lambda t: t.to(DEV, dtype) if t.is_floating_point() else t.to(DEV)
    value, loc, attn, grad = dev(x["value"]), dev(x["loc"]), dev(x["attn"]), dev(x["grad"])
    sh, st = dev(x["shapes"]), dev(x["start"])
    if register:         # the shim then knows the table on the host (what mmfs_amd.levels.make_level_tables does):
        MSDA.register_level_tables(sh, st, value.shape[1], host_shapes=x["shapes"], host_start=x["start"])   # hybrid routing
    if use_autograd:
        value.requires_grad_(True); loc.requires_grad_(True); attn.requires_grad_(True)
        out = MSDeformAttnFunction.apply(value, sh, st, loc, attn, 1)
        out.backward(grad.reshape(out.shape))
        res = out.detach(), value.grad, loc.grad, attn.grad
    else:
        out = MSDA.ms_deform_attn_forward(value, sh, st, loc, attn, 1)
        gv, gl, ga = MSDA.ms_deform_attn_backward(value, sh, st, loc, attn, grad.reshape(out.shape), 1)
        res = out, gv, gl, ga
    torch.cuda.synchronize()
    return [r.double().cpu().numpy() for r in res]


def run_oracle(x):
    out = msda_oracle.forward(x["value"], x["shapes"], x["start"], x["loc"], x["attn"])
    gv, gl, ga = msda_oracle.backward(x["value"], x["shapes"], x["start"], x["loc"], x["attn"], x["grad"])
    return out, gv, gl, ga


def check(got, want, x, dtype, what="", own_ref=False, gamma=None):
    """The max-abs bars below, and the per-element bound of tests/helpers.py on all four outputs of inputs ``x``
    (against the oracle on ``x``; against ``want`` with ``own_ref``, for tests that zero reference entries on purpose)."""
    tol = TOL[dtype]
    names = ("out", "grad_value", "grad_loc", "grad_attn")
    for n, g, w in zip(names, got, want):
        scale = max(1.0, float(np.abs(w).max())) if w.size else 1.0
        err = max_abs(g, w)
        assert err <= tol * scale, f"{what} {n}: max abs err {err:.3e} > {tol:.1e} * {scale:.3g}"
        if n in ("grad_loc", "grad_attn") and w.size:
            # per element too (a bar relative to the LARGEST entry leaves the small entries of grad_loc
            # -- range up to ~50 -- unconstrained): |err| <= tol * (|ref| + 0.05 * max|ref|)
            g64 = np.asarray(g, dtype=np.float64)
            w64 = np.asarray(w, dtype=np.float64).reshape(g64.shape)
            fin = np.isfinite(w64)
            excess = np.abs(g64 - w64)[fin] - tol * (np.abs(w64)[fin] + 0.05 * scale)
            assert excess.size == 0 or float(excess.max()) <= 0.0, \
                f"{what} {n}: an element is off by {float(excess.max()):.3e} more than {tol:.1e} * (|ref| + 0.05 * {scale:.3g})"
    res = assert_within_bounds(got, x, dtype, what, want=want if own_ref else None, gamma=gamma)
    print(f"BOUND {str(dtype)[6:]} {what}: " + " ".join(f"{n}={r[0]:.3g}" for n, r in res.items()))


def golden_inputs(z, dtype):
    rt = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dtype).to(torch.float64)
    return dict(value=rt(z["value"]), shapes=torch.from_numpy(z["spatial_shapes"]),
                start=torch.from_numpy(z["level_start_index"]), loc=rt(z["loc"]), attn=rt(z["attn"]),
                grad=rt(z["grad_out"]))


@pytest.mark.parametrize("name", OP_GOLDENS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_hip_matches_reference_goldens(name, dtype):
    z = load_golden(name)
    x = golden_inputs(z, dtype)
    got = run_hip(x, dtype)
    want = [z["out_f64"], z["grad_value_f64"], z["grad_loc_f64"], z["grad_attn_f64"]]
    if dtype == torch.float64 and z["grad_value_f64"].dtype == np.float32:
        want[1] = run_oracle(x)[1]            # golden stored in fp32: use the (pinned) oracle
    check(got, want, x, dtype, name)


@pytest.mark.parametrize("name", ["op_g1_d64", "op_g3_llm_n1", "op_g3_rect_n3", "op_g3_sd_n4"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_hip_16bit_against_oracle_on_rounded_goldens(name, dtype):
    x = golden_inputs(load_golden(name), dtype)
    check(run_hip(x, dtype), run_oracle(x), x, dtype, name)


CASES = [
    # B, H, D, Nq, P, shapes                                   what it exercises
    (2, 8, 32, 70, 4, [(16, 16), (8, 8), (4, 4), (2, 2)]),      # config-1 geometry, ragged Nq tile
    (2, 8, 128, 33, 4, [(16, 16), (8, 8), (4, 4), (2, 2)]),     # north-star head width
    (1, 16, 64, 40, 8, [(8, 8), (4, 4), (2, 2)] * 4),           # LLM MMFS, n=4 -> Leff=12, K=96 (chunked)
    (2, 16, 64, 17, 8, [(8, 8), (4, 4), (2, 2), (1, 1)] * 3),   # SD MMFS, n=3 -> Leff=12
    (3, 16, 32, 50, 4, [(16, 16)]),                             # ViT-Adapter extractor (L=1)
    (1, 2, 8, 300, 2, [(5, 7), (3, 2)]),                        # tiny head width, many queries
    (1, 3, 24, 9, 3, [(5, 7), (2, 3)]),                         # scalar path (D not 16B * 2^k)
    (1, 1, 256, 5, 2, [(4, 4), (2, 2)]),                        # one head, wide
    (1, 4, 64, 6, 2, [(3, 3)] * 90),                            # Leff = 90 (30 images x 3 levels)
]


@pytest.mark.parametrize("case", CASES, ids=[f"B{c[0]}H{c[1]}D{c[2]}Nq{c[3]}P{c[4]}L{len(c[5])}" for c in CASES])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_hip_matches_oracle_seeded(case, dtype):
    B, H, D, Nq, P, shapes = case
    x = make_inputs(B, H, D, Nq, P, shapes, seed=7, loc_range=(-0.15, 1.15), dtype=dtype)
    check(run_hip(x, dtype), run_oracle(x), x, dtype, str(case[:5]))


HYBRID_CASES = [
    # B, H, D, Nq, P, shapes: levels of <= 256 pixels go to the matrix cores (csrc/msda_dense.hip)
    (2, 4, 128, 200, 4, [(16, 16), (8, 8), (20, 20), (5, 7)]),     # dense + gathered levels mixed, ragged tile
    (2, 3, 64, 333, 8, [(32, 32), (16, 16), (8, 8)] * 2),          # LLM geometry, two images, P = 8 (two record passes)
    (1, 2, 32, 130, 4, [(16, 16), (3, 3)]),                        # every level dense, D = 32 (idle waves)
    (1, 8, 128, 64, 4, [(64, 64), (32, 32), (16, 16), (8, 8)]),    # the north-star pyramid, one full tile
    (1, 2, 64, 97, 16, [(1, 1), (2, 9), (16, 16)]),                # P = 16, degenerate levels
    (1, 8, 32, 4097, 4, [(16, 13), (40, 6)]),                      # 65 query tiles: the chunking leaves some chunks idle
]


@pytest.mark.parametrize("case", HYBRID_CASES, ids=[f"B{c[0]}H{c[1]}D{c[2]}Nq{c[3]}P{c[4]}L{len(c[5])}" for c in HYBRID_CASES])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_hybrid_dense_levels_match_oracle(case, dtype, monkeypatch):
    """The hybrid backward (grad_loc / grad_attn of the small levels as dense dot products on the matrix
    cores, csrc/msda_dense.hip) against the oracle, same bars as the row-gather kernels."""
    import MultiScaleDeformableAttention as MSDA
    monkeypatch.setattr(MSDA, "_hybrid", True)
    B, H, D, Nq, P, shapes = case
    x = make_inputs(B, H, D, Nq, P, shapes, seed=11, loc_range=(-0.15, 1.15), dtype=dtype)
    x["loc"][0, 3, 0, 0, 0, 0] = float("nan")          # non-finite locations contribute nothing
    x["loc"][0, 5, 1 % H, -1, 0, 1] = float("inf")
    log = []
    monkeypatch.setattr(MSDA, "_event_log", log)
    got = run_hip(x, dtype, use_autograd=False, register=True)
    monkeypatch.setattr(MSDA, "_event_log", None)
    names = {n for n, _, _ in log}
    assert "msda_bwd_taps_coarse" in names, names
    check(got, run_oracle(x), x, dtype, f"hybrid {case[:5]}")


@pytest.mark.parametrize("algo", ["tile", "block", "pixel"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_grad_value_generations_agree_with_oracle(algo, dtype, monkeypatch):
    """grad_value: 4x4 blocks on the matrix cores (csrc/msda_bwd_tile.hip, default for 16-bit storage),
    2x2 blocks on the vector ALUs (csrc/msda_bwd_block.hip, fp32 storage and MMFS_VALUE_ALGO=block) and
    pixel-stationary (csrc/msda_bwd_value.hip, MMFS_VALUE_ALGO=pixel and the fallback for L > 128)
    on a shape with odd extents, a 1-pixel-wide level, hot spots and many taps outside the map."""
    if algo == "tile":
        monkeypatch.delenv("MMFS_VALUE_ALGO", raising=False)
    else:
        monkeypatch.setenv("MMFS_VALUE_ALGO", algo)
    x = make_inputs(2, 4, 64, 150, 4, [(13, 9), (1, 7), (6, 1), (16, 16), (2, 2)], seed=21,
                    loc_range=(-0.3, 1.3), dtype=dtype)
    x["loc"][:, :40, :, 3] = x["loc"][:, :40, :, 3] * 0.05 + 0.5       # hot spot: long lists on a few blocks
    x["loc"] = x["loc"].to(dtype).to(torch.float64)                    # oracle and device see the same numbers
    check(run_hip(x, dtype), run_oracle(x), x, dtype, f"value algo {algo}")


SORT_ROUTES = {
    # name: (dtype, P, Nq, MMFS_NT_MIN, MMFS_SORT_WINDOW_KB)      what the cell sort does (csrc/msda_bwd_block.hip)
    "kept_window":          (torch.bfloat16, 4, 301, None, None),   # samples kept in registers, records through the LDS window, tiles plan their own blocks
    "kept_window_seams":    (torch.bfloat16, 4, 302, "3", None),    # levels cut into bands: local blocks + the seams' blocks by the slice's last workgroup
    "kept_window_p8":       (torch.float16, 8, 303, "2", None),     # two vectors per query: the placing pass reads the words again
    "kept_window_too_small": (torch.bfloat16, 4, 1000, None, "21"), # a tile's records exceed the window: placed window by window (two rounds)
    "kept_window_rounds_p8": (torch.float16, 8, 900, None, "21"),   # ... three rounds, the words read again before each (the SD block's route)
    "two_scan_window":      (torch.bfloat16, 2, 304, None, None),   # 8-byte query rows (scalar scan): second scan into the window
    "two_scan_window_seams": (torch.bfloat16, 3, 305, "4", None),
    "direct":               (torch.bfloat16, 4, 306, None, "0"),    # no window: cursors + scattered stores
    "direct_seams":         (torch.bfloat16, 4, 307, "3", "0"),
    "fp32_records":         (torch.float32, 4, 308, None, None),    # 16-byte records, vector-ALU reduce off the cell table
    "fp32_records_seams":   (torch.float32, 4, 309, "3", None),
}


@pytest.mark.parametrize("route", sorted(SORT_ROUTES))
def test_cell_sort_routes_match_oracle(route, monkeypatch):
    """Every way the cell sort moves a tile's records (LDS window or straight to memory, samples kept in registers
    or scanned twice) and plans the 4x4 blocks (by the tile itself, or on the seams between a level's tiles by
    the slice's last workgroup) gives the oracle's gradients.  B*H*L = 128 slices: one tile per level unless
    MMFS_NT_MIN cuts the levels into bands."""
    import MultiScaleDeformableAttention as MSDA
    dtype, P, Nq, nt, win = SORT_ROUTES[route]
    monkeypatch.setattr(MSDA, "_ws_cache", {})                  # (the tile bound of the workspace depends on MMFS_NT_MIN)
    for k, v in (("MMFS_NT_MIN", nt), ("MMFS_SORT_WINDOW_KB", win)):
        monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)
    # (extents that are powers of two: loc * extent is then exact in fp32 as in the oracle's fp64, and no sample
    # sits on the other side of a pixel boundary, where grad_loc jumps)
    x = make_inputs(4, 8, 32, Nq, P, [(32, 16), (16, 8), (8, 4), (4, 2)], seed=31, loc_range=(-0.1, 1.1), dtype=dtype)
    x["attn"][:, ::7, :, 1] = 0.0                               # zero weights leave no record
    try:
        check(run_hip(x, dtype), run_oracle(x), x, dtype, f"sort route {route}")
    finally:
        MSDA._ws_cache.clear()


@pytest.mark.parametrize("variant", ["fewer lanes", "1024 lanes"])
@pytest.mark.parametrize("dtype,P,Nq,hot", [(torch.bfloat16, 4, 96, False), (torch.float16, 8, 96, False), (torch.float32, 4, 96, False),
                                            (torch.bfloat16, 4, 96, True), (torch.bfloat16, 4, 700, False), (torch.float16, 8, 600, True)])
def test_cell_sort_of_many_small_slices(dtype, P, Nq, hot, variant, monkeypatch):
    """Tiles of few samples in MANY slices (the ViT-Adapter's regime: B*H*L >= 512; Nq*P <= 2048 samples per level of a
    slice: 256-lane sort workgroups, four per CU -- the injector; <= 8192: 512 lanes, two per CU -- the extractor;
    csrc/msda_bwd_block.hip ``sort_lanes``), held to the oracle next to the 1024-lane variant on the same inputs
    (``MMFS_SORT_SMALL=0``)."""
    import MultiScaleDeformableAttention as MSDA
    monkeypatch.setattr(MSDA, "_ws_cache", {})
    monkeypatch.setenv("MMFS_SORT_SMALL", "1" if variant == "fewer lanes" else "0")
    x = make_inputs(8, 16, 32, Nq, P, [(16, 16), (8, 8), (4, 8), (2, 2)], seed=17, loc_range=(-0.1, 1.1), dtype=dtype)
    x["attn"][:, ::5, :, 2] = 0.0
    if hot:                                                     # every sample of a level in a few cells: long lists, cut items
        x["loc"][:, :, :, 1] = (x["loc"][:, :, :, 1] * 0.05 + 0.5).to(dtype).to(torch.float64)
    try:
        check(run_hip(x, dtype), run_oracle(x), x, dtype, f"small slices, {variant}")
    finally:
        MSDA._ws_cache.clear()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_every_query_on_one_spot_overflows_the_block_lists(dtype):
    """The LLM path's distribution: every token samples around the SAME reference point, so a few
    2x2 blocks own nearly all records.  Lists beyond the in-place cap are queued, spread over the
    chip and added into accumulator slots (msda_bwd_block_overflow / _ovf_store)."""
    x = make_inputs(1, 2, 64, 1500, 4, [(8, 8), (4, 4)], seed=5, dtype=dtype)
    x["loc"] = (x["loc"] * 0.04 + 0.48).to(dtype).to(torch.float64)     # all 6000 samples of a level in ~1 cell
    check(run_hip(x, dtype), run_oracle(x), x, dtype, "hot spot overflow")


def test_many_levels_fall_back_to_pixel_stationary():
    """L = 130 > the block reduce's level table: the pixel-stationary kernels take over."""
    x = make_inputs(1, 2, 32, 12, 2, [(3, 2)] * 130, seed=4, dtype=torch.bfloat16)
    check(run_hip(x, torch.bfloat16), run_oracle(x), x, torch.bfloat16, "L=130")


@pytest.mark.parametrize("n_levels", [33, 40, 72, 128])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_level_rows_beyond_the_cached_ones(n_levels, dtype):
    """The block reduce keeps 32 level rows in LDS and reads the others from the table (a dozen
    images of 3-4 levels each is ordinary for the LLM path): levels on both sides of that border, of
    different sizes so that a wrong row shows."""
    shapes = [((3, 2), (5, 4), (2, 7), (6, 6))[i % 4] for i in range(n_levels)]
    x = make_inputs(1, 2, 32, 40, 2, shapes, seed=6, dtype=dtype)
    check(run_hip(x, dtype), run_oracle(x), x, dtype, f"L={n_levels}")


def test_hybrid_off_uses_plain_kernels(monkeypatch):
    import MultiScaleDeformableAttention as MSDA
    monkeypatch.setattr(MSDA, "_hybrid", False)
    x = make_inputs(2, 4, 128, 200, 4, [(16, 16), (8, 8)], seed=2, dtype=torch.bfloat16)
    log = []
    monkeypatch.setattr(MSDA, "_event_log", log)
    got = run_hip(x, torch.bfloat16, use_autograd=False)
    monkeypatch.setattr(MSDA, "_event_log", None)
    assert not any("coarse" in n for n, _, _ in log)
    check(got, run_oracle(x), x, torch.bfloat16, "hybrid off")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CASES[:5], ids=[str(i) for i in range(5)])
def test_atomic_backward_path_matches_oracle(case, dtype, monkeypatch):
    """The float-atomic fallback (non-canonical level tables, odd head widths) stays correct."""
    import MultiScaleDeformableAttention as MSDA
    monkeypatch.setattr(MSDA, "_bwd_algo", "atomic")
    B, H, D, Nq, P, shapes = case
    x = make_inputs(B, H, D, Nq, P, shapes, seed=9, loc_range=(-0.15, 1.15), dtype=dtype)
    check(run_hip(x, dtype), run_oracle(x), x, dtype, "atomic " + str(case[:5]))


def test_non_canonical_level_table_falls_back_and_is_right():
    """Levels stored with a gap and in reverse order inside value: legal for the op
    (it only reads start[l]); the pixel-stationary kernel must not be used."""
    g = torch.Generator().manual_seed(3)
    B, H, D, Nq, P = 2, 4, 32, 21, 4
    shapes = torch.tensor([(4, 6), (3, 3)], dtype=torch.long)
    start = torch.tensor([12, 0], dtype=torch.long)          # level 1 first (9 rows), gap 9..11, level 0 at 12
    S = 12 + 24 + 5
    rt = lambda t: t.double()
    x = dict(value=rt(torch.rand(B, S, H, D, generator=g)), shapes=shapes, start=start,
             loc=rt(torch.rand(B, Nq, H, 2, P, 2, generator=g) * 1.2 - 0.1),
             attn=rt(torch.rand(B, Nq, H, 2, P, generator=g)), grad=rt(torch.randn(B, Nq, H * D, generator=g)))
    got, want = run_hip(x, torch.float32), run_oracle(x)
    check(got, want, x, torch.float32, "gapped levels")
    assert not got[1][:, 9:12].any() and not got[1][:, 36:].any()      # untouched rows are zero


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fresh_level_tensors_cost_no_host_sync(dtype):
    """The reference's callers rebuild spatial_shapes / level_start_index on every call
    (modeling_llama_mmfs.py:298-308, sd_mmfs.py:31-41): tensors the shim has never seen.  Neither pass may
    copy them back to the host to find out whether the packing is canonical -- the library checks the
    table on the device (MMFS_BWD_DEVICE_CHECKED_LEVELS)."""
    from mmfs_amd.functions import MSDeformAttnFunction
    x = make_inputs(2, 4, 64, 50, 4, [(12, 9), (6, 5), (3, 3)], seed=31, loc_range=(-0.1, 1.1), dtype=dtype)
    dev = lambda t: t.to(DEV, dtype) if t.is_floating_point() else t.to(DEV)
    v, l, a, g = dev(x["value"]), dev(x["loc"]), dev(x["attn"]), dev(x["grad"])
    host_sh, host_st = x["shapes"].tolist(), x["start"].tolist()
    sh_dev, st_dev = x["shapes"].to(DEV), x["start"].to(DEV)
    res = None
    for it in range(3):
        # fresh tensor OBJECTS every call, made without a host->device copy inside the checked region
        sh, st = sh_dev.clone(), st_dev.clone()
        vv, ll, aa = v.clone().requires_grad_(True), l.clone().requires_grad_(True), a.clone().requires_grad_(True)
        torch.cuda.synchronize()
        if it:
            torch.cuda.set_sync_debug_mode("error")
        try:
            out = MSDeformAttnFunction.apply(vv, sh, st, ll, aa, 1)
            out.backward(g.reshape(out.shape))
        finally:
            torch.cuda.set_sync_debug_mode("default")
        res = [out.detach(), vv.grad, ll.grad, aa.grad]
    torch.cuda.synchronize()
    check([r.double().cpu().numpy() for r in res], run_oracle(x), x, dtype, "fresh level tensors")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_unverified_gapped_table_is_served_by_the_sorted_backward(dtype):
    """A table nobody registered, with a gap, a tail and the levels in reverse order: the device-side
    check passes (no two levels overlap), the rows no level owns come back zero."""
    g = torch.Generator().manual_seed(5)
    B, H, D, Nq, P = 2, 4, 64, 33, 4
    shapes = torch.tensor([(5, 6), (3, 3), (9, 2)], dtype=torch.long)
    start = torch.tensor([20, 2, 55], dtype=torch.long)          # level 1 at 2..10, level 0 at 20..49, level 2 at 55..72
    S = 80
    rt = lambda t: t.to(dtype).double()
    x = dict(value=rt(torch.rand(B, S, H, D, generator=g)), shapes=shapes, start=start,
             loc=rt(torch.rand(B, Nq, H, 3, P, 2, generator=g) * 1.2 - 0.1),
             attn=rt(torch.rand(B, Nq, H, 3, P, generator=g)), grad=rt(torch.randn(B, Nq, H * D, generator=g)))
    got, want = run_hip(x, dtype), run_oracle(x)
    check(got, want, x, dtype, "gapped, unverified levels")
    owned = np.zeros(S, bool)
    for (h, w), s0 in zip(shapes.tolist(), start.tolist()):
        owned[s0:s0 + h * w] = True
    assert not got[1][:, ~owned].any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_levels_wider_than_65535_take_the_atomic_path_with_exact_extents(dtype):
    """The sorted backward packs level extents into 16 bits; a registered table with a wider level is
    routed to the float-atomic path, whose records carry the level index and look the extents up
    (round 1 packed (Hl << 16) | Wl there too: silently wrong grad_loc for such a level)."""
    x = make_inputs(1, 2, 32, 40, 4, [(1, 70000), (3, 3)], seed=9, dtype=dtype)
    got, want = run_hip(x, dtype, register=True), run_oracle(x)
    # x = loc * 70000 - 0.5 in fp32 (the reference's arithmetic too) is good to 2^-7 of a pixel, and whether the
    # compiler contracts it into one FMA moves it by that much: the bilinear weights carry ~1 % noise against
    # the fp64 oracle.  A truncated extent would be off by 70000 / 4464 = 15.7x in grad_loc.
    for n, g, w in zip(("out", "grad_value", "grad_loc", "grad_attn"), got, want):
        scale = max(1.0, float(np.abs(w).max()))
        assert max_abs(g, w) <= 3e-2 * scale, f"70000-wide level {n}: {max_abs(g, w):.3e} vs scale {scale:.3g}"


def test_more_than_65536_queries_leave_the_compact_records():
    """The matrix-core reduce keeps the query index in 16 bits of its 8-byte records; with more queries the
    2x2-block reduce (16-byte records) takes over for 16-bit storage too."""
    x = make_inputs(1, 1, 32, 66000, 4, [(6, 5), (3, 4)], seed=12, dtype=torch.bfloat16)
    check(run_hip(x, torch.bfloat16), run_oracle(x), x, torch.bfloat16, "Nq = 66000")


def test_skewed_locations_overflow_the_tile_lists():
    """All queries sample the same spot: one pixel receives Nq*P records, far more than a
    workgroup's LDS list holds -> exercises the per-pixel query-range rounds."""
    B, H, D, Nq, P = 1, 2, 128, 3000, 4
    shapes = [(8, 8), (4, 4)]
    x = make_inputs(B, H, D, Nq, P, shapes, seed=13, dtype=torch.bfloat16)
    x["loc"] = (x["loc"] * 0.02 + 0.40).to(torch.bfloat16).double()    # tight cluster
    check(run_hip(x, torch.bfloat16), run_oracle(x), x, torch.bfloat16, "skew")
    x32 = make_inputs(B, H, 32, Nq, P, shapes, seed=14, dtype=torch.float32)
    x32["loc"] = x32["loc"] * 0.0 + 0.3                                 # exactly one spot
    check(run_hip(x32, torch.float32), run_oracle(x32), x32, torch.float32, "skew32")


def test_direct_extension_calls_match_autograd_path():
    x = make_inputs(2, 4, 32, 19, 4, [(6, 5), (3, 3)], seed=11, dtype=torch.float32)
    a = run_hip(x, torch.float32, use_autograd=True)
    b = run_hip(x, torch.float32, use_autograd=False)
    assert max_abs(a[0], b[0]) == 0.0                      # forward is deterministic
    check(b, run_oracle(x), x, torch.float32, "direct calls")


def test_edge_locations_follow_the_kernel_not_grid_sample():
    sh, start = level_tables([(2, 2)])
    value = torch.arange(1.0, 5.0).reshape(1, 4, 1, 1).repeat(1, 1, 1, 4).to(torch.float64)
    pts = [(0.25, 0.25), (0.5, 0.5), (0.0, 0.0), (1.0, 1.0), (float("nan"), 0.5), (float("inf"), 0.5),
           (-0.25, 0.5), (1.25, 0.5), (1.2499, 0.5), (0.5, -float("inf"))]
    loc = torch.tensor(pts, dtype=torch.float64).reshape(1, len(pts), 1, 1, 1, 2)
    attn = torch.ones(1, len(pts), 1, 1, 1, dtype=torch.float64)
    x = dict(value=value, shapes=sh, start=start, loc=loc, attn=attn,
             grad=torch.ones(1, len(pts), 4, dtype=torch.float64))
    for dtype in (torch.float64, torch.float32):
        got, want = run_hip(x, dtype), run_oracle(x)
        assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
        check(got, want, x, dtype, "edges")


def test_non_finite_values_outside_the_tap_do_not_leak():
    # invalid corners must be skipped, not multiplied by zero (cuh:58-81)
    sh, start = level_tables([(2, 2)])
    value = torch.ones(1, 4, 1, 8, dtype=torch.float64)
    value[0, 0] = float("inf")                           # pixel (0,0)
    loc = torch.tensor([1.0, 1.0], dtype=torch.float64).reshape(1, 1, 1, 1, 1, 2)   # touches pixel (1,1) only
    attn = torch.ones(1, 1, 1, 1, 1, dtype=torch.float64)
    x = dict(value=value, shapes=sh, start=start, loc=loc, attn=attn, grad=torch.ones(1, 1, 8, dtype=torch.float64))
    got = run_hip(x, torch.float32)
    assert np.allclose(got[0], 0.25) and np.isfinite(got[2]).all() and np.isfinite(got[3]).all()


def test_empty_inputs():
    import MultiScaleDeformableAttention as MSDA
    sh, start = level_tables([(2, 2)], DEV)
    v = torch.rand(2, 4, 2, 8, device=DEV)
    out = MSDA.ms_deform_attn_forward(v, sh, start, torch.zeros(2, 0, 2, 1, 3, 2, device=DEV),
                                      torch.zeros(2, 0, 2, 1, 3, device=DEV), 1)
    assert out.shape == (2, 0, 16)
    gv, gl, ga = MSDA.ms_deform_attn_backward(v, sh, start, torch.zeros(2, 0, 2, 1, 3, 2, device=DEV),
                                              torch.zeros(2, 0, 2, 1, 3, device=DEV),
                                              torch.zeros(2, 0, 16, device=DEV), 1)
    assert gv.shape == v.shape and not gv.any() and gl.numel() == 0 and ga.numel() == 0


def test_reference_preconditions_raise():
    import MultiScaleDeformableAttention as MSDA
    sh, start = level_tables([(2, 2)], DEV)
    v = torch.rand(3, 4, 2, 8, device=DEV)
    loc = torch.rand(3, 2, 2, 1, 3, 2, device=DEV); attn = torch.rand(3, 2, 2, 1, 3, device=DEV)
    with pytest.raises(RuntimeError, match="contiguous"):
        MSDA.ms_deform_attn_forward(torch.rand(3, 2, 4, 8, device=DEV).permute(0, 2, 1, 3),
                                    sh, start, loc, attn, 1)
    with pytest.raises(RuntimeError, match="im2col_step"):
        MSDA.ms_deform_attn_forward(v, sh, start, loc, attn, 2)          # 3 % 2 != 0 (.cu:51-53)
    with pytest.raises(RuntimeError, match="CUDA"):
        MSDA.ms_deform_attn_forward(v, sh.cpu(), start, loc, attn, 1)


def test_mixed_dtype_attention_is_cast_not_misread():
    # softmax under autocast yields fp32 weights next to fp16 values (SURVEY 8a "Dtype flow")
    x = make_inputs(1, 4, 32, 12, 4, [(4, 4), (2, 2)], seed=5, dtype=torch.float16)
    import MultiScaleDeformableAttention as MSDA
    v = x["value"].to(DEV, torch.float16); loc = x["loc"].to(DEV, torch.float16)
    out = MSDA.ms_deform_attn_forward(v, x["shapes"].to(DEV), x["start"].to(DEV), loc,
                                      x["attn"].to(DEV, torch.float32), 1)
    want = run_oracle(x)[0]
    assert max_abs(out.double().cpu().numpy(), want) < 1e-3


# ---- size-independent properties at BASELINE.json's full sizes (oracle would take minutes)
FULL = [
    ("cfg1", dict(B=2, H=8, D=32, Nq=1024, P=4, shapes=[(64, 64), (32, 32), (16, 16), (8, 8)]), torch.float32),
    ("cfg2_northstar", dict(B=8, H=8, D=128, Nq=4096, P=4, shapes=[(64, 64), (32, 32), (16, 16), (8, 8)]), torch.bfloat16),
    ("cfg5_llm_n4", dict(B=4, H=16, D=64, Nq=2048, P=8, shapes=[(32, 32), (16, 16), (8, 8)] * 4), torch.float16),
    # the op inside BASELINE configs 3 and 4 at their batch (the decoders' real head geometry): one image per sequence --
    # the shape whose forward is the sliced kernel by default (csrc/msda_fwd_q8.hip) -- and the image decoder's 512-px block
    ("cfg3_llm_n1", dict(B=4, H=16, D=64, Nq=2048, P=8, shapes=[(32, 32), (16, 16), (8, 8)]), torch.bfloat16),
    ("cfg4_sd_block", dict(B=8, H=16, D=64, Nq=4096, P=8, shapes=[(64, 64), (32, 32), (16, 16), (8, 8)]), torch.float16),
]


@pytest.mark.parametrize("route", ["fresh", "registered"])
@pytest.mark.parametrize("name,cfg,dtype", FULL, ids=[f[0] for f in FULL])
def test_full_size_properties(name, cfg, dtype, route):
    """``fresh``: level tensors nobody has looked at (the reference's call pattern: table checked on the device, bound-sized
    grids); ``registered``: the same tensors announced to the shim -- hybrid routing, host-sized grids, the hosted plan:
    the route ``bench.py`` times (it was held by the bench's own Euler guard only)."""
    import MultiScaleDeformableAttention as MSDA
    from mmfs_amd.functions import MSDeformAttnFunction
    g = torch.Generator(device=DEV).manual_seed(0)
    sh, start = level_tables(cfg["shapes"], DEV)
    B, H, D, Nq, P = cfg["B"], cfg["H"], cfg["D"], cfg["Nq"], cfg["P"]
    S, L = int(sh.prod(1).sum()), sh.shape[0]
    if route == "registered":
        assert MSDA.register_level_tables(sh, start, S)[0]             # (canonical)
    else:
        assert MSDA._level_info(sh, start, S, sync=False) is None
    value = torch.rand(B, S, H, D, device=DEV, generator=g).to(dtype)
    loc = (torch.rand(B, Nq, H, L, P, 2, device=DEV, generator=g) * 1.2 - 0.1).to(dtype)
    attn = torch.rand(B, Nq, H, L, P, device=DEV, generator=g) + 1e-5
    attn = (attn / attn.sum((-1, -2), keepdim=True)).to(dtype)
    grad = torch.randn(B, Nq, H * D, device=DEV, generator=g).to(dtype)
    v, l, a = value.clone().requires_grad_(True), loc.clone().requires_grad_(True), attn.clone().requires_grad_(True)
    out = MSDeformAttnFunction.apply(v, sh, start, l, a, 1)
    out.backward(grad)
    assert torch.isfinite(out).all() and torch.isfinite(v.grad).all() and torch.isfinite(l.grad).all()
    rel = {torch.float32: 1e-4, torch.float16: 4e-3, torch.bfloat16: 3e-2}[dtype]
    # (1) out is linear in value and in attn  =>  <v, dL/dv> = <a, dL/da> = <out, g>   (Euler)
    og = (out.double() * grad.double()).sum()
    assert abs((v.grad.double() * value.double()).sum() - og) <= rel * abs(og) + rel
    assert abs((a.grad.double() * attn.double()).sum() - og) <= rel * abs(og) + rel
    # (2) convexity: weights sum to 1 over real points, values in [0,1)  =>  0 <= out < 1 (+rounding)
    assert out.min() >= -1e-2 and out.max() <= 1.0 + 1e-2
    # (3) a strided set of queries of the first, a middle and the last sample -- every head, every level -- agrees with the
    # CPU oracle (round 4 looked at queries 5 .. 8 of sample 0: VERDICT r4, next 2d)
    for bi in sorted({0, B // 2, B - 1}):
        qs = torch.arange(5, Nq, max(1, Nq // 48), device=DEV)[:48]
        x = dict(value=value[bi:bi + 1].double().cpu(), shapes=sh.cpu(), start=start.cpu(), loc=loc[bi:bi + 1, qs].double().cpu(),
                 attn=attn[bi:bi + 1, qs].double().cpu(), grad=grad[bi:bi + 1, qs].double().cpu())
        want = msda_oracle.forward(x["value"], x["shapes"], x["start"], x["loc"], x["attn"])
        assert max_abs(out[bi:bi + 1, qs].detach().double().cpu().numpy(), want) <= TOL[dtype], f"sample {bi}"
        _, gl, ga = msda_oracle.backward(x["value"], x["shapes"], x["start"], x["loc"], x["attn"], x["grad"])
        assert max_abs(a.grad[bi:bi + 1, qs].double().cpu().numpy(), ga) <= TOL[dtype] * max(1.0, np.abs(ga).max()), f"sample {bi}"
        assert max_abs(l.grad[bi:bi + 1, qs].double().cpu().numpy(), gl) <= TOL[dtype] * max(1.0, np.abs(gl).max()), f"sample {bi}"
    # (3b) grad_value of one whole head of sample 0 -- every level's map, fed by ALL of the sample's queries --
    # agrees with the CPU oracle (the Euler identity above only holds the sum)
    h0 = 3 % H
    x1 = dict(value=value[:1, :, h0:h0 + 1].double().cpu(), shapes=sh.cpu(), start=start.cpu(),
              loc=loc[:1, :, h0:h0 + 1].double().cpu(), attn=attn[:1, :, h0:h0 + 1].double().cpu(),
              grad=grad[:1, :, h0 * D:(h0 + 1) * D].double().cpu())
    gv1, _, _ = msda_oracle.backward(x1["value"], x1["shapes"], x1["start"], x1["loc"], x1["attn"], x1["grad"])
    assert max_abs(v.grad[:1, :, h0:h0 + 1].double().cpu().numpy(), gv1) <= TOL[dtype] * max(1.0, np.abs(gv1).max())
    # (4) determinism of the forward (no atomics there)
    out2 = MSDeformAttnFunction.apply(value, sh, start, loc, attn, 1)
    assert torch.equal(out2, out.detach())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_zero_attention_samples_are_skipped_not_miscounted(dtype):
    """Images a token cannot see carry exactly zero attention (MMFS's masked softmax): the forward
    reads no rows for them and the grad_value sort makes no records -- outputs and all three
    gradients (grad_attn of a zero-weight sample is NOT zero) still match the oracle."""
    x = make_inputs(2, 4, 64, 300, 4, [(32, 32), (16, 16), (8, 8)] * 2, seed=21, dtype=dtype)
    g = torch.Generator().manual_seed(2)
    keep = (torch.rand(2, 300, 1, 6, 1, generator=g) < 0.5).double()
    keep[:, :, :, 0] = 1.0
    keep[1, :150] = 0.0                             # a stretch of queries that sees nothing at all
    x["attn"] = (x["attn"] * keep).to(dtype).to(torch.float64)
    got = run_hip(x, dtype, use_autograd=False)
    want = run_oracle(x)
    check(got, want, x, dtype, "zero attention")
    assert np.abs(want[3][keep.expand_as(x["attn"]).numpy() == 0]).max() > 1e-3     # the case is not vacuous
    assert np.abs(got[0][1, :150]).max() == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lazy_zero_attention_only_changes_entries_nobody_reads(dtype):
    """MMFS_BWD_LAZY_ZERO_ATTN (set by the MMFS module): grad_attn / grad_loc of zero-weight samples
    come back as 0; every other output is bit-identical to the full backward."""
    import MultiScaleDeformableAttention as MSDA
    x = make_inputs(2, 4, 64, 300, 4, [(40, 40), (16, 16), (8, 8)] * 2, seed=23, dtype=dtype)
    g = torch.Generator().manual_seed(4)
    keep = (torch.rand(2, 300, 1, 6, 1, generator=g) < 0.5).double()
    keep[0, 100:200] = 0.0
    keep[0, 100:200, :, 2] = 1.0                   # whole waves blind to all but one level
    x["attn"] = (x["attn"] * keep).to(dtype).to(torch.float64)
    dev = lambda t: t.to(DEV, dtype) if t.is_floating_point() else t.to(DEV)
    args = [dev(x[k]) for k in ("value", "shapes", "start", "loc", "attn")] + [dev(x["grad"]).reshape(2, 300, -1), 1]
    full = MSDA.ms_deform_attn_backward(*args)
    lazy = MSDA.ms_deform_attn_backward(*args, lazy_zero_attn=True)
    zero = (args[4] == 0)
    # (grad_value: same records, but their order inside a cell -- and so the order of the fp32 sums --
    # is not fixed from run to run)
    assert float((lazy[0].double() - full[0].double()).abs().max()) <= TOL[dtype] * max(1.0, float(full[0].abs().max()))
    assert torch.equal(lazy[2][~zero], full[2][~zero]) and torch.equal(lazy[1][~zero], full[1][~zero])
    assert float(full[2][zero].abs().max()) > 1e-3
    # a hint: honoured by the 16-bit route's row-gather kernel (here: the two 40x40 levels), ignored by
    # the dense dot products of the small levels and by the fp32 route
    assert bool(((lazy[2][zero] == 0) | (lazy[2][zero] == full[2][zero])).all())
    if dtype == torch.bfloat16:
        big = torch.zeros_like(zero)
        big[:, :, :, [0, 3]] = True
        assert float(lazy[2][zero & big].abs().max()) == 0.0 and float(lazy[1][zero & big].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------
# The forward's second formulation (csrc/msda_fwd_mma.hip): levels that fit in LDS live there and are
# sampled by the matrix cores, the others by row gather.  The default routing takes it from 256 queries per
# (b, h) slab on; here it is forced (mmfs_msda_forward_flags, MMFS_FWD_LDS_LEVELS) on shapes of every kind.
LDS_CASES = [
    # B, H, D, Nq, P, shapes                                           what it exercises
    (1, 8, 128, 64, 4, [(64, 64), (32, 32), (16, 16), (8, 8)]),         # the north-star pyramid: two levels resident, K = 16
    (2, 3, 128, 333, 4, [(16, 16), (8, 8), (20, 20), (5, 7)]),          # every level resident (two product batches), ragged run
    (2, 16, 64, 200, 8, [(64, 64), (32, 32), (16, 16), (8, 8)]),        # SD geometry, D = 64 (8 queries per wave), K = 32: two chunks
    (1, 16, 64, 300, 8, [(32, 32), (16, 16), (8, 8)] * 4),              # LLM n = 4: K = 96; the 8x8 levels and ONE 16x16 level fit
    (1, 2, 128, 70, 3, [(9, 5), (40, 40), (3, 3), (1, 1), (2, 9)]),     # K = 15: a ragged chunk; non-square and degenerate levels
    (1, 2, 64, 40, 2, [(3, 3)] * 60),                                   # L = 60, K = 120: eight chunks, everything resident
    (1, 4, 128, 50, 4, [(70, 70), (50, 50)]),                           # nothing fits: pure row gather inside the new kernel
    (3, 8, 128, 1, 4, [(16, 16), (8, 8)]),                              # one query (decode)
    (1, 2, 64, 5000, 4, [(24, 24), (12, 12), (6, 6)]),                  # many runs per (b, h): 20 workgroups per slab
]


def run_fwd(x, dtype, algo):
    import MultiScaleDeformableAttention as MSDA
    dev = lambda t: t.to(DEV, dtype) if t.is_floating_point() else t.to(DEV)
    old = MSDA._fwd_algo
    MSDA._fwd_algo = algo
    try:
        out = MSDA.ms_deform_attn_forward(dev(x["value"]), dev(x["shapes"]), dev(x["start"]), dev(x["loc"]), dev(x["attn"]), 1)
        torch.cuda.synchronize()
    finally:
        MSDA._fwd_algo = old
    return out.double().cpu().numpy()


@pytest.mark.parametrize("case", LDS_CASES, ids=[f"B{c[0]}H{c[1]}D{c[2]}Nq{c[3]}P{c[4]}L{len(c[5])}" for c in LDS_CASES])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_lds_levels_forward_matches_oracle(case, dtype):
    B, H, D, Nq, P, shapes = case
    x = make_inputs(B, H, D, Nq, P, shapes, seed=21, loc_range=(-0.15, 1.15), dtype=dtype)
    x["loc"][0, 0, 0, 0, 0, 0] = float("nan")            # non-finite locations contribute nothing
    x["loc"][0, Nq // 2, 1 % H, -1, 0, 1] = float("inf")
    x["attn"][0, Nq - 1, 0, -1] = 0.0                     # zero weights read nothing
    want = msda_oracle.forward(x["value"], x["shapes"], x["start"], x["loc"], x["attn"])
    got = run_fwd(x, dtype, "lds")
    scale = max(1.0, float(np.abs(want).max()))
    assert max_abs(got, want) <= TOL[dtype] * scale, f"{case[:5]}: {max_abs(got, want):.3e}"
    # and against the row-gather kernel: the same fp32 products, sums in another order, weights of the
    # resident levels carried as hi + lo 16-bit parts (>= 16 significant bits)
    ref = run_fwd(x, dtype, "gather")
    assert max_abs(got, ref) <= 0.5 * TOL[dtype] * scale


@pytest.mark.parametrize("D", [128, 64])
def test_lds_levels_forward_non_finite_rows_stay_with_their_queries(D):
    """A product on the matrix cores multiplies every row of its weight operand with every value row it is handed.
    The kernel gives each query a product of its own, so a non-finite value row reaches the queries that sample
    it and no other (cuh:58-81); corners outside the map and zero weights point at a row of zeros."""
    sh, start = level_tables([(4, 4), (2, 2)])
    H, Nq = 2, 24
    value = torch.ones(1, 20, H, D, dtype=torch.float64)
    value[0, 5, 0] = float("inf")                         # pixel (1, 1) of level 0, head 0
    value[0, 16, 1] = float("nan")                        # pixel (0, 0) of level 1, head 1
    loc = torch.full((1, Nq, H, 2, 2, 2), 0.875, dtype=torch.float64)        # level 0: pixels (2..3, 2..3); level 1: (1, 1) + outside
    attn = torch.full((1, Nq, H, 2, 2), 0.25, dtype=torch.float64)
    loc[0, 3, 0, 0, 0] = torch.tensor([0.375, 0.375])     # query 3, head 0 touches pixel (1, 1) of level 0
    loc[0, 7, 1, 1, 1] = torch.tensor([0.25, 0.25])       # query 7, head 1 touches pixel (0, 0) of level 1
    loc[0, 9, 0, 0, 1] = torch.tensor([0.375, 0.375]); attn[0, 9, 0, 0, 1] = 0.0      # zero weight: reads nothing
    x = dict(value=value, shapes=sh, start=start, loc=loc, attn=attn)
    got = run_fwd(x, torch.bfloat16, "lds").reshape(Nq, H, D)
    bad = ~np.isfinite(got).all(-1)
    want_bad = np.zeros((Nq, H), dtype=bool)
    want_bad[3, 0] = True; want_bad[7, 1] = True
    assert (bad == want_bad).all(), np.argwhere(bad != want_bad)
    same = ~want_bad
    same[9, 0] = False                                     # (the query with the zeroed weight sums to less)
    assert np.allclose(got[same], got[0, 0, 0]) and got[9, 0, 0] < got[0, 0, 0]


# ---------------------------------------------------------------------------------------------------------
# The forward's third formulation (csrc/msda_fwd_q8.hip, round 4): a workgroup owns a 32-channel SLICE of a (b, h); every
# level whose slice fits in LDS is sampled by the matrix cores in tiles of 8 queries (one product per sample index of
# the 8 queries and 16 channels, block-diagonal weights), the others by row gather inside the same kernel.
SLICE_CASES = LDS_CASES + [
    # B, H, D, Nq, P, shapes                                           what it exercises
    (2, 16, 64, 130, 8, [(32, 32), (16, 16), (8, 8)]),                  # the LLM's real geometry, one image: everything resident, two slices
    (1, 8, 128, 700, 4, [(64, 64), (32, 32), (16, 16), (8, 8)]),        # north star, four slices, two runs of 512 queries (the second ragged)
    (2, 16, 32, 97, 4, [(32, 32), (16, 16), (8, 8)]),                   # the encoder's head width: ONE slice
    (1, 3, 96, 45, 5, [(7, 9), (13, 4), (2, 2)]),                       # three slices; widths that need 1, 2, 3 pad pixels per line; P = 5
    (1, 2, 256, 20, 2, [(6, 6), (3, 3)]),                               # eight slices
    (1, 4, 64, 9, 8, [(33, 31), (40, 40), (16, 16)]),                   # 33 x 31 + 16 x 16 fit next to each other, 40 x 40 does not: mixed passes
]


@pytest.mark.parametrize("case", SLICE_CASES, ids=[f"B{c[0]}H{c[1]}D{c[2]}Nq{c[3]}P{c[4]}L{len(c[5])}" for c in SLICE_CASES])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_sliced_forward_matches_oracle(case, dtype):
    B, H, D, Nq, P, shapes = case
    x = make_inputs(B, H, D, Nq, P, shapes, seed=21, loc_range=(-0.15, 1.15), dtype=dtype)
    x["loc"][0, 0, 0, 0, 0, 0] = float("nan")            # non-finite locations contribute nothing
    x["loc"][0, Nq // 2, 1 % H, -1, 0, 1] = float("inf")
    x["attn"][0, Nq - 1, 0, -1] = 0.0                     # zero weights read nothing
    x["loc"][0, Nq // 3, 0, 0, -1] = torch.tensor([0.0, 1.0])            # a corner of the map: three of four corners outside
    want = msda_oracle.forward(x["value"], x["shapes"], x["start"], x["loc"], x["attn"])
    got = run_fwd(x, dtype, "slices")
    scale = max(1.0, float(np.abs(want).max()))
    assert max_abs(got, want) <= TOL[dtype] * scale, f"{case[:5]}: {max_abs(got, want):.3e}"
    ref = run_fwd(x, dtype, "gather")
    assert max_abs(got, ref) <= 0.5 * TOL[dtype] * scale


@pytest.mark.parametrize("kb", [60, 80, 130])
def test_sliced_forward_with_less_lds_moves_levels_to_the_row_gather(kb, monkeypatch):
    """Which levels are resident is decided on the device from the LDS the launch was given (MMFS_FWD_Q8_LDS_KB: a test
    knob): with 60 KB none of the north-star pyramid's levels, with 80 KB 16x16 + 8x8, with 130 KB 32x32 too --
    the same outputs to the rounding of the weights' hi + lo parts."""
    x = make_inputs(1, 4, 128, 150, 4, [(64, 64), (32, 32), (16, 16), (8, 8)], seed=3, loc_range=(-0.1, 1.1), dtype=torch.bfloat16)
    want = msda_oracle.forward(x["value"], x["shapes"], x["start"], x["loc"], x["attn"])
    code = ("import os, sys, numpy as np, torch; sys.path[:0] = [%r, %r]; os.environ['MMFS_FWD_Q8_LDS_KB'] = '%d';"
            "import MultiScaleDeformableAttention as MSDA; MSDA._fwd_algo = 'slices';"
            "z = np.load(sys.argv[1]); dev = lambda a: torch.from_numpy(a).cuda();"
            "f = lambda a: dev(a).to(torch.bfloat16);"
            "o = MSDA.ms_deform_attn_forward(f(z['value']), dev(z['shapes']), dev(z['start']), f(z['loc']), f(z['attn']), 1);"
            "np.save(sys.argv[2], o.double().cpu().numpy())") % (ROOT, os.path.join(ROOT, "mm-interleaved_amd"), kb)
    import subprocess, tempfile
    with tempfile.TemporaryDirectory() as td:              # (the knob is read once per process)
        np.savez(os.path.join(td, "in.npz"), **{k: v.numpy() for k, v in x.items() if k != "grad"})
        subprocess.run([sys.executable, "-c", code, os.path.join(td, "in.npz"), os.path.join(td, "out.npy")], check=True)
        got = np.load(os.path.join(td, "out.npy"))
    assert max_abs(got, want) <= TOL[torch.bfloat16] * max(1.0, float(np.abs(want).max()))


def test_sliced_forward_is_the_default_where_the_whole_pyramid_is_resident():
    """Heads of 32 / 64 channels whose levels all fit in the image (judged from S on the host: the entry point sees
    device pointers only) take the sliced formulation by default from 128 queries and 3072 samples per (b, h) on -- the
    LLM layer's real geometry with one image, the ViT-Adapter's injector (256 queries x 3 levels x 4 points, heads of
    32 channels); heads of 128 channels, shapes with a level left to the row gather, and short runs keep what they had.
    Round 5 (r05ae): and only launches with enough queries per CU (768 query-slices at heads of 64 channels, 384 at 32) -- at
    the LLM layer's geometry 2048 tokens take it (49.6 us against the row gather's 63.2), 1024 and 512 do not (41.5 / 23.0
    against 31.2 / 18.5)."""
    llm = [(32, 32), (16, 16), (8, 8)]
    x = make_inputs(4, 16, 64, 2048, 8, llm, seed=5, loc_range=(-0.1, 1.1), dtype=torch.bfloat16)    # BASELINE config 3 at 2048 tokens
    a = run_fwd(x, torch.bfloat16, "auto")
    assert max_abs(a, run_fwd(x, torch.bfloat16, "slices")) == 0.0
    assert max_abs(a, run_fwd(x, torch.bfloat16, "gather")) > 0.0         # (another summation order: not bit-equal)
    x = make_inputs(4, 16, 64, 512, 8, llm, seed=5, loc_range=(-0.1, 1.1), dtype=torch.bfloat16)     # ... at 512 tokens: the row gather
    assert max_abs(run_fwd(x, torch.bfloat16, "auto"), run_fwd(x, torch.bfloat16, "gather")) == 0.0
    x = make_inputs(32, 16, 32, 256, 4, llm, seed=6, loc_range=(-0.1, 1.1), dtype=torch.bfloat16)    # the injector's shape and batch
    a = run_fwd(x, torch.bfloat16, "auto")
    assert max_abs(a, run_fwd(x, torch.bfloat16, "slices")) == 0.0 and max_abs(a, run_fwd(x, torch.bfloat16, "gather")) > 0.0
    x = make_inputs(1, 16, 64, 100, 8, llm, seed=5, loc_range=(-0.1, 1.1), dtype=torch.bfloat16)     # fewer than 128 queries
    assert max_abs(run_fwd(x, torch.bfloat16, "auto"), run_fwd(x, torch.bfloat16, "gather")) == 0.0
    x = make_inputs(1, 16, 64, 200, 8, [(64, 64)] + llm, seed=5, loc_range=(-0.1, 1.1), dtype=torch.bfloat16)   # 64 x 64 does not fit
    assert max_abs(run_fwd(x, torch.bfloat16, "auto"), run_fwd(x, torch.bfloat16, "gather")) == 0.0
    x = make_inputs(8, 8, 128, 512, 4, llm, seed=5, loc_range=(-0.1, 1.1), dtype=torch.bfloat16)     # heads of 128 channels, 512 runs of 64
    assert max_abs(run_fwd(x, torch.bfloat16, "auto"), run_fwd(x, torch.bfloat16, "waves")) == 0.0


def _non_finite_element_case(dtype, D, algo, H=2):
    """Single non-finite ELEMENTS (and one whole row) of `value` in a level that is read from memory and in two that are
    LDS-resident; the forced formulation's output against the oracle element for element: which outputs are finite, NaN
    vs +-Inf, and the finite values (cuh:58-81, :275-299: a non-finite element reaches its own channel of the queries that
    sample its row with a valid corner, nothing else)."""
    shapes = [(64, 64), (4, 4), (2, 2)]                   # level 0 does not fit in LDS (rows from memory), the others do
    B, Nq, P = 1, 600, 2
    x = make_inputs(B, H, D, Nq, P, shapes, seed=5, loc_range=(0.05, 0.95), dtype=dtype)
    value = x["value"]
    value[0, 65 * 20, 0, 3] = float("inf")                # level 0, single channels: pixel (20, 20)
    value[0, 65 * 20 + 1, 0, D - 28] = float("-inf")      # ... (20, 21)
    value[0, 65 * 10, 1, D // 2 + 13] = float("nan")
    value[0, 4096 + 5, 1, D // 2] = float("nan")          # level 1
    value[0, 4096 + 16 + 1, 0, D - 1] = float("inf")      # level 2
    value[0, 65 * 30, 1, :] = float("nan")                # a whole row of level 0
    x["attn"][0, 3, 0] = 0.0                              # a query that reads nothing at all in head 0
    x["loc"][0, 5, 0] = 2.0                               # ... and one whose samples all fail the range test
    x["loc"][0, 7, 0, 0, 0] = torch.tensor([20.5 / 64, 20.5 / 64])      # exactly on pixel (20, 20) in every arithmetic: its right
                                                                        # neighbour weighs 0 x -Inf = NaN, as in the reference
    want = msda_oracle.forward(value, x["shapes"], x["start"], x["loc"], x["attn"])
    got = run_fwd(x, dtype, algo)
    fin_w, fin_g = np.isfinite(want), np.isfinite(got)
    # (the library reads nothing where the attention weight is exactly 0, DESIGN 4.1: query 3 of head 0 is finite here)
    want3 = want.reshape(Nq, H, D)[3, 0]
    if not np.isfinite(want3).all():
        fin_w.reshape(Nq, H, D)[3, 0] = True; want.reshape(Nq, H, D)[3, 0] = 0.0
    assert (fin_w == fin_g).all(), np.argwhere(fin_w != fin_g)[:10]
    assert (~fin_w).any() and fin_w.any()
    n_bad_queries = int((~fin_w.reshape(Nq, H, D)).any(-1).sum())
    assert 0 < n_bad_queries < Nq * H                      # (the 2 x 2 level's non-finite pixel is seen by most queries)
    scale = max(1.0, float(np.abs(want[fin_w]).max()))
    assert np.abs(got[fin_w] - want[fin_w]).max() <= TOL[dtype] * scale
    assert (np.isnan(want) == np.isnan(got)).all()         # NaN vs +-Inf as the reference has them
    assert (want[np.isinf(want)] == got[np.isinf(want)]).all()
    ref = run_fwd(x, dtype, "gather")                     # the row gather agrees element for element on what is finite
    assert (np.isfinite(ref) == fin_g).all()


@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_sliced_forward_non_finite_values_stay_with_their_queries(D, dtype):
    """A product of the sliced forward multiplies the rows of EIGHT queries with a block-diagonal weight tile: a non-finite
    value row turns the zeros of the other queries' weights into NaN.  Round 4 documented that as a deviation (a non-finite
    row reached the up to 8 queries of its tile); round 5: a tile with a non-finite sum is recomputed channel by channel
    (q8::exact8), and the result is the reference's element for element (cuh:58-81) -- as for the other formulations."""
    _non_finite_element_case(dtype, D, "slices")


@pytest.mark.parametrize("shape", [(2, 8, 8192), (1, 16, 4096 * 3 + 77), (3, 4, 300)])
def test_persistent_workgroups_compute_what_one_workgroup_per_run_does(shape, monkeypatch):
    """The LDS-resident kernels run as one persistent workgroup per CU when there are at least two runs of queries
    per CU (msda_mma_common.h, persistent_grid): a workgroup then serves several runs -- other (b, h) slabs: the image
    is refilled behind a barrier -- instead of one.  Which workgroup serves a run changes nothing a query sees:
    forward and both gradients bit-equal to one workgroup per run (MMFS_MMA_PERSIST=0), also with only 8 workgroups
    for everything (MMFS_MMA_GRID=8), also where a workgroup's last run is a ragged one."""
    import MultiScaleDeformableAttention as MSDA
    B, H, Nq = shape
    x = make_inputs(B, H, 128, Nq, 4, [(24, 24), (16, 16), (8, 8)], seed=9, loc_range=(-0.1, 1.1), dtype=torch.bfloat16)
    dev = lambda t: t.to(DEV, torch.bfloat16) if t.is_floating_point() else t.to(DEV)
    args = [dev(x[k]) for k in ("value", "shapes", "start", "loc", "attn")]
    grad = torch.randn(B, Nq, H * 128, generator=torch.Generator().manual_seed(2)).to(DEV, torch.bfloat16)
    old_f, old_t = MSDA._fwd_algo, MSDA._taps_algo
    MSDA._fwd_algo, MSDA._taps_algo = "lds", "lds"
    res = {}
    try:
        for name, env in (("default", {}), ("per_run", {"MMFS_MMA_PERSIST": "0"}), ("grid8", {"MMFS_MMA_GRID": "8"})):
            monkeypatch.delenv("MMFS_MMA_PERSIST", raising=False)
            monkeypatch.delenv("MMFS_MMA_GRID", raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            out = MSDA.ms_deform_attn_forward(*args, 1)
            gv, gl, ga = MSDA.ms_deform_attn_backward(*args, grad, 1)
            torch.cuda.synchronize()
            res[name] = (out, gl, ga)
    finally:
        MSDA._fwd_algo, MSDA._taps_algo = old_f, old_t
    for name in ("per_run", "grid8"):
        for a, b in zip(res["default"], res[name]):
            assert torch.equal(a, b), name
    want = msda_oracle.forward(x["value"], x["shapes"], x["start"], x["loc"], x["attn"])
    assert max_abs(res["default"][0].double().cpu().numpy(), want) <= TOL[torch.bfloat16] * max(1.0, float(np.abs(want).max()))


def test_query_wave_forward_is_the_default_for_long_runs(monkeypatch):
    """From 4096 samples per (b, h) slab on (and at least 64 queries), 16-bit heads of 128 channels take the wave-per-query
    formulation (round 5; rounds 3-4: the LDS-resident one of msda_fwd_mma.hip) -- and the autograd function's outputs and
    gradients still match the oracle on such a shape; below, the row gather.  Round 5 (r05ac): and only launches that give every
    CU two runs of queries -- 1024-lane workgroups that each fill an LDS image do not fill the chip otherwise (at the north
    star's dimensions and 256 queries the row gather is twice as fast); runs are 256 queries, or 128 / 64 for fewer queries."""
    x = make_inputs(1, 4, 128, 100, 4, [(24, 24), (16, 16), (8, 8)], seed=5, loc_range=(-0.1, 1.1), dtype=torch.bfloat16)
    assert max_abs(run_fwd(x, torch.bfloat16, "auto"), run_fwd(x, torch.bfloat16, "gather")) == 0.0     # 1200 samples
    x = make_inputs(1, 4, 128, 352, 4, [(24, 24), (16, 16), (8, 8)], seed=5, loc_range=(-0.1, 1.1), dtype=torch.bfloat16)
    assert max_abs(run_fwd(x, torch.bfloat16, "auto"), run_fwd(x, torch.bfloat16, "gather")) == 0.0     # 4 slabs: 24 runs of 64
    x = make_inputs(8, 8, 128, 520, 4, [(24, 24), (16, 16), (8, 8)], seed=5, loc_range=(-0.1, 1.1), dtype=torch.bfloat16)
    a, g = run_fwd(x, torch.bfloat16, "auto"), run_fwd(x, torch.bfloat16, "waves")
    assert max_abs(a, g) == 0.0
    assert max_abs(a, run_fwd(x, torch.bfloat16, "gather")) > 0.0        # (a different summation order: not bit-equal)
    check(run_hip(x, torch.bfloat16), run_oracle(x), x, torch.bfloat16, "auto-routed")


# ---------------------------------------------------------------------------------------------------------
def _overlapping_case(dtype, seed=8):
    g = torch.Generator().manual_seed(seed)
    B, H, D, Nq, P = 2, 4, 64, 40, 4
    shapes = torch.tensor([(4, 6), (3, 3)], dtype=torch.long)
    start = torch.tensor([0, 20], dtype=torch.long)            # level 1 starts inside level 0 (rows 20..23 shared)
    S = 29
    rt = (lambda t: t.to(dtype).double()) if dtype != torch.float32 else (lambda t: t.float().double())
    return dict(value=rt(torch.rand(B, S, H, D, generator=g)), shapes=shapes, start=start,
                loc=rt(torch.rand(B, Nq, H, 2, P, 2, generator=g) * 1.2 - 0.1), attn=rt(torch.rand(B, Nq, H, 2, P, generator=g)),
                grad=rt(torch.randn(B, Nq, H * D, generator=g)))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
def test_unverified_overlapping_table_is_served_by_the_atomic_fallback(dtype):
    """VERDICT r2 / ADVICE r2: a table nobody registered whose levels OVERLAP cannot be served by the sorted
    backward (two levels would own the same grad_value rows); it used to end in a device-side trap.  VERDICT r3 /
    ADVICE r3: round 3's answer -- zeros for grad_value behind a call that reported success, an exception at the
    NEXT call -- was a wrong result.  Now the same call ends with the reference's float-atomic scatter
    (csrc/msda_bwd_refused.hip): every gradient matches the oracle, nothing raises, the shim warns once."""
    import warnings
    import MultiScaleDeformableAttention as MSDA
    x = _overlapping_case(dtype)
    dev = lambda t: t.to(DEV, dtype) if t.is_floating_point() else t.to(DEV)
    v, l, a, gr = dev(x["value"]), dev(x["loc"]), dev(x["attn"]), dev(x["grad"])
    sh, st = x["shapes"].to(DEV), x["start"].to(DEV)           # never registered
    MSDA.check_level_table_status(synchronize=True)             # (clean slate)
    MSDA._bad_table_warned = False
    want = run_oracle(x)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for rep in range(2):                                    # (a recycled workspace must not remember the first verdict)
            gv, gl, ga = MSDA.ms_deform_attn_backward(v, sh, st, l, a, gr, 1)
            for name, got, ref in (("grad_value", gv, want[1]), ("grad_loc", gl, want[2]), ("grad_attn", ga, want[3])):
                err = max_abs(got.double().cpu().numpy(), ref)
                assert err <= TOL[dtype] * max(1.0, float(np.abs(ref).max())), (name, rep, err)
        assert MSDA.check_level_table_status(synchronize=True) is True      # the slow path was taken ...
        assert MSDA.check_level_table_status(synchronize=True) is False     # (the flag is consumed)
    said = [m for m in w if "register_level_tables" in str(m.message)]
    assert len(said) == 1 and said[0].category is RuntimeWarning            # ... and the shim says so, once
    # an ordinary fresh table right after it, through the same (recycled) workspace: the fallback stays out of the way
    x2 = make_inputs(2, 4, 64, 50, 4, [(12, 9), (6, 5), (3, 3)], seed=31, dtype=dtype)
    check(run_hip(x2, dtype), run_oracle(x2), x2, dtype, "after a refused table")
    assert MSDA.check_level_table_status(synchronize=True) is False
    # out-of-range: level 1 points past the end of value -- the reference would write out of bounds; here the rows
    # that exist get their gradients, the others are skipped, nothing faults
    st_bad = torch.tensor([0, 26], dtype=torch.long).to(DEV)
    gv2, _, _ = MSDA.ms_deform_attn_backward(v, sh, st_bad, l, a, gr, 1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gv2.float()).all())
    assert MSDA.check_level_table_status(synchronize=True) is True
    # registered (the shim then knows it is not canonical): the float-atomic path serves it directly
    check(run_hip(x, dtype, use_autograd=False, register=True), want, x, dtype, "overlapping, registered")


# ---------------------------------------------------------------------------------------------------------
# Many points per level.  No caller in the reference goes beyond P = 8, but the only workload the reference ever
# TIMED is P = 64 (ops/tests/speed_test.py:67-88: bs 32, levels 16^2 / 8^2, 128 queries, 8 heads of 128 channels,
# fp16 then fp32); the dense matrix-core taps refuse P > 16 (csrc/msda_dense.hip), everything else is generic.
MANY_POINT_CASES = [
    # B, H, D, Nq, P, shapes
    (2, 8, 128, 128, 64, [(16, 16), (8, 8)]),                  # the reference's speed test, batch cut to 2
    (1, 4, 64, 70, 32, [(12, 9), (6, 5), (3, 3)]),             # P = 32, K = 96, odd extents
    (1, 2, 32, 33, 64, [(20, 20), (7, 4)]),                    # D = 32 (scalar record scan), a level of 400 pixels
    (1, 2, 64, 300, 16, [(9, 9), (4, 4)]),                     # 4 vectors x 300 queries = 1200 virtual queries: one vector each, two trips' worth of threads
    (1, 2, 64, 1500, 12, [(9, 9), (4, 4)]),                    # 3 vectors per query, 4500 virtual queries: too many for one trip -> the scalar scan
]


@pytest.mark.parametrize("case", MANY_POINT_CASES, ids=[f"B{c[0]}H{c[1]}D{c[2]}Nq{c[3]}P{c[4]}L{len(c[5])}" for c in MANY_POINT_CASES])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("route", ["registered", "fresh", "atomic"])
def test_many_points_per_level(case, dtype, route, monkeypatch):
    """P in {32, 64} through every backward route: host-registered table (hybrid routing offered and declined by the
    dense kernel, sorted grad_value), a table the shim has never seen (checked on the device), float atomics."""
    import MultiScaleDeformableAttention as MSDA
    B, H, D, Nq, P, shapes = case
    x = make_inputs(B, H, D, Nq, P, shapes, seed=13, loc_range=(-0.1, 1.1), dtype=dtype)
    if route == "atomic":
        monkeypatch.setattr(MSDA, "_bwd_algo", "atomic")
    got = run_hip(x, dtype, use_autograd=False, register=(route == "registered"))
    want = run_oracle(x)
    check(got, want, x, dtype, f"P={P} {route}")
    if route == "registered":
        # many vectors per query: the kept scan takes them as groups of virtual queries (default) -- or the scalar scan does
        monkeypatch.setenv("MMFS_SORT_MANY_POINTS", "0")
        check(run_hip(x, dtype, use_autograd=False, register=True), want, x, dtype, f"P={P} scalar scan")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_many_points_lds_forward(dtype):
    """The reference's speed-test shape through the LDS-resident forward: both levels live in LDS, K = 128 is eight
    chunks of two product batches each."""
    x = make_inputs(2, 8, 128, 128, 64, [(16, 16), (8, 8)], seed=14, loc_range=(-0.1, 1.1), dtype=dtype)
    want = msda_oracle.forward(x["value"], x["shapes"], x["start"], x["loc"], x["attn"])
    got = run_fwd(x, dtype, "lds")
    assert max_abs(got, want) <= TOL[dtype] * max(1.0, float(np.abs(want).max()))


# ---------------------------------------------------------------------------------------------------------
# grad_loc / grad_attn, second formulation (csrc/msda_taps_mma.hip): one kernel for all levels, those that fit in
# LDS contracted on the matrix cores from gathered rows, the others by row gather.  Default from 256 queries per
# (b, h) slab on for heads of 128 channels; forced here (MMFS_BWD_TAPS_LDS_LEVELS) on shapes of every kind.
TAPS_LDS_CASES = [
    # B, H, D, Nq, P, shapes
    (1, 8, 128, 64, 4, [(64, 64), (32, 32), (16, 16), (8, 8)]),         # the north-star pyramid: two levels resident, K = 16
    (2, 3, 128, 333, 4, [(16, 16), (8, 8), (20, 20), (5, 7)]),          # every level resident: four tiles per query, ragged run
    (1, 2, 128, 70, 3, [(9, 5), (40, 40), (3, 3), (1, 1), (2, 9)]),     # K = 15: ragged chunk, ragged last tile, degenerate levels
    (1, 4, 128, 50, 4, [(70, 70), (50, 50)]),                           # nothing fits: pure row gather inside the new kernel
    (3, 8, 128, 1, 4, [(16, 16), (8, 8)]),                              # one query
    (1, 2, 128, 300, 8, [(32, 32), (16, 16), (8, 8)] * 2),              # K = 48: three chunks per query group
    (2, 8, 128, 128, 64, [(16, 16), (8, 8)]),                           # the reference's speed-test shape: K = 128, all resident
    # heads of 64 channels (round 5): eight queries per wave, two staging passes, 8-lane dot groups
    (2, 16, 64, 200, 8, [(64, 64), (32, 32), (16, 16), (8, 8)]),        # the image decoder's geometry: K = 32, 16^2 + 8^2 resident
    (1, 16, 64, 300, 8, [(32, 32), (16, 16), (8, 8)] * 4),              # the LLM's, four images: K = 96; the 8^2 maps and one 16^2 fit
    (1, 2, 64, 70, 3, [(9, 5), (40, 40), (3, 3), (1, 1), (2, 9)]),      # K = 15: ragged chunk, ragged last tile, degenerate levels
    (3, 4, 64, 5, 4, [(16, 16), (8, 8)]),                               # five queries: a ragged group of eight
    (1, 2, 64, 50, 4, [(70, 70), (50, 50)]),                            # nothing fits
]


@pytest.mark.parametrize("case", TAPS_LDS_CASES, ids=[f"B{c[0]}H{c[1]}D{c[2]}Nq{c[3]}P{c[4]}L{len(c[5])}" for c in TAPS_LDS_CASES])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("route", ["registered", "fresh"])
def test_lds_levels_taps_match_oracle(case, dtype, route, monkeypatch):
    import MultiScaleDeformableAttention as MSDA
    monkeypatch.setattr(MSDA, "_taps_algo", "lds")
    B, H, D, Nq, P, shapes = case
    x = make_inputs(B, H, D, Nq, P, shapes, seed=17, loc_range=(-0.15, 1.15), dtype=dtype)
    x["loc"][0, 0, 0, 0, 0, 0] = float("nan")            # non-finite locations: zero gradients
    x["loc"][0, Nq // 2, 1 % H, -1, 0, 1] = float("inf")
    x["attn"][0, Nq - 1, 0, -1] = 0.0                     # zero weight: grad_attn is NOT zero, grad_loc is
    log = []
    monkeypatch.setattr(MSDA, "_event_log", log)
    got = run_hip(x, dtype, use_autograd=False, register=(route == "registered"))
    monkeypatch.setattr(MSDA, "_event_log", None)
    assert not any("coarse" in n for n, _, _ in log), [n for n, _, _ in log]         # one kernel does every level
    check(got, run_oracle(x), x, dtype, f"taps lds {route} {case[:5]}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_lds_levels_taps_are_the_default_and_agree_with_the_row_gather(dtype, monkeypatch):
    """From 4096 samples per slab on, heads of 128 channels take the fused kernel; against the row gather + dense pair
    the same dots come out in another summation order, the algebra after them is the same code."""
    import MultiScaleDeformableAttention as MSDA
    x = make_inputs(2, 4, 128, 352, 4, [(24, 24), (16, 16), (8, 8)], seed=19, loc_range=(-0.1, 1.1), dtype=dtype)
    keep = (torch.rand(2, 352, 1, 3, 1, generator=torch.Generator().manual_seed(1)) < 0.6).double()
    x["attn"] = (x["attn"] * keep).to(dtype).to(torch.float64)
    res = {}
    for algo in ("auto", "lds", "gather"):
        monkeypatch.setattr(MSDA, "_taps_algo", algo)
        res[algo] = run_hip(x, dtype, use_autograd=False, register=True)
    for a, b in zip(res["auto"][2:], res["lds"][2:]):
        assert max_abs(a, b) == 0.0                                                  # auto IS the fused kernel here
    want = run_oracle(x)
    for algo in ("lds", "gather"):
        check(res[algo], want, x, dtype, algo)
    # the lazy hint (MMFS's softmax never reads the gradients of a zero weight): zeros there, the rest bit-equal
    dev = lambda t: t.to(DEV, dtype) if t.is_floating_point() else t.to(DEV)
    args = [dev(x[k]) for k in ("value", "shapes", "start", "loc", "attn")] + [dev(x["grad"]).reshape(2, 352, -1), 1]
    monkeypatch.setattr(MSDA, "_taps_algo", "lds")
    full = MSDA.ms_deform_attn_backward(*args)
    lazy = MSDA.ms_deform_attn_backward(*args, lazy_zero_attn=True)
    zero = args[4] == 0
    assert zero.any() and torch.equal(lazy[2][~zero], full[2][~zero]) and torch.equal(lazy[1][~zero], full[1][~zero])
    assert not lazy[2][zero].any() and not lazy[1][zero].any()


def test_staged_sort_and_reduce_on_a_foreign_workspace_do_nothing():
    """``mmfs_msda_backward_hybrid`` lets a caller launch the pass stage by stage, and its sort / reduce
    stages trust the plan in the workspace.  The plan stamps its header with the call's dimensions; a sort or a
    reduce that finds another stamp (a workspace prepared for another shape, or by nobody) returns without
    following the header's pointers -- no trap, no fault, the context stays usable."""
    import numpy as np_
    import MultiScaleDeformableAttention as MSDA
    lib = MSDA._lib
    x = make_inputs(2, 4, 64, 50, 4, [(12, 9), (6, 5), (3, 3)], seed=3, dtype=torch.bfloat16)
    dev = lambda t: t.to(DEV, torch.bfloat16) if t.is_floating_point() else t.to(DEV)
    v, l, a_ = dev(x["value"]), dev(x["loc"]), dev(x["attn"])
    sh, st, go = dev(x["shapes"]), dev(x["start"]), dev(x["grad"]).reshape(2, 50, -1).contiguous()
    hs = np_.ascontiguousarray(x["shapes"].numpy(), dtype=np_.int64); hst = np_.ascontiguousarray(x["start"].numpy(), dtype=np_.int64)
    B, S, H, D, L, Nq, P = 2, int(x["value"].shape[1]), 4, 64, 3, 50, 4
    flags = MSDA._BWD_CANONICAL_LEVELS | MSDA._BWD_DENSE_TAPS
    nbytes = lib.mmfs_msda_backward_hybrid_workspace_bytes(2, hs.ctypes.data, hst.ctypes.data, B, S, H, D, L, Nq, P, flags)
    assert nbytes > 0
    SORT, REDUCE = 8, 16                                        # MMFS_HYB_BWD_VALUE_SORT, _REDUCE
    for fill in (0, 0x5a):                                      # no plan at all / garbage
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        gv = torch.full((B, S, H, D), 7.0, dtype=torch.bfloat16, device=DEV)
        gl, ga = torch.empty_like(l), torch.empty_like(a_)
        for stage in (SORT, REDUCE):
            rc = lib.mmfs_msda_backward_hybrid(2, v.data_ptr(), sh.data_ptr(), st.data_ptr(), hs.ctypes.data, hst.ctypes.data,
                                               l.data_ptr(), a_.data_ptr(), go.data_ptr(), gv.data_ptr(), gl.data_ptr(), ga.data_ptr(),
                                               ws.data_ptr(), nbytes, B, S, H, D, L, Nq, P, flags, stage, MSDA._stream(gv.device))
            assert rc == 0
        torch.cuda.synchronize()
        assert bool((gv == 7.0).all())                          # nothing was written
    check(run_hip(x, torch.bfloat16, register=True), run_oracle(x), x, torch.bfloat16, "after staged calls on foreign workspaces")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_value_plan_hosted_by_the_taps_kernel(dtype, monkeypatch):
    """One-call backward on a registered table, heads of 128 channels, >= 256 queries: the grad_value half's opening
    launch (clear the sort's cursors, plan) is done by the first workgroup of the grad_loc / grad_attn kernel
    (csrc/msda_plan.h, PrepareJob).  Same gradients as with the launch of its own (MMFS_PREPARE_IN_TAPS=0) and as the
    oracle's; repeated calls on recycled workspaces keep agreeing (the cursors ARE cleared)."""
    import MultiScaleDeformableAttention as MSDA
    x = make_inputs(2, 8, 128, 515, 4, [(64, 64), (32, 32), (16, 16), (8, 8)], seed=37, loc_range=(-0.1, 1.1), dtype=dtype)
    want = run_oracle(x)
    for setting in ("1", "0", "1"):
        monkeypatch.setenv("MMFS_PREPARE_IN_TAPS", setting)
        for _ in range(3):
            check(run_hip(x, dtype, use_autograd=False, register=True), want, x, dtype, f"plan in taps = {setting}")
    # heads of 64 channels: the dense-levels kernel (csrc/msda_dense.hip) is the host
    x = make_inputs(2, 4, 64, 300, 8, [(32, 32), (16, 16), (8, 8)] * 2, seed=41, loc_range=(-0.1, 1.1), dtype=dtype)
    want = run_oracle(x)
    for setting in ("1", "0", "1"):
        monkeypatch.setenv("MMFS_PREPARE_IN_TAPS", setting)
        for _ in range(2):
            check(run_hip(x, dtype, use_autograd=False, register=True), want, x, dtype, f"plan in dense taps = {setting}")


# ---------------------------------------------------------------------------------------------------------
# The forward's fourth formulation (csrc/msda_fwd_wq.hip, round 5): a wave per query; a sample's four pixel rows -- one
# wave-wide load from memory or from the LDS image -- are the B operand of ONE matrix-core product whose A operand carries
# the four bilinear weights on a diagonal.  Heads of 128 channels, 16-bit storage; the default at the north-star shape.
WAVE_CASES = [
    # B, H, D, Nq, P, shapes                                           what it exercises
    (1, 8, 128, 64, 4, [(64, 64), (32, 32), (16, 16), (8, 8)]),         # the north-star pyramid: two levels resident, K = 16
    (1, 8, 128, 700, 4, [(64, 64), (32, 32), (16, 16), (8, 8)]),        # three runs of queries per slab, the last ragged
    (2, 3, 128, 333, 4, [(16, 16), (8, 8), (20, 20), (5, 7)]),          # every level resident, ragged run, H not a power of two
    (1, 2, 128, 70, 3, [(9, 5), (40, 40), (3, 3), (1, 1), (2, 9)]),     # K = 15: a ragged chunk; tails of the batches of four
    (1, 4, 128, 50, 4, [(70, 70), (50, 50)]),                           # nothing fits: every product's rows from memory
    (3, 8, 128, 1, 4, [(16, 16), (8, 8)]),                              # one query (decode)
    (1, 2, 128, 90, 8, [(64, 64), (32, 32), (16, 16), (8, 8)]),         # K = 32: two chunks per query, the sums carried across
    (1, 2, 128, 40, 2, [(3, 3)] * 60),                                  # L = 60, K = 120: eight chunks, everything resident
    (1, 2, 128, 33, 5, [(32, 32), (16, 16), (8, 8)] * 4),               # 12 levels, K = 60: three full chunks and a ragged one; some levels resident
    (2, 1, 128, 5000, 4, [(24, 24), (12, 12), (6, 6)]),                 # many runs per slab
]


@pytest.mark.parametrize("case", WAVE_CASES, ids=[f"B{c[0]}H{c[1]}D{c[2]}Nq{c[3]}P{c[4]}L{len(c[5])}" for c in WAVE_CASES])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_query_wave_forward_matches_oracle(case, dtype):
    B, H, D, Nq, P, shapes = case
    x = make_inputs(B, H, D, Nq, P, shapes, seed=23, loc_range=(-0.15, 1.15), dtype=dtype)
    x["loc"][0, 0, 0, 0, 0, 0] = float("nan")            # non-finite locations contribute nothing
    x["loc"][0, Nq // 2, 1 % H, -1, 0, 1] = float("inf")
    x["attn"][0, Nq - 1, 0, -1] = 0.0                     # zero weights read nothing
    x["loc"][0, Nq // 3, 0, 0, -1] = torch.tensor([0.0, 1.0])            # a corner of the map: three of four corners outside
    want = msda_oracle.forward(x["value"], x["shapes"], x["start"], x["loc"], x["attn"])
    got = run_fwd(x, dtype, "waves")
    scale = max(1.0, float(np.abs(want).max()))
    assert max_abs(got, want) <= TOL[dtype] * scale, f"{case[:5]}: {max_abs(got, want):.3e}"
    # and against the row-gather kernel: fp32 sums in another order, the weights as hi + lo 16-bit parts
    ref = run_fwd(x, dtype, "gather")
    assert max_abs(got, ref) <= 0.5 * TOL[dtype] * scale


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_query_wave_forward_non_finite_values_stay_in_their_channel(dtype):
    """The product's zero weights multiply the other channels of a sampled row (0 x Inf = NaN inside the 8-channel group of
    a lane).  The kernel tests every query's sums and recomputes a query with a non-finite one channel by channel
    (wq::exact_query): element for element the reference's result (cuh:58-81, :275-299) -- an Inf / NaN in ONE channel
    of a row reaches that channel of the queries that sample the row with a valid corner, nothing else."""
    _non_finite_element_case(dtype, 128, "waves")


@pytest.mark.parametrize("D", [64, 128])
def test_lds_levels_forward_non_finite_elements_match_the_reference(D):
    """The same element-level case through the LDS-resident formulation (one product per query: msda_fwd_mma.hip)."""
    _non_finite_element_case(torch.bfloat16, D, "lds")


def test_query_wave_forward_is_the_default_at_the_north_star_shape():
    llm = [(64, 64), (32, 32), (16, 16), (8, 8)]
    x = make_inputs(8, 8, 128, 1024, 4, llm, seed=5, loc_range=(-0.1, 1.1), dtype=torch.bfloat16)    # (runs of 128 queries: 512 of them)
    assert max_abs(run_fwd(x, torch.bfloat16, "auto"), run_fwd(x, torch.bfloat16, "waves")) == 0.0
    x = make_inputs(8, 8, 128, 256, 4, llm, seed=5, loc_range=(-0.1, 1.1), dtype=torch.bfloat16)     # 256 runs of 64: the row gather
    assert max_abs(run_fwd(x, torch.bfloat16, "auto"), run_fwd(x, torch.bfloat16, "gather")) == 0.0


@pytest.mark.parametrize("algo", ["waves", "lds", "slices", "gather"])
def test_forward_formulations_take_locations_that_start_on_an_odd_element(algo):
    """``sampling_loc`` / ``attn_weight`` as views that start one 16-bit element into their storage (a slice of a larger
    buffer: contiguous, 2-byte aligned, NOT 4-byte aligned): the kernels read an (x, y) pair as one 4-byte word only when the
    base allows it (``pair_ok``), else as two halfwords -- the same results either way."""
    import MultiScaleDeformableAttention as MSDA
    B, H, D, Nq, P, shapes = 1, 4, 128, 300, 4, [(40, 40), (16, 16), (8, 8), (5, 3)]
    x = make_inputs(B, H, D, Nq, P, shapes, seed=31, loc_range=(-0.1, 1.1), dtype=torch.bfloat16)
    dev = lambda t: t.to(DEV, torch.bfloat16) if t.is_floating_point() else t.to(DEV)
    value, sh, st, loc, attn = (dev(x[k]) for k in ("value", "shapes", "start", "loc", "attn"))

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 4 == 2
        return v

    old = MSDA._fwd_algo
    MSDA._fwd_algo = algo
    try:
        a = MSDA.ms_deform_attn_forward(value, sh, st, loc, attn, 1)
        b = MSDA.ms_deform_attn_forward(value, sh, st, shifted(loc), shifted(attn), 1)
        torch.cuda.synchronize()
    finally:
        MSDA._fwd_algo = old
    assert torch.equal(a, b)
    want = msda_oracle.forward(x["value"], x["shapes"], x["start"], x["loc"], x["attn"])
    assert max_abs(a.double().cpu().numpy(), want) <= TOL[torch.bfloat16]


WALKS = [
    # dtype, D: lanes per query = D * element size / 16; a chunk holds 2 * lanes samples per query
    (torch.float32, 16, "4 lanes: the 8 samples are one chunk of the pipelined walk"),
    (torch.bfloat16, 32, "4 lanes, 16-bit rows"),
    (torch.float32, 256, "64 lanes: the walk without live words, a wave per query"),
    (torch.bfloat16, 8, "1 lane: chunks of 2 samples, four per query"),
]


@pytest.mark.parametrize("live", [0, 1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("dtype,D,what", WALKS, ids=[f"{str(w[0])[6:]}-D{w[1]}" for w in WALKS])
def test_row_gather_walks_at_their_smallest(dtype, D, what, live):
    """The row gather's walks over a chunk's tap records at the shapes where each branch is alone: three queries (a ragged
    tile) of 8 samples each, of which the first ``live`` weigh something -- the other weights are exactly 0, so their taps
    are not walked: no live tap at all, the odd prologue alone (1), the pair without the loop (2, 3), one loop trip (4, 5),
    every tap (8).  The middle query weighs nothing at all: with 64 lanes per query it is a wave that skips every pair.
    Against the oracle under the per-element bound."""
    x = make_inputs(1, 1, D, 3, 4, [(3, 5), (2, 2)], seed=41, loc_range=(0.1, 0.9), dtype=dtype)
    keep = torch.zeros(1, 3, 1, 8, dtype=torch.float64)
    keep[..., :live] = 1.0
    keep[:, 1] = 0.0
    x["attn"] = x["attn"] * keep.reshape(1, 3, 1, 2, 4)
    got = run_fwd(x, dtype, "gather")
    assert_within_bounds([got, None, None, None], x, dtype, f"{what}, {live} live", outputs=("out",))
    assert not got[0, 1].any() and (live == 0) == (not got.any())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,code", [(torch.float32, 0), (torch.float16, 1), (torch.bfloat16, 2)])
def test_cast_from_f32_entry_point(dtype, code):
    """``mmfs_msda_cast_from_f32`` (the float-atomic path's closing pass, ms_deform_attn_cuda.cu:156-165): fp32 -> storage type,
    any length, bit for bit the framework's rounding; for fp32 storage a copy -- issued as a kernel, like every clear and copy
    on a launch path since round 5 (a memset / memcpy NODE of a recorded graph does not order like a kernel: DESIGN 4.8c)."""
    import ctypes
    import MultiScaleDeformableAttention as MSDA
    g = torch.Generator().manual_seed(3)
    for n in (1, 7, 4096, 100003):
        src = (torch.randn(n, generator=g) * 37.0).to("cuda")
        dst = torch.full((n + 5,), 123.0, device="cuda", dtype=dtype)
        rc = MSDA._lib.mmfs_msda_cast_from_f32(code, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), n,
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        assert torch.equal(dst[:n], src.to(dtype)) and bool((dst[n:] == 123.0).all())
