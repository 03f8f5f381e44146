"""GPU: the routes that only an environment knob reaches (csrc/msda_env.hip lists the knobs), one case per knob value, at
the smallest shape at which the knob changes what is launched -- every output against the oracle under the per-element
bound of tests/helpers.py, and bit for bit against the default where the knob only regroups work.

Which kernel a knob selects is not visible from Python (``MSDA._event_log`` holds the shim's stage names, not kernel
names): a case confirms the change through the library's host-only queries where one answers it (MMFS_TAPS_ALGO,
MMFS_HYBRID, MMFS_DOT_CHUNKS), through ``route_counts`` (the sorted route), through results that differ in some bit where
the arithmetic differs (the ``*_LDS_KB`` knobs, MMFS_FWD_ALGO), and otherwise rests on the shape: each case's comment
derives, from the launcher's code, that the default and the knob launch different things there.

The last test (no GPU) walks ``mmfs_env_knob`` and fails for a knob no file under tests/ names."""
import ctypes
import glob
import os

import pytest
import torch

from helpers import OUTPUTS, assert_bit_equal, assert_within_bounds, bound_library, make_inputs

DEV = "cuda"
gpu = pytest.mark.gpu
SHAPES = [(5, 7), (2, 3)]            # two levels, neither a multiple of the 4x4 block; 41 pixels


def run_op(monkeypatch, x, dtype, fwd="auto", taps="auto", hybrid=True, prefer_sorted=False, register=True, backward=True, log=None):
    """-> [out, grad_value, grad_loc, grad_attn] (device tensors; the gradients None without ``backward``) of the shim's
    forward and backward on ``x`` with the shim's own switches as given and the level table registered; ``log``: a list that
    gets the shim's stage names (one launch per stage then)."""
    import MultiScaleDeformableAttention as MSDA
    dev = lambda t: t.to(DEV, dtype) if t.is_floating_point() else t.to(DEV)
    value, sh, st, loc, attn = (dev(x[k]) for k in ("value", "shapes", "start", "loc", "attn"))
    if register:
        MSDA.register_level_tables(sh, st, value.shape[1], host_shapes=x["shapes"], host_start=x["start"])
    with monkeypatch.context() as m:
        for k, v in (("_fwd_algo", fwd), ("_taps_algo", taps), ("_hybrid", hybrid), ("_taps_prefer_sorted", prefer_sorted),
                     ("_ws_cache", {}), ("_event_log", None if log is None else [])):
            m.setattr(MSDA, k, v)                          # (_ws_cache: the workspace sizes depend on the knobs, nothing memoised)
        out = MSDA.ms_deform_attn_forward(value, sh, st, loc, attn, 1)
        grads = [None] * 3
        if backward:
            grads = MSDA.ms_deform_attn_backward(value, sh, st, loc, attn, dev(x["grad"]).reshape(out.shape), 1)
        torch.cuda.synchronize()
        if log is not None:
            log.extend(n for n, _, _ in MSDA._event_log)
    return [out, *grads]


# grad_value comes from the cell sort, whose record order -- hence a pixel's fp32 sum -- is not fixed from run to run once a
# slice's samples span several waves (more than 64 queries: tests/test_stress_gpu.py): its bits are compared at smaller shapes only
NOT_GRAD_VALUE = ("out", "grad_loc", "grad_attn")


def held(got, x, dtype, what):
    outputs = tuple(n for n, g in zip(OUTPUTS, got) if g is not None)
    res = assert_within_bounds([None if g is None else g.double().cpu().numpy() for g in got], x, dtype, what, outputs=outputs)
    print(f"BOUND knob {what}: " + " ".join(f"{n}={r[0]:.3g}" for n, r in res.items()))


def same_bits(a, b, what, names=OUTPUTS):
    for n, p, q in zip(OUTPUTS, a, b):
        if n in names and p is not None:
            assert_bit_equal(p, q, f"{what}: {n}")


def some_bit_differs(a, b):
    return any(p is not None and not torch.equal(p, q) for p, q in zip(a, b))


def with_knobs(monkeypatch, knobs, fn):
    with monkeypatch.context() as m:
        for k, v in knobs.items():
            m.setenv(k, v)
        return fn()


# ---------------------------------------------------------------------------------------------------- the forwards
# Queries per run (msda_mma_common.h ``pick_queries_per_run``, msda_fwd_q8.hip ``launch_q8``): with 2 (b, h) slabs the default
# halves 256 down to its floor -- 64 queries for msda_fwd_mma / msda_fwd_wq (units of 16 waves x 4 queries), 128 for
# msda_fwd_q8 (16 waves x 8) -- so 150 queries are runs of 64 + 64 + 22 (q8: 128 + 22) by default and 128 + 22 (q8: one run
# of 256) under the knob.  "queries per run" (msda_env.hip) regroups queries; a query's sums are its own: not a bit changes.
RUN_KNOBS = [("MMFS_FWD_MMA_QPW", "128", "lds", 128), ("MMFS_FWD_WQ_QPW", "128", "waves", 128), ("MMFS_FWD_Q8_QPR", "256", "slices", 64),
             ("MMFS_FWD_MMA_QPW", "128", "lds", 64)]


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("knob,value,algo,D", RUN_KNOBS, ids=[f"{k[0]}={k[1]}-D{k[3]}" for k in RUN_KNOBS])
def test_forward_queries_per_run_regroup_and_change_no_bit(knob, value, algo, D, dtype, monkeypatch):
    x = make_inputs(1, 2, D, 150, 4, SHAPES, seed=71, loc_range=(-0.1, 1.1), dtype=dtype)
    default = run_op(monkeypatch, x, dtype, fwd=algo, backward=False)
    got = with_knobs(monkeypatch, {knob: value}, lambda: run_op(monkeypatch, x, dtype, fwd=algo, backward=False))
    held(got, x, dtype, f"{knob}={value} {algo}")
    same_bits(got, default, f"{knob}={value} against the default run length")


# LDS budgets (msda_mma_common.h ``lds_bytes``: at least 1 KiB of image): which levels are resident is decided on the device
# from the LDS the launch got.  A row of the image is D * 2 + 32 = 288 bytes: the 16x16 level (>= 72 KiB) is resident by
# default (160 KiB) and not under 48; under 1 (clamped to the tables + 1 KiB) not even the 5x7 level (>= 9.8 KiB) is.  A level
# moved to the row gather is sampled by msda_fwd_mma with fp32 weights, not hi + lo 16-bit parts: held by the bound, and some bit
# differs.  msda_fwd_wq multiplies a gathered row by the same weights as a resident one (msda_fwd_wq.hip, header: "the same
# product with the B operand read by ds_read_b128"), but a query's samples are chained in another ORDER once a level moves:
# its live row-gather samples are taken from the bottom of the chunk's records and its live LDS samples from the top
# (msda_fwd_wq.hip, "records of a query").  So the fp32 chain may round differently -- or, at a shape like this one, not in any
# bit that survives the rounding to bf16: neither equality nor a difference is asserted for it, the bound alone.
LDS_SHAPES = [(16, 16), (5, 7), (2, 3)]


@gpu
@pytest.mark.parametrize("kb", ["1", "48"])
@pytest.mark.parametrize("knob,algo", [("MMFS_FWD_MMA_LDS_KB", "lds"), ("MMFS_FWD_WQ_LDS_KB", "waves")])
def test_forward_with_less_lds_moves_levels_to_the_row_gather(knob, algo, kb, monkeypatch):
    dtype = torch.bfloat16
    x = make_inputs(1, 2, 128, 150, 4, LDS_SHAPES, seed=72, loc_range=(-0.1, 1.1), dtype=dtype)
    default = run_op(monkeypatch, x, dtype, fwd=algo, backward=False)
    got = with_knobs(monkeypatch, {knob: kb}, lambda: run_op(monkeypatch, x, dtype, fwd=algo, backward=False))
    held(got, x, dtype, f"{knob}={kb}")
    held(default, x, dtype, f"{algo} with the whole CU's LDS")
    if algo == "lds":
        assert some_bit_differs(got, default), f"{knob}={kb}: bit-equal to the default -- the levels were still resident?"


# MMFS_FWD_ALGO names the formulation wherever it is supported (msda_fwd_mma.hip / _q8 / _wq ``*_applies``): under "auto" it is
# the kernel the shim's flag names, bit for bit; the default at this shape (600 samples per slab) is the row gather.
@gpu
@pytest.mark.parametrize("value,algo", [("vec", "gather"), ("mma", "lds"), ("q8", "slices"), ("wq", "waves")])
def test_forward_algo_knob_selects_the_named_formulation(value, algo, monkeypatch):
    dtype = torch.bfloat16
    x = make_inputs(1, 2, 128, 150, 4, SHAPES, seed=73, loc_range=(-0.1, 1.1), dtype=dtype)
    named = run_op(monkeypatch, x, dtype, fwd=algo, backward=False)
    got = with_knobs(monkeypatch, {"MMFS_FWD_ALGO": value}, lambda: run_op(monkeypatch, x, dtype, backward=False))
    held(got, x, dtype, f"MMFS_FWD_ALGO={value}")
    same_bits(got, named, f"MMFS_FWD_ALGO={value} against the shim's '{algo}'")
    if value != "vec":
        gather = run_op(monkeypatch, x, dtype, fwd="gather", backward=False)
        assert some_bit_differs(got, gather), f"MMFS_FWD_ALGO={value}: the row gather's bits"


# ---------------------------------------------------------------------------------------------------- grad_loc / grad_attn
def bwd_dims(x, D):
    B, S, H = x["value"].shape[:3]
    Nq, L, P = x["loc"].shape[1], x["loc"].shape[3], x["loc"].shape[4]
    return (B, S, H, D, L, Nq, P)


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=lambda d: str(d)[6:])
def test_taps_queries_per_run_regroup_and_change_no_bit(dtype, monkeypatch):
    """msda_taps_mma.hip ``launch``: ``pick_queries_per_run`` as for the forwards (runs of 64 by default here, 128 under
    MMFS_TAPS_MMA_QPW=128).  A query's gradients are its own; grad_value does not come from this kernel."""
    x = make_inputs(1, 2, 128, 150, 4, SHAPES, seed=74, loc_range=(-0.1, 1.1), dtype=dtype)
    default = run_op(monkeypatch, x, dtype, taps="lds")
    got = with_knobs(monkeypatch, {"MMFS_TAPS_MMA_QPW": "128"}, lambda: run_op(monkeypatch, x, dtype, taps="lds"))
    held(got, x, dtype, "MMFS_TAPS_MMA_QPW=128")
    same_bits(got, default, "MMFS_TAPS_MMA_QPW=128 against the default run length", names=NOT_GRAD_VALUE)


@gpu
@pytest.mark.parametrize("value,algo", [("vec", "gather"), ("mma", "lds")])
def test_taps_algo_knob_selects_the_named_kernel(value, algo, monkeypatch):
    """MMFS_TAPS_ALGO (msda_taps_mma.hip ``taps_mma_applies``): "mma" takes the LDS-levels kernel wherever the shape allows --
    heads of 64 channels are opt-in, so the default does not -- and "vec" never does; either one refuses
    mmfs_msda_backward_sorted (msda_bwd_block.hip ``taps_sorted_supported``).  The library's host-only queries say so, and
    the gradients are the bits of the kernel the shim's flag names."""
    import MultiScaleDeformableAttention as MSDA
    dtype, D = torch.bfloat16, 64
    x = make_inputs(1, 2, D, 150, 4, SHAPES, seed=75, loc_range=(-0.1, 1.1), dtype=dtype)
    dims, canonical = bwd_dims(x, D), MSDA._BWD_CANONICAL_LEVELS
    L = MSDA._lib
    assert L.mmfs_msda_backward_taps_fused(2, *dims, canonical) == 0
    assert L.mmfs_msda_backward_sorted_workspace_bytes(2, *dims, canonical) > 0
    named = run_op(monkeypatch, x, dtype, taps=algo, hybrid=False)

    def under_the_knob():
        assert L.mmfs_msda_backward_taps_fused(2, *dims, canonical) == (1 if value == "mma" else 0)
        assert L.mmfs_msda_backward_sorted_workspace_bytes(2, *dims, canonical) == 0
        return run_op(monkeypatch, x, dtype, hybrid=False)
    got = with_knobs(monkeypatch, {"MMFS_TAPS_ALGO": value}, under_the_knob)
    held(got, x, dtype, f"MMFS_TAPS_ALGO={value}")
    same_bits(got, named, f"MMFS_TAPS_ALGO={value} against the shim's '{algo}'", names=NOT_GRAD_VALUE)


def hybrid_bytes(x, D, dense=True):
    import MultiScaleDeformableAttention as MSDA
    sh = x["shapes"].numpy().astype("int64").copy()
    st = x["start"].numpy().astype("int64").copy()
    flags = MSDA._BWD_CANONICAL_LEVELS | (MSDA._BWD_DENSE_TAPS if dense else 0)
    return MSDA._lib.mmfs_msda_backward_hybrid_workspace_bytes(2, sh.ctypes.data, st.ctypes.data, *bwd_dims(x, D), flags)


@gpu
def test_dense_taps_of_a_level_of_several_chunks(monkeypatch):
    """MMFS_DOT_CHUNKS=1 (msda_dense.hip ``make_dense_plan``): a level of more than 256 pixels -- 24x24 = 576 <= 190 * P -- is
    walked as chunks of whole rows by the dense product; by default such a level goes to the row gather, and with no other
    level the hybrid route has nothing dense and refuses (0 bytes): the knob is what makes it apply, and the shim's stage
    log shows the dense stage.  (264 samples rounded to bf16: the two kernels' results need not differ in any bit.)"""
    dtype, D = torch.bfloat16, 32
    x = make_inputs(1, 2, D, 33, 4, [(24, 24)], seed=76, loc_range=(-0.1, 1.1), dtype=dtype)
    assert hybrid_bytes(x, D) == 0
    stages = []
    default = run_op(monkeypatch, x, dtype, log=stages)
    assert "msda_bwd_taps_coarse" not in stages and "msda_bwd_taps" in stages, stages
    held(default, x, dtype, "24x24 by the row gather")

    def under_the_knob():
        assert hybrid_bytes(x, D) > 0
        return run_op(monkeypatch, x, dtype, log=stages)
    del stages[:]
    got = with_knobs(monkeypatch, {"MMFS_DOT_CHUNKS": "1"}, under_the_knob)
    assert "msda_bwd_taps_coarse" in stages, stages
    held(got, x, dtype, "MMFS_DOT_CHUNKS=1")


@gpu
def test_hybrid_knob_off_in_the_library_is_the_shims_switch(monkeypatch):
    """MMFS_HYBRID=0 read by the library (msda_dense.hip ``make_dense_plan``): no dense level, so the hybrid route refuses
    (0 bytes) and the shim takes the library's own sequence -- the bits of ``MSDA._hybrid = False``."""
    dtype, D = torch.bfloat16, 32
    x = make_inputs(1, 2, D, 33, 4, SHAPES, seed=77, loc_range=(-0.1, 1.1), dtype=dtype)
    assert hybrid_bytes(x, D) > 0
    off = run_op(monkeypatch, x, dtype, hybrid=False)

    def under_the_knob():
        assert hybrid_bytes(x, D) == 0
        return run_op(monkeypatch, x, dtype, hybrid=True)
    got = with_knobs(monkeypatch, {"MMFS_HYBRID": "0"}, under_the_knob)
    held(got, x, dtype, "MMFS_HYBRID=0")
    same_bits(got, off, "MMFS_HYBRID=0 against MSDA._hybrid = False")


# ---------------------------------------------------------------------------------------------------- the cell sort
@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=lambda d: str(d)[6:])
def test_sort_repack_knob_takes_the_branch_of_a_misaligned_loc(dtype, monkeypatch):
    """MMFS_SORT_REPACK=1 (msda_bwd_block.hip ``sort_reads_in_place``): loc / attn are re-packed level-major into the workspace
    before the sort although it could read them in place.  The re-packed copy holds the same numbers and the sort makes the
    same records in the same order from either (tests/test_placement_gpu.py holds that on element-aligned operands too):
    every output bit-equal to the default."""
    x = make_inputs(1, 2, 32, 33, 4, SHAPES, seed=78, loc_range=(-0.1, 1.1), dtype=dtype)
    default = run_op(monkeypatch, x, dtype)
    got = with_knobs(monkeypatch, {"MMFS_SORT_REPACK": "1"}, lambda: run_op(monkeypatch, x, dtype))
    held(got, x, dtype, "MMFS_SORT_REPACK=1")
    same_bits(got, default, "MMFS_SORT_REPACK=1 against reading in place", names=("out", "grad_loc", "grad_attn"))
    same_bits(got, default, "MMFS_SORT_REPACK=1 against reading in place", names=("grad_value",))


@gpu
@pytest.mark.parametrize("hgroup", ["1", "2", "4", "0"])
def test_sort_head_groups_regroup_and_change_no_bit(hgroup, monkeypatch):
    """MMFS_SORT_HGROUP (msda_bwd_block.hip ``launch_sort``): heads whose workgroups share an XCD -- which workgroup index
    sorts which (b, h) slice, nothing a slice's records see ("heads that share a workgroup's sector reads").  L * P * 2 = 16
    bytes of attn per head: the default is groups of 4 (H = 4), so 1 and 2 launch another grid and 4 the same."""
    dtype = torch.bfloat16
    x = make_inputs(3, 4, 32, 33, 4, SHAPES, seed=79, loc_range=(-0.1, 1.1), dtype=dtype)
    default = run_op(monkeypatch, x, dtype)
    got = with_knobs(monkeypatch, {"MMFS_SORT_HGROUP": hgroup}, lambda: run_op(monkeypatch, x, dtype))
    held(got, x, dtype, f"MMFS_SORT_HGROUP={hgroup}")
    same_bits(got, default, f"MMFS_SORT_HGROUP={hgroup} against groups of 4")


@gpu
@pytest.mark.parametrize("wide,P,dtype", [("0", 8, torch.float16), ("0", 8, torch.bfloat16), ("2", 4, torch.bfloat16), ("2", 4, torch.float16)])
def test_sort_wide_knob_moves_queries_between_the_512_and_1024_lane_sorts(wide, P, dtype, monkeypatch):
    """MMFS_SORT_WIDE (msda_bwd_block.hip ``launch_sort``): two-vector queries (P = 8 of 16-bit storage) sort on 512 lanes with
    eight samples each by default and on the 1024-lane kernel under "0"; one-vector queries (P = 4) on 1024 lanes by default
    and on 512 under "2" -- with fewer than 512 slices (``sort_lanes``: 1024 lanes) and compact records, as here.  The order of
    a cell's records may differ, so grad_value is held by the bound; grad_loc / grad_attn do not come from the sort."""
    x = make_inputs(1, 2, 32, 133, P, SHAPES, seed=80, loc_range=(-0.1, 1.1), dtype=dtype)
    default = run_op(monkeypatch, x, dtype)
    got = with_knobs(monkeypatch, {"MMFS_SORT_WIDE": wide}, lambda: run_op(monkeypatch, x, dtype))
    held(got, x, dtype, f"MMFS_SORT_WIDE={wide} P={P}")
    same_bits(got, default, f"MMFS_SORT_WIDE={wide}", names=("out", "grad_loc", "grad_attn"))


# More records than the largest window (msda_bwd_block.hip ``sort_window_bytes``): 2100 queries x 8 points are 16800 records of
# 8 bytes per level of a slice, 134400 > 128 KiB, with MMFS_NT_MIN=1 keeping each level ONE tile (4 slices would otherwise be
# cut into 32 bands a level).  Default: the kept scan places them in two window rounds.  MMFS_SORT_ROUNDS=0: no window at all
# -- the sort no longer keeps its samples, loc / attn are re-packed, and the records go out through cursors and scattered
# stores (the "direct" path of test_op_gpu.py's SORT_ROUTES, reached there through MMFS_SORT_WINDOW_KB=0).
ROUNDS_SHAPE = dict(B=1, H=2, D=32, Nq=2100, P=8)


def rounds_inputs(dtype):
    s = ROUNDS_SHAPE
    x = make_inputs(s["B"], s["H"], s["D"], s["Nq"], s["P"], SHAPES, seed=81, loc_range=(-0.1, 1.1), dtype=dtype)
    x["attn"][:, ::7, :, 1] = 0.0                               # zero weights leave no record
    return x


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=lambda d: str(d)[6:])
def test_sort_without_window_rounds(dtype, monkeypatch):
    x = rounds_inputs(dtype)
    default = with_knobs(monkeypatch, {"MMFS_NT_MIN": "1"}, lambda: run_op(monkeypatch, x, dtype))
    held(default, x, dtype, "two window rounds")
    got = with_knobs(monkeypatch, {"MMFS_NT_MIN": "1", "MMFS_SORT_ROUNDS": "0"}, lambda: run_op(monkeypatch, x, dtype))
    held(got, x, dtype, "MMFS_SORT_ROUNDS=0")
    same_bits(got, default, "MMFS_SORT_ROUNDS=0", names=("out", "grad_loc", "grad_attn"))


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=lambda d: str(d)[6:])
def test_sort_without_window_rounds_on_the_sorted_taps_route(dtype, monkeypatch):
    """The combination ADVICE.md's fourth finding is about: with grad_loc / grad_attn taken from the sort's records
    (``_taps_prefer_sorted`` on a registered table) the window never falls below a tile's cells + 16 bytes, so
    MMFS_SORT_ROUNDS=0 does not give the direct path but the kept scan over a 20 KiB window -- 2560 records a round, seven
    rounds for a level's 16800.  Whatever it launches, the four outputs are the oracle's; and the route did run."""
    import MultiScaleDeformableAttention as MSDA
    x = rounds_inputs(dtype)
    before = MSDA.route_counts["sorted"]
    got = with_knobs(monkeypatch, {"MMFS_NT_MIN": "1", "MMFS_SORT_ROUNDS": "0"},
                     lambda: run_op(monkeypatch, x, dtype, prefer_sorted=True))
    assert MSDA.route_counts["sorted"] == before + 1, "the sorted route refused: nothing was tested"
    held(got, x, dtype, "MMFS_SORT_ROUNDS=0, sorted taps")
    default = with_knobs(monkeypatch, {"MMFS_NT_MIN": "1"}, lambda: run_op(monkeypatch, x, dtype, prefer_sorted=True))
    assert MSDA.route_counts["sorted"] == before + 2
    held(default, x, dtype, "two window rounds, sorted taps")


# ---------------------------------------------------------------------------------------------------- query prep
@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=lambda d: str(d)[6:])
def test_query_prep_with_a_smaller_tile(dtype, monkeypatch):
    """MMFS_QUERY_LDS_KB (csrc/mmfs_query.hip ``query_tile_shift``): pixels per tile.  The (2, 64, 5, 8) layout shape is one
    ragged tile of 64 pixels by default (40 pixels); a budget of 4 KiB leaves 16 pixels a tile (32 x (64 + pad) x 2 bytes is
    over): three tiles, the last half full.  A token's statistics and output are its own: against fp64 under the bound of
    front_end_refs.py, and the default's bits."""
    import front_end_refs as R
    from front_end_refs import worst
    from test_front_end_gpu import CODE, query_case, stream
    import MultiScaleDeformableAttention as MSDA
    L, eps, shape = MSDA._lib, 1e-6, (2, 64, 5, 8)
    B, C, H, W = shape
    HW = H * W
    x, w, b, pos = query_case(dtype, shape, 43)

    def run():
        q = torch.full((B, HW, C), float("nan"), device=DEV, dtype=dtype)
        mean, rstd = (torch.full((B, HW), float("nan"), device=DEV, dtype=torch.float32) for _ in range(2))
        assert L.mmfs_query_prep(CODE[dtype], x.data_ptr(), w.data_ptr(), b.data_ptr(), pos.data_ptr(), q.data_ptr(), mean.data_ptr(),
                                 rstd.data_ptr(), B, C, HW, eps, stream()) == 0
        torch.cuda.synchronize()
        return q, mean, rstd
    default = run()
    got = with_knobs(monkeypatch, {"MMFS_QUERY_LDS_KB": "4"}, run)
    f = R.layer_norm_tokens64(x, w, b, pos, eps, dtype)
    fb = R.layer_norm_tokens_bounds(f, dtype, C, eps)
    for name, t, d in zip(("q", "mean", "rstd"), got, default):
        ratio = worst(t, f[name], fb[name])
        print(f"BOUND knob MMFS_QUERY_LDS_KB=4 {name}: {ratio[0]:.3g}")
        assert ratio[0] <= 1.0, f"MMFS_QUERY_LDS_KB=4 {name}: bound broken (ratio, index, got, ref, bound): {ratio}"
        assert_bit_equal(t, d, f"MMFS_QUERY_LDS_KB=4 {name} against the default tile")


# ---------------------------------------------------------------------------------------------------- every knob has a case
def test_every_knob_is_named_by_a_test():
    """Walks ``mmfs_env_knob`` (the library loads without a GPU): every knob of csrc/msda_env.hip appears, by name, in at least
    one file under tests/ -- a knob added without a case fails here."""
    lib = bound_library()
    here = os.path.dirname(os.path.abspath(__file__))
    text = "\n".join(open(p).read() for p in sorted(glob.glob(os.path.join(here, "*.py"))))
    names, k = [], 0
    while True:
        name = ctypes.c_char_p()
        if lib.mmfs_env_knob(k, ctypes.byref(name), None, None) != 0:
            break
        names.append(name.value.decode())
        k += 1
    assert len(names) >= 30 and len(set(names)) == len(names)
    import re
    missing = [n for n in names if not re.search(r"\b%s\b" % n, text)]
    assert not missing, f"knobs of csrc/msda_env.hip that no file under tests/ names: {missing}"
