"""Level tables at the edges of the branches the kernels take on a level's extent, through every forward kernel and every
backward route that takes them, against the fp64 oracle with the per-element bound of tests/helpers.py:

  * empty levels (H * W == 0: (0, W), (H, 0), (0, 0)) first, in the middle, last (start index == S), two side by side,
    a table with one level that has pixels -- the oracle gives their samples exactly 0 (grad_loc, grad_attn) and the
    forward of the table without them;
  * one-pixel strips and the sort tiles' edge: kMaxTileCells = 5120 cells of (H + 1)(W + 1) (csrc/msda_bwd_block.h),
    the strip branch Wc > 5120;
  * the older grad_value tiles' 4096 pixels (kMaxTilePx), the dense grad_loc levels' 256 pixels / 128 columns;
  * the LDS image of the matrix-core forwards: a pyramid whose resident set ends exactly at the image budget of the
    query-wave kernel at D = 128, then one row over; and rows of 1024 / 1025 pixels.  (Those rows do NOT decide the side
    limit of build_level_table, Hl <= 1024 && Wl <= 1024: a one-pixel-high row of 1024 pixels already exceeds every
    kernel's byte budget -- 256 KiB against the query-wave image's 105 KiB at D = 128; 96 / 160 / 288 KiB against the
    matrix-core image's ~26 / 92 / 125 KiB at D = 32 / 64 / 128 -- so both go to the row gather for the byte count.  The
    sliced kernel's side limit is 2048 and its byte budget is smaller still.  At these head widths the side limit never
    decides; the rows test the "does not fit" path of a long level.)

Every allocation of the op is poisoned (helpers.poison_allocations): an output element no kernel writes is NaN and breaks
the bound, instead of passing on the answer the previous identical call left in a recycled block.  Each table's routes
run twice -- one call (what users run) and staged under MSDA._event_log (what bench.py and the log-driven tests run).

Which backward route ran is read off the library entry point the shim called (counted by wrapping the ctypes functions)
and its flags -- mmfs_msda_backward_sorted, mmfs_msda_backward_hybrid, mmfs_msda_backward_checked (forced atomic /
device-checked / canonical: the library's own sequence), the staged mmfs_msda_backward_taps -- not off the knobs that
asked for it: a route the shim falls back from is recorded as what ran instead.  Which grad_value kernel
(MMFS_VALUE_ALGO tile / block / pixel) and which grad_loc kernel (taps gather / lds) runs INSIDE an entry point is the
library's choice and cannot be seen from the host: those routes are recorded by the entry point and the flags they
passed, and the numbers are checked, nothing more is claimed."""
import contextlib
import functools
import io
import os

import pytest
import torch

from helpers import OUTPUTS, bound_ratios, error_bounds, level_tables, make_inputs, poison_allocations

pytestmark = pytest.mark.gpu
DEV = "cuda"

# The query-wave forward's image budget at D = 128 (csrc/msda_fwd_wq.hip, launch_wq / wq::Image):
#   table   TAB_BYTES = round_up(kMmaMaxLevels 64 * kTabInts 6 * 4 + 64, 256)            =   1 792 bytes
#   waves   kMmaWaves 16 * kWaveRec (kGroup 4 * kQStride (4 batches * 208 bytes))          =  53 248
#   IMG0    round_up(1 792 + 53 248, 256) = 55 040;  budget = kLdsTotal 160 KiB - IMG0   = 108 800
# A level takes ceil(H * W * 256 bytes / 1 KiB) KiB and is resident (smallest first) while the running sum + the 1 KiB
# row of zeros <= 108 800, i.e. while the sum <= 105 KiB.  (4, 41) = 164 px = 41 KiB, then (16, 16) = 64 KiB: 105 KiB,
# both resident, the budget's last whole KiB used.  (17, 16) = 68 KiB: 109 KiB, the larger level goes to the row gather.
# The other three LDS-resident kernels' budgets: BUDGET_TABLES below, computed from their formulas.
TABLES = [
    # name                 shapes
    ("empty_first_0xW",    [(0, 7), (8, 8), (4, 4)]),
    ("empty_mid_Hx0",      [(8, 8), (5, 0), (4, 4)]),
    ("empty_last_0x0",     [(8, 8), (4, 4), (0, 0)]),                  # start index of the last level == S
    ("two_empty_adjacent", [(6, 6), (0, 3), (0, 0), (3, 5)]),
    ("one_level_has_px",   [(0, 4), (9, 7), (0, 0)]),
    ("px1_and_empty",      [(1, 1), (0, 2), (2, 1)]),
    ("strip_5120_cells",   [(1, 2559), (4, 4), (0, 5)]),               # (1 + 1)(2559 + 1) = 5120: one tile
    ("strip_5122_cells",   [(1, 2560), (0, 0), (2, 2)]),               # 5122: two tiles
    ("square_5041_cells",  [(70, 70), (0, 9)]),
    ("square_5184_cells",  [(71, 71), (3, 3)]),
    ("wide_3x5121",        [(3, 5121), (0, 1)]),                       # Wc = 5122 > 5120: the strip branch
    ("wide_4x20000",       [(4, 20000)]),
    ("tall_20000x4",       [(20000, 4), (0, 4)]),
    ("rect_37x1000",       [(37, 1000), (1000, 37)]),
    ("old_tile_4096px",    [(64, 64), (0, 6)]),
    ("old_tile_4160px",    [(64, 65), (2, 2)]),
    ("row_4097px",         [(1, 4097), (2, 3)]),
    ("dense_edges",        [(16, 16), (0, 16), (1, 128), (1, 129)]),   # 256 px; 128 vs 129 columns
    ("row_1024px",         [(1, 1024), (0, 0), (2, 2)]),               # (see the module's docstring: over every byte budget)
    ("row_1025px",         [(1, 1025), (2, 2)]),
    ("wq_budget_exact",    [(16, 16), (0, 3), (4, 41)]),
    ("wq_budget_over",     [(17, 16), (0, 3), (4, 41)]),
    # two levels of equal pixel count around an empty one: the lower index is placed first, the empty level takes no room
    # and is never resident.  Both fit every image; of the second pair one level alone fits the images at D = 128 (query
    # waves: 80 KiB each of 105; matrix cores: 95 232 and 93 440 bytes of 127 968 / 111 584)
    ("equal_px_both_fit",  [(6, 10), (0, 3), (10, 6)]),
    ("equal_px_one_fits",  [(16, 20), (0, 3), (20, 16)]),
]


# ---- the exact-budget boundary of the other LDS-resident kernels, from their own formulas (csrc/msda_mma_common.h,
# csrc/msda_fwd_q8.hip, csrc/msda_taps_mma.hip); kLdsTotal = 160 KiB, 16 waves, level table of 64 levels.
def _round_up(x, m):
    return (x + m - 1) // m * m


def _mma_image(D, extra):
    """(bytes of a level, largest admissible sum of the resident levels' bytes) of the matrix-core image at head width D:
    pixel rows RP = 2 D + 32 bytes apart, lines at line_pitch; wave-private bytes = the sample records (QPW queries x 33 x
    16 bytes) + ``extra``; a level is placed while sum + RP (the zero row) <= kLdsTotal - IMG0."""
    RP, QPW = 2 * D + 32, 64 // (2 * D // 16)
    img0 = _round_up(_round_up(64 * 6 * 4 + 64, 256) + 16 * (QPW * 33 * 16 + extra), 256)
    pitch = lambda W: W * RP + ((64 - W * RP % 256) & 255)
    return (lambda Hl, Wl: Hl * pitch(Wl)), 160 * 1024 - img0 - RP


def _q8_image():
    """The sliced forward's: Hl + 2 lines of line_pixels(Wl) pixels of 64 bytes; placed while kImg0 + sum <= kLdsTotal,
    kImg0 = round_up(table 64 * 8 * 4 + per-sample table 128 * 32 + 16 waves * 3072, 256)."""
    img0 = _round_up(64 * 8 * 4 + 128 * 32 + 16 * 3072, 256)
    line_pixels = lambda W: W + 2 + ((4 - (W & 3)) & 3)
    return (lambda Hl, Wl: (Hl + 2) * line_pixels(Wl) * 64), 160 * 1024 - img0


def _budget_pair(level_bytes, limit):
    """Two levels, the second with more pixels, whose bytes end as close under ``limit`` as two levels of this image can
    (exactly on it where the formula's granularity allows: asserted per kernel below), and the same pair with one more
    line of the larger level: over the limit.  -> (shapes that fit, shapes one line over, bytes left under the limit)"""
    best = None
    for h1 in (3, 4, 5):
        for w1 in range(3, 13):
            for w2 in range(13, 73):
                per_line = level_bytes(2, w2) - level_bytes(1, w2)                # (bytes are affine in the lines)
                h2 = 1 + (limit - level_bytes(h1, w1) - level_bytes(1, w2)) // per_line
                if not 13 <= h2 <= 72:
                    continue
                left = limit - level_bytes(h1, w1) - level_bytes(h2, w2)
                if best is None or left < best[0]:
                    best = (left, [(h2, w2), (0, 3), (h1, w1)], [(h2 + 1, w2), (0, 3), (h1, w1)])
    left, fits, over = best
    assert left >= 0 and limit - sum(level_bytes(h, w) for h, w in over if h * w) < 0
    return fits, over, left


# kernel (forced by fwd="lds" / "slices", taps="lds"), head width -> its image.  msda_taps_mma keeps the wave's grad_out
# rows (QPW * 2 D = 1024 bytes) besides the records.
_IMAGES = {"mma128": (128, _mma_image(128, 0)), "mma64": (64, _mma_image(64, 0)),
           "taps128": (128, _mma_image(128, 1024)), "taps64": (64, _mma_image(64, 1024)), "q8": (64, _q8_image())}
BUDGET_TABLES, BUDGET_D = [], {}
for _k, (_D, (_bytes, _limit)) in _IMAGES.items():
    _fits, _over, _left = _budget_pair(_bytes, _limit)
    # the matrix-core image's levels are multiples of 64 bytes and its limit is 32 short of one: 32 bytes stay free on the
    # last admissible sum; the sliced image's limit is met to the byte
    assert _left == (0 if _k == "q8" else 32), (_k, _left)
    BUDGET_TABLES += [(f"{_k}_budget_exact", _fits), (f"{_k}_budget_over", _over)]
    BUDGET_D.update({f"{_k}_budget_exact": _D, f"{_k}_budget_over": _D})
TABLES += BUDGET_TABLES
NAMES = [n for n, _ in TABLES]
SHAPES = dict(TABLES)
B, H, NQ, P = 1, 2, 48, 4
FWD_ALGOS = ("auto", "gather", "lds", "slices", "waves")
# (name, settings, what must have run for the route to count as taken): a registered (host-known) table or fresh
# tensors, the shim's knobs, library knobs from the environment
BWD_ROUTES = [
    ("sorted", dict(register=True, prefer_sorted=True), ("sorted",)),
    ("hybrid", dict(register=True), ("hybrid",)),
    ("plain", dict(register=True, hybrid=False), ("sequence",)),
    ("device-checked", dict(register=False), ("device-checked",)),
    ("atomic", dict(register=True, bwd="atomic"), ("atomic",)),
    ("value=block", dict(register=True, hybrid=False, env={"MMFS_VALUE_ALGO": "block"}), ("sequence",)),
    ("value=pixel", dict(register=True, hybrid=False, env={"MMFS_VALUE_ALGO": "pixel"}), ("sequence",)),
    ("taps=gather", dict(register=True, taps="gather"), ("hybrid+gather", "sequence+gather")),
    ("taps=lds", dict(register=True, taps="lds"), ("hybrid+lds", "sequence+lds")),
]
# flags arguments of the entry points (include/mmfs_msda.h): their position in the call
_FLAG_ARG = {"mmfs_msda_backward_sorted": 20, "mmfs_msda_backward_hybrid": 21, "mmfs_msda_backward_checked": 19}
_ENTRIES = tuple(_FLAG_ARG) + ("mmfs_msda_backward_taps",)


def has_empty(shapes):
    return any(h * w == 0 for h, w in shapes)


def head_widths(shapes, name=None):
    """D = 128 for the query-wave kernel, 64 and 32 for the sliced / matrix-core ones, 24 and 8 for the scalar gather;
    only 32 on the tables of tens of thousands of pixels (the bound's arrays are S * H * D doubles); a budget table of
    BUDGET_TABLES at the head width its sizes were computed for."""
    if name in BUDGET_D:
        return (BUDGET_D[name],)
    return (32,) if sum(h * w for h, w in shapes) > 30000 else (128, 64, 32, 24, 8)


def dtypes_of(name, shapes):
    if name == "empty_mid_Hx0":
        return (torch.bfloat16, torch.float16, torch.float32, torch.float64)
    return (torch.bfloat16, torch.float16, torch.float32) if has_empty(shapes) else (torch.bfloat16, torch.float32)


class knobs:
    """The shim's routing knobs and library environment knobs of one route, for a ``with`` block; all back afterwards."""

    def __init__(self, MSDA, hybrid=True, bwd="auto", taps="auto", prefer_sorted=False, fwd="auto", env=None, **_):
        self.MSDA, self.env = MSDA, env or {}
        self.want = dict(_hybrid=hybrid, _bwd_algo=bwd, _taps_algo=taps, _taps_prefer_sorted=prefer_sorted, _fwd_algo=fwd)

    def __enter__(self):
        self.keep = {k: getattr(self.MSDA, k) for k in self.want}
        self.keep_env = {k: os.environ.get(k) for k in self.env}
        for k, v in self.want.items():
            setattr(self.MSDA, k, v)
        os.environ.update(self.env)
        if self.env:
            self.MSDA.reload_env()
        return self

    def __exit__(self, *exc):
        for k, v in self.keep.items():
            setattr(self.MSDA, k, v)
        for k, v in self.keep_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        if self.env:
            self.MSDA.reload_env()
        return False


@contextlib.contextmanager
def entry_calls(MSDA):
    """Yields a list that collects (entry point, flags) of every backward entry point of the library the shim calls."""
    calls, lib = [], MSDA._lib
    keep = {name: getattr(lib, name) for name in _ENTRIES}

    def wrap(name, fn):
        def call(*args):
            calls.append((name, int(args[_FLAG_ARG[name]]) if name in _FLAG_ARG else 0))
            return fn(*args)
        return call
    for name, fn in keep.items():
        setattr(lib, name, wrap(name, fn))
    try:
        yield calls
    finally:
        for name, fn in keep.items():
            setattr(lib, name, fn)


def evidence(MSDA, calls):
    """What ran, from the entry points called: sorted / hybrid / atomic / device-checked / sequence (the canonical
    sequence: one call of mmfs_msda_backward_checked, or staged from mmfs_msda_backward_taps on); "+gather" / "+lds"
    when the call carried the taps formulation's flag."""
    names = [n for n, _ in calls]
    if "mmfs_msda_backward_sorted" in names:
        return "sorted"
    taps = lambda f: "+gather" if f & MSDA._BWD_TAPS_ROW_GATHER else "+lds" if f & MSDA._BWD_TAPS_LDS_LEVELS else ""
    if "mmfs_msda_backward_hybrid" in names:
        return "hybrid" + taps(dict(calls)["mmfs_msda_backward_hybrid"])
    if "mmfs_msda_backward_checked" in names:
        f = dict(calls)["mmfs_msda_backward_checked"]
        if f & MSDA._BWD_FORCE_ATOMIC:
            return "atomic"
        if f & MSDA._BWD_DEVICE_CHECKED_LEVELS:
            return "device-checked"
        return ("sequence" + taps(f)) if f & MSDA._BWD_CANONICAL_LEVELS else "unknown"
    return "sequence" if "mmfs_msda_backward_taps" in names else "none"


def _case(shapes, D, dtype, seed):
    x = make_inputs(B, H, D, NQ, P, shapes, seed=seed, loc_range=(-0.15, 1.15), dtype=dtype)
    x["loc"][0, 1, 0, 0, 0, 0] = float("nan")          # non-finite locations: no contribution, zero gradients
    x["attn"][0, 2, 1 % H] = 0.0                        # zero weights: grad_value gets nothing, grad_attn is not zero
    return x, error_bounds(x, dtype)[0]


def _fails(got, x, dtype, bounds, what, outputs=OUTPUTS):
    res = bound_ratios(got, x, dtype, outputs, bounds=bounds)
    return [f"{what}: {n} {r[0]:.3g} x the bound at {r[1]} (err {r[2]:.3e}, bound {r[3]:.3e})"
            for n, r in res.items() if not r[0] <= 1.0]


@functools.lru_cache(maxsize=None)
def _run_table(name):
    """-> (failures, {forward kernel: [(D, dtype)]}, {backward route: {what ran}}) over every head width, storage type,
    forward kernel and backward route of table ``name``.  Failures are collected, not raised: one run shows every route
    that breaks."""
    import MultiScaleDeformableAttention as MSDA
    shapes = SHAPES[name]
    fails, fwd_ran, bwd_ran = [], {}, {}
    for D in head_widths(shapes, name):
        for dtype in dtypes_of(name, shapes):
            if dtype == torch.float64 and D != 32:
                continue
            x, bounds = _case(shapes, D, dtype, seed=NAMES.index(name) * 1000 + D)
            dev = lambda t: t.to(DEV, dtype) if t.is_floating_point() else t.to(DEV)
            value, loc, attn, grad = dev(x["value"]), dev(x["loc"]), dev(x["attn"]), dev(x["grad"]).reshape(B, NQ, H * D)
            S = value.shape[1]
            tag = f"{name} D={D} {str(dtype)[6:]}"
            # ---- forward kernels (a forced kernel may refuse the shape: _E_UNSUPPORTED, as tests/fuzz_op.py accepts)
            for algo in FWD_ALGOS:
                with knobs(MSDA, fwd=algo):
                    try:
                        out = MSDA.ms_deform_attn_forward(value, dev(x["shapes"]), dev(x["start"]), loc, attn, 1)
                        torch.cuda.synchronize()
                    except RuntimeError as e:
                        if algo == "auto" or f"status {MSDA._E_UNSUPPORTED}" not in str(e):
                            fails.append(f"{tag} fwd={algo}: {e}")
                        continue
                fwd_ran.setdefault(algo, []).append((D, str(dtype)[6:]))
                fails += _fails([out.double().cpu(), None, None, None], x, dtype, bounds, f"{tag} fwd={algo}", ("out",))
            # ---- backward routes, one call and staged
            for route, cfg, _ in BWD_ROUTES:
                for staged in (False, True):
                    sh, st = dev(x["shapes"]), dev(x["start"])          # (fresh tensors: unregistered unless registered here)
                    if cfg["register"]:
                        MSDA.register_level_tables(sh, st, S, host_shapes=x["shapes"], host_start=x["start"])
                    log = [] if staged else None
                    took = MSDA.route_counts["sorted"]
                    out = MSDA.ms_deform_attn_forward(value, sh, st, loc, attn, 1)
                    with knobs(MSDA, **cfg), entry_calls(MSDA) as calls:
                        MSDA._event_log = log
                        try:
                            gv, gl, ga = MSDA.ms_deform_attn_backward(value, sh, st, loc, attn, grad, 1)
                            torch.cuda.synchronize()
                        except RuntimeError as e:
                            if not (cfg.get("taps") == "lds" and f"status {MSDA._E_UNSUPPORTED}" in str(e)):
                                fails.append(f"{tag} bwd={route} staged={staged}: {e}")
                            continue
                        finally:
                            MSDA._event_log = None
                    what = f"{tag} bwd={route} staged={staged}"
                    ran = evidence(MSDA, calls)
                    if (ran == "sorted") != (MSDA.route_counts["sorted"] > took):
                        fails.append(f"{what}: route_counts['sorted'] disagrees with the entry point called ({ran})")
                    if staged:
                        launches = [n for n, _, _ in log]
                        if ran == "atomic" and launches != ["msda_bwd_atomic"]:
                            fails.append(f"{what}: forced atomic launched {launches}")
                        if ran == "sorted" and launches[-4:] != ["msda_bwd_value_prepare", "msda_bwd_value_sort",
                                                                 "msda_bwd_taps", "msda_bwd_value_reduce"]:
                            fails.append(f"{what}: sorted route launched {launches}")
                    fails += _fails([t.double().cpu() for t in (out, gv, gl, ga)], x, dtype, bounds, what)
                    bwd_ran.setdefault(route, set()).add(ran)
    return fails, fwd_ran, bwd_ran


@pytest.fixture
def poisoned(monkeypatch):
    poison_allocations(monkeypatch)
    yield


@pytest.mark.parametrize("name", NAMES)
def test_level_table_through_every_route(name, poisoned):
    fails = _run_table(name)[0]
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


@pytest.mark.parametrize("name", ["empty_mid_Hx0", "two_empty_adjacent", "strip_5122_cells", "wq_budget_exact"])
@pytest.mark.parametrize("repeat", ["tile", "interleave"])
def test_shared_bank_forward_on_level_table(name, repeat, poisoned):
    """value_repeat: a bank of Bv = 2 rows serves 4 query rows -- within the bound of the bank expanded in that order
    (rows 0 1 0 1 for "tile", 0 0 1 1 for "interleave": a swapped layout breaks the bound)."""
    import MultiScaleDeformableAttention as MSDA
    dtype, D = torch.bfloat16, 32
    x = make_inputs(4, H, D, NQ, P, SHAPES[name], seed=5, loc_range=(-0.1, 1.1), dtype=dtype)
    bank = x["value"][:2]
    x["value"] = bank.repeat(2, 1, 1, 1) if repeat == "tile" else bank.repeat_interleave(2, 0)
    dev = lambda t: t.to(DEV, dtype) if t.is_floating_point() else t.to(DEV)
    out = MSDA.ms_deform_attn_forward(dev(bank), dev(x["shapes"]), dev(x["start"]), dev(x["loc"]),
                                      dev(x["attn"]), 1, value_repeat=repeat)
    torch.cuda.synchronize()
    fails = _fails([out.double().cpu(), None, None, None], x, dtype, error_bounds(x, dtype)[0],
                   f"{name} repeat={repeat}", ("out",))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", ["empty_first_0xW", "empty_last_0x0", "one_level_has_px", "row_1024px"])
@pytest.mark.parametrize("D", [32, 128])
def test_fp8_bank_forward_on_level_table(name, D, poisoned):
    """The fp8 forward (value_scale=): within the bound of the dequantised bank."""
    import MultiScaleDeformableAttention as MSDA
    dtype = torch.bfloat16
    x = make_inputs(B, H, D, NQ, P, SHAPES[name], seed=6, loc_range=(-0.1, 1.1), dtype=dtype)
    q, s = MSDA.quantize_bank_fp8(x["value"].float().to(DEV))
    x["value"] = MSDA.dequantize_bank_fp8(q, s, torch.float64).cpu()
    dev = lambda t: t.to(DEV, dtype) if t.is_floating_point() else t.to(DEV)
    out = MSDA.ms_deform_attn_forward(q, dev(x["shapes"]), dev(x["start"]), dev(x["loc"]), dev(x["attn"]), 1, value_scale=s)
    torch.cuda.synchronize()
    fails = _fails([out.double().cpu(), None, None, None], x, dtype, error_bounds(x, dtype)[0], f"{name} fp8 D={D}", ("out",))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("decode", ["0", "1"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_fused_sampler_on_a_table_with_an_empty_level(decode, dtype, poisoned):
    """The fused sampler (plan -> sampler in one kernel, mmfs_sample_fwd; with MMFS_SAMPLE_DECODE=1 and few queries the
    decode kernel) on images whose middle level is (0, 3): the plan divides the offsets by the level's extent, so that
    level's locations are non-finite and it samples nothing -- as the two-kernel path (plan kernel + op) computes it.
    Bit-identical to that path on the in-order kernel, within the storage type's rounding on the decode kernel, finite."""
    import MultiScaleDeformableAttention as MSDA
    from mmfs_amd.functions.mmfs_plan_func import sample_forward_groups
    from mmfs_amd.levels import make_level_tables
    from mmfs_amd.modules import MMFS
    Hh, D, L, P_, n, N, Lq, dq = 2, 32, 3, 4, 2, 2, 5, 24
    g = torch.Generator().manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        m = MMFS(d_model=Hh * D, d_query=dq, d_value=16, d_out=dq, n_levels=L, n_heads=Hh, n_points=P_, ratio=1.0,
                 offset_init_magnitude=1, spatial_shapes=[4, 0, 2], base_spatial_shape=4, max_num_image_per_seq=6)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    m = m.to(DEV, dtype).eval()
    shapes, start, S = make_level_tables([(4, 4), (0, 3), (2, 2)], n, DEV)
    query = torch.randn(N, Lq, dq, generator=g).to(DEV, dtype)
    feat = torch.randn(N, n, S // n, 16, generator=g).to(DEV, dtype)
    ref = torch.rand(1, Lq, 1, 2, generator=g).to(DEV, dtype)
    mask = torch.ones(N, n, device=DEV)
    keep = os.environ.get("MMFS_SAMPLE_DECODE")
    os.environ["MMFS_SAMPLE_DECODE"] = decode
    MSDA.reload_env()
    try:
        outs = {}
        for fused in (True, False):
            m.fused_sampler = fused
            with torch.no_grad():
                outs[fused] = m(query, ref, feat, shapes, start, None, mask)
        torch.cuda.synchronize()
    finally:
        if keep is None:
            os.environ.pop("MMFS_SAMPLE_DECODE", None)
        else:
            os.environ["MMFS_SAMPLE_DECODE"] = keep
        MSDA.reload_env()
    a, b = outs[True], outs[False]
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    if decode == "0" or sample_forward_groups(dtype, Lq, D, n * L, P_) <= 1:
        assert torch.equal(a, b)
    else:
        tol = {torch.float32: 1e-5, torch.bfloat16: 1.6e-2}[dtype]
        assert float((a.double() - b.double()).abs().max()) <= tol * max(1.0, float(b.double().abs().max()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_every_level_empty(dtype, poisoned):
    """S = 0: out is 0, grad_value is empty, grad_loc and grad_attn are 0 -- registered and device-checked tables, forced
    atomics; with the sorted route preferred too, which refuses S = 0 (the call goes elsewhere: asserted)."""
    import MultiScaleDeformableAttention as MSDA
    sh, st = level_tables([(0, 3), (0, 0), (5, 0)])
    D = 32
    g = torch.Generator().manual_seed(1)
    value = torch.zeros(B, 0, H, D).to(DEV, dtype)
    loc = torch.rand(B, NQ, H, 3, P, 2, generator=g).to(DEV, dtype)
    attn = torch.rand(B, NQ, H, 3, P, generator=g).to(DEV, dtype)
    grad = torch.randn(B, NQ, H * D, generator=g).to(DEV, dtype)
    for route, cfg in [("default", dict(register=True)), ("device-checked", dict(register=False)),
                       ("sorted preferred", dict(register=True, prefer_sorted=True)),
                       ("atomic", dict(register=True, bwd="atomic"))]:
        dsh, dst = sh.to(DEV), st.to(DEV)
        if cfg["register"]:
            MSDA.register_level_tables(dsh, dst, 0, host_shapes=sh, host_start=st)
        took = MSDA.route_counts["sorted"]
        with knobs(MSDA, **cfg), entry_calls(MSDA) as calls:
            out = MSDA.ms_deform_attn_forward(value, dsh, dst, loc, attn, 1)
            gv, gl, ga = MSDA.ms_deform_attn_backward(value, dsh, dst, loc, attn, grad, 1)
        torch.cuda.synchronize()
        assert MSDA.route_counts["sorted"] == took and "mmfs_msda_backward_sorted" not in [c for c, _ in calls], route
        assert out.shape == (B, NQ, H * D) and bool((out == 0).all()), route
        assert gv.shape == value.shape and gv.numel() == 0, route
        assert bool((gl == 0).all()) and bool((ga == 0).all()), route


def test_every_forward_kernel_and_backward_route_ran_on_an_empty_level(poisoned):
    """Which forward kernel and which backward entry point ran on which table; every forward kernel, and every backward
    route's own entry point (one of BWD_ROUTES' third column), on at least one table with an empty level.  (Runs the tables
    itself where the parametrised test has not.)"""
    fwd_seen, bwd_seen, rows = set(), set(), []
    for name in NAMES:
        _, fwd, bwd = _run_table(name)
        rows.append(f"ROUTES {name:20s} {str(SHAPES[name]):40s} fwd: {' '.join(a for a in FWD_ALGOS if a in fwd):30s} bwd: "
                    + " ".join(f"{r}={'/'.join(sorted(bwd.get(r, ())))}" for r, _, _ in BWD_ROUTES))
        if has_empty(SHAPES[name]):
            fwd_seen |= set(fwd)
            bwd_seen |= {r for r, _, want in BWD_ROUTES if set(want) & bwd.get(r, set())}
    print("\n".join(rows))
    assert fwd_seen == set(FWD_ALGOS), sorted(set(FWD_ALGOS) - fwd_seen)
    assert bwd_seen == {r for r, _, _ in BWD_ROUTES}, sorted({r for r, _, _ in BWD_ROUTES} - bwd_seen)
