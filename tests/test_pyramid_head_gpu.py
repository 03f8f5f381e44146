"""The ViT-Adapter's output pyramid from the tokens on the GPU (csrc/mmfs_pyramid.hip).

1. forward and backward through the C ABI, every element against ``pyramid64`` (test_pyramid_head.py: the formulas in
   fp64, tied to the reference's fixture there) on the same storage-rounded inputs under a derived bound, outputs
   allocated poisoned;  2. non-finite inputs, determinism, unsupported problems;  3. ``AdapterPyramidHead`` on the
   reference's fixture, with a route counter, and under graph capture.

Worst ratios to the bound measured on an MI355X are recorded in profiles/vit_adapter.md."""
import ctypes

import pytest
import torch

import helpers
from helpers import STORAGE_T, STORAGE_U
from test_pyramid_head import (golden, head_of, inputs_of, level_sizes, packed_grad, pyramid64, pyramid64_backward,
                               tokens_of)
from test_vit_adapter import T, rel
from test_vit_adapter_gpu import worst

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
U32 = 2.0 ** -24
# term counts by the rule in the header comment of csrc/mmfs_pyramid.hip
N_FWD = (6, 5, 2, 5)            # up, c1, 4 taps | c2, 4 taps | c3, x3 | c4, 4 pixels; + 1 with a position table
N_BWD = (64, 16, 1, 1)          # g_x1 .. g_x4


def lib():
    from mmfs_amd.functions import pyramid_func
    return pyramid_func._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def levels_of(mask):
    return tuple(l for l in range(4) if (mask >> l) & 1)


def make_case(dtype, B, H, W, C, nhwc, tables, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g).to(dtype)     # noqa: E731
    x = {"c": rn(B, 21 * H * W // 4, C), "up": rn(B, 4 * H * W, 4 * C)}
    x["xs"] = [rn(B, H * W, C) for _ in range(4)]
    x["c1"] = rn(B, 4 * H, 4 * W, C).permute(0, 3, 1, 2) if nhwc else rn(B, C, 4 * H, 4 * W)
    x["pos"] = [torch.randn(h * w, C, device=DEV, generator=g) for h, w in level_sizes(H, W)] if tables else None
    x["g"] = rn(B, sum(h * w for h, w in level_sizes(H, W)), C)            # (a mask takes its levels' rows of this)
    return x


def run_forward(dtype, x, H, W, mask, nhwc):
    B, _, C = x["c"].shape
    on = [(mask >> l) & 1 for l in range(4)]
    S = sum(h * w for (h, w), o in zip(level_sizes(H, W), on) if o)
    out = helpers.poison(torch.empty(B, S, C, device=DEV, dtype=dtype))
    xs = [t if o else None for t, o in zip(x["xs"], on)]
    pos = [t if o else None for t, o in zip(x["pos"], on)] if x["pos"] is not None else [None] * 4
    rc = lib().mmfs_pyramid_head_forward(CODE[dtype], x["c"].data_ptr(), *map(ptr, xs), ptr(x["up"]) if on[0] else None,
                                         ptr(x["c1"]) if on[0] else None, *map(ptr, pos), out.data_ptr(), B, H, W, C, mask,
                                         int(nhwc), stream())
    assert rc == 0, rc
    return out


def run_backward(dtype, g, B, H, W, C, mask, nhwc):
    on = [(mask >> l) & 1 for l in range(4)]
    gx = [helpers.poison(torch.empty(B, H * W, C, device=DEV, dtype=dtype)) if o else None for o in on]
    g_up = g_c1 = None
    if on[0]:
        g_up = helpers.poison(torch.empty(B, 4 * H * W, 4 * C, device=DEV, dtype=dtype))
        g_c1 = helpers.poison(torch.empty(B, 4 * H, 4 * W, C, device=DEV, dtype=dtype).permute(0, 3, 1, 2) if nhwc
                              else torch.empty(B, C, 4 * H, 4 * W, device=DEV, dtype=dtype))
    rc = lib().mmfs_pyramid_head_backward(CODE[dtype], g.data_ptr(), ptr(g_up), ptr(g_c1), *map(ptr, gx), B, H, W, C, mask,
                                          int(nhwc), stream())
    assert rc == 0, rc
    return g_up, g_c1, gx


def split_levels(t, H, W, levels):
    out, lo = {}, 0
    for l in levels:
        h, w = level_sizes(H, W)[l]
        out[l] = t[:, lo:lo + h * w]
        lo += h * w
    assert lo == t.shape[1]
    return out


def rows_of(x, H, W, levels):
    """the rows of the case's upstream gradient that belong to ``levels``, packed"""
    full = split_levels(x["g"], H, W, (0, 1, 2, 3))
    return torch.cat([full[l] for l in levels], 1).contiguous()


def check_case(dtype, B, H, W, C, nhwc, mask, tables, seed, report):
    """One problem, forward and backward, every element of every output under its bound."""
    u, t = STORAGE_U[dtype], STORAGE_T[dtype]
    levels = levels_of(mask)
    x = make_case(dtype, B, H, W, C, nhwc, tables, seed)
    what = f"{dtype} B={B} H={H} W={W} C={C} nhwc={nhwc} mask={mask} tables={tables}"
    out = split_levels(run_forward(dtype, x, H, W, mask, nhwc), H, W, levels)
    d = lambda v: v.double()     # noqa: E731
    pos64 = [d(p) for p in x["pos"]] if tables else None
    want = pyramid64(d(x["c"]), [d(v) for v in x["xs"]], d(x["up"]), d(x["c1"]), pos64, H, W, levels)
    A = pyramid64(d(x["c"]).abs(), [d(v).abs() for v in x["xs"]], d(x["up"]).abs(), d(x["c1"]).abs(),
                  [p.abs() for p in pos64] if tables else None, H, W, levels)
    res = {}
    for l in levels:
        n = N_FWD[l] + int(tables)
        res[f"out{l + 1}"] = worst(out[l], want[l], u * want[l].abs() + (n + 1) * U32 * A[l] + t)
    # backward
    g = rows_of(x, H, W, levels)
    g_up, g_c1, gx = run_backward(dtype, g, B, H, W, C, mask, nhwc)
    g64 = split_levels(d(g), H, W, levels)
    bw = pyramid64_backward(g64, H, W, (B, C, 4 * H, 4 * W))
    bA = pyramid64_backward({l: v.abs() for l, v in g64.items()}, H, W, (B, C, 4 * H, 4 * W))
    for l in levels:
        ref = bw["x"][l]
        res[f"g_x{l + 1}"] = worst(gx[l], ref, u * ref.abs() + (N_BWD[l] + 1) * U32 * bA["x"][l] + t)
    if 0 in levels:                                          # copies: n = 1, and every bit the gradient's
        res["g_up"] = worst(g_up, bw["up"], u * bw["up"].abs() + 2 * U32 * bA["up"] + t)
        res["g_c1"] = worst(g_c1, bw["c1"], u * bw["c1"].abs() + 2 * U32 * bA["c1"] + t)
        assert torch.equal(g_up.double(), bw["up"]) and torch.equal(g_c1.double(), bw["c1"]), what
        assert g_c1.is_contiguous(memory_format=torch.channels_last if nhwc else torch.contiguous_format)
    for k, v in res.items():
        report[k] = max(report.get(k, 0.0), v[0])
    bad = {k: v for k, v in res.items() if not v[0] <= 1.0}
    assert not bad, f"{what}: bound broken: {bad}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_and_backward_element_by_element(dtype):
    """Every element of every level and of g_up, g_c1, g_x1..4 against fp64 on the same storage-rounded inputs:
        |got - want| <= u_T |want| + (n + 1) u_32 sum |terms| + t_T
    u_T the storage type's rounding, t_T its subnormal floor (helpers.STORAGE_U / STORAGE_T), u_32 = 2^-24, n the element's
    term count by the rule in the kernel file's header: forward 6 / 5 / 2 / 5 per level + 1 with a position table (at most
    7), backward 64 / 16 / 1 / 1 for g_x1..4 and 1 for the copies g_up / g_c1 (which must also equal the gradient's bits).
    A term is an exact fp32 weight times a value and joins the sum with one rounding, n in all; + 1 for the conversion.
    sum |terms| is pyramid64 on the absolute values (all weights are >= 0).  Outputs are allocated poisoned: an element
    no lane writes is NaN and fails.  No element is left out.
    The grid: C in {8, 32, 72, 256, 1024} x (H, W) in {(2, 2), (4, 6), (6, 10), (8, 8), (16, 16)} x B in {1, 3} x both c1
    layouts x masks {all, without level 1, each of the four levels alone} x tables on / off, the full cross product:
    1200 problems per dtype."""
    report, seed = {}, 0
    for C in (8, 32, 72, 256, 1024):
        for H, W in ((2, 2), (4, 6), (6, 10), (8, 8), (16, 16)):
            for B in (1, 3):
                for nhwc in (False, True):
                    for tables in (False, True):
                        seed += 1                            # (one draw per (C, map, B, layout, tables); its six masks share it)
                        for mask in (15, 14, 1, 2, 4, 8):
                            check_case(dtype, B, H, W, C, nhwc, mask, tables, seed, report)
    print(f"PYRAMID-BOUNDS {str(dtype)[6:]} worst ratios " + " ".join(f"{k} {v:.3f}" for k, v in sorted(report.items())))


@pytest.mark.parametrize("nhwc", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_inputs_reach_exactly_their_outputs(dtype, nhwc):
    """One Inf or NaN in every input, several next to the clamped first row / column: the non-finite outputs are exactly
    those that hold the element under a NON-ZERO weight (pyramid64 on the indicator of the non-finite elements is > 0
    there: all weights are >= 0); every other element stays within its bound.  At the clamped border pixels the
    framework multiplies the second tap by 0 and returns NaN; the kernel does not read a tap of weight 0.  The backward
    the same way with non-finite gradient rows."""
    u, t = STORAGE_U[dtype], STORAGE_T[dtype]
    B, H, W, C = 2, 4, 6, 32
    x = make_case(dtype, B, H, W, C, nhwc, True, 77)
    inf, nan = float("inf"), float("nan")
    x["xs"][0][0, 1 * W + 1, 3] = inf          # x1 (1, 1): weight 0 in output rows / columns 0, 1
    x["xs"][0][1, H * W - 1, 9] = nan          # x1 last pixel: both taps of the far border
    x["xs"][1][0, 1 * W + 0, 5] = nan          # x2 (1, 0): weight 0 in output row 0
    x["xs"][1][1, 0 * W + 1, 6] = -inf         # x2 (0, 1): weight 0 in output column 0
    x["xs"][2][0, 7, 0] = inf
    x["xs"][3][1, 2 * W + 3, 31] = nan
    x["c"][0, 5, 1] = nan                      # c2
    x["c"][1, 4 * H * W + 2, 2] = inf          # c3
    x["c"][0, 5 * H * W + 1, 8] = inf          # c4
    x["up"][1, 3, 2 * C + 4] = nan             # block (1, 0) of row (0, 3)
    x["c1"][0, 17, 4 * H - 1, 4 * W - 1] = inf
    for l in range(4):
        x["pos"][l][l + 1, 20 + l] = nan
    out = split_levels(run_forward(dtype, x, H, W, 15, nhwc), H, W, (0, 1, 2, 3))
    d = lambda v: v.double()     # noqa: E731
    ind = lambda v: (~torch.isfinite(v)).double()     # noqa: E731
    fin = lambda v: torch.where(torch.isfinite(v), v, torch.zeros_like(v)).double()     # noqa: E731
    reach = pyramid64(ind(x["c"]), [ind(v) for v in x["xs"]], ind(x["up"]), ind(x["c1"]), [ind(p) for p in x["pos"]], H, W)
    want = pyramid64(fin(x["c"]), [fin(v) for v in x["xs"]], fin(x["up"]), fin(x["c1"]), [fin(p) for p in x["pos"]], H, W)
    A = pyramid64(fin(x["c"]).abs(), [fin(v).abs() for v in x["xs"]], fin(x["up"]).abs(), fin(x["c1"]).abs(),
                  [fin(p).abs() for p in x["pos"]], H, W)
    counts = []
    for l in range(4):
        bad = reach[l] > 0
        assert torch.equal(~torch.isfinite(d(out[l])), bad), l
        ok = ~bad
        err = (d(out[l]) - want[l]).abs()
        bound = u * want[l].abs() + (N_FWD[l] + 2) * U32 * A[l] + t
        assert bool((err[ok] <= bound[ok]).all()), l
        counts.append(int(bad.sum()))
    # x1 (1, 1) reaches output rows / columns 2..9 only (not 0, 1: weight 0), the last pixel the last 6 x 6; + up, c1, pos
    assert counts[0] == 8 * 8 + 6 * 6 + 1 + 1 + B
    # x2 (1, 0) reaches rows 1..4 (not 0) x columns 0, 1, 2; x2 (0, 1) rows 0..2 x columns 1..4; + c2, pos
    assert counts[1] == 4 * 3 + 3 * 4 + 1 + B
    assert counts[2] == 1 + 1 + B and counts[3] == 1 + 1 + B
    # backward: non-finite gradient rows
    g = x["g"].clone()
    lo = [0, 16 * H * W, 20 * H * W, 21 * H * W]
    g[0, lo[0] + 0 * 4 * W + 0, 2] = inf       # level 1 (0, 0): reaches x1 (0, 0) only
    g[1, lo[0] + 6 * 4 * W + 6, 3] = nan       # level 1 (6, 6): x1 (1..2, 1..2)
    g[0, lo[1] + 0 * 2 * W + 3, 4] = nan       # level 2 (0, 3): x2 (0, 1..2)
    g[1, lo[2] + 5, 5] = inf
    g[0, lo[3] + 1 * (W // 2) + 2, 6] = -inf   # level 4 (1, 2): x4 (2..3, 4..5)
    g_up, g_c1, gx = run_backward(dtype, g, B, H, W, C, 15, nhwc)
    g_l = split_levels(g, H, W, (0, 1, 2, 3))
    reach = pyramid64_backward({l: ind(v) for l, v in g_l.items()}, H, W, (B, C, 4 * H, 4 * W))
    ref = pyramid64_backward({l: fin(v) for l, v in g_l.items()}, H, W, (B, C, 4 * H, 4 * W))
    refA = pyramid64_backward({l: fin(v).abs() for l, v in g_l.items()}, H, W, (B, C, 4 * H, 4 * W))
    for l in range(4):
        bad = reach["x"][l] > 0
        assert torch.equal(~torch.isfinite(d(gx[l])), bad), l
        ok = ~bad
        bound = u * ref["x"][l].abs() + (N_BWD[l] + 1) * U32 * refA["x"][l] + t
        assert bool(((d(gx[l]) - ref["x"][l]).abs()[ok] <= bound[ok]).all()), l
    assert [int((reach["x"][l] > 0).sum()) for l in range(4)] == [1 + 4, 2, 1, 4]
    assert torch.equal(~torch.isfinite(g_up), reach["up"] > 0) and torch.equal(~torch.isfinite(g_c1), reach["c1"] > 0)
    assert int((~torch.isfinite(g_up)).sum()) == 2 and int((~torch.isfinite(g_c1)).sum()) == 2


@pytest.mark.parametrize("nhwc", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_backward_runs_are_bit_equal(dtype, nhwc):
    B, H, W, C = 3, 8, 8, 72
    x = make_case(dtype, B, H, W, C, nhwc, False, 31)
    first = run_backward(dtype, x["g"], B, H, W, C, 15, nhwc)
    junk = torch.randn(1 << 20, device=DEV)                # (another allocation pattern between the calls)
    second = run_backward(dtype, x["g"], B, H, W, C, 15, nhwc)
    del junk
    for a, b in zip(first[:2] + tuple(first[2]), second[:2] + tuple(second[2])):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    # ... and two forwards
    assert torch.equal(run_forward(dtype, x, H, W, 15, nhwc), run_forward(dtype, x, H, W, 15, nhwc))


@pytest.mark.parametrize("nhwc", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_outputs_nobody_needs_are_left_alone_and_masked_pointers_are_not_looked_at(dtype, nhwc):
    """A NULL output of the backward is not computed and the others keep their bits, for every single output and for
    level 1 alone with NCHW c1 (the tile kernels on their own); a misaligned pointer of a level outside the mask is
    not looked at by either call."""
    B, H, W, C = 2, 4, 6, 32
    x = make_case(dtype, B, H, W, C, nhwc, True, 51)
    full = run_backward(dtype, x["g"], B, H, W, C, 15, nhwc)
    names = ["up", "c1", "x1", "x2", "x3", "x4"]
    flat = dict(zip(names, [full[0], full[1]] + full[2]))
    for skip in names + ["x1+x2+x3+x4", "up+c1"]:
        out = {k: helpers.poison(torch.empty_like(v)) for k, v in flat.items() if k not in skip.split("+")}
        rc = lib().mmfs_pyramid_head_backward(CODE[dtype], x["g"].data_ptr(), *[ptr(out.get(k)) for k in names], B, H, W, C, 15,
                                              int(nhwc), stream())
        assert rc == 0, (skip, rc)
        for k, v in out.items():
            assert torch.equal(v, flat[k]), (skip, k)
    # level 1 alone, only g_c1 wanted / only g_x1 wanted
    g1 = rows_of(x, H, W, (0,))
    for want in ("c1", "x1", "up"):
        out = {want: helpers.poison(torch.empty_like(flat[want]))}
        rc = lib().mmfs_pyramid_head_backward(CODE[dtype], g1.data_ptr(), *[ptr(out.get(k)) for k in names], B, H, W, C, 1,
                                              int(nhwc), stream())
        assert rc == 0 and torch.equal(out[want], flat[want]), want
    # pointers of levels outside the mask: misaligned and never dereferenced
    odd = x["c"].data_ptr() + 2
    ref = run_forward(dtype, x, H, W, 14, nhwc)
    got = helpers.poison(torch.empty_like(ref))
    rc = lib().mmfs_pyramid_head_forward(CODE[dtype], x["c"].data_ptr(), odd, *[t.data_ptr() for t in x["xs"][1:]], odd, odd, odd,
                                         *[t.data_ptr() for t in x["pos"][1:]], got.data_ptr(), B, H, W, C, 14, int(nhwc), stream())
    assert rc == 0 and torch.equal(got, ref)
    g = rows_of(x, H, W, (1, 2, 3))
    gx = [helpers.poison(torch.empty_like(flat["x2"])) for _ in range(3)]
    rc = lib().mmfs_pyramid_head_backward(CODE[dtype], g.data_ptr(), odd, odd, odd, *map(ptr, gx), B, H, W, C, 14, int(nhwc), stream())
    assert rc == 0 and all(torch.equal(a, flat[k]) for a, k in zip(gx, ("x2", "x3", "x4")))


def test_frozen_inputs_get_no_gradient_and_cost_no_output():
    """With a frozen ViT (x1..x4 without grad) and c1 without grad the backward computes g_up only; the adapter's
    gradients are those of the run where everything needs one."""
    from mmfs_amd.blocks import AdapterPyramidHead
    torch.manual_seed(5)
    B, H, W, C = 2, 4, 4, 32
    m = AdapterPyramidHead(C).to(DEV, torch.float32)
    m.token_kernel = True
    x = make_case(torch.float32, B, H, W, C, False, False, 52)
    res = {}
    for frozen in (False, True):
        c = x["c"].clone().requires_grad_(True)
        xs = [t.clone().requires_grad_(not frozen) for t in x["xs"]]
        c1 = x["c1"].clone().requires_grad_(not frozen)
        m.zero_grad()
        m(c, xs, c1, H, W).backward(x["g"])
        assert all((t.grad is None) == frozen for t in xs + [c1])
        res[frozen] = (c.grad.clone(), m.adapter_up.weight.grad.clone(), m.adapter_up.bias.grad.clone())
    assert all(torch.equal(a, b) for a, b in zip(res[False], res[True]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_unsupported_problems_are_refused_and_the_module_takes_the_framework_statement(dtype):
    from mmfs_amd.blocks import AdapterPyramidHead
    from mmfs_amd.functions import pyramid_func, pyramid_head_supported
    H = W = 4
    C = 12 if dtype != torch.float32 else 6                 # a width the 16-byte lanes cannot take
    x = make_case(dtype, 2, H, W, C, False, False, 5)
    assert lib().mmfs_pyramid_head_supported(CODE[dtype], C, H, W, 15) == 0
    assert not pyramid_head_supported(x["c"], x["xs"], x["c1"], None, H, W, 15)
    out = torch.empty(2, 340, C, device=DEV, dtype=dtype)
    args = (x["c"].data_ptr(), *[t.data_ptr() for t in x["xs"]], x["up"].data_ptr(), x["c1"].data_ptr(), None, None, None, None,
            out.data_ptr())
    assert lib().mmfs_pyramid_head_forward(CODE[dtype], *args, 2, H, W, C, 15, 0, stream()) == -5
    assert lib().mmfs_pyramid_head_forward(CODE[dtype], *args, 2, 3, W, 16, 15, 0, stream()) == -5      # odd H
    assert lib().mmfs_pyramid_head_backward(CODE[dtype], out.data_ptr(), *args[5:7], *args[1:5], 2, H, W, C, 15, 0, stream()) == -5
    m = AdapterPyramidHead(C).to(DEV, dtype)
    m.token_kernel = True
    before = dict(pyramid_func.launches)
    got = m(x["c"], x["xs"], x["c1"], H, W)
    m.token_kernel = False
    assert torch.equal(got, m(x["c"], x["xs"], x["c1"], H, W)) and pyramid_func.launches == before
    # a supported width: the kernel; mixed dtypes and autocast: the framework statement
    ok = AdapterPyramidHead(32).to(DEV, dtype)
    ok.token_kernel = True
    y = make_case(dtype, 2, H, W, 32, False, False, 6)
    assert pyramid_head_supported(y["c"], y["xs"], y["c1"], None, H, W, 15)
    ok(y["c"], y["xs"], y["c1"], H, W)
    assert pyramid_func.launches["forward"] == before["forward"] + 1
    other = torch.float16 if dtype != torch.float16 else torch.bfloat16
    assert not pyramid_head_supported(y["c"], [y["xs"][0].to(other)] + y["xs"][1:], y["c1"], None, H, W, 15)
    assert not pyramid_head_supported(y["c"], y["xs"], y["c1"].to(other), None, H, W, 15)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ok(y["c"], y["xs"], y["c1"], H, W)
    assert pyramid_func.launches["forward"] == before["forward"] + 1
    # B = 0: an empty result and gradients of the right shapes
    z = make_case(dtype, 0, H, W, 32, False, False, 7)
    z["c"].requires_grad_(True)
    e = ok(z["c"], z["xs"], z["c1"], H, W)
    assert tuple(e.shape) == (0, 340, 32)
    (gc,) = torch.autograd.grad(e, [z["c"]], torch.zeros_like(e))
    assert gc.shape == z["c"].shape


# ------------------------------------------------------------------ the module on the reference's fixture
def head_step(z, H, W, dtype, on, nhwc, with_pos, levels=(0, 1, 2, 3), grad=True):
    from mmfs_amd.functions import pyramid_func
    m = head_of(z, dtype, DEV)
    m.token_kernel = on
    x = inputs_of(z, dtype, DEV, grad=False)
    if nhwc:
        x["c1"] = x["c1"].contiguous(memory_format=torch.channels_last)
    for v in x.values():
        v.requires_grad_(grad)
    pos = T(z["pos_embed"], None, DEV) if with_pos else None
    before = dict(pyramid_func.launches)
    out = m(x["c"], [x[f"x{k}"] for k in range(1, 5)], x["c1"], H, W, pos_embed=pos, levels=levels)
    if grad:
        out.backward(packed_grad(z, levels, dtype, DEV))
    counts = tuple(pyramid_func.launches[k] - before[k] for k in ("forward", "backward"))
    return m, x, out, counts


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("nhwc", [False, True])
@pytest.mark.parametrize("on", [True, False])
def test_head_fp32_against_the_reference_with_the_switch(on, nhwc, with_pos):
    """The bars test_vit_adapter_gpu.py holds for its fp32 blocks: outputs 2e-5, input and parameter gradients 1e-4 of
    the largest reference entry; with the switch on the kernels run once forward and once backward, off never."""
    z, H, W = golden()
    m, x, out, counts = head_step(z, H, W, torch.float32, on, nhwc, with_pos)
    assert counts == ((1, 1) if on else (0, 0)), counts
    key = "out_pos.l" if with_pos else "out.l"
    e_out = {l: rel(o, tokens_of(T(z[key + str(l)])).numpy()) for l, o in split_levels(out, H, W, (0, 1, 2, 3)).items()}
    e_in = {k: rel(v.grad, z["grad_in." + k]) for k, v in x.items()}
    e_par = {k: rel(p.grad, z["grad." + k]) for k, p in m.named_parameters()}
    print(f"PYRAMID-HEAD fp32 kernel={on} nhwc={nhwc} pos={with_pos} out {max(e_out.values()):.2e} "
          f"grad_in {max(e_in.values()):.2e} grad_param {max(e_par.values()):.2e}")
    assert all(v <= 2e-5 for v in e_out.values()), e_out
    assert all(v <= 1e-4 for v in e_in.values()), e_in
    assert all(v <= 1e-4 for v in e_par.values()), e_par
    if on:                                                   # (the kernel returns c1's gradient in c1's layout)
        assert x["c1"].grad.is_contiguous(memory_format=torch.channels_last if nhwc else torch.contiguous_format)


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("nhwc", [False, True])
@pytest.mark.parametrize("dtype,tag", [(torch.bfloat16, "bf16"), (torch.float16, "fp16")])
def test_head_16bit_against_the_references_own_error(dtype, tag, nhwc, with_pos):
    """The bar is twice the error of the reference's own 16-bit CPU run against its fp64 run (``ref_err[_pos].<dtype>.l<k>``
    of the fixture), the margin test_vit_adapter_gpu.py gives the blocks: one rounding here (two at level 1, whose GEMM
    result is stored) against the reference's several."""
    z, H, W = golden()
    _, _, out, counts = head_step(z, H, W, dtype, True, nhwc, with_pos, grad=False)
    assert counts == (1, 0) and out.dtype == dtype
    key, ekey = ("out_pos.l", "ref_err_pos") if with_pos else ("out.l", "ref_err")
    errs = {l: (rel(o, tokens_of(T(z[key + str(l)])).numpy()), 2.0 * float(z[f"{ekey}.{tag}.l{l}"]))
            for l, o in split_levels(out, H, W, (0, 1, 2, 3)).items()}
    print(f"PYRAMID-HEAD-16BIT {tag} nhwc={nhwc} pos={with_pos} " + " ".join(f"l{l} {e:.2e} (bar {b:.2e})" for l, (e, b) in errs.items()))
    assert all(e <= b for e, b in errs.values()), errs


def test_masks_and_level_views_on_the_gpu():
    """A partial mask gives the full result's rows bit for bit (and its inputs' gradients; an input of levels that are
    not produced gets none); ``packed=False`` returns views of the packed tensor in the reference's shapes."""
    z, H, W = golden()
    _, xf, full, _ = head_step(z, H, W, torch.float32, True, False, True)
    rows = split_levels(full, H, W, (0, 1, 2, 3))
    for levels in ((1, 2, 3), (3,), (0, 2)):
        m, x, out, counts = head_step(z, H, W, torch.float32, True, False, True, levels=levels)
        assert counts == (1, 1)
        assert torch.equal(out, torch.cat([rows[l] for l in levels], 1))
        for k in range(4):
            g = x[f"x{k + 1}"].grad
            assert (g is None) if k not in levels else torch.equal(g, xf[f"x{k + 1}"].grad), k
        assert (x["c1"].grad is None) == (0 not in levels) and (m.adapter_up.weight.grad is None) == (0 not in levels)
        if 0 not in levels:
            n2, n3 = 4 * H * W, H * W
            gc = x["c"].grad
            for l, (lo, hi) in ((1, (0, n2)), (2, (n2, n2 + n3)), (3, (n2 + n3, gc.shape[1]))):
                want = packed_grad(z, (l,), torch.float32, DEV) if l in levels else torch.zeros_like(gc[:, lo:hi])
                assert torch.equal(gc[:, lo:hi], want), l
        x = inputs_of(z, torch.float32, DEV, grad=False)
        feats = m(x["c"], [x[f"x{k}"] for k in range(1, 5)], x["c1"], H, W, pos_embed=T(z["pos_embed"], None, DEV),
                  levels=levels, packed=False)
        for l, f in zip(levels, feats):
            assert tuple(f.shape) == tuple(z[f"out_pos.l{l}"].shape)
            assert torch.equal(tokens_of(f), rows[l])


@pytest.mark.parametrize("nhwc", [False, True])
def test_forward_backward_replays_from_a_graph_bit_for_bit(nhwc):
    """AdapterPyramidHead in bf16, forward + backward captured and replayed at the default queue count: every result
    equals the eager call's bit for bit (the extents travel by value: nothing in the launch reads a table that capture
    could not see)."""
    from mmfs_amd.blocks import AdapterPyramidHead
    from mmfs_amd.functions import pyramid_func
    torch.manual_seed(3)
    B, H, W, C = 3, 8, 8, 64
    m = AdapterPyramidHead(C).to(DEV, torch.bfloat16).train()
    m.token_kernel = True
    x = make_case(torch.bfloat16, B, H, W, C, nhwc, True, 41)
    leaves = [x["c"], x["c1"]] + x["xs"]
    for v in leaves:
        v.requires_grad_(True)
    params = list(m.parameters())

    def step():
        out = m(x["c"], x["xs"], x["c1"], H, W, pos_embed=x["pos"])
        return (out,) + torch.autograd.grad(out, leaves + params, x["g"])

    before = dict(pyramid_func.launches)
    want = [t.detach().clone() for t in step()]
    assert pyramid_func.launches == {"forward": before["forward"] + 1, "backward": before["backward"] + 1}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert all(torch.isfinite(a).all() for a in captured)
    assert all(torch.equal(a.detach(), b) for a, b in zip(captured, want))
