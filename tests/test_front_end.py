"""Host side of the per-element tests of the kernels around the op (tests/test_front_end_gpu.py holds the kernels).

1. Teeth and no false alarms of front_end_refs' bounds, after test_error_bounds.py: an fp32 torch restatement of each
   kernel stands in for the kernel and passes, the fp64 result rounded to storage passes, every planted fault fails --
   and the bars the suite held these kernels to before accept two of the faults.
2. Argument checks of the C ABI's entry points for these kernels: every return code the host code has, through calls
   that return before a launch (safe without a GPU)."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch

import front_end_refs as R
from front_end_refs import worst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def ratios_of(got, ref, bounds):
    return {k: worst(got[k], ref[k], bounds[k])[0] for k in bounds if k in got}


# --------------------------------------------------------------------------------------------- the plan: stand-ins
N, LQ, H, NI, L, P, M = 2, 19, 2, 3, 3, 4, 6          # (n = L: the "summed over levels" fault keeps its shape)


def plan_problem(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    rt = lambda t: t.to(dtype)          # noqa: E731
    c = dict(off_q=rt(torch.randn(N, LQ, H * P * 2, generator=g) * 2), att_q=rt(torch.rand(N, LQ, H * L * P, generator=g) * 8 - 4),
             off_tab=rt(torch.randn(M, H * P * 2, generator=g)), att_tab=rt(torch.rand(M, H * L * P, generator=g) * 8 - 4),
             relpos=torch.randint(1, M - 1, (N, LQ, NI), generator=g), ref=torch.rand(N, LQ, 2, generator=g),
             shapes=torch.tensor([[5, 9], [3, 3], [1, 7], [40, 2], [6, 6], [2, 11], [8, 3], [4, 4], [9, 1]]),
             ratios=torch.rand(L, generator=g) * 1.5 + 0.5)
    c["relpos"][:, :, 0] = 0                        # one image invisible for all queries
    c["relpos"][0, 7:, 1] = 4                       # a change inside a run of 8
    c["g_loc"] = rt(torch.randn(N, LQ, H, NI * L, P, 2, generator=g))
    c["g_attn"] = rt(torch.randn(N, LQ, H, NI * L, P, generator=g))
    c["g_sink"] = torch.randn(N, LQ, H, generator=g)
    return c


def plan_forward_f32(c, dtype, penalty_of=None, shapes=None):
    """plan_forward_kernel in torch fp32 (sums in the framework's order).  ``penalty_of``: the relpos the visibility
    penalty is taken from (a fault: an entry made visible keeps table row 0 but loses the penalty)."""
    f = torch.float32
    r = c["relpos"]
    pen_r = r if penalty_of is None else penalty_of
    sh = (c["shapes"] if shapes is None else shapes).to(f).reshape(NI, L, 2)
    aq, at = c["att_q"].to(f).reshape(N, LQ, H, L, P), c["att_tab"].to(f).reshape(M, H, L, P)
    lg = aq[:, :, :, None] + at[r].permute(0, 1, 3, 2, 4, 5)
    lg = lg + torch.where(pen_r == 0, -10000.0, 0.0).to(f)[:, :, None, :, None, None]
    sl = torch.tensor(-math.log(NI * L), dtype=f)
    m = torch.maximum(lg.amax((3, 4, 5), keepdim=True), sl)
    e = torch.exp(lg - m)
    es = torch.exp(sl - m)
    inv = 1.0 / (e.sum((3, 4, 5), keepdim=True) + NI * L * es)
    oq, ot = c["off_q"].to(f).reshape(N, LQ, H, P, 2), c["off_tab"].to(f).reshape(M, H, P, 2)
    scale = c["ratios"].to(f).reshape(1, L, 1) / sh.flip(-1)
    loc = c["ref"].to(f)[:, :, None, None, None, None, :] + \
        (oq[:, :, :, None, None] + ot[r].permute(0, 1, 3, 2, 4, 5)[:, :, :, :, None]) * scale[None, None, None, :, :, None, :]
    return dict(attn=(e * inv).reshape(N, LQ, H, NI * L, P).to(dtype), sink=(NI * L * es * inv).reshape(N, LQ, H),
                loc=loc.reshape(N, LQ, H, NI * L, P, 2).to(dtype))


def plan_backward_f32(c, attn, sink, with_sink=True, scatter=None, over_levels=False):
    """plan_backward_kernel in torch fp32.  ``scatter``: the rows the table gradients are added to (faults: row M = nowhere,
    r + 1 = the neighbour)."""
    f = torch.float32
    a, g = attn.to(f).reshape(N, LQ, H, NI, L, P), c["g_attn"].to(f).reshape(N, LQ, H, NI, L, P)
    dot = (a * g).sum((3, 4, 5))
    if with_sink:
        dot = dot + c["g_sink"] * sink
    dl = a * (g - dot[..., None, None, None])
    scale = c["ratios"].to(f).reshape(1, L, 1) / c["shapes"].to(f).reshape(NI, L, 2).flip(-1)
    doff = c["g_loc"].to(f).reshape(N, LQ, H, NI, L, P, 2) * scale[None, None, None, :, :, None, :]
    rows = (c["relpos"] if scatter is None else scatter).reshape(-1)

    def table(src, tail):
        return torch.zeros(M + 1, H, *tail).index_add_(0, rows, src.movedim(3, 2).reshape(N * LQ * NI, H, *tail))[:M]

    return dict(d_att_q=dl.sum(4 if over_levels else 3), d_off_q=doff.sum((3, 4)), d_att_tab=table(dl, (L, P)),
                d_off_tab=table(doff.sum(4), (P, 2)))


def plan_refs(c, dtype):
    fw = R.plan_forward64(c["off_q"], c["att_q"], c["off_tab"], c["att_tab"], c["relpos"], c["ref"], c["shapes"], c["ratios"], H, L, P)
    return fw, R.plan_forward_bounds(fw, dtype)


def plan_back_refs(c, attn, sink, dtype):
    refs, sums = R.plan_backward64(c["g_loc"], c["g_attn"], c["g_sink"], attn, sink, c["relpos"], c["shapes"], c["ratios"], H, L, P, M)
    return refs, R.plan_backward_bounds(refs, sums, c["relpos"], N, LQ, L, NI, M, dtype, torch.float32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_plan_bounds_pass_the_honest_and_fail_the_planted_faults(dtype):
    c = plan_problem(dtype)
    fw, fb = plan_refs(c, dtype)
    got = plan_forward_f32(c, dtype)
    honest = ratios_of(got, fw, fb)
    assert all(v <= 1.0 for v in honest.values()), honest
    rounded = dict(attn=fw["attn"].to(dtype), sink=fw["sink"].float(), loc=fw["loc"].to(dtype))
    assert all(v <= 1.0 for v in ratios_of(rounded, fw, fb).values())
    assert not bool(got["attn"].reshape(N, LQ, H, NI, L, P)[:, :, :, 0].any())             # the invisible image: exactly 0
    # the penalty of one invisible image dropped (one query of one sample)
    seen = c["relpos"].clone()
    seen[1, 3, 0] = 1
    bad = ratios_of(plan_forward_f32(c, dtype, penalty_of=seen), fw, fb)
    assert bad["attn"] > 1.0 and bad["sink"] > 1.0, bad
    # W and H exchanged in loc on the non-square levels
    bad = ratios_of(plan_forward_f32(c, dtype, shapes=c["shapes"].flip(-1)), fw, fb)
    assert bad["loc"] > 1.0 and bad["attn"] <= 1.0, bad

    attn, sink = got["attn"], got["sink"]
    refs, bb = plan_back_refs(c, attn, sink, dtype)
    honest = ratios_of(plan_backward_f32(c, attn, sink), refs, bb)
    assert all(v <= 1.0 for v in honest.values()), honest
    assert all(v <= 1.0 for v in ratios_of({k: v.float() for k, v in refs.items()}, refs, bb).values())
    # the sink's term left out of dot
    bad = ratios_of(plan_backward_f32(c, attn, sink, with_sink=False), refs, bb)
    assert bad["d_att_q"] > 1.0 and bad["d_att_tab"] > 1.0, bad
    # one (query, image) contribution to a table row dropped; one added to the neighbouring row
    for row in (M, None):
        sc = c["relpos"].clone()
        sc[1, 11, 2] = M if row is M else sc[1, 11, 2] + 1
        bad = ratios_of(plan_backward_f32(c, attn, sink, scatter=sc), refs, bb)
        assert bad["d_att_tab"] > 1.0 and bad["d_off_tab"] > 1.0 and bad["d_att_q"] <= 1.0, (row, bad)
    # d_att_q summed over levels instead of images
    bad = ratios_of(plan_backward_f32(c, attn, sink, over_levels=True), refs, bb)
    assert bad["d_att_q"] > 1.0 and bad["d_att_tab"] <= 1.0, bad


def test_the_old_bar_accepts_a_dropped_table_contribution_in_bf16(monkeypatch):
    """The modules' bf16 bar -- 1.6e-2 of the largest entry of the tensor, the tightest any 16-bit test of the plan held
    -- passes a table gradient from which the contribution of one (query, image) is missing, when that contribution
    is a small one (600 queries: a row sums ~600 of them); its own per-element bound does not."""
    monkeypatch.setattr(sys.modules[__name__], "LQ", 600)
    dtype = torch.bfloat16
    c = plan_problem(dtype)
    got = plan_forward_f32(c, dtype)
    refs, bb = plan_back_refs(c, got["attn"], got["sink"], dtype)
    honest = plan_backward_f32(c, got["attn"], got["sink"])
    # the visible (sample, query, image) with the smallest contribution a (g - dot) to its row of the attention table
    w, g = got["attn"].double().reshape(N, LQ, H, NI, L, P), c["g_attn"].double().reshape(N, LQ, H, NI, L, P)
    dot = (w * g).sum((3, 4, 5)) + c["g_sink"].double() * got["sink"].double()
    a = (w * (g - dot[..., None, None, None])).abs().amax((2, 4, 5))
    a[c["relpos"] == 0] = float("inf")
    nb, q, k = (int(v) for v in torch.unravel_index(a.argmin(), a.shape))
    sc = c["relpos"].clone()
    sc[nb, q, k] = M
    bad = plan_backward_f32(c, got["attn"], got["sink"], scatter=sc)
    old = float((bad["d_att_tab"].double() - refs["d_att_tab"]).abs().max() / refs["d_att_tab"].abs().max())
    assert not torch.equal(bad["d_att_tab"], honest["d_att_tab"])
    assert old <= 1.6e-2, old
    assert worst(bad["d_att_tab"], refs["d_att_tab"], bb["d_att_tab"])[0] > 1.0


# --------------------------------------------------------------------------------------------- the RMS norm: stand-ins
def norm_problem(dtype, rows, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.randn(rows, C, generator=g) * 3).to(dtype), (torch.rand(C, generator=g) + 0.5).to(dtype),
            torch.randn(rows, C, generator=g).to(dtype))


def rms_forward_f32(x, w, eps, dtype, shift=False):
    x32 = x.float()
    rstd = torch.rsqrt(x32.pow(2).mean(-1) + eps)
    used = torch.roll(rstd, 1) if shift else rstd                  # (fault: rstd of row r used for row r + 1)
    xn = x32 * used[:, None]
    y = w.float() * (xn.to(dtype).float() if dtype != torch.float32 else xn)
    return dict(y=y.to(dtype), rstd=rstd)


def rms_backward_f32(dy, x, w, rstd, dtype, skip_row=None):
    x32, g32 = x.float(), dy.float()
    xn = x32 * rstd[:, None]
    gw = g32 * w.float()
    dot = (gw * xn).mean(-1, keepdim=True)
    terms = g32 * (xn.to(dtype).float() if dtype != torch.float32 else xn)
    if skip_row is not None:
        terms = torch.cat((terms[:skip_row], terms[skip_row + 1:]))
    return dict(dx=(rstd[:, None] * (gw - xn * dot)).to(dtype), dw=terms.sum(0))


@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsnorm_bounds_pass_the_honest_and_fail_the_planted_faults(dtype):
    rows, C, eps = 24581, 64, 1e-6
    x, w, dy = norm_problem(dtype, rows, C)
    f = R.rmsnorm64(x, w, eps, dtype)
    fb = R.rmsnorm_forward_bounds(f, w, dtype, C)
    got = rms_forward_f32(x, w, eps, dtype)
    honest = ratios_of(got, f, fb)
    assert all(v <= 1.0 for v in honest.values()), honest
    assert worst(f["y"].to(dtype), f["y"], fb["y"])[0] <= 1.0 and worst(f["rstd"].float(), f["rstd"], fb["rstd"])[0] <= 1.0
    bad = ratios_of(rms_forward_f32(x, w, eps, dtype, shift=True), f, fb)
    assert bad["y"] > 1.0 and bad["rstd"] <= 1.0, bad
    # backward, on the stand-in's own rstd; the grid of the partials entry point
    rstd = got["rstd"]
    b = R.rmsnorm_backward64(dy, x, w, rstd, dtype)
    for atomic in (False, True):
        grid = R.norm_grid(rows, 128 if atomic else 512)               # (the two entry points' default grids)
        bb, chain = R.rmsnorm_backward_bounds(b, dtype, rows, C, grid, atomic)
        assert chain == -(-rows // (4 * grid)) + 5 + (grid if atomic else 0)
        honest = ratios_of(rms_backward_f32(dy, x, w, rstd, dtype), b, bb)
        assert all(v <= 1.0 for v in honest.values()), honest
        assert worst(b["dx"].to(dtype), b["dx"], bb["dx"])[0] <= 1.0 and worst(b["dw"].float(), b["dw"], bb["dw"])[0] <= 1.0
        # one row of 24 581 missing from the fp32 gain gradient; in EVERY column an average-sized term is above the bound
        bad = rms_backward_f32(dy, x, w, rstd, dtype, skip_row=12345)
        assert worst(bad["dw"], b["dw"], bb["dw"])[0] > 1.0
        assert float((b["dw_sum"] / rows / bb["dw"]).min()) >= 2.0, float((b["dw_sum"] / rows / bb["dw"]).min())


def test_the_old_bar_accepts_a_dropped_row_in_bf16():
    """test_rmsnorm_kernel_matches_the_reference_norm held the gain gradient AFTER its rounding to bf16 to 2 x 1.6e-2 of
    its largest entry: a row missing from a sum of 24 581 passes that, and not the fp32 per-element bound."""
    dtype, rows, C = torch.bfloat16, 24581, 64
    x, w, dy = norm_problem(dtype, rows, C)
    rstd = rms_forward_f32(x, w, 1e-6, dtype)["rstd"]
    b = R.rmsnorm_backward64(dy, x, w, rstd, dtype)
    bad = rms_backward_f32(dy, x, w, rstd, dtype, skip_row=12345)["dw"]
    old = float((bad.to(dtype).double() - b["dw"]).abs().max() / b["dw"].abs().max())
    assert old <= 2 * 1.6e-2, old
    bb, _ = R.rmsnorm_backward_bounds(b, dtype, rows, C, R.norm_grid(rows, 512), False)
    assert worst(bad, b["dw"], bb["dw"])[0] > 1.0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_near_tie_flags_every_rounding_that_parts(dtype):
    """Where an fp32 evaluation of xn rounds to another 16-bit number than the fp64 one, near_tie has flagged it."""
    rows, C = 6000, 256
    x, w, _ = norm_problem(dtype, rows, C, seed=3)
    f = R.rmsnorm64(x, w, 1e-6, dtype)
    x32 = x.float()
    xn32 = x32 * torch.rsqrt(x32.pow(2).mean(-1, keepdim=True) + 1e-6)
    parted = xn32.to(dtype).double() != f["xn_r"]
    flagged = R.near_tie(f["xn"], dtype, R.rms_delta(dtype, C))
    assert bool(parted.any()) and not bool((parted & ~flagged).any())
    assert float(flagged.double().mean()) < 0.05


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_layer_norm_bounds_pass_the_honest_and_fail_a_misplaced_mean(dtype):
    g = torch.Generator().manual_seed(5)
    B, C, HW, eps = 2, 40, 24, 1e-6
    x = (torch.randn(B, C, HW, generator=g) * 1.5 + 0.3).to(dtype)
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).to(dtype), (0.1 * torch.randn(C, generator=g)).to(dtype)
    pos = torch.randn(HW, C, generator=g).to(dtype)
    for p in (pos, None):
        f = R.layer_norm_tokens64(x, gamma, beta, p, eps, dtype)
        fb = R.layer_norm_tokens_bounds(f, dtype, C, eps)
        tok = x.float().transpose(1, 2)
        mean = tok.mean(-1)
        rstd = torch.rsqrt((tok - mean[..., None]).pow(2).mean(-1) + eps)
        o = ((tok - mean[..., None]) * rstd[..., None] * gamma.float() + beta.float()).to(dtype)
        q = o if p is None else (o.float() + p.float()).to(dtype)
        honest = ratios_of(dict(q=q, mean=mean, rstd=rstd), f, fb)
        assert all(v <= 1.0 for v in honest.values()), honest
        bad = ratios_of(dict(q=q, mean=torch.roll(mean, 1, 1), rstd=rstd), f, fb)              # mean written at the wrong token
        assert bad["mean"] > 1.0 and bad["rstd"] <= 1.0, bad


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_linear_bound_passes_fp32_sums_and_fails_a_dropped_piece(dtype):
    g = torch.Generator().manual_seed(9)
    Mr, Nr, K = 3, 37, 5120
    x, w = torch.randn(Mr, K, generator=g).to(dtype), (torch.randn(Nr, K, generator=g) / K ** 0.5).to(dtype)
    b, res = torch.randn(Nr, generator=g).to(dtype), torch.randn(Mr, Nr, generator=g).to(dtype)
    y64, s = R.linear64(x, w, b)
    assert R.linear_chain(K) == 9 * 10 + 7
    y32 = (x.float() @ w.float().t() + b.float()).to(dtype)
    assert worst(y32, y64, R.linear_bounds(y64, s, K, dtype))[0] <= 1.0
    two = (y32.float() + res.float()).to(dtype)
    assert worst(two, y64 + res.double(), R.linear_bounds(y64, s, K, dtype, res))[0] <= 1.0
    x2 = x.clone()
    x2[:, 4096:4104] = 0                                        # the first piece of the weight loop's second trip
    bad = (x2.float() @ w.float().t() + b.float()).to(dtype)
    assert worst(bad, y64, R.linear_bounds(y64, s, K, dtype))[0] > 1.0


# --------------------------------------------------------------------------------------------- argument checks
OK, E_DTYPE, E_DIMS, E_NULL, E_ALIGN, E_UNSUP = 0, -1, -2, -3, -4, -5


from helpers import bound_library as _lib  # noqa: E402


def in_a_child_without_devices(check):
    """Run ``check`` of this module in a fresh interpreter that is shown no GPU.  Every call of the argument checks
    returns before a launch; should one ever get past the host code, it ends as "no device" there, not as a kernel on
    made-up pointers."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=os.pathsep.join(sys.path))
    res = subprocess.run([sys.executable, "-c", f"import test_front_end as t; t.{check}()"], env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]


FAKE = ctypes.c_void_p(4096)        # aligned, never dereferenced on these paths
ODD = ctypes.c_void_p(4100)
#            N  Lq  H  L  P  n   M  Lr  Nr
PLAN_DIMS = [2, 5, 4, 3, 8, 2, 12, 5, 2]


def check_plan_arguments():
    lib = _lib()

    def fwd(dt, dims, ptr=FAKE, ld=None, first=None):
        a = [first or ptr, ptr]
        if ld is None:
            return lib.mmfs_plan_forward(dt, *a, *[ptr] * 9, *dims, None)
        return lib.mmfs_plan_forward_heads(dt, *a, ld[0], ld[1], ptr, ptr, ld[2], ld[3], *[ptr] * 7, *dims, None)

    def bwd(dt, dims, ptr=FAKE, ld=None, first=None, qst=0):
        if ld is None:
            return lib.mmfs_plan_backward(dt, *[ptr] * 8, first or ptr, *[ptr] * 3, *dims, None)
        return lib.mmfs_plan_backward_heads(dt, *[ptr] * 8, first or ptr, ptr, ld[0], ld[1], qst, ptr, ptr, ld[2], ld[3], *dims, None)

    def with_(i, v):
        return PLAN_DIMS[:i] + [v] + PLAN_DIMS[i + 1:]

    cols_off, cols_att = 4 * 2 * 8, 4 * 3 * 8
    for f in (fwd, bwd):
        for packed in (True, False):
            kw = {} if packed else {"ld": (0, 0, 0, 0)}
            assert f(9, PLAN_DIMS, **kw) == E_DTYPE and f(3, PLAN_DIMS, **kw) == E_DTYPE and f(-1, PLAN_DIMS, **kw) == E_DTYPE
            for i in range(7):
                assert f(2, with_(i, -1), **kw) == E_DIMS, i                          # a negative dimension
            for i in (2, 3, 4, 5, 6):
                assert f(2, with_(i, 0), **kw) == E_DIMS, i                           # H, L, P, n, M of 0
            for i in (0, 1, 2, 5, 6):
                assert f(2, with_(i, 2 ** 31), **kw) == E_DIMS, i                     # beyond the 32-bit index range
            assert f(2, with_(7, 3), **kw) == E_DIMS and f(2, with_(7, 0), **kw) == E_DIMS          # Lr not 1 | Lq
            assert f(2, with_(8, 3), **kw) == E_DIMS and f(2, with_(8, 0), **kw) == E_DIMS          # Nr not 1 | N
            for p in (1, 2, 3, 6, 12, 32):
                assert f(2, with_(4, p), **kw) == E_UNSUP, p                          # P outside {4, 8, 16}
            assert f(2, with_(5, 22), **kw) == E_UNSUP                                # n L = 66 > 64
            assert f(2, [40000, 40000, 4, 3, 8, 2, 12, 40000, 1], **kw) == E_DIMS     # N Lq H beyond the index range
            assert f(2, [0, 5, 4, 3, 8, 2, 12, 5, 1], ptr=None, **kw) == OK and f(2, [2, 0, 4, 3, 8, 2, 12, 0, 2], ptr=None, **kw) == OK
            assert f(2, PLAN_DIMS, ptr=None, **kw) == E_NULL
            assert f(2, PLAN_DIMS, first=ODD, **kw) == E_ALIGN                        # off_q / d_off_q off the vector width
        # M up to 2^31 - 1 is admitted by the dimension check (the backward's row key carries 32 bits of it)
        assert f(2, with_(6, 2 ** 31 - 1), ptr=None) == E_NULL
        # the stacked entry points: a leading dimension below the row, or off the 16-byte vector
        assert f(2, PLAN_DIMS, ld=(cols_off - 8, 0, 0, 0)) == E_DIMS and f(2, PLAN_DIMS, ld=(0, cols_att - 8, 0, 0)) == E_DIMS
        assert f(2, PLAN_DIMS, ld=(0, 0, cols_off - 8, 0)) == E_DIMS and f(2, PLAN_DIMS, ld=(0, 0, 0, cols_att - 8)) == E_DIMS
        assert f(2, PLAN_DIMS, ld=(2 ** 31, 0, 0, 0)) == E_DIMS
    # forward: the heads' and the tables' rows are read as 16-byte vectors of 2-byte elements
    for i in range(4):
        ld = [0, 0, 0, 0]
        ld[i] = (cols_att if i % 2 else cols_off) + 4
        assert fwd(2, PLAN_DIMS, ld=ld) == E_ALIGN, i
    # backward: fp32 query gradients want 16-byte rows of 4-byte elements, those in the storage type of 2-byte ones (the
    # tables' rows are fp32 scalars: any pitch that holds the row)
    assert bwd(2, PLAN_DIMS, ld=(cols_off + 2, 0, 0, 0), qst=0) == E_ALIGN and bwd(2, PLAN_DIMS, ld=(0, cols_att + 2, 0, 0), qst=0) == E_ALIGN
    assert bwd(2, PLAN_DIMS, ld=(cols_off + 4, 0, 0, 0), qst=1) == E_ALIGN and bwd(2, PLAN_DIMS, ld=(0, cols_att + 4, 0, 0), qst=1) == E_ALIGN


def check_rmsnorm_arguments():
    lib = _lib()
    sup = lib.mmfs_rmsnorm_supported
    for dt, n in ((0, 4), (1, 8), (2, 8)):
        for C in (0, -8, 4, 8, 12, 72, 4096, 8192, 8200, 16384):
            assert sup(dt, C) == int(C > 0 and C % n == 0 and C // n <= 1024), (dt, C)
    assert sup(3, 64) == 0 and sup(-1, 64) == 0
    for rows, want in ((0, 0), (-3, 0), (1, 1), (5, 2), (2048, 512), (10 ** 6, 512)):
        assert lib.mmfs_rmsnorm_backward_partials_rows(rows) == want

    def fwd(dt, rows, C, x=FAKE, w=FAKE, y=FAKE, rstd=FAKE):
        return lib.mmfs_rmsnorm_forward(dt, x, w, y, rstd, rows, C, 1e-6, None)

    def bwd(f):
        return lambda dt, rows, C, p=FAKE, rstd=FAKE, gw=FAKE, first=None: f(dt, first or p, p, p, rstd, p, gw, rows, C, None)

    assert fwd(9, 4, 64) == E_DTYPE and fwd(-1, 4, 64) == E_DTYPE
    assert fwd(2, -1, 64) == E_DIMS and fwd(2, 4, -8) == E_DIMS
    assert fwd(2, 0, 64, None, None, None, None) == OK and fwd(2, 4, 0, None, None, None, None) == OK
    assert fwd(2, 4, 12) == E_UNSUP and fwd(0, 4, 6) == E_UNSUP and fwd(2, 4, 8200) == E_UNSUP and fwd(0, 4, 8192) == E_UNSUP
    assert fwd(2, 4, 64, x=None) == E_NULL and fwd(2, 4, 64, w=None) == E_NULL and fwd(2, 4, 64, y=None) == E_NULL
    assert fwd(2, 4, 64, x=ODD) == E_ALIGN and fwd(2, 4, 64, w=ODD) == E_ALIGN and fwd(2, 4, 64, y=ODD) == E_ALIGN
    for f in (bwd(lib.mmfs_rmsnorm_backward), bwd(lib.mmfs_rmsnorm_backward_partials)):
        assert f(9, 4, 64) == E_DTYPE and f(2, -1, 64) == E_DIMS and f(2, 4, -8) == E_DIMS
        assert f(2, 0, 64, p=None, rstd=None, gw=None) == OK and f(2, 4, 0, p=None, rstd=None, gw=None) == OK
        assert f(2, 4, 12) == E_UNSUP and f(0, 4, 8192) == E_UNSUP
        assert f(2, 4, 64, p=None) == E_NULL and f(2, 4, 64, rstd=None) == E_NULL and f(2, 4, 64, gw=None) == E_NULL
        assert f(2, 4, 64, first=ODD) == E_ALIGN


def check_layout_arguments():
    lib = _lib()
    sup = lib.mmfs_query_prep_supported
    for dt in (0, 1, 2, 3):
        for C in (0, 8, 12, 40, 2048, 2056):
            for HW in (0, 8, 12, 4096):
                assert sup(dt, C, HW) == int(dt in (1, 2) and 0 < C <= 2048 and C % 8 == 0 and HW > 0 and HW % 8 == 0), (dt, C, HW)

    def prep(dt, B, C, HW, p=FAKE, mean=FAKE, rstd=FAKE, pos=FAKE, first=None):
        return lib.mmfs_query_prep(dt, first or p, p, p, pos, p, mean, rstd, B, C, HW, 1e-6, None)

    def add(dt, B, C, HW, p=FAKE, mean=None, rstd=None, pos=None, first=None):
        return lib.mmfs_tokens_add(dt, first or p, p, p, B, C, HW, None)

    for f in (prep, add):
        assert f(9, 2, 64, 16) == E_DTYPE and f(3, 2, 64, 16) == E_DTYPE and f(-1, 2, 64, 16) == E_DTYPE
        assert f(2, -1, 64, 16) == E_DIMS and f(2, 2, -8, 16) == E_DIMS and f(2, 2, 64, -8) == E_DIMS
        for dims in ((0, 64, 16), (2, 0, 16), (2, 64, 0)):
            assert f(2, *dims, p=None, mean=None, rstd=None, pos=None) == OK
        assert f(0, 2, 64, 16) == E_UNSUP                                              # fp32 storage stays on the framework
        assert f(2, 2, 12, 16) == E_UNSUP and f(2, 2, 64, 12) == E_UNSUP and f(2, 2, 2056, 16) == E_UNSUP
        assert f(2, 65536, 64, 16) == E_UNSUP
        assert f(2, 2, 64, 16, p=None) == E_NULL
        assert f(2, 2, 64, 16, first=ODD) == E_ALIGN
    assert prep(2, 2, 64, 16, rstd=None) == E_NULL and prep(2, 2, 64, 16, mean=None) == E_NULL      # statistics: both or none
    assert prep(2, 2, 64, 16, pos=ODD) == E_ALIGN


def check_linear_arguments():
    lib = _lib()
    sup = lib.mmfs_linear_small_supported
    for dt in (0, 1, 2, 3):
        for Mr in (0, 1, 4, 5, 8, 9):
            for K in (0, 4, 8, 12, 4096, 4104, 8192, 8200):
                want = int(dt in (1, 2) and 1 <= Mr <= 8 and K >= 8 and K % 8 == 0 and (4 if Mr <= 4 else 8) * K * 2 <= 65536)
                assert sup(dt, Mr, 37, K) == want, (dt, Mr, K)
    assert sup(2, 4, 0, 64) == 0 and sup(2, 4, 2 ** 30, 64) == 0 and sup(2, 4, 2 ** 30 - 1, 64) == 1

    def add(dt, Mr, Nr, K, ldx=None, ldy=None, ldr=None, x=FAKE, w=FAKE, y=FAKE, res=FAKE):
        return lib.mmfs_linear_small_add(dt, x, w, FAKE, res, y, Mr, Nr, K, K if ldx is None else ldx, Nr if ldy is None else ldy,
                                         Nr if ldr is None else ldr, None)

    def plain(dt, Mr, Nr, K, ldx=None, ldy=None, ldr=None, x=FAKE, w=FAKE, y=FAKE, res=None):
        return lib.mmfs_linear_small(dt, x, w, FAKE, y, Mr, Nr, K, K if ldx is None else ldx, Nr if ldy is None else ldy, None)

    for f in (add, plain):
        assert f(9, 4, 37, 64) == E_DTYPE and f(3, 4, 37, 64) == E_DTYPE and f(-1, 4, 37, 64) == E_DTYPE
        assert f(2, -1, 37, 64) == E_DIMS and f(2, 4, -1, 64) == E_DIMS and f(2, 4, 37, -8) == E_DIMS
        assert f(2, 0, 37, 64, x=None, w=None, y=None, res=None) == OK and f(2, 4, 0, 64, x=None, w=None, y=None, res=None) == OK
        assert f(0, 4, 37, 64) == E_UNSUP and f(2, 9, 37, 64) == E_UNSUP and f(2, 4, 37, 12) == E_UNSUP
        assert f(2, 4, 37, 0) == E_UNSUP and f(2, 4, 37, 8200) == E_UNSUP and f(2, 8, 37, 4104) == E_UNSUP
        assert f(2, 4, 37, 64, x=None) == E_NULL and f(2, 4, 37, 64, w=None) == E_NULL and f(2, 4, 37, 64, y=None) == E_NULL
        assert f(2, 4, 37, 64, ldx=56) == E_DIMS and f(2, 4, 37, 64, ldy=36) == E_DIMS
        assert f(2, 4, 37, 64, x=ODD) == E_ALIGN and f(2, 4, 37, 64, w=ODD) == E_ALIGN
        assert f(2, 4, 37, 64, ldx=68) == E_ALIGN                                      # rows of x off the 16-byte vector
    assert add(2, 4, 37, 64, ldr=36) == E_DIMS


@pytest.mark.parametrize("check", ["check_plan_arguments", "check_rmsnorm_arguments", "check_layout_arguments",
                                   "check_linear_arguments"])
def test_argument_errors_and_empty_problems_return_before_any_launch(check):
    """mmfs_plan_forward[_heads], mmfs_plan_backward[_heads], mmfs_rmsnorm_forward / _backward / _backward_partials /
    _supported, mmfs_query_prep / mmfs_tokens_add / _supported, mmfs_linear_small[_add] / _supported: dtype, negative and
    oversized dimensions, Lr / Nr, P, n L > 64, NULL, misaligned pointers, leading dimensions below the row or off the
    vector width, unsupported shapes, and empty problems that look at nothing."""
    in_a_child_without_devices(check)
