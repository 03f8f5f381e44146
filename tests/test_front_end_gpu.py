"""The kernels around the op -- sampling plan, RMS norm, layout kernels, decode Linear -- through the C ABI, every element
of every output against the fp64 statement of front_end_refs.py under its derived bound, outputs allocated poisoned.

Gaps of the earlier tests that the cases here close (each named again in its test's docstring):
    csrc/mmfs_plan.hip    P = 16; every lane-group width G; the ``_heads`` strides; q_grads_in_storage_type; grad_sink = NULL;
                          Lq < 8; the mid-run flush; the cross-group merge; a table higher than 2^20 rows
    csrc/mmfs_norm.hip    rows past one pass of the grid for all three kernels; the atomic backward; fp32 partials
    csrc/mmfs_query.hip   mean / rstd; C < 64; HW = 8; a 64 x 64 map
    csrc/mmfs_linear.hip  K > 4096; MMFS_LIN_ROWS / MMFS_LIN_UNROLL / MMFS_LIN_EARLY"""
import pytest
import torch

import front_end_refs as R
import helpers
from front_end_refs import worst
from helpers import STORAGE_T, STORAGE_U

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
HALVES = [torch.float16, torch.bfloat16]
CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def lib():
    import MultiScaleDeformableAttention as MSDA
    return MSDA._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def name(dtype):
    return str(dtype)[6:]


def collect(report, res, what):
    for k, v in res.items():
        report[k] = max(report.get(k, 0.0), v[0])
    bad = {k: v for k, v in res.items() if not v[0] <= 1.0}
    assert not bad, f"{what}: bound broken (ratio, index, got, ref, bound): {bad}"


def line(tag, report):
    return tag + " worst ratios " + " ".join(f"{k} {v:.3f}" for k, v in report.items())


# --------------------------------------------------------------------------------------------- the sampling plan
#   (n, L): n L = 3, 4, 6, 12, 16, 20, 33, 64 -- G = 4, 4, 8, 16, 16, 32, 64, 64: a full group and a partly filled one of
#   each width;  Lq 1, 3, 8, 37;  Lr = Lq | 1;  Nr = N | 1;  stacked (``_heads``, ld = C, H = 4) | packed (H = 3);
#   q_grads_in_storage_type;  grad_sink given | NULL;  relpos variants:
#     a  one image invisible for all queries          b  one query (Lr = Lq) / one sample (Lr = 1) with every image invisible
#     c  a relative position that changes inside a run of 8 queries and again at a run's end        d  two samples share rows
PLAN_CASES = [
    # n,  L, Lq, Lr=Lq, Nr=N, stacked, qst, sink, variants
    (1, 3, 37, True, True, False, 0, True, "bc"),
    (2, 2, 8, True, False, True, 1, True, "abd"),
    (2, 3, 3, False, True, False, 0, False, "b"),
    (3, 4, 37, True, False, True, 0, True, "acd"),
    (4, 4, 1, True, True, True, 1, False, "ab"),
    (5, 4, 37, False, True, False, 0, True, "ad"),
    (11, 3, 37, True, True, True, 1, True, "abcd"),
    (16, 4, 8, True, False, False, 0, False, "abc"),
]
N_PLAN, M_PLAN = 2, 12


def make_relpos(n, Lq, Lr, variants, g):
    rp = torch.randint(1, M_PLAN, (N_PLAN, Lr, n), device=DEV, generator=g)
    if "c" in variants and Lr > 16:
        q = torch.arange(Lr, device=DEV)
        rp[0, :, n - 1] = torch.where(q < 5, 3, torch.where(q < 16, 7, 9))          # changes inside run 0 and at the end of run 1
    if "d" in variants:
        rp[1] = rp[0]
    if "a" in variants and n > 1:
        rp[:, :, 0] = 0
    if "b" in variants:
        rp[1 if Lr > 1 else 0, Lr // 2] = 0
    return rp


def plan_inputs(dtype, n, L, Lq, Lr, Nr, H, P, variants, seed, M=M_PLAN, relpos=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    N, n_off = N_PLAN, H * P * 2
    C = n_off + H * L * P

    def stacked(rows):
        t = torch.empty(*rows, C, device=DEV, dtype=torch.float32)
        t[..., :n_off] = torch.randn(*rows, n_off, device=DEV, generator=g) * (2.0 if len(rows) == 2 else 1.0)
        t[..., n_off:] = torch.rand(*rows, C - n_off, device=DEV, generator=g) * 8.0 - 4.0      # |att_q + att_tab| <= 8
        return t.to(dtype)

    both, tabs = stacked((N, Lq)), stacked((M,))
    if relpos is None:
        relpos = make_relpos(n, Lq, Lr, variants, g)
    return dict(both=both, tabs=tabs, relpos=relpos, n_off=n_off, C=C,
                ref=torch.rand(Nr, Lq, 2, device=DEV, generator=g),
                shapes=torch.randint(1, 41, (n * L, 2), device=DEV, generator=g),
                ratios=torch.rand(L, device=DEV, generator=g) * 1.5 + 0.5)


def plan_forward(dtype, c, dims, stacked):
    N, Lq, H, L, P, n, M, Lr, Nr = dims
    es, n_off, C = c["both"].element_size(), c["n_off"], c["C"]
    loc = torch.empty(N, Lq, H, n * L, P, 2, device=DEV, dtype=dtype)
    attn = torch.empty(N, Lq, H, n * L, P, device=DEV, dtype=dtype)
    sink = torch.empty(N, Lq, H, device=DEV, dtype=torch.float32)
    tail = (c["relpos"].data_ptr(), c["ref"].data_ptr(), c["shapes"].data_ptr(), c["ratios"].data_ptr(), loc.data_ptr(),
            attn.data_ptr(), sink.data_ptr(), *dims, stream())
    if stacked:
        rc = lib().mmfs_plan_forward_heads(CODE[dtype], c["both"].data_ptr(), c["both"].data_ptr() + n_off * es, C, C,
                                           c["tabs"].data_ptr(), c["tabs"].data_ptr() + n_off * es, C, C, *tail)
    else:
        c["packed"] = [t.contiguous() for t in (c["both"][..., :n_off], c["both"][..., n_off:], c["tabs"][..., :n_off],
                                                c["tabs"][..., n_off:])]
        rc = lib().mmfs_plan_forward(CODE[dtype], *[t.data_ptr() for t in c["packed"]], *tail)
    assert rc == 0, rc
    return loc, attn, sink


def plan_backward(dtype, c, dims, stacked, qst, g_loc, g_attn, g_sink, attn, sink):
    N, Lq, H, L, P, n, M, Lr, Nr = dims
    n_off, C = c["n_off"], c["C"]
    qt = dtype if (qst and stacked) else torch.float32
    head = (CODE[dtype], g_loc.data_ptr(), g_attn.data_ptr(), None if g_sink is None else g_sink.data_ptr(), attn.data_ptr(),
            sink.data_ptr(), c["relpos"].data_ptr(), c["shapes"].data_ptr(), c["ratios"].data_ptr())
    if stacked:
        d_both = torch.empty(N, Lq, C, device=DEV, dtype=qt)
        d_tabs = torch.zeros(M, C, device=DEV, dtype=torch.float32)            # (accumulated into: zeroed as the package does)
        rc = lib().mmfs_plan_backward_heads(*head, d_both.data_ptr(), d_both.data_ptr() + n_off * d_both.element_size(), C, C,
                                            int(bool(qst)), d_tabs.data_ptr(), d_tabs.data_ptr() + n_off * 4, C, C, *dims, stream())
        out = (d_both[..., :n_off], d_both[..., n_off:], d_tabs[..., :n_off], d_tabs[..., n_off:])
    else:
        out = (torch.empty(N, Lq, n_off, device=DEV), torch.empty(N, Lq, C - n_off, device=DEV),
               torch.zeros(M, n_off, device=DEV), torch.zeros(M, C - n_off, device=DEV))
        rc = lib().mmfs_plan_backward(*head, *[t.data_ptr() for t in out], *dims, stream())
    assert rc == 0, rc
    return dict(zip(("d_off_q", "d_att_q", "d_off_tab", "d_att_tab"), out)), qt


def check_plan(dtype, P, case, seed, report, M=M_PLAN, relpos=None):
    n, L, Lq, lr_q, nr_n, stacked, qst, with_sink, variants = case
    N, H = N_PLAN, (4 if stacked else 3)
    Lr, Nr = (Lq if lr_q else 1), (N if nr_n else 1)
    dims = (N, Lq, H, L, P, n, M, Lr, Nr)
    c = plan_inputs(dtype, n, L, Lq, Lr, Nr, H, P, variants, seed, M, relpos)
    what = f"plan {name(dtype)} P={P} n={n} L={L} Lq={Lq} Lr={Lr} Nr={Nr} stacked={stacked} qst={qst} sink={with_sink} {variants}"
    loc, attn, sink = plan_forward(dtype, c, dims, stacked)
    n_off = c["n_off"]
    f = R.plan_forward64(c["both"][..., :n_off], c["both"][..., n_off:], c["tabs"][..., :n_off], c["tabs"][..., n_off:],
                         c["relpos"], c["ref"], c["shapes"], c["ratios"], H, L, P)
    fb = R.plan_forward_bounds(f, dtype)
    res = {k: worst(t, f[k], fb[k]) for k, t in (("attn", attn), ("loc", loc), ("sink", sink))}
    # every weight of an invisible image is exactly 0, and where every image is invisible the sink takes everything
    gone = (c["relpos"].expand(N, Lq, n) == 0)
    rows = gone[:, :, None, :, None, None].expand(N, Lq, H, n, L, P).reshape(attn.shape)
    assert not bool(attn[rows].any()), what
    if "b" in variants:
        assert bool(gone.all(-1).any()) and bool((sink[gone.all(-1)] - 1.0).abs().max() <= 2.0 ** -22), what
    g = torch.Generator(device=DEV).manual_seed(seed + 5)
    g_loc = torch.randn(loc.shape, device=DEV, generator=g).to(dtype)
    g_attn = torch.randn(attn.shape, device=DEV, generator=g).to(dtype)
    g_sink = torch.randn(sink.shape, device=DEV, generator=g) if with_sink else None
    got, qt = plan_backward(dtype, c, dims, stacked, qst, g_loc, g_attn, g_sink, attn, sink)
    refs, sums = R.plan_backward64(g_loc, g_attn, g_sink, attn, sink, c["relpos"], c["shapes"], c["ratios"], H, L, P, M)
    bb = R.plan_backward_bounds(refs, sums, c["relpos"], N, Lq, L, n, M, dtype, qt)
    res.update({k: worst(got[k], refs[k], bb[k]) for k in refs})
    used = torch.zeros(M, dtype=torch.bool, device=DEV)
    used[c["relpos"].reshape(-1)] = True
    assert not bool(got["d_att_tab"][~used].any()) and not bool(got["d_off_tab"][~used].any()), what
    collect(report, res, what)
    return c, dims, loc, attn


@pytest.mark.parametrize("P", [4, 8, 16])
@pytest.mark.parametrize("dtype", DTYPES)
def test_plan_kernels_element_by_element(dtype, P, monkeypatch):
    """mmfs_plan_forward[_heads] / mmfs_plan_backward[_heads] through the C ABI: attn, loc, sink, d_off_q, d_att_q and the
    two fp32 table gradients, every element under front_end_refs' bounds; weights of invisible images exactly 0; table
    rows no sample refers to exactly 0.  Closes: P = 16 (dispatched and admitted, never run before); every lane-group
    width G = 4 .. 64 with a full and a partly filled group (n L = 3, 4, 6, 12, 16, 20, 33, 64) for every P; the
    ``_heads`` strides (both tensors stacked in one row, ld = C); q_grads_in_storage_type 0 and 1; grad_sink given and
    NULL; Lq = 1, 3 (< 8); the mid-run flush (variant c) and the cross-group merge (variant d: two samples, equal rows).
    The backward runs on the kernel's own stored attn / sink, as the operator package saves them."""
    helpers.poison_allocations(monkeypatch)
    report = {}
    for i, case in enumerate(PLAN_CASES):
        check_plan(dtype, P, case, 100 * P + i, report)
    print(line(f"PLAN-MMFS-BOUNDS {name(dtype)} P={P}", report))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_plan_backward_table_rows_above_2_to_the_20(dtype, monkeypatch):
    """A table of 2^20 + 6 rows, H = 1, Lq = 4: sample 0 at relative position 2^20 + 5 and sample 1 at 5.  The key that
    names a lane's table row in the cross-group merge used to pack the position into 20 bits, so these two rows shared a
    key: sample 1's gradient was added to row 2^20 + 5 and row 5 stayed 0.  The key now carries 32 bits of each part."""
    helpers.poison_allocations(monkeypatch)
    M = 2 ** 20 + 6
    relpos = torch.tensor([[[M - 1]], [[5]]], device=DEV)
    report = {}
    c, _, _, _ = check_plan(dtype, 4, (1, 1, 4, False, True, False, 0, True, ""), 7, report, M=M, relpos=relpos)
    print(line(f"PLAN-MMFS-BOUNDS {name(dtype)} M=2^20+6", report))


@pytest.mark.parametrize("P", [4, 8, 16])
@pytest.mark.parametrize("dtype", HALVES)
def test_sampler_after_the_plan_on_the_plans_own_numbers(dtype, P, monkeypatch):
    """The kernel's own loc / attn, read back as stored, are what the sampler that follows must have used: the fused
    sampler (mmfs_sample_forward_heads) at P = 4 and 8 and, at P = 16, which the fused sampler refuses, the op itself,
    against the fp64 oracle under helpers' bound."""
    import MultiScaleDeformableAttention as MSDA
    from mmfs_amd.functions.mmfs_plan_func import mmfs_sample_forward
    helpers.poison_allocations(monkeypatch)
    n, L, Lq, D, H = 2, 3, 37, 32, 3
    report = {}
    c, dims, loc, attn = check_plan(dtype, P, (n, L, Lq, True, True, False, 0, True, "a"), 900 + P, report)
    sh, st = helpers.level_tables(c["shapes"].tolist(), DEV)
    g = torch.Generator(device=DEV).manual_seed(3)
    value = torch.rand(N_PLAN, int(sh.prod(1).sum()), H, D, device=DEV, generator=g).to(dtype)
    fused = mmfs_sample_forward(value, sh, st, *c["packed"], c["relpos"], c["ref"], c["ratios"], H, L, P)
    if P == 16:
        assert fused is None
        out = MSDA.ms_deform_attn_forward(value, sh, st, loc, attn, 64)
    else:
        assert fused is not None
        out = fused[0]
    torch.cuda.synchronize()
    x = dict(value=value.double().cpu(), shapes=sh.cpu(), start=st.cpu(), loc=loc.double().cpu(), attn=attn.double().cpu(),
             grad=torch.zeros(N_PLAN, Lq, H * D, dtype=torch.float64))
    rep = {}
    helpers.assert_within_bounds((out.double().cpu().numpy(), None, None, None), x, dtype, what=f"sampler P={P}",
                                 outputs=("out",), report=rep)
    print(f"PLAN-MMFS-BOUNDS {name(dtype)} P={P} sampler on the plan's numbers: out {rep['out']:.3f}")


SAMPLER_WALKS = [
    # dtype, D: lanes per query = D * element size / 16; a chunk holds max(2 * lanes, P) samples per query
    (torch.float32, 16, "4 lanes: the 8 samples are one chunk of the pipelined walk"),
    (torch.bfloat16, 32, "4 lanes, 16-bit rows"),
    (torch.float32, 256, "64 lanes: the walk without live words, a wave per query"),
    (torch.bfloat16, 8, "1 lane: chunks of 4 samples, two per query"),
]


@pytest.mark.parametrize("live", [0, 1, 2, 3, 4, 5, 8, "image"])
@pytest.mark.parametrize("dtype,D,what", SAMPLER_WALKS, ids=[f"{name(w[0])}-D{w[1]}" for w in SAMPLER_WALKS])
def test_fused_sampler_walks_at_their_smallest(dtype, D, what, live, monkeypatch):
    """mmfs_sample_fwd's walks over a chunk's tap records where each branch is alone, equal bit for bit to the plan kernel
    followed by the op's row gather: three queries (a ragged tile) of one head with 8 samples each (levels 3 x 5 and
    2 x 2, P = 4), of which the first ``live`` keep their logit and the others get -1e4 -- a softmax weight of exactly 0
    in every storage type, so their taps are not walked: no live tap, the odd prologue alone, the pair without the loop,
    one loop trip, every tap.  "image": two images of one level each, the first one invisible (relpos 0).  The middle
    query of sample 0 weighs nothing at all: with 64 lanes per query it is a wave that skips every pair."""
    import MultiScaleDeformableAttention as MSDA
    from mmfs_amd.functions.mmfs_plan_func import mmfs_sample_forward, sample_forward_groups
    helpers.poison_allocations(monkeypatch)
    monkeypatch.setenv("MMFS_SAMPLE_DECODE", "0")            # (3 queries are decode-sized: this is about mmfs_sample_fwd)
    n, L = (2, 1) if live == "image" else (1, 2)
    Lq, H, P, N = 3, 1, 4, N_PLAN
    assert sample_forward_groups(dtype, Lq, D, n * L, P) == 1
    c = plan_inputs(dtype, n, L, Lq, Lq, N, H, P, "", seed=77)
    c["shapes"] = torch.tensor([(3, 5), (2, 2)], device=DEV)
    att = c["both"][..., c["n_off"]:]                        # [N, Lq, L * P]: the logits in sample order for one image
    if live == "image":
        c["relpos"][:, :, 0] = 0
        dead = torch.arange(8, device=DEV) < 4
    else:
        dead = torch.arange(8, device=DEV) >= live
        att[..., dead] = -1e4
        att[0, 1] = -1e4
    dims = (N, Lq, H, L, P, n, M_PLAN, Lq, N)
    loc, attn, sink = plan_forward(dtype, c, dims, stacked=False)
    assert not bool(attn.reshape(N, Lq, 8)[..., dead].any()) and bool(attn.reshape(N, Lq, 8)[1][..., ~dead].all())
    sh, st = helpers.level_tables(c["shapes"].tolist(), DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    value = torch.rand(N, 19, H, D, device=DEV, generator=g).to(dtype)
    token = torch.randn(H, D, device=DEV, generator=g).to(dtype)
    old, MSDA._fwd_algo = MSDA._fwd_algo, "gather"
    try:
        op = MSDA.ms_deform_attn_forward(value, sh, st, loc, attn, 64)
    finally:
        MSDA._fwd_algo = old
    for tok in (None, token):
        fused = mmfs_sample_forward(value, sh, st, *c["packed"], c["relpos"], c["ref"], c["ratios"], H, L, P, token=tok)
        assert fused is not None, what
        want = op if tok is None else op + (tok.reshape(1, 1, H * D) * sink.to(dtype).repeat_interleave(D, -1)).to(dtype)
        assert torch.equal(fused[0], want) and torch.equal(fused[1], sink), what
    if live == 0:
        assert not bool(op.any())


# --------------------------------------------------------------------------------------------- the RMS norm
NORM_ROWS = (1, 3, 5, 74, 2049, 24581)


def norm_widths(dtype):
    return (4, 72, 1024, 4096) if dtype == torch.float32 else (8, 72, 1024, 4096, 5120, 8192)


def check_norm(dtype, rows, C, seed, report, grid_env=0):
    L = lib()
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(rows, C, device=DEV, generator=g) * 3).to(dtype)
    w = (torch.rand(C, device=DEV, generator=g) + 0.5).to(dtype)
    dy = torch.randn(rows, C, device=DEV, generator=g).to(dtype)
    eps, what = 1e-6, f"rmsnorm {name(dtype)} rows={rows} C={C} grid={grid_env}"
    y, y2 = torch.empty_like(x), torch.empty_like(x)
    rstd = torch.empty(rows, device=DEV, dtype=torch.float32)
    assert L.mmfs_rmsnorm_forward(CODE[dtype], x.data_ptr(), w.data_ptr(), y.data_ptr(), rstd.data_ptr(), rows, C, eps, stream()) == 0
    assert L.mmfs_rmsnorm_forward(CODE[dtype], x.data_ptr(), w.data_ptr(), y2.data_ptr(), None, rows, C, eps, stream()) == 0
    assert torch.equal(y, y2), what + ": the call without rstd returns other bits"
    f = R.rmsnorm64(x, w, eps, dtype)
    fb = R.rmsnorm_forward_bounds(f, w, dtype, C)
    res = {"y": worst(y, f["y"], fb["y"]), "rstd": worst(rstd, f["rstd"], fb["rstd"])}
    del f, fb, y2
    b = R.rmsnorm_backward64(dy, x, w, rstd, dtype)
    grid_p = L.mmfs_rmsnorm_backward_partials_rows(rows)
    assert grid_p == R.norm_grid(rows, grid_env or 512)
    dx = torch.empty_like(x)
    parts = torch.empty(grid_p, C, device=DEV, dtype=torch.float32)
    assert L.mmfs_rmsnorm_backward_partials(CODE[dtype], dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                            parts.data_ptr(), rows, C, stream()) == 0
    bp, _ = R.rmsnorm_backward_bounds(b, dtype, rows, C, grid_p, atomic=False)
    res["dx"] = worst(dx, b["dx"], bp["dx"])
    assert bool(torch.isfinite(parts).all()), what + ": a partial nobody wrote"
    res["dw_partials"] = worst(parts.double().sum(0), b["dw"], bp["dw"])           # (fp32 partials, summed in fp64)
    grid_a = R.norm_grid(rows, grid_env or 128)
    dx_a = torch.empty_like(x)
    dw = torch.zeros(C, device=DEV, dtype=torch.float32)
    assert L.mmfs_rmsnorm_backward(CODE[dtype], dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), dx_a.data_ptr(),
                                   dw.data_ptr(), rows, C, stream()) == 0
    ba, _ = R.rmsnorm_backward_bounds(b, dtype, rows, C, grid_a, atomic=True)
    res["dx_atomic"] = worst(dx_a, b["dx"], ba["dx"])
    res["dw_atomic"] = worst(dw, b["dw"], ba["dw"])
    collect(report, res, what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsnorm_kernels_element_by_element(dtype, monkeypatch):
    """mmfs_rmsnorm_forward (with and without rstd: the same bits), mmfs_rmsnorm_backward_partials and the atomic
    mmfs_rmsnorm_backward, which no test called: y, rstd, dx, the fp64 sum of the fp32 partials and the atomic dw, every
    element.  Closes: rows past one pass of the grid for all three kernels -- 24 581 rows are three passes of the
    forward's 8192-row grid, twelve of the partials' and 48 of the atomic backward's, 2049 rows one and a bit of the
    partials' -- so the grid-stride loops and the sum over a wave's rows iterate; every NV and a partly filled last vector
    slot (C = 72, 5120); the 7B and 13B widths; MMFS_NORM_BWD_GRID = 7 once (878 rows per wave)."""
    helpers.poison_allocations(monkeypatch)
    report, seed = {}, 0
    for C in norm_widths(dtype):
        for rows in NORM_ROWS:
            if rows > 4096 and C > 1024:
                continue
            seed += 1
            check_norm(dtype, rows, C, seed, report)
    monkeypatch.setenv("MMFS_NORM_BWD_GRID", "7")
    check_norm(dtype, 24581, 72, 99, report, grid_env=7)
    print(line(f"RMSNORM-BOUNDS {name(dtype)}", report))


# --------------------------------------------------------------------------------------------- the layout kernels
QUERY_SHAPES = [(2, 320, 16, 16), (3, 640, 8, 8), (1, 1280, 8, 16), (2, 64, 5, 8), (1, 2048, 4, 6), (2, 328, 12, 10),
                (2, 8, 1, 8), (1, 40, 2, 4), (1, 320, 64, 64), (2, 1280, 16, 16)]


def query_case(dtype, shape, seed):
    B, C, H, W = shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(B, C, H * W, device=DEV, generator=g) * 1.5 + 0.3).to(dtype)
    w = (1.0 + 0.2 * torch.randn(C, device=DEV, generator=g)).to(dtype)
    b = (0.1 * torch.randn(C, device=DEV, generator=g)).to(dtype)
    pos = torch.randn(H * W, C, device=DEV, generator=g).to(dtype)
    return x, w, b, pos


@pytest.mark.parametrize("dtype", HALVES)
def test_query_prep_statistics_and_output_element_by_element(dtype, monkeypatch):
    """mmfs_query_prep with statistics: mean and rstd per token -- which QueryPrepFunction.backward feeds to the
    LayerNorm backward and nothing compared with anything -- and q, every element against fp64; the call without
    statistics returns the same bits.  Closes: mean / rstd; C < 64 (one partly filled swizzle row: C = 8, 40); HW = 8; a
    map of the real 64 x 64 size; mmfs_tokens_add bit-exact at the added shapes."""
    helpers.poison_allocations(monkeypatch)
    L, report, eps = lib(), {}, 1e-6
    for i, shape in enumerate(QUERY_SHAPES):
        B, C, H, W = shape
        HW = H * W
        x, w, b, pos = query_case(dtype, shape, 40 + i)
        for with_pos in (True, False):
            p = pos if with_pos else None
            q, q2 = (torch.empty(B, HW, C, device=DEV, dtype=dtype) for _ in range(2))
            mean, rstd = (torch.empty(B, HW, device=DEV, dtype=torch.float32) for _ in range(2))
            args = (CODE[dtype], x.data_ptr(), w.data_ptr(), b.data_ptr(), None if p is None else p.data_ptr())
            assert L.mmfs_query_prep(*args, q.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, C, HW, eps, stream()) == 0
            assert L.mmfs_query_prep(*args, q2.data_ptr(), None, None, B, C, HW, eps, stream()) == 0
            assert torch.equal(q, q2), f"{shape}: the call without statistics returns other bits"
            f = R.layer_norm_tokens64(x, w, b, p, eps, dtype)
            fb = R.layer_norm_tokens_bounds(f, dtype, C, eps)
            collect(report, {k: worst(t, f[k], fb[k]) for k, t in (("q", q), ("mean", mean), ("rstd", rstd))},
                    f"query_prep {name(dtype)} {shape} pos={with_pos}")
        tok = torch.randn(B, HW, C, device=DEV).to(dtype)
        y = torch.empty(B, C, HW, device=DEV, dtype=dtype)
        assert L.mmfs_tokens_add(CODE[dtype], tok.data_ptr(), x.data_ptr(), y.data_ptr(), B, C, HW, stream()) == 0
        assert torch.equal(y, x + tok.transpose(1, 2)), f"tokens_add {shape}"
    print(line(f"QUERY-BOUNDS {name(dtype)}", report))


@pytest.mark.parametrize("shape", [(2, 64, 5, 8), (3, 320, 16, 16)])
@pytest.mark.parametrize("dtype", HALVES)
def test_layout_functions_gradients_element_by_element(dtype, shape, monkeypatch):
    """QueryPrepFunction / TokensAddFunction: the gradients of sample, weight, bias and pos against fp64 autograd of the
    framework statement, every element (front_end_refs.layer_norm_backward_bounds); the transposed add hands its
    gradient through bit for bit."""
    from mmfs_amd.functions.query_func import QueryPrepFunction, TokensAddFunction
    helpers.poison_allocations(monkeypatch)
    B, C, H, W = shape
    eps = 1e-6
    x, w, b, pos = query_case(dtype, shape, 7)
    g = torch.Generator(device=DEV).manual_seed(8)
    gq = torch.randn(B, H * W, C, device=DEV, generator=g).to(dtype)
    leaves = [t.clone().requires_grad_(True) for t in (x.view(B, C, H, W), w, b, pos)]
    q = QueryPrepFunction.apply(leaves[0], leaves[1], leaves[2], eps, leaves[3])
    q.backward(gq)
    l64 = [t.double().requires_grad_(True) for t in (x, w, b, pos)]
    q64 = torch.nn.functional.layer_norm(l64[0].transpose(1, 2), (C,), l64[1], l64[2], eps) + l64[3]
    q64.backward(gq.double())
    f = R.layer_norm_tokens64(x, w, b, pos, eps, dtype)
    fb = R.layer_norm_tokens_bounds(f, dtype, C, eps)
    ref_gx = l64[0].grad.transpose(1, 2)                                     # as tokens
    bb = R.layer_norm_backward_bounds(f, fb, gq, ref_gx, l64[1].grad, l64[2].grad, l64[3].grad, dtype, C)
    res = {"gx": worst(leaves[0].grad.flatten(2).transpose(1, 2), ref_gx, bb["gx"]), "gw": worst(leaves[1].grad, l64[1].grad, bb["gw"]),
           "gb": worst(leaves[2].grad, l64[2].grad, bb["gb"]), "gpos": worst(leaves[3].grad, l64[3].grad, bb["gpos"])}
    report = {}
    collect(report, res, f"QueryPrepFunction {name(dtype)} {shape}")
    tok = torch.randn(B, H * W, C, device=DEV, generator=g).to(dtype).requires_grad_(True)
    res_in = x.view(B, C, H, W).clone().requires_grad_(True)
    gy = torch.randn(B, C, H, W, device=DEV, generator=g).to(dtype)
    TokensAddFunction.apply(tok, res_in).backward(gy)
    assert torch.equal(tok.grad, gy.flatten(2).transpose(1, 2)) and torch.equal(res_in.grad, gy)
    print(line(f"QUERY-BOUNDS {name(dtype)} {shape} gradients", report))


# --------------------------------------------------------------------------------------------- the decode Linear
LINEAR_SHAPES = [(4, 640, 4096), (1, 4096, 1024), (8, 640, 4096), (3, 37, 72), (5, 1, 8), (2, 1000, 2048),
                 (4, 37, 8192), (1, 1001, 5120), (3, 5, 4104), (8, 3, 4096), (2, 1, 8)]


def check_linear(dtype, shape, seed, report, pad=0):
    """One problem with and without bias and residual, rows ``pad`` elements wider than they need be."""
    L = lib()
    M, N, K = shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    ldx, ldy, ldr = K + pad, N + (pad and 3), N + (pad and 5)
    xs = torch.randn(M, ldx, device=DEV, generator=g).to(dtype)
    w = (torch.randn(N, K, device=DEV, generator=g) / K ** 0.5).to(dtype)
    bias = torch.randn(N, device=DEV, generator=g).to(dtype)
    rs = torch.randn(M, ldr, device=DEV, generator=g).to(dtype)
    x, r = xs[:, :K], rs[:, :N]
    for b, res in ((bias, None), (None, None), (bias, r)):
        ys = torch.empty(M, ldy, device=DEV, dtype=dtype)
        ys2 = torch.empty(M, ldy, device=DEV, dtype=dtype)
        for out in (ys, ys2):
            rc = L.mmfs_linear_small_add(CODE[dtype], xs.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(),
                                         None if res is None else rs.data_ptr(), out.data_ptr(), M, N, K, ldx, ldy, ldr, stream())
            assert rc == 0, rc
        assert torch.equal(ys[:, :N], ys2[:, :N]), f"linear {shape}: a repeat call returns other bits"
        y64, s = R.linear64(x, w, b)
        bound = R.linear_bounds(y64, s, K, dtype, res)
        want = y64 if res is None else y64 + res.double()
        key = "y" if res is None else "y_residual"
        collect(report, {key: worst(ys[:, :N], want, bound)},
                f"linear {name(dtype)} {shape} bias={b is not None} residual={res is not None} pad={pad}")


@pytest.mark.parametrize("knobs", [{}, {"MMFS_LIN_ROWS": "2"}, {"MMFS_LIN_UNROLL": "4"}, {"MMFS_LIN_EARLY": "0"},
                                   {"MMFS_LIN_ROWS": "2", "MMFS_LIN_UNROLL": "4", "MMFS_LIN_EARLY": "0"}],
                         ids=lambda k: "-".join(f"{n[9:]}{v}" for n, v in k.items()) or "default")
@pytest.mark.parametrize("dtype", HALVES)
def test_linear_small_element_by_element(dtype, knobs, monkeypatch):
    """mmfs_linear_small_add, every element: u |ref| + c 2^-24 (sum |x w| + |b|) + t with c from the kernel's chain
    (front_end_refs.linear_chain) -- an entry below 1 no longer has the absolute bar of the largest one.  Closes:
    K > 4096 (the second trip of the weight loop: K = 8192, 5120, 4104); the compiled variants behind MMFS_LIN_ROWS = 2,
    MMFS_LIN_UNROLL = 4 and MMFS_LIN_EARLY = 0, which nothing ran (odd N under two rows per wave exercises the row clamp);
    strided ldx / ldy / ldr; the residual form against the two-rounding statement; a repeat call bit-equal."""
    helpers.poison_allocations(monkeypatch)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    report = {}
    for i, shape in enumerate(LINEAR_SHAPES):
        check_linear(dtype, shape, 60 + i, report)
    check_linear(dtype, (3, 37, 72), 80, report, pad=8)
    print(line(f"LINEAR-BOUNDS {name(dtype)} {knobs or 'default'}", report))
