"""fp64 statements of the kernels around the op -- the MMFS sampling plan (csrc/mmfs_plan.hip), the RMS norm
(csrc/mmfs_norm.hip), the token-layout LayerNorm (csrc/mmfs_query.hip) and the decode Linear (csrc/mmfs_linear.hip) --
each a direct statement of the formula in the kernel's header comment on the storage-rounded inputs, and next to each
the per-element bound a result is held to:

    |got - ref| <= u |ref| + c 2^-24 (sum of |terms|) + t          u, t: helpers.STORAGE_U / STORAGE_T

Plain torch: every function runs on the CPU and on the device (tests/test_front_end.py holds fp32 restatements of the
kernels and planted faults against these bounds without a GPU; tests/test_front_end_gpu.py the kernels themselves).
Every constant is derived in the docstring of its function from the kernel's arithmetic; none is fitted."""
import math

import torch

from helpers import STORAGE_T, STORAGE_U

E24 = 2.0 ** -24            # one fp32 rounding, relative
SIGNIFICAND = {torch.float16: 11, torch.bfloat16: 8}
MIN_EXPONENT = {torch.float16: -14, torch.bfloat16: -126}


# --------------------------------------------------------------------------------------------- the sampling plan
K_SOFTMAX = 2.0 ** -17
"""Relative error of one weight of the plan's softmax (plan_forward_kernel; the arithmetic of msda_deform_plan.hip, whose
2^-17 this restates), with |att_q + att_tab| <= 8 and hence, the sink logit -log(n L) >= -4.16 being one of the entries,
x = logit - max in [-16, 0]:
    the fp32 sum of the two logits        <= 2^-22 absolute (half a unit in the last place below 8)
    logit - max                           <= 2^-21 absolute (below 16)
    __expf(x) = exp2(x * log2 e):  the constant's rounding 2^-25 * 16 * 1.45 < 2^-21 absolute in x; the product
                                   (below 32) 2^-20 absolute in the exponent = 0.69 * 2^-20 in x; the hardware
                                   exponential one unit in the last place, 2^-23 relative
  -> one exponential: 2^-22 + 2^-21 + 2^-21 + 0.69 * 2^-20 + 2^-23 = 2.07 * 2^-20 relative;
    the normalising sum, all terms positive: the same relative error, + P in-lane additions + the sink's + 6 butterfly
    steps = at most 23 fp32 roundings, 1.44 * 2^-20;  1 / z and the product: 2^-23 + 2^-24.
  Total 2.07 + 2.07 + 1.44 + 0.19 = 5.77 * 2^-20 = 2^-17.47 < 2^-17.  The sink's share adds the 6 steps of its own sum
  (6 * 2^-24 = 0.375 * 2^-20: 2^-17.36, still below).  The sink logit is -logf((float)(n L)): at most 2^-22 absolute, the
  size of the logits' own term.  An invisible image's logits are below -9990: exp underflows to exactly 0 in fp32 and in
  fp64, so those weights must be exactly 0."""
K_LOC = 2.0 ** -22
"""loc = fmaf(off_q + off_tab, ratio / extent, ref): the sum 2^-24, the quotient at most 2.5 units (the accuracy
ROCm's HIP math tables give for fp32 division when it is not the correctly rounded one), the fused product-sum one
rounding of the result: (1 + 2.5) 2^-24 |scaled offset| + 2^-24 (|ref| + |scaled offset|) < 2^-22 (|ref| + |scaled offset|)."""
C_DLOGIT = 32
"""dlogit = a (g - dot), dot = sum a g + g_sink sink: products of two 16-bit numbers are exact in fp32 (8 + 8 and 11 + 11
significand bits <= 24; fp32 storage: one rounding each), summed over P <= 16 in-lane additions, 6 butterfly steps, the
sink's product and addition: <= 24 + 2 roundings on dot against sum a |g| + |g_sink| sink =: D; the subtraction and the
product with a: 2 more, against a (|g| + D).  26 + the products' own (fp32 storage) <= 32."""
C_DOFF = 4
"""doff = g_loc * (ratio / extent): the quotient <= 2.5 units, the product 1: <= 4."""
QUERY_RUN = 8               # kQueryRun
PLAN_THREADS = 256


def group_width(nL):
    """G of for_group(): the power of two >= n L, at least 4"""
    g = 4
    while g < nL:
        g *= 2
    return g


def _plan_views(relpos, shapes, ratios, N, Lq, L):
    n = relpos.shape[-1]
    r = relpos.expand(N, Lq, n)
    sh = shapes.double().reshape(n, L, 2)
    scale = ratios.double().reshape(1, L, 1) / sh.flip(-1)             # [n, L, (x: / W, y: / H)]
    return n, r, scale


def plan_forward64(off_q, att_q, off_tab, att_tab, relpos, ref, shapes, ratios, H, L, P):
    """off_q [N, Lq, H*P*2], att_q [N, Lq, H*L*P], off_tab [M, H*P*2], att_tab [M, H*L*P], relpos [N, Lr, n] int64,
    ref [Nr, Lq, 2], shapes [n*L, 2] (H_l, W_l), ratios [L] -> dict of fp64 tensors: attn [N, Lq, H, n*L, P],
    sink [N, Lq, H], loc [N, Lq, H, n*L, P, 2], and the pieces of loc's bound (point, scaled).
    logits att_q + att_tab[r_k], minus 10000 where r_k == 0; one sink logit -log(n L) per (image, level) row; softmax
    over all n L (P + 1) entries; loc = ref + (off_q + off_tab[r_k]) * ratio_l / (W, H)."""
    N, Lq = off_q.shape[:2]
    n, r, scale = _plan_views(relpos, shapes, ratios, N, Lq, L)
    nL = n * L
    oq, aq = off_q.double().reshape(N, Lq, H, P, 2), att_q.double().reshape(N, Lq, H, L, P)
    ot, at = off_tab.double().reshape(-1, H, P, 2), att_tab.double().reshape(-1, H, L, P)
    logit = aq[:, :, :, None] + at[r].permute(0, 1, 3, 2, 4, 5)                       # [N, Lq, H, n, L, P]
    logit = logit - 10000.0 * (r == 0)[:, :, None, :, None, None]
    sl = -math.log(nL)
    m = logit.amax((3, 4, 5), keepdim=True).clamp_min(sl)
    e = torch.exp(logit - m)
    es = nL * torch.exp(sl - m)
    z = e.sum((3, 4, 5), keepdim=True) + es
    scaled = (oq[:, :, :, None, None] + ot[r].permute(0, 1, 3, 2, 4, 5)[:, :, :, :, None]) * scale[None, None, None, :, :, None, :]
    point = ref.double().expand(N, Lq, 2)[:, :, None, None, None, None, :]
    return dict(attn=(e / z).reshape(N, Lq, H, nL, P), sink=(es / z).reshape(N, Lq, H),
                loc=(point + scaled).reshape(N, Lq, H, nL, P, 2),
                point=point.expand_as(scaled).reshape(N, Lq, H, nL, P, 2), scaled=scaled.reshape(N, Lq, H, nL, P, 2))


def plan_forward_bounds(f, dtype):
    """{attn, sink, loc}: per-element bounds of plan_forward64's result ``f`` for storage type ``dtype`` (sink is fp32
    whatever the storage type).  A weight whose reference is exactly 0 (an invisible image) has bound 0."""
    u, t = STORAGE_U[dtype], STORAGE_T[dtype]
    return dict(attn=(u + K_SOFTMAX) * f["attn"] + t * (f["attn"] > 0),
                sink=(E24 + K_SOFTMAX) * f["sink"],
                loc=u * f["loc"].abs() + K_LOC * (f["point"].abs() + f["scaled"].abs()) + t)


def plan_backward64(g_loc, g_attn, g_sink, attn, sink, relpos, shapes, ratios, H, L, P, M):
    """The plan's backward on the SAVED attn (storage type) and sink (fp32): dot = sum a g + g_sink sink,
    dlogit = a (g - dot); d_att_q [N, Lq, H, L, P] its sum over the images; d_off_q [N, Lq, H, P, 2] the sum of
    g_loc * scale over images and levels; d_att_tab [M, H, L, P] / d_off_tab [M, H, P, 2] the same terms summed over every
    (sample, query, image) whose relative position is that row (offsets also over the levels).  -> (refs, sums): two dicts
    with those four keys, ``sums`` the matching sums of |terms| (for dlogit: a (|g| + D))."""
    N, Lq = attn.shape[:2]
    n, r, scale = _plan_views(relpos, shapes, ratios, N, Lq, L)
    a = attn.double().reshape(N, Lq, H, n, L, P)
    g = g_attn.double().reshape(N, Lq, H, n, L, P)
    dot, dabs = (a * g).sum((3, 4, 5)), (a * g.abs()).sum((3, 4, 5))
    if g_sink is not None:
        dot = dot + g_sink.double() * sink.double()
        dabs = dabs + g_sink.double().abs() * sink.double()
    dl = a * (g - dot[..., None, None, None])
    dl_abs = a * (g.abs() + dabs[..., None, None, None])
    doff = g_loc.double().reshape(N, Lq, H, n, L, P, 2) * scale[None, None, None, :, :, None, :]
    rows = r.reshape(-1)

    def table(src, tail):                                              # src [N, Lq, H, n, ...] -> [M, H, ...]
        src = src.movedim(3, 2).reshape(N * Lq * n, H, *tail)
        return torch.zeros(M, H, *tail, dtype=torch.float64, device=src.device).index_add_(0, rows, src)

    refs = dict(d_att_q=dl.sum(3), d_off_q=doff.sum((3, 4)), d_att_tab=table(dl, (L, P)), d_off_tab=table(doff.sum(4), (P, 2)))
    sums = dict(d_att_q=dl_abs.sum(3), d_off_q=doff.abs().sum((3, 4)), d_att_tab=table(dl_abs, (L, P)),
                d_off_tab=table(doff.abs().sum(4), (P, 2)))
    return refs, sums


def plan_table_chain(relpos, N, Lq, L, M):
    """-> (c_att [M], c_off [M]): the longest chain of fp32 additions into one element of a table row, from the structure
    of plan_backward_kernel: a lane adds up a run of QUERY_RUN queries (8), the first group of an equal-key segment the
    sums of the workgroup's other groups (256 / G - 1), and every stretch of equal relative positions inside a run ends in
    ONE atomic per element -- as many atomics into row r as there are such stretches with value r over all (sample,
    image, run), counted here exactly; the offsets' rows take the atomics of all L lanes of an image."""
    n = relpos.shape[-1]
    rp = relpos.expand(N, Lq, n)
    first = torch.ones_like(rp, dtype=torch.bool)
    first[:, 1:] = rp[:, 1:] != rp[:, :-1]
    first[:, ::QUERY_RUN] = True
    stretches = torch.bincount(rp[first].reshape(-1), minlength=M).double()
    merge = PLAN_THREADS // group_width(n * L) - 1
    return QUERY_RUN + merge + stretches, QUERY_RUN + merge + L * stretches


def plan_backward_bounds(refs, sums, relpos, N, Lq, L, n, M, dtype, q_dtype):
    """Bounds of the four gradients.  ``q_dtype``: the type the query-side gradients are stored in (fp32, or the storage
    type under q_grads_in_storage_type); the tables are fp32 and read as they are.
        d_att_q: the n images are added one after the other (n - 1 additions): c = C_DLOGIT + n - 1
        d_off_q: the n L rows likewise: c = C_DOFF + n L - 1
        tables:  c = the term's own constant + plan_table_chain
    Rows no sample refers to have sums of 0: their bound is 0, they must stay exactly 0."""
    uq, tq = STORAGE_U[q_dtype], STORAGE_T[q_dtype]
    c_att, c_off = plan_table_chain(relpos, N, Lq, L, M)
    return dict(
        d_att_q=uq * refs["d_att_q"].abs() + (C_DLOGIT + n - 1) * E24 * sums["d_att_q"] + tq,
        d_off_q=uq * refs["d_off_q"].abs() + (C_DOFF + n * L - 1) * E24 * sums["d_off_q"] + tq,
        d_att_tab=E24 * refs["d_att_tab"].abs() + (C_DLOGIT + c_att).view(-1, 1, 1, 1) * E24 * sums["d_att_tab"],
        d_off_tab=E24 * refs["d_off_tab"].abs() + (C_DOFF + c_off).view(-1, 1, 1, 1) * E24 * sums["d_off_tab"])


# --------------------------------------------------------------------------------------------- the RMS norm
NORM_THREADS = 256


def elements_per_lane(dtype, C):
    """Elements of a row one lane of the norm / LayerNorm kernels sums before the butterfly: its 16-byte vectors."""
    n = 16 // torch.empty(0, dtype=dtype).element_size()
    return -(-(C // n) // 64) * n


def rms_delta(dtype, C):
    """Relative error of the forward kernel's fp32 xn = x * rstd.  The sum of squares: one fused multiply-add per element
    of the lane (elements_per_lane) + 6 butterfly steps, all terms positive, then the division by C and the addition of
    eps: (per_lane + 8) 2^-24 relative on the argument, HALF of it on its inverse square root; rsqrtf: one unit in the
    last place of the hardware instruction, 2^-23; the product with x: 2^-24."""
    return ((elements_per_lane(dtype, C) + 8) / 2 + 3) * E24


def near_tie(v, dtype, delta):
    """bool: |v| lies within delta |v| of a rounding tie of ``dtype`` (an odd multiple of half the spacing there), so an
    evaluation of v that is off by delta relative may round to the other neighbour.  Exact: frexp and powers of two."""
    a = v.abs()
    _, ex = torch.frexp(a)
    e = (ex - 1).clamp_min(MIN_EXPONENT[dtype]) - (SIGNIFICAND[dtype] - 1)
    ulp = torch.ldexp(torch.ones_like(a), e)
    k = a / ulp                                                        # (exact: a power of two)
    return ((k - torch.floor(k) - 0.5).abs() * ulp <= delta * a) & (a > 0)


def rmsnorm64(x, w, eps, dtype):
    """x [rows, C], w [C] -> dict(y, rstd [rows], xn, xn_r): rstd = (mean x^2 + eps)^-1/2, xn = x rstd,
    y = w * round_T(xn) for 16-bit T (the reference's ``.to(dtype)`` between the two products), w * xn for fp32."""
    x64 = x.double()
    rstd = (x64.pow(2).mean(-1) + eps).rsqrt()
    xn = x64 * rstd[:, None]
    xn_r = xn.to(dtype).double() if dtype in SIGNIFICAND else xn
    return dict(y=w.double() * xn_r, rstd=rstd, xn=xn, xn_r=xn_r)


def rmsnorm_forward_bounds(f, w, dtype, C):
    """y, 16-bit: the product of two 16-bit numbers is exact in fp32, so where the kernel's xn rounds as the reference's
    the two results are ONE rounding apart: u |ref| + t; the roundings of xn part only within rms_delta of a tie, found
    exactly (near_tie), and there the difference is one spacing of xn, <= 2 u |xn|, times |w|.  fp32: xn's error and the
    product's.  rstd (fp32): its own error (rms_delta less the product) + the store's."""
    u, t, d = STORAGE_U[dtype], STORAGE_T[dtype], rms_delta(dtype, C)
    if dtype in SIGNIFICAND:
        y = u * f["y"].abs() + t + near_tie(f["xn"], dtype, d) * 2 * u * (1 + u) * (w.double() * f["xn"]).abs()
    else:
        y = (u + d + E24) * f["y"].abs() + t
    return dict(y=y, rstd=d * f["rstd"])               # (rms_delta less xn's product, plus the store: d again)


DELTA_BWD = 2.0 ** -23
"""The backward kernel's xn is ONE fp32 product of the stored x and the rstd it is given (2^-24; the reference uses the
same rstd), taken as 2^-23 to cover the fp64 evaluation's own conversion through fp32 on the way to 16 bits."""


def rmsnorm_backward64(dy, x, w, rstd, dtype):
    """On the rstd the forward SAVED: xn = x rstd, g = dy w, dx = rstd (g - xn mean(g xn)); the gain gradient
    dw = sum_rows dy * round_T(xn).  -> dict(dx, dw, dx_sum (the |terms| of dx's bound), dw_sum, dw_ties)."""
    x64, dy64, r = x.double(), dy.double(), rstd.double()[:, None]
    xn = x64 * r
    g = dy64 * w.double()
    dot = (g * xn).mean(-1, keepdim=True)
    dot_abs = (g * xn).abs().mean(-1, keepdim=True)
    xn_r = xn.to(dtype).double() if dtype in SIGNIFICAND else xn
    ties = torch.zeros_like(xn[0])
    if dtype in SIGNIFICAND:
        ties = (near_tie(xn, dtype, DELTA_BWD) * 2 * STORAGE_U[dtype] * (dy64 * xn).abs()).sum(0)
    return dict(dx=r * (g - xn * dot), dw=(dy64 * xn_r).sum(0), dw_sum=(dy64 * xn_r).abs().sum(0), dw_ties=ties,
                dx_terms=r * (g.abs() + xn.abs() * dot.abs()), dx_dot=r * xn.abs() * dot_abs)


def norm_grid(rows, cap):
    return max(1, min(-(-rows // (NORM_THREADS // 64)), 2048, cap))


def rmsnorm_backward_bounds(b, dtype, rows, C, grid, atomic):
    """dx = rstd * (g w - x rstd dot): g w exact for 16-bit storage (one rounding for fp32), x rstd, its product with dot,
    the subtraction, the product with rstd: <= 4 roundings (5) against rstd (|g| + |xn dot|); dot itself: one fused
    multiply-add per element of the lane + 6 butterfly steps + the product g w, the product x rstd and the division:
    (per_lane + 9) 2^-24 against mean |g xn|, carried to dx by rstd |xn|.
    dw: a wave adds one fused multiply-add per row it owns (ceil(rows / (4 grid)) of them), wave 0 its three LDS
    partners; ``atomic``: one atomic per workgroup into the column (grid more), else the workgroups' rows are summed by
    the caller in fp64.  + 2: xn's own product (fp32 storage) and the store.  Elements whose 16-bit rounding of xn may
    part from the reference's add 2 u |dy xn| each (dw_ties)."""
    u, t = STORAGE_U[dtype], STORAGE_T[dtype]
    per_lane = elements_per_lane(dtype, C)
    chain = -(-rows // (NORM_THREADS // 64 * grid)) + 3 + (grid if atomic else 0) + 2
    return dict(dx=u * b["dx"].abs() + t + E24 * (5 * b["dx_terms"] + (per_lane + 9) * b["dx_dot"]),
                dw=chain * E24 * b["dw_sum"] + b["dw_ties"]), chain


# --------------------------------------------------------------------------------------------- the token-layout LayerNorm
def layer_norm_tokens64(x, gamma, beta, pos, eps, dtype):
    """x [B, C, HW] -> tokens [B, HW, C]: mean, rstd per token (biased variance), o = (tok - mean) rstd gamma + beta,
    q = o (+ pos [HW, C]) -- UNROUNDED: the kernel rounds o to the storage type before it adds pos, as the framework's two
    kernels do, and the bound carries that rounding (a reference that rounded its own o would part from the kernel's at
    every tie).  -> dict(q, o, mean, rstd, ...)."""
    tok = x.double().transpose(1, 2)
    mean = tok.mean(-1, keepdim=True)
    d = tok - mean
    var = d.pow(2).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    o = d * rstd * gamma.double() + beta.double()
    q = o if pos is None else o + pos.double()
    return dict(q=q, o=o, mean=mean.squeeze(-1), rstd=rstd.squeeze(-1), d=d, var=var.squeeze(-1),
                mean_abs=tok.abs().mean(-1), gamma=gamma.double(), pos=None if pos is None else pos.double())


def layer_norm_tokens_bounds(f, dtype, C, eps):
    """mean (fp32): the lane's elements one after the other + 6 butterfly steps + the product with 1 / C (itself
    rounded: 2 roundings): (per_lane + 8) 2^-24 mean|x|, + the store.
    rstd (fp32): each deviation x - mean carries the mean's error b_m (common to the row: it changes the variance by
    b_m^2 only) and one rounding (2^-23 on its square); the fused sum per_lane + 6, the product with 1 / C 2, eps 1:
    (per_lane + 11) 2^-24 + b_m^2 / (var + eps) on the argument, half of it on rstd, + 2^-23 (rsqrtf) + the store.
    q: o = fma((x - mean) rstd, gamma, beta): |gamma| rstd (b_m + 2^-24 |d|) from the deviation, (rstd's error +
    2 * 2^-24) |d rstd gamma| from the two products, 2^-24 |o| from the sum =: e_o; without pos one rounding of o:
    u |o| + e_o + t; with pos two roundings: u (|o| + |q|) + 2 t + e_o.  (Against the UNROUNDED o: no tie can matter.)"""
    u, t = STORAGE_U[dtype], STORAGE_T[dtype]
    per_lane = -(-(C // 8) // 64) * 8
    b_m = (per_lane + 8) * E24 * f["mean_abs"] + E24 * f["mean"].abs()
    rel_r = ((per_lane + 11) * E24 + b_m ** 2 / (f["var"] + eps)) / 2 + 2 * E24 + E24
    d = f["d"].abs()
    dg = (d * f["rstd"][..., None] * f["gamma"]).abs()
    e_o = (f["gamma"].abs() * f["rstd"][..., None] * (b_m[..., None] + E24 * d) + (rel_r[..., None] + 2 * E24) * dg
           + E24 * f["o"].abs()) * (1 + u)
    q = u * f["o"].abs() + e_o + t
    if f["pos"] is not None:
        q = q + u * f["q"].abs() + t
    return dict(mean=b_m, rstd=rel_r * f["rstd"], q=q)


def layer_norm_backward_bounds(f, fb, gq, ref_gx, ref_gw, ref_gb, ref_gpos, dtype, C):
    """QueryPrepFunction.backward: the framework's LayerNorm backward in the storage type (fp32 inside, results rounded) on
    the KERNEL's mean / rstd, against fp64 autograd with statistics of its own.  With gg = g gamma, xhat = (x - mean) rstd,
    s1 = mean gg, s2 = mean gg xhat:  gx = rstd (gg - s1 - xhat s2),  gw = sum_tokens g xhat,  gb = sum_tokens g,
    g_pos = sum_batch g.  The framework's summation order is not ours to know: ANY order of n fp32 additions is off by at
    most (n - 1) 2^-24 sum |terms|, which is what the sums are given (n = C, the B HW tokens, B); elementwise steps three
    roundings each; the statistics' errors are the forward's bounds (b_m on the mean, rel_r on rstd), carried through
    xhat: |d xhat| <= rstd b_m + |xhat| (rel_r + 2 * 2^-24)."""
    u, t = STORAGE_U[dtype], STORAGE_T[dtype]
    g = gq.double()
    gg = g * f["gamma"]
    rstd, b_m = f["rstd"][..., None], fb["mean"][..., None]
    rel_r = (fb["rstd"] / f["rstd"])[..., None]
    xhat = f["d"] * rstd
    dxh = rstd * b_m + xhat.abs() * (rel_r + 2 * E24)
    s1, s2 = gg.mean(-1, keepdim=True), (gg * xhat).mean(-1, keepdim=True)
    e1 = (C + 1) * E24 * gg.abs().mean(-1, keepdim=True)
    e2 = (C + 3) * E24 * (gg * xhat).abs().mean(-1, keepdim=True) + (gg.abs() * dxh).mean(-1, keepdim=True)
    terms = rstd * (gg.abs() + s1.abs() + xhat.abs() * s2.abs())
    tokens, batch = g.shape[0] * g.shape[1], g.shape[0]
    return dict(
        gx=u * ref_gx.abs() + t + rstd * (3 * E24 * gg.abs() + e1 + xhat.abs() * e2 + dxh * s2.abs()) + (rel_r + 3 * E24) * terms,
        gw=u * ref_gw.abs() + t + (tokens + 2) * E24 * (g * xhat).abs().sum((0, 1)) + (g.abs() * dxh).sum((0, 1)),
        gb=u * ref_gb.abs() + t + (tokens - 1) * E24 * g.abs().sum((0, 1)),
        gpos=u * ref_gpos.abs() + t + (batch - 1) * E24 * g.abs().sum(0))


# --------------------------------------------------------------------------------------------- the decode Linear
def linear64(x, w, b=None):
    """x [M, K], w [N, K], b [N] | None -> (y [M, N], the sum of |x w| + |b|)"""
    y = x.double() @ w.double().t()
    s = x.double().abs() @ w.double().abs().t()
    if b is not None:
        y, s = y + b.double(), s + b.double().abs()
    return y, s


def linear_chain(K):
    """c of the Linear's bound, from linear_small: a lane owns ceil(K / 512) 16-byte pieces of the weight row; a piece is
    four packed dot-product instructions, each two products and two additions into the fp32 accumulator (the products
    of two 16-bit numbers are exact in fp32: 8 + 8 significand bits for bf16, 11 + 11 for fp16, <= 24; counted as two
    roundings per instruction, which also covers a unit that does not fuse the additions) and one addition of the
    piece's sum: 9 per piece; six butterfly steps; the bias."""
    return 9 * -(-K // 512) + 6 + 1


def linear_bounds(y, s, K, dtype, residual=None):
    """One rounding of the fp32 result: u |ref| + c 2^-24 (sum |x w| + |b|) + t.  With a residual the kernel rounds the
    result, adds the stored residual in fp32 and rounds again (the framework's add that would follow): against
    ref + residual that is the first bound + u |ref + residual| + t."""
    u, t = STORAGE_U[dtype], STORAGE_T[dtype]
    bound = u * y.abs() + linear_chain(K) * E24 * s + t
    if residual is not None:
        bound = bound + u * (y + residual.double()).abs() + t
    return bound


# --------------------------------------------------------------------------------------------- comparing
def worst(got, ref, bound):
    """(worst |got - ref| / bound, its index, got, ref, bound there); inf for a non-finite element (an unwritten, poisoned
    one) and for any error at all where the bound is 0."""
    got = got.double().reshape(ref.shape)
    bound = bound.expand_as(ref)
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))
    ratio = torch.where(torch.isfinite(got), ratio, float("inf"))
    if ratio.numel() == 0:
        return (0.0, (), 0.0, 0.0, 0.0)
    k = int(ratio.argmax())
    where, rem = [], k
    for s in reversed(ratio.shape):
        where.append(rem % s)
        rem //= s
    return (float(ratio.flatten()[k]), tuple(reversed(where)), float(got.flatten()[k]), float(ref.flatten()[k]),
            float(bound.flatten()[k]))
