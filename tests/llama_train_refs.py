"""The LLM's self-attention in training in fp64 on the STORED q, k, v and upstream gradient, with the error bounds of
csrc/mmfs_llama_train.hip's header evaluated element by element (tests/test_llama_train_gpu.py holds the kernels to them,
tests/test_llama_train.py the framework's statement in T and four defective variants of it).

    r = train64(q, k, v [B, L, H 128], position_ids [B, L], cos, sin, heads, dtype, upstream=dO or None)

-> dict: ``q_rot``, ``k_rot``, ``context``, ``lse`` [B, H, L], ``dq``, ``dk``, ``dv`` and ``E_<name>`` for each.  The forward
builds on llama_attn_refs.rope64 / attend64; the backward is written out (qk_attn_refs.attention64's ``norm=None`` branch
with the causal mask and the inverse rotation), so that every intermediate a bound needs is at hand.

Rounding points the bounds assume: q_rot, k_rot, P and dS are rounded to T; lse and delta are fp32; dq, dk, dv and the
context are rounded once.  The framework's statement rounds more often; where it does, the bound counts its roundings.

The per-element bounds add absolute values where the errors of 128 channels and up to L keys largely cancel: on dq and dk
they are wider than the gradient itself at unit-normal rows, so a second, tight check goes with them (``row_error``).
"""
import torch

from llama_attn_refs import C_NORM, D, E32, SCALE, TINY, UNIT, attend64, heads_of, merge, rope64, swap_halves


def causal_mask(L):
    """[1, 1, L, L] fp64: -Inf where key t > query j, 0 elsewhere"""
    future = torch.ones(L, L, dtype=torch.bool).triu(1)
    return torch.zeros(L, L, dtype=torch.float64).masked_fill(future, float("-inf"))[None, None]


def unrotate64(g, G, position_ids, cos, sin, heads, dtype):
    """g [B, H, L, 128]: the gradient of a rotated row, known to G -> (R^T g, its bound) as [B, L, H 128]:
    x = g cos - rotate_half(g) sin = g cos + g' sin, g' the partner channel with the sign of its half."""
    u, t = UNIT[dtype], TINY[dtype]
    pos = position_ids.long().cpu()
    ok = (pos >= 0) & (pos < cos.shape[0])
    at = pos.clamp(0, cos.shape[0] - 1)
    c = torch.cat((cos, cos), dim=-1).double().cpu()[at][:, None]               # [B, 1, L, 128]
    s = torch.cat((sin, sin), dim=-1).double().cpu()[at][:, None]
    sign = torch.cat((torch.ones(D // 2), -torch.ones(D // 2))).double()
    gp = swap_halves(g)
    x = g * c + sign * gp * s
    A = (g * c).abs() + (gp * s).abs()
    E = G * c.abs() + swap_halves(G) * s.abs() + (2 * u + 3 * u * u + 4 * E32) * A + u * x.abs() + t
    keep = ok[:, None, :, None].expand_as(x)
    nan = torch.full_like(x, float("nan"))
    return merge(torch.where(keep, x, nan)), merge(torch.where(keep, E, nan))


def train64(q, k, v, position_ids, cos, sin, heads, dtype, upstream=None):
    u, t = UNIT[dtype], TINY[dtype]
    q, k, v = q.cpu(), k.cpu(), v.cpu()
    B, L, _ = q.shape
    c = 256 + L                                                                 # the header's c_e
    q_rot, E_q = rope64(q, position_ids, cos, sin, heads, dtype)
    k_rot, E_k = rope64(k, position_ids, cos, sin, heads, dtype)
    qh, kh, vh = heads_of(q_rot, heads), heads_of(k_rot, heads), heads_of(v, heads)
    eq, ek = heads_of(E_q, heads), heads_of(E_k, heads)
    mask = causal_mask(L)
    fwd = attend64(q_rot, kh, vh, heads, mask=mask, dtype=dtype, E_q=E_q, E_k=ek)
    r = {"q_rot": q_rot, "E_q_rot": E_q, "k_rot": k_rot, "E_k_rot": E_k, "context": fwd["context"],
         "E_context": fwd["E_context"], "p": fwd["p"]}
    # E_s and E_p as attend64 forms them (it does not hand them out)
    live = (mask == 0).expand(B, heads, L, L)
    s0 = qh @ kh.transpose(-1, -2) * SCALE
    A = qh.abs() @ kh.abs().transpose(-1, -2) * SCALE
    E_s = (u + 2 * u * u) * A + 2 * u * s0.abs() + C_NORM * E32 * (A + s0.abs())
    E_s = E_s + (eq @ kh.abs().transpose(-1, -2) + qh.abs() @ ek.transpose(-1, -2)) * SCALE * (1 + 3 * u)
    s = torch.where(live, s0, torch.full_like(s0, float("-inf")))
    p = torch.softmax(s, -1)
    E_s = torch.where(live & (p > 0), E_s, torch.zeros_like(E_s))
    row = (p * E_s).sum(-1, keepdim=True)
    E_p = p * (E_s + row + u + c * E32)
    lse = torch.logsumexp(s, -1)
    r["lse"], r["E_lse"] = lse, row.squeeze(-1) + c * E32 * (1 + lse.abs())
    if upstream is None:
        return r
    ctx = p @ vh
    do = heads_of(upstream.cpu(), heads)
    W = (E_p + (2 * u + c * E32) * p) @ vh.abs() + t                            # what a product with the rounded p is known to
    dP = do @ vh.transpose(-1, -2)
    delta = (do * ctx).sum(-1, keepdim=True)
    E_delta = (do.abs() * W).sum(-1, keepdim=True)
    ds = p * (dP - delta)
    E_ds = E_p * (dP - delta).abs() + p * (u * dP.abs() + E_delta) + 3 * u * ds.abs()
    dv = p.transpose(-1, -2) @ do
    r["dv"] = merge(dv)
    r["E_dv"] = merge(E_p.transpose(-1, -2) @ do.abs() + c * E32 * (p.transpose(-1, -2) @ do.abs()) + 2 * u * dv.abs() + t)
    gq, gk = ds @ kh * SCALE, ds.transpose(-1, -2) @ qh * SCALE
    G_q = (E_ds @ kh.abs() + ds.abs() @ ek + (u + c * E32) * (ds.abs() @ kh.abs())) * SCALE + u * gq.abs()
    G_k = (E_ds.transpose(-1, -2) @ qh.abs() + ds.abs().transpose(-1, -2) @ eq +
           (u + c * E32) * (ds.abs().transpose(-1, -2) @ qh.abs())) * SCALE + u * gk.abs()
    # what the tight check (row_error) adds to a row's own size: the share of delta's error.  delta is formed from the STORED
    # context, 128 products dO_c O_c with O rounded: its error has the size D_j = |dO_j o O_j|_2 (times u / 2 rms) whatever the
    # row's gradient is, and enters dq_j as p(j, .) k sc -- the p-weighted mean key -- and dk_t as sum_j p(j, t) q_j sc.
    Dj = (do * ctx).norm(dim=-1)                                                # [B, H, L]
    r["S_dq"] = (Dj * (p @ kh).norm(dim=-1) * SCALE).transpose(1, 2)            # [B, L, H]
    r["S_dk"] = ((p.pow(2).transpose(-1, -2) @ (Dj * qh.norm(dim=-1)).pow(2)[..., None]).squeeze(-1).sqrt() * SCALE).transpose(1, 2)
    r["dq"], r["E_dq"] = unrotate64(gq, G_q, position_ids, cos, sin, heads, dtype)
    r["dk"], r["E_dk"] = unrotate64(gk, G_k, position_ids, cos, sin, heads, dtype)
    return r


def worst(got, ref, bound):
    """max |got - ref| / bound over the elements whose reference is finite; a NaN of ``got`` there is Inf.  Where the
    reference is NaN (a position outside the table), ``got`` must be NaN too."""
    got, ref, bound = got.detach().double().cpu().reshape(ref.shape), ref.double(), bound.double()
    fin = torch.isfinite(ref)
    if not bool((torch.isnan(got) == ~fin).all()):
        return float("inf")
    if not bool(fin.any()):
        return 0.0
    ratio = (got - ref).abs()[fin] / bound[fin]
    return float(ratio.max())


# ---------------------------------------------------------------------------------------------------------------------
# The tight check: the error of every row (one token of one head, 128 channels) in the 2-norm against the row's own norm.
#
#     |got_row - ref_row|_2  <=  TIGHT u (|ref_row|_2 + S_row + 2^-6 R),        R the rms of |ref_row|_2 over the tensor,
#                                                                             S_row delta's share (dq, dk; train64's S_dq, S_dk)
#
# Where the factor comes from.  To first order, with roundings that are independent and of rms about u / 2 relative each
# (round to nearest, averaged over the significand), a term ds(j, t) k(t) of dq carries: the score's error, which is the
# relative error of p -- s sums 128 products of two rounded factors (q_rot, k_rot):  sc (u / 2) sqrt(2 . 128) rms(q) rms(k), which
# is 0.7 u rms(q) rms(k) (1.1 u at unit-normal q and k of deviation 1.5); the rounding of dS (P for dv); the rounding of k_rot
# (dO is exact); and the result's own rounding.  In quadrature about 1.4 u.  The terms of a row have mixed signs, so the
# row's error and the row itself grow alike with the number of terms: the relative error of the ROW in the 2-norm is that
# of a term, about 1.4 u, whatever L is (delta and lse add less: they average 128 channels / the row's keys).  TIGHT = 8
# leaves a factor of about 5 for the tails over some 10^3 .. 10^4 rows and for rows of few terms.  A sign error is 2, a
# missing 1 / sqrt(128) is 10, half a gradient is 0.5 in this measure: 8 u is 0.031 in bf16 and 0.004 in fp16.
# S_row: delta = rowsum(dO O) is formed from the stored context, as the issue has it, and the rounding of O leaves delta off by
# about (u / 2) |dO o O|_2 -- an error that does not shrink with the row's gradient.  A row whose softmax is peaked (the first
# rows: few keys) has a gradient far below that: dP - delta nearly cancels at the key that holds the weight.  The share is
# stated by train64 from fp64 quantities alone and enters with the same factor TIGHT u as the row itself.
# The floor 2^-6 R serves the rows whose exact gradient is (next to) nothing -- dq of row 0 is exactly 0, and the kernels
# leave fp32 noise of dP - delta there: they are held at a 64th of the typical row.
# This measure holds the KERNELS' order of roundings (q_rot, k_rot, P, dS and the result, once each).  The framework's
# statement in T rounds the scores themselves to T (u |s|, |s| up to 10) and is held to the per-element bounds alone.
# ---------------------------------------------------------------------------------------------------------------------
TIGHT = 8
TIGHT_NAMES = ("context", "dq", "dk", "dv")


def row_error(got, ref, dtype, share=None):
    """worst |got_row - ref_row|_2 / (TIGHT u (|ref_row|_2 + share_row + 2^-6 R)) over the rows (a token of a head) of
    [B, L, H 128] tensors, ``share`` [B, L, H] or None; a non-finite entry of ``got`` is Inf.  <= 1 passes."""
    ref = ref.double().cpu()
    got = got.detach().double().cpu().reshape(ref.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    B, L, C = ref.shape
    err = (got - ref).reshape(B, L, C // D, D).norm(dim=-1)
    size = ref.reshape(B, L, C // D, D).norm(dim=-1)
    R = float(size.pow(2).mean().sqrt())
    if share is not None:
        size = size + share
    return float((err / (TIGHT * UNIT[dtype] * (size + 2.0 ** -6 * R))).max())


def tight_ratios(got, ref, dtype):
    """{name: row_error} of context, dq, dk, dv (``got`` and ``ref`` dicts; ref from train64)"""
    return {n: row_error(got[n], ref[n], dtype, ref.get("S_" + n)) for n in TIGHT_NAMES}


def draw(seed, L, dtype, B, H, first=5, device="cpu", qk=1.0):
    """the inputs of the GPU tests (tests/test_llama_train_gpu.py) and of the yardstick that shows what the checks catch at
    exactly them (tests/test_llama_train.py): unit-normal rows, k scaled by 1.5 and shifted by 0.25, positions that start
    at a per-row offset"""
    gen = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, L, H * D, generator=gen) * qk).to(device, dtype)
    k = ((torch.randn(B, L, H * D, generator=gen) * 1.5 + 0.25) * qk).to(device, dtype)
    v = torch.randn(B, L, H * D, generator=gen).to(device, dtype)
    up = torch.randn(B, L, H * D, generator=gen).to(device, dtype)
    pos = torch.stack([torch.arange(L) + first + 17 * b for b in range(B)]).to(device)
    return q, k, v, up, pos
