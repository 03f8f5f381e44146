"""The Q-Former attention with per-head q/k LayerNorm in fp64 on the STORED q, k, v, with the error bounds of
csrc/mmfs_attn.hip's header evaluated element by element (tests/test_qk_attn_gpu.py holds the kernels AND the framework
route to them; tests/test_qk_attn.py pins this statement to the reference's goldens).

    r = attention64(q, k, v, heads, norm=(qw, qb, kw, kb) or None, eps=.., bias=[B, Nk] or None, upstream=dO, dtype=T)

-> dict: ``context``, ``lse``, ``dq``, ``dk``, ``dv``, ``dparams`` ([4, 64]: d q_norm.weight, d q_norm.bias,
d k_norm.weight, d k_norm.bias) and ``E_<name>`` for each.  The backward is written out (not autograd), so that every
intermediate a bound needs is at hand."""
import torch

D = 64
UNIT = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12, torch.float32: 2.0 ** -24, torch.float64: 0.0}
TINY = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14, torch.float32: 2.0 ** -126, torch.float64: 0.0}
E32 = 2.0 ** -24
C_NORM = 96


def _heads(x, H):
    B, N, _ = x.shape
    return x.double().reshape(B, N, H, D).transpose(1, 2)          # [B, H, N, 64]


def _merge(x):
    B, H, N, _ = x.shape
    return x.transpose(1, 2).reshape(B, N, H * D)


def _normalise(x, w, b, eps):
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    xh = (x - mean) * rstd
    return xh * w + b, xh, rstd


def _norm_backward(dy, dy_err, xh, rstd, w, u, t, c):
    """dx = rstd (g - mean g - x^ mean(g x^)), g = dy w; with dy known to dy_err -> (dx, its bound, dw, db, their bounds)"""
    g, ge = dy * w, dy_err * w.abs()
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    size = rstd * (g.abs() + g.abs().mean(-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    err = rstd * (ge + ge.mean(-1, keepdim=True) + xh.abs() * (ge * xh.abs()).mean(-1, keepdim=True))
    e_dx = err + c * E32 * size + 2 * u * dx.abs() + t
    dw, db = (dy * xh).sum((0, 1, 2)), dy.sum((0, 1, 2))
    e_dw = (dy_err * xh.abs()).sum((0, 1, 2)) + c * E32 * (dy * xh).abs().sum((0, 1, 2)) + 2 * u * dw.abs() + t
    e_db = dy_err.sum((0, 1, 2)) + c * E32 * dy.abs().sum((0, 1, 2)) + 2 * u * db.abs() + t
    return dx, e_dx, dw, db, e_dw, e_db


def attention64(q, k, v, heads, norm=None, eps=0.0, bias=None, upstream=None, dtype=None):
    dtype = dtype or q.dtype
    u, t = UNIT[dtype], TINY[dtype]
    H = heads
    qh, kh, vh = _heads(q, H), _heads(k, H), _heads(v, H)
    Nq, Nk = qh.shape[2], kh.shape[2]
    c = 256 + Nq + Nk                                                  # the header's c_e: exp and the sums' chains
    if norm is not None:
        qw, qb, kw, kb = (p.double() for p in norm)
        qn, qx, qr = _normalise(qh, qw, qb, eps)
        kn, kx, kr = _normalise(kh, kw, kb, eps)
        un = u
    else:
        qn, kn, un = qh, kh, 0.0
    s0 = qn @ kn.transpose(-1, -2) / 8
    A = qn.abs() @ kn.abs().transpose(-1, -2) / 8
    E_s = 2 * un * A + 3 * u * s0.abs() + C_NORM * E32 * (A + s0.abs())
    s = s0
    if bias is not None:
        # a bias at or below finfo(T).min marks a masked key: its score is the bias (the sum in T absorbs the score)
        kb = bias.double()[:, None, None, :].expand_as(s0)
        masked = kb <= torch.finfo(dtype).min
        s = torch.where(masked, kb, s0 + kb)
        E_s = torch.where(masked, torch.zeros_like(E_s), E_s)
    lse = torch.logsumexp(s, -1)
    p = torch.softmax(s, -1)
    E_s = torch.where(p > 0, E_s, torch.zeros_like(E_s))              # (a masked key's score error moves nothing)
    row = (p * E_s).sum(-1, keepdim=True)
    E_p = p * (E_s + row + u + c * E32)
    ctx = p @ vh
    W = (E_p + (2 * u + c * E32) * p) @ vh.abs() + t                  # what a product with the rounded p is known to
    r = {"context": _merge(ctx), "E_context": _merge(E_p @ vh.abs() + c * E32 * (p @ vh.abs()) + 2 * u * ctx.abs() + t),
         "lse": lse, "E_lse": row.squeeze(-1) + c * E32 * (1 + lse.abs()), "p": p}
    if upstream is None:
        return r
    do = _heads(upstream, H)
    dP = do @ vh.transpose(-1, -2)
    delta = (do * ctx).sum(-1, keepdim=True)
    E_delta = (do.abs() * W).sum(-1, keepdim=True)
    ds = p * (dP - delta)
    E_ds = E_p * (dP - delta).abs() + p * (u * dP.abs() + E_delta) + 3 * u * ds.abs()
    dv = p.transpose(-1, -2) @ do
    r["dv"] = _merge(dv)
    r["E_dv"] = _merge(E_p.transpose(-1, -2) @ do.abs() + c * E32 * (p.transpose(-1, -2) @ do.abs()) + 2 * u * dv.abs() + t)
    dqn, dkn = ds @ kn / 8, ds.transpose(-1, -2) @ qn / 8
    G_q = (E_ds @ kn.abs() + (un + c * E32) * (ds.abs() @ kn.abs())) / 8 + u * dqn.abs()
    G_k = (E_ds.transpose(-1, -2) @ qn.abs() + (un + c * E32) * (ds.abs().transpose(-1, -2) @ qn.abs())) / 8 + u * dkn.abs()
    if norm is None:
        r.update(dq=_merge(dqn), E_dq=_merge(G_q + u * dqn.abs() + t), dk=_merge(dkn), E_dk=_merge(G_k + u * dkn.abs() + t))
        return r
    dq, e_dq, dqw, dqb, e_dqw, e_dqb = _norm_backward(dqn, G_q, qx, qr, qw, u, t, c)
    dk, e_dk, dkw, dkb, e_dkw, e_dkb = _norm_backward(dkn, G_k, kx, kr, kw, u, t, c)
    r.update(dq=_merge(dq), E_dq=_merge(e_dq), dk=_merge(dk), E_dk=_merge(e_dk),
             dparams=torch.stack((dqw, dqb, dkw, dkb)), E_dparams=torch.stack((e_dqw, e_dqb, e_dkw, e_dkb)))
    return r
