"""The LLM's self-attention at decode in fp64 on STORED inputs, with the error bounds of csrc/mmfs_llama_attn.hip's header
evaluated element by element (tests/test_llama_attn_gpu.py holds the kernels AND the framework route to them;
tests/test_llama_attn.py pins this statement to the reference's goldens).

    rope64(x [B, L, H 128], position_ids [B, L], cos, sin, heads, dtype, E_x=None)  -> (rotated, bound)
    attend64(q_rot [B, Lq, H 128], keys, values [B, H, kv, 128], heads, mask=[B or 1, 1, Lq or 1, kv] or None, dtype=T,
             E_q=None, E_k=None, E_v=None)                                          -> dict: context, E_context, p
    linear64(x, weight, dtype, E_x=None)                                            -> (x W^T, bound)

``E_*`` arguments: the inputs are themselves only known to that bound (the module against the reference's fp64 tensors:
the Linear layers' rounding, the rope's); without them the bounds are those of the header on the stored inputs."""
import torch

D = 128
# unit roundoff: half the spacing of T's numbers at 1 (8 significand bits in bf16, 11 in fp16)
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24, torch.float64: 0.0}
TINY = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14, torch.float32: 2.0 ** -126, torch.float64: 0.0}
E32 = 2.0 ** -24
C_NORM = 160
SCALE = D ** -0.5


def heads_of(x, H):
    B, N, _ = x.shape
    return x.double().reshape(B, N, H, D).transpose(1, 2)          # [B, H, N, 128]


def merge(x):
    B, H, N, _ = x.shape
    return x.transpose(1, 2).reshape(B, N, H * D)


def swap_halves(x):
    return torch.cat((x[..., D // 2:], x[..., :D // 2]), dim=-1)


def rope64(x, position_ids, cos, sin, heads, dtype, E_x=None):
    """x cos + rotate_half(x) sin per head with the fp32 table's entries, in fp64 -> (r, E_rope), both [B, L, H 128].
    A position outside the table gives NaN in r (and in the bound)."""
    u, t = UNIT[dtype], TINY[dtype]
    B, L, C = x.shape
    pos = position_ids.long().cpu()
    ok = (pos >= 0) & (pos < cos.shape[0])
    at = pos.clamp(0, cos.shape[0] - 1)
    c = torch.cat((cos, cos), dim=-1).double().cpu()[at][:, :, None, :]          # [B, L, 1, 128]
    s = torch.cat((sin, sin), dim=-1).double().cpu()[at][:, :, None, :]
    xh = x.double().cpu().reshape(B, L, heads, D)
    yh = swap_halves(xh)
    sign = torch.cat((-torch.ones(D // 2), torch.ones(D // 2))).double()
    r = xh * c + sign * yh * s
    A = (xh * c).abs() + (yh * s).abs()
    E = (2 * u + 3 * u * u + 4 * E32) * A + u * r.abs() + t
    if E_x is not None:
        ex = E_x.double().cpu().reshape(B, L, heads, D)
        E = E + (ex * c.abs() + swap_halves(ex) * s.abs()) * (1 + 3 * u)
    nan = torch.full_like(r, float("nan"))
    keep = ok[:, :, None, None].expand_as(r)
    return torch.where(keep, r, nan).reshape(B, L, C), torch.where(keep, E, nan).reshape(B, L, C)


def attend64(q_rot, keys, values, heads, mask=None, dtype=None, E_q=None, E_k=None, E_v=None):
    """softmax(q K^T / sqrt(128) + mask) V in fp64 with the header's bounds; q_rot [B, Lq, H 128], keys / values
    [B, H, kv, 128] (the logical rows: what the reference's tuple holds)"""
    dtype = dtype or q_rot.dtype
    u, t = UNIT[dtype], TINY[dtype]
    qh = heads_of(q_rot.cpu(), heads)
    kh, vh = keys.double().cpu(), values.double().cpu()
    n = kh.shape[2]
    c = 256 + n
    s0 = qh @ kh.transpose(-1, -2) * SCALE
    A = qh.abs() @ kh.abs().transpose(-1, -2) * SCALE
    E_s = (u + 2 * u * u) * A + 2 * u * s0.abs() + C_NORM * E32 * (A + s0.abs())        # (no bias: s = s0)
    if E_q is not None:
        E_s = E_s + (heads_of(E_q.cpu(), heads) @ kh.abs().transpose(-1, -2)) * SCALE * (1 + 3 * u)
    if E_k is not None:
        E_s = E_s + (qh.abs() @ E_k.double().cpu().transpose(-1, -2)) * SCALE * (1 + 3 * u)
    s = s0
    if mask is not None:
        mb = mask.double().cpu().expand(s0.shape[0], 1, s0.shape[2], n).expand_as(s0)
        # a bias at or below finfo(T).min marks a masked key: its score is the bias (the sum and the clamp in T leave it)
        masked = mb <= torch.finfo(dtype).min
        s = torch.where(masked, mb, s0 + mb)
        live = torch.where(masked, torch.zeros_like(mb), mb).abs()
        E_s = torch.where(masked, torch.zeros_like(E_s), E_s + (u + C_NORM * E32) * live)     # u |s| <= u |s0| + u |bias|
    p = torch.softmax(s, -1)
    E_s = torch.where(p > 0, E_s, torch.zeros_like(E_s))              # (a key without weight moves nothing)
    row = (p * E_s).sum(-1, keepdim=True)
    E_p = p * (E_s + row + u + c * E32)
    ctx = p @ vh
    E_ctx = E_p @ vh.abs() + c * E32 * (p @ vh.abs()) + 2 * u * ctx.abs() + t
    if E_v is not None:
        E_ctx = E_ctx + ((p + E_p) @ E_v.double().cpu()) * (1 + 3 * u)
    return {"context": merge(ctx), "E_context": merge(E_ctx), "p": p}


def linear64(x, weight, dtype, E_x=None):
    """x W^T in fp64 and what a Linear layer in T (fp32 accumulation, one rounding) is known to"""
    u, t = UNIT[dtype], TINY[dtype]
    x, w = x.double().cpu(), weight.double().cpu()
    y = x @ w.T
    size = x.abs() @ w.abs().T
    E = u * y.abs() + (w.shape[1] + 8) * E32 * size + t
    if E_x is not None:
        E = E + (E_x.double().cpu() @ w.abs().T) * (1 + u)
    return y, E
