"""The Q-Former's attention with per-head q/k LayerNorm on the device (csrc/mmfs_attn.hip; C ABI ``mmfs_qk_attn_*`` in
include/mmfs_msda.h): q [B, Nq, H 64], k, v [B, Nk, H 64] as the Linear layers return them -> context [B, Nq, H 64], one
launch forward, one (+ a 256-lane sum of the LayerNorm parameter gradients) backward.  Nothing here reads a value back
from the device: every call can be captured into a graph.

``qk_attn_supported`` tells ``mmfs_amd.resampler`` whether the kernels apply; otherwise it states the same mathematics
with framework ops.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import MultiScaleDeformableAttention as MSDA

_lib = MSDA._lib
_CODE = MSDA._DTYPE_CODE
HEAD_DIM = 64

# kernel launches since import, for tests and tools that ask which route the module took
launches = {"forward": 0, "backward": 0}


def qk_attn_supported(q, k, v, num_heads, key_bias=None):
    """The kernels apply: device tensors q [B, Nq, H 64], k, v [B, Nk, H 64] of one type, bf16 or fp16, 1 <= Nq <= 128,
    1 <= Nk <= 8192, an optional per-key bias [B, Nk], outside autocast."""
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 3 for t in (q, k, v)):
        return False
    if torch.is_autocast_enabled() or not (q.dtype == k.dtype == v.dtype) or q.dtype not in _CODE:
        return False
    B, Nq, C = q.shape
    if num_heads < 1 or C % num_heads or k.shape != v.shape or k.shape[0] != B or k.shape[2] != C:
        return False
    if key_bias is not None and (tuple(key_bias.shape) != (B, k.shape[1]) or key_bias.device != q.device):
        return False
    return bool(_lib.mmfs_qk_attn_supported(_CODE[q.dtype], C // num_heads, Nq, k.shape[1]))


def _small(ts, dev, dt):
    """the LayerNorm parameters / the key bias as the kernels read them: of fp32 or of the inputs' type, where they lie
    (no launch); anything else is cast to fp32.  -> (tensors, dtype code)"""
    if all(t is None for t in ts):
        return list(ts), 0
    kind = ts[0].dtype
    if kind not in (torch.float32, dt) or any(t.dtype != kind or t.device != dev for t in ts):
        kind = torch.float32
    out = []
    for t in ts:
        t = t.detach()
        if t.dtype != kind or t.device != dev:
            t = t.to(device=dev, dtype=kind)
        if not t.is_contiguous() or t.data_ptr() % t.element_size():
            t = t.clone(memory_format=torch.contiguous_format)
        out.append(t)
    return out, _CODE[kind]


def _bias(key_bias, dev, dt, B, Nk):
    """-> (tensor or None, dtype code, batch stride): [B, Nk] rows Nk apart, or one row shared by the batch (stride 0)"""
    if key_bias is None:
        return None, 0, 0
    shared = key_bias.stride(0) == 0 or key_bias.shape[0] == 1
    (t,), code = _small([key_bias[0] if shared and B else key_bias], dev, dt)
    return t, code, 0 if shared else Nk



class QKNormAttentionFunction(Function):
    """(q, k, v, q_norm_weight, q_norm_bias, k_norm_weight, k_norm_bias, eps, key_bias, num_heads) -> (context, lse):
    context [B, Nq, H 64] of the inputs' type, lse [B, H, Nq] fp32 (not differentiable).  The four LayerNorm tensors
    ([64]) are all given or all None; ``key_bias`` [B, Nk] (added to the scaled scores; not differentiated) or None.
    Parameters and bias of fp32 or of the inputs' type are read where they lie: a call launches its kernels and nothing else.
    Gradients of q, k, v have their type, every element written once; the parameters' are fp32 sums cast to the
    parameters' type.  Bit-reproducible."""

    @staticmethod
    def forward(ctx, q, k, v, qw, qb, kw, kb, eps, key_bias, num_heads):
        dev, dt = q.device, q.dtype
        B, Nq, C = q.shape
        Nk, H = k.shape[1], num_heads
        q, k, v = (MSDA._aligned(t.contiguous()) for t in (q, k, v))
        norm, ncode = _small([qw, qb, kw, kb], dev, dt)
        bias, bcode, bstride = _bias(key_bias, dev, dt, B, Nk)
        out = torch.empty((B, Nq, C), dtype=dt, device=dev)
        # one allocation: lse | (m, l)
        buf = torch.empty(3 * B * H * Nq, dtype=torch.float32, device=dev)
        lse, stats = buf.split((B * H * Nq, 2 * B * H * Nq))
        MSDA._call("qk_attn_fwd", "mmfs_qk_attn_forward", dev, _CODE[dt], q.data_ptr(), k.data_ptr(), v.data_ptr(),
                   *(MSDA._ptr(t) for t in norm), ncode, float(eps), MSDA._ptr(bias), bcode, bstride, out.data_ptr(),
                   lse.data_ptr(), stats.data_ptr(), B, H, C // H, Nq, Nk)
        launches["forward"] += 1
        ctx.save_for_backward(q, k, v, out, stats, bias, *(t for t in norm if t is not None))
        ctx.conf = (B, H, Nq, Nk, C, float(eps), norm[0] is not None, key_bias is not None, ncode, bcode, bstride,
                    tuple(None if t is None else t.dtype for t in (qw, qb, kw, kb)))
        lse = lse.view(B, H, Nq)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_lse):
        B, H, Nq, Nk, C, eps, has_norm, has_bias, ncode, bcode, bstride, ptypes = ctx.conf
        q, k, v, out, stats, *rest = ctx.saved_tensors
        bias = rest[0] if has_bias else None
        norm = rest[1:] if has_norm else [None] * 4
        dev, dt = q.device, q.dtype
        g = MSDA._aligned(g.to(dt).contiguous())
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        partials = torch.empty((B * H, 4, HEAD_DIM), dtype=torch.float32, device=dev) if has_norm else None
        dparams = torch.empty((4, HEAD_DIM), dtype=torch.float32, device=dev) if has_norm else None
        MSDA._call("qk_attn_bwd", "mmfs_qk_attn_backward", dev, _CODE[dt], q.data_ptr(), k.data_ptr(), v.data_ptr(),
                   *(MSDA._ptr(t) for t in norm), ncode, eps, MSDA._ptr(bias), bcode, bstride, out.data_ptr(), g.data_ptr(),
                   stats.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), MSDA._ptr(partials), MSDA._ptr(dparams), B,
                   H, C // H, Nq, Nk)
        launches["backward"] += 2 if has_norm else 1
        gp = [None] * 4
        if has_norm:
            gp = [dparams[i].to(ptypes[i]) if ctx.needs_input_grad[3 + i] else None for i in range(4)]
        return (dq, dk, dv, *gp, None, None, None)
