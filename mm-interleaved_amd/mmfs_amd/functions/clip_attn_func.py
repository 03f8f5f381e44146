"""The CLIP ViT's self-attention on the device (csrc/mmfs_clip_attn.hip; C ABI ``mmfs_clip_attn_*`` in
include/mmfs_clip_attn.h): full attention of heads of 64 channels and its backward, q, k, v [B, L, H 64] as the Linear layers
return them -> context [B, L, H 64].  What the reference's ``CLIPXAttention`` asks of
``xformers.ops.memory_efficient_attention(q, k, v)``.  Nothing of size L x L exists at any time; nothing reads a value back
from the device: forward and backward can be captured into a graph.  Bit-reproducible.

    context = mmfs_amd.clip_attention(q, k, v, heads)

``mmfs_amd.clip_attn.CLIPSelfAttention`` takes this on its kernel route.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import MultiScaleDeformableAttention as MSDA

_CODE = MSDA._DTYPE_CODE
HEAD_DIM = 64
# how the kernels cut their work, where their paths change: the query rows of a workgroup (forward, dq), the keys of a
# forward tile, the keys of a dkdv workgroup, the queries of a dkdv tile, the query rows of a wave
CLIP_TILES = MSDA._tiles("mmfs_clip_attn_tiles", 5)

# kernel launches since import, for tests and tools that ask which route the module took
launches = {"forward": 0, "backward": 0}


def clip_attn_supported(q, heads):
    """The kernels apply: a device tensor q [B, L, H 64] of bf16 or fp16, L >= 1, outside autocast."""
    return MSDA._attn_supported(q, heads, "mmfs_clip_attn_supported")


def clip_forward(q, k, v, heads, want_lse=True):
    """-> (context [B, L, H 64], lse [B, H, L] fp32 or None); the arguments as ``MSDA._plain`` leaves them"""
    B, L, C = q.shape
    out = torch.empty_like(q)
    lse = torch.empty((B, heads, L), dtype=torch.float32, device=q.device) if want_lse else None
    MSDA._call("clip_attn_fwd", "mmfs_clip_attn_forward", q.device, _CODE[q.dtype], q.data_ptr(), k.data_ptr(), v.data_ptr(),
               out.data_ptr(), MSDA._ptr(lse), B, L, heads, C // heads)
    launches["forward"] += 1
    return out, lse


def clip_backward(q, k, v, out, grad, lse, heads):
    """-> (dq, dk, dv)"""
    B, L, C = q.shape
    dev = q.device
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    ws = MSDA._float_workspace("mmfs_clip_attn_workspace_bytes", dev, B, heads, L)      # delta
    MSDA._call("clip_attn_bwd", "mmfs_clip_attn_backward", dev, _CODE[q.dtype], q.data_ptr(), k.data_ptr(), v.data_ptr(),
               out.data_ptr(), grad.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr(),
               ws.numel() * 4, B, L, heads, C // heads)
    launches["backward"] += 2
    return dq, dk, dv


class ClipAttentionFunction(Function):
    """(q, k, v, heads) -> context [B, L, H 64] of the inputs' type.  Saved for the backward: q, k, v, the context and lse
    [B, H, L] -- nothing of size L x L.  Gradients of the inputs' type, every element written once.  Where nothing requires
    grad the forward writes no lse."""

    @staticmethod
    def forward(ctx, q, k, v, heads):
        need = any(ctx.needs_input_grad[:3])
        q, k, v = MSDA._plain(q), MSDA._plain(k), MSDA._plain(v)
        out, lse = clip_forward(q, k, v, heads, want_lse=need)
        if need:
            ctx.save_for_backward(q, k, v, out, lse)
        ctx.heads = heads
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        q, k, v, out, lse = ctx.saved_tensors
        grad = MSDA._aligned(grad.to(q.dtype).contiguous())
        dq, dk, dv = clip_backward(q, k, v, out, grad, lse, ctx.heads)
        return dq, dk, dv, None


def clip_attention(q, k, v, heads):
    """q, k, v [B, L, H 64] device tensors of bf16 or fp16 as the Linear layers return them -> context [B, L, H 64]:
    softmax over all keys t of q[b, j] . k[b, t] / 8, times v.  Differentiable in q, k and v."""
    MSDA._require_qkv("clip_attention", q, k, v, heads, HEAD_DIM)
    return ClipAttentionFunction.apply(q, k, v, heads)
