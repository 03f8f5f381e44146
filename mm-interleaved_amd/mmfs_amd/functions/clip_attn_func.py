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

_lib = MSDA._lib
_CODE = MSDA._DTYPE_CODE
HEAD_DIM = 64
# how the kernels cut their work, where their paths change: the query rows of a workgroup (forward, dq), the keys of a
# forward tile, the keys of a dkdv workgroup, the queries of a dkdv tile, the query rows of a wave
CLIP_TILES = tuple(int(_lib.mmfs_clip_attn_tiles(i)) for i in range(5))

# kernel launches since import, for tests and tools that ask which route the module took
launches = {"forward": 0, "backward": 0}


def clip_attn_supported(q, heads):
    """The kernels apply: a device tensor q [B, L, H 64] of bf16 or fp16, L >= 1, outside autocast."""
    if not (isinstance(q, torch.Tensor) and q.is_cuda and q.dim() == 3) or torch.is_autocast_enabled():
        return False
    if q.dtype not in (torch.float16, torch.bfloat16) or heads < 1 or q.shape[2] % heads:
        return False
    return bool(_lib.mmfs_clip_attn_supported(_CODE[q.dtype], q.shape[2] // heads, q.shape[1]))


def _plain(t):
    t = t.detach()
    return MSDA._aligned(t if t.is_contiguous() else t.contiguous())


def clip_forward(q, k, v, heads, want_lse=True):
    """-> (context [B, L, H 64], lse [B, H, L] fp32 or None); the arguments as ``_plain`` leaves them"""
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
    # delta (the caching allocator's, like the outputs: no device allocation in a steady loop)
    ws = torch.empty(max(_lib.mmfs_clip_attn_workspace_bytes(B, heads, L) // 4, 4), dtype=torch.float32, device=dev)
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
        q, k, v = _plain(q), _plain(k), _plain(v)
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


def _require(cond, what):
    if not cond:
        raise RuntimeError(what)


def clip_attention(q, k, v, heads):
    """q, k, v [B, L, H 64] device tensors of bf16 or fp16 as the Linear layers return them -> context [B, L, H 64]:
    softmax over all keys t of q[b, j] . k[b, t] / 8, times v.  Differentiable in q, k and v."""
    _require(all(isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 3 for t in (q, k, v)) and
             q.dtype in (torch.float16, torch.bfloat16), "clip_attention: q, k, v must be device tensors [B, L, H 64] of bf16 or fp16")
    _require(k.shape == q.shape and v.shape == q.shape and k.dtype == q.dtype and v.dtype == q.dtype and
             k.device == q.device and v.device == q.device, "clip_attention: k and v must have q's shape, type and device")
    _require(heads >= 1 and q.shape[2] == heads * HEAD_DIM, f"clip_attention: {q.shape[2]} channels are not {heads} heads of 64")
    _require(not torch.is_autocast_enabled(), "clip_attention: not under autocast")
    return ClipAttentionFunction.apply(q, k, v, heads)
