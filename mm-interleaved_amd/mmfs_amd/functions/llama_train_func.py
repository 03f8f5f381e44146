"""The LLM's self-attention in training on the device (csrc/mmfs_llama_train.hip; C ABI ``mmfs_llama_attn_train_*`` in
include/mmfs_msda.h): the rotary embedding of q and k, causal attention and its backward, q, k, v [B, L, H 128] as the Linear
layers return them -> context [B, L, H 128].  What the reference's ``_forward_train`` asks of ``flash_attn_func(q, k, v, 0.0,
softmax_scale=None, causal=True)``.  Nothing of size L x L exists at any time; nothing reads a value back from the device:
forward and backward can be captured into a graph.  Bit-reproducible.

    context = mmfs_amd.llama_attn_train(q, k, v, position_ids, cos, sin, heads)

``mmfs_amd.llama_attn.LlamaSelfAttention`` takes this on its training route.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import MultiScaleDeformableAttention as MSDA

_CODE = MSDA._DTYPE_CODE
HEAD_DIM = 128
# how the kernels cut their work, where their paths change: the query rows of a workgroup (forward, dq), the keys of a
# forward tile, the keys of a dkdv workgroup, the queries of a dkdv tile, the query rows of a wave
TRAIN_TILES = MSDA._tiles("mmfs_llama_attn_train_tiles", 5)

# kernel launches since import, for tests and tools that ask which route the module took
launches = {"rope": 0, "forward": 0, "backward": 0}


def llama_attn_train_supported(q, heads):
    """The kernels apply: a device tensor q [B, L, H 128] of bf16 or fp16, L >= 1, outside autocast."""
    return MSDA._attn_supported(q, heads, "mmfs_llama_attn_train_supported")


def _positions(position_ids, B, L, dev):
    pos = position_ids.detach()
    if pos.dtype != torch.int64 or pos.device != dev or not pos.is_contiguous() or tuple(pos.shape) != (B, L):
        pos = pos.to(device=dev, dtype=torch.int64).expand(B, L).contiguous()
    return pos


def train_rope(q, k, pos, cos, sin, heads):
    """-> (q_rot, k_rot); the arguments as ``_positions`` and ``MSDA._plain`` leave them"""
    B, L, C = q.shape
    q_rot, k_rot = torch.empty_like(q), torch.empty_like(k)
    MSDA._call("llama_train_rope", "mmfs_llama_attn_train_rope", q.device, _CODE[q.dtype], q.data_ptr(), k.data_ptr(),
               pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), cos.shape[0], q_rot.data_ptr(), k_rot.data_ptr(), B, L, heads,
               C // heads)
    launches["rope"] += 1
    return q_rot, k_rot


def train_forward(q_rot, k_rot, v, heads):
    """-> (context [B, L, H 128], lse [B, H, L] fp32)"""
    B, L, C = q_rot.shape
    out = torch.empty_like(q_rot)
    lse = torch.empty((B, heads, L), dtype=torch.float32, device=q_rot.device)
    MSDA._call("llama_train_fwd", "mmfs_llama_attn_train_forward", q_rot.device, _CODE[q_rot.dtype], q_rot.data_ptr(),
               k_rot.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), B, L, heads, C // heads)
    launches["forward"] += 1
    return out, lse


def train_backward(q_rot, k_rot, v, out, grad, lse, pos, cos, sin, heads):
    """-> (dq, dk, dv) of the unrotated q and k and of v"""
    B, L, C = q_rot.shape
    dev = q_rot.device
    dq, dk, dv = torch.empty_like(q_rot), torch.empty_like(q_rot), torch.empty_like(q_rot)
    ws = MSDA._float_workspace("mmfs_llama_attn_train_workspace_bytes", dev, B, heads, L)       # delta
    MSDA._call("llama_train_bwd", "mmfs_llama_attn_train_backward", dev, _CODE[q_rot.dtype], q_rot.data_ptr(), k_rot.data_ptr(),
               v.data_ptr(), out.data_ptr(), grad.data_ptr(), lse.data_ptr(), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(),
               cos.shape[0], dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr(), B, L, heads, C // heads)
    launches["backward"] += 2
    return dq, dk, dv


class LlamaAttnTrainFunction(Function):
    """(q, k, v, position_ids, cos, sin, heads) -> context [B, L, H 128] of the inputs' type: causal attention of the rotated
    q and k.  Saved for the backward: q_rot, k_rot, v, the context and lse [B, H, L] -- nothing of size L x L.  Gradients flow
    to q, k and v only, of their type, every element written once."""

    @staticmethod
    def forward(ctx, q, k, v, position_ids, cos, sin, heads):
        B, L, _ = q.shape
        q, k, v = MSDA._plain(q), MSDA._plain(k), MSDA._plain(v)
        pos = _positions(position_ids, B, L, q.device)
        q_rot, k_rot = train_rope(q, k, pos, cos, sin, heads)
        out, lse = train_forward(q_rot, k_rot, v, heads)
        ctx.save_for_backward(q_rot, k_rot, v, out, lse, pos, cos, sin)
        ctx.heads = heads
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        q_rot, k_rot, v, out, lse, pos, cos, sin = ctx.saved_tensors
        grad = MSDA._aligned(grad.to(q_rot.dtype).contiguous())
        dq, dk, dv = train_backward(q_rot, k_rot, v, out, grad, lse, pos, cos, sin, ctx.heads)
        return dq, dk, dv, None, None, None, None


def llama_attn_train(q, k, v, position_ids, cos, sin, heads):
    """q, k, v [B, L, H 128] device tensors of bf16 or fp16 as the Linear layers return them, position_ids [B, L] (or
    [1, L]) integers, (cos, sin) of ``rope_table`` on the device -> context [B, L, H 128]:
    softmax over the keys t <= j of rope(q)[b, j] . rope(k)[b, t] / sqrt(128), times v.  Differentiable in q, k and v."""
    MSDA._require_qkv("llama_attn_train", q, k, v, heads, HEAD_DIM)
    B, L, _ = q.shape
    for name, t in (("cos", cos), ("sin", sin)):
        MSDA._require(t.dtype == torch.float32 and t.device == q.device and t.is_contiguous() and t.dim() == 2 and
                 t.shape[1] == HEAD_DIM // 2 and t.shape == cos.shape and t.data_ptr() % 16 == 0,
                 f"llama_attn_train: {name} must be contiguous fp32 [max_pos, 64] on q's device (rope_table)")
    MSDA._require(position_ids.numel() in (L, B * L), "llama_attn_train: position_ids must be [B, L] (or [1, L])")
    return LlamaAttnTrainFunction.apply(q, k, v, position_ids, cos, sin, heads)
