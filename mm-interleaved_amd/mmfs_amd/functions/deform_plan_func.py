"""Fused front end of the image encoder's ``MSDeformAttn`` (ViT-Adapter): everything the reference module runs
between its two Linear heads and the op
(mm_interleaved/models/encoders/vit_adapter/ops/modules/ms_deform_attn.py:108-127 -- softmax, division by the level
extent, add of the reference point, cast, two copies) as one gfx950 kernel each way, and plan + sampler as ONE kernel
for calls without gradients.  C ABI: ``mmfs_deform_plan_forward`` / ``mmfs_deform_plan_backward`` /
``mmfs_deform_sample_forward`` in include/mmfs_msda.h; kernels in csrc/msda_deform_plan.hip.

``deform_plan_supported`` tells the module whether the fused route applies; otherwise the module evaluates the same
mathematics with framework ops -- that is NOT a CPU fallback of the sampling op, only of this front end, and it is
what the CPU parity tests of the module and of the adapter blocks exercise.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import MultiScaleDeformableAttention as MSDA

_lib = MSDA._lib
_CODE = MSDA._FLOAT_CODE


def _ref_ok(reference_points, N, L):
    return (reference_points.dim() == 4 and reference_points.shape[0] in (1, N) and reference_points.shape[2] in (1, L)
            and reference_points.shape[3] in (2, 4))


def deform_plan_supported(query, reference_points, spatial_shapes, n_levels, n_points):
    """The fused front end applies: device tensors of f32 / f16 / bf16, P in {2, 4, 8}, L <= 8, reference points
    [1 | N, Lq, 1 | L, 2 | 4] that need no gradient, a contiguous int64 level table."""
    return bool(query.is_cuda and query.dtype in _CODE and reference_points.is_cuda
                and _ref_ok(reference_points, query.shape[0], n_levels)
                and not (reference_points.requires_grad and torch.is_grad_enabled())
                and spatial_shapes.is_cuda and spatial_shapes.dtype == torch.int64 and spatial_shapes.is_contiguous()
                and tuple(spatial_shapes.shape) == (n_levels, 2)
                and _lib.mmfs_deform_plan_supported(_CODE[query.dtype], n_levels, n_points, reference_points.shape[3], 0) & 1)


def _ref32(reference_points):
    r = reference_points.detach()
    return r if r.dtype == torch.float32 and r.is_contiguous() else r.float().contiguous()


def _stacked_ok(C, n_off, es):
    """The kernels' vector accesses (at most 16 bytes) take the two column ranges of a [.., C] row as they lie."""
    return (C * es) % 16 == 0 and (n_off * es) % 16 == 0


def _heads(both, n_off):
    """-> (off tensor, logit tensor, pointers, leading dimensions): the column ranges of ``both`` as they lie, or -- rows
    the vector accesses cannot take (an odd H * L at P = 2) -- two packed copies."""
    C, es = both.shape[-1], both.element_size()
    if _stacked_ok(C, n_off, es) and both.data_ptr() % 16 == 0:
        return both, both, both.data_ptr(), both.data_ptr() + n_off * es, C, C
    off, logit = both[..., :n_off].contiguous(), both[..., n_off:].contiguous()
    return off, logit, off.data_ptr(), logit.data_ptr(), 0, 0


class DeformPlanFunction(Function):
    """(both [N, Lq, H*L*P*2 + H*L*P] -- the two heads' result as ONE GEMM's, offsets' columns first --,
    ref [Nr, Lq, Lref, R], shapes [L, 2] long, H, L, P) -> loc [N, Lq, H, L, P, 2], attn [N, Lq, H, L, P].
    The kernels read and write the column ranges as they lie; the backward returns ONE gradient for ``both``."""

    @staticmethod
    def forward(ctx, both, ref, shapes, H, L, P):
        dt, dev = both.dtype, both.device
        N, Lq, C = both.shape
        n_off = H * L * P * 2
        assert C == n_off + H * L * P, "both must hold the offsets' and the logits' columns"
        both, ref = both.contiguous(), _ref32(ref)
        Nr, Lref, R = ref.shape[0], ref.shape[2], ref.shape[3]
        loc = torch.empty((N, Lq, H, L, P, 2), dtype=dt, device=dev)
        attn = torch.empty((N, Lq, H, L, P), dtype=dt, device=dev)
        dims = (N, Lq, H, L, P, Nr, Lref, R)
        off, logit, p_off, p_att, ld_off, ld_att = _heads(both, n_off)
        MSDA._call("deform_plan_fwd", "mmfs_deform_plan_forward", dev, _CODE[dt], p_off, p_att, ld_off, ld_att,
                   ref.data_ptr(), shapes.data_ptr(), loc.data_ptr(), attn.data_ptr(), *dims)
        ctx.save_for_backward(attn, ref, shapes)
        ctx.dims = dims
        return loc, attn

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loc, g_attn):
        attn, ref, shapes = ctx.saved_tensors
        dt, dev = attn.dtype, attn.device
        N, Lq, H, L, P, Nr, Lref, R = ctx.dims
        n_off = H * L * P * 2
        C = n_off + H * L * P
        g_loc, g_attn = g_loc.to(dt).contiguous(), g_attn.to(dt).contiguous()
        stacked = _stacked_ok(C, n_off, attn.element_size())
        if stacked:
            d_both = torch.empty((N, Lq, C), dtype=dt, device=dev)
            p_off, p_att, ld = d_both.data_ptr(), d_both.data_ptr() + n_off * d_both.element_size(), C
        else:
            d_off = torch.empty((N, Lq, n_off), dtype=dt, device=dev)
            d_att = torch.empty((N, Lq, C - n_off), dtype=dt, device=dev)
            p_off, p_att, ld = d_off.data_ptr(), d_att.data_ptr(), 0
        MSDA._call("deform_plan_bwd", "mmfs_deform_plan_backward", dev, _CODE[dt], g_loc.data_ptr(), g_attn.data_ptr(),
                   attn.data_ptr(), ref.data_ptr(), shapes.data_ptr(), p_off, p_att, ld, ld, *ctx.dims)
        return (d_both if stacked else torch.cat((d_off, d_att), -1)), None, None, None, None, None


def deform_sample_forward(value, shapes, start, both, ref, H, L, P):
    """Plan -> sampler in ONE kernel (``mmfs_deform_sample_forward``): loc / attn are never written.  No autograd
    graph.  value [N, S, H, D]; ``both`` / ``ref`` / ``shapes`` as for ``DeformPlanFunction``; ``start`` [L] long.
    Returns out [N, Lq, H*D], or None when the shape is outside the fused kernel's range (the caller then runs
    ``DeformPlanFunction`` + the op)."""
    dt, dev = value.dtype, value.device
    if dt not in _CODE or both.dtype != dt or not value.is_cuda:
        return None
    N, S, Hh, D = value.shape
    Lq, C = both.shape[1], both.shape[2]
    n_off = H * L * P * 2
    if Hh != H or both.shape[0] != N or C != n_off + H * L * P or start.dtype != torch.int64 or start.numel() != L:
        return None
    ref = _ref32(ref)
    if not (_lib.mmfs_deform_plan_supported(_CODE[dt], L, P, ref.shape[3], D) & 2) or S == 0:
        return None
    value, both, start = MSDA._aligned(value.contiguous()), both.contiguous(), start.contiguous()
    out = torch.empty((N, Lq, H * D), dtype=dt, device=dev)
    off, logit, p_off, p_att, ld_off, ld_att = _heads(both, n_off)
    if MSDA._call("deform_sample_fwd", "mmfs_deform_sample_forward", dev, _CODE[dt], value.data_ptr(), shapes.data_ptr(),
                  start.data_ptr(), p_off, p_att, ld_off, ld_att, ref.data_ptr(), out.data_ptr(), N, S, Lq, H, D, L, P,
                  ref.shape[0], ref.shape[2], ref.shape[3], refuse_ok=True):
        return None
    return out
