"""The ViT-Adapter's output pyramid from the tokens, packed token-major for the feature bank
(mm_interleaved/models/encoders/vit_adapter/vit_adapter_hf.py:137-153 + encoders/visual_tokenizer.py:74-82: transposed
copies of the adapter's tokens and the four ViT maps, ``adapter_up``, three bilinear resizes, five adds, a position add
per level -- and the bank builder's transposition back) as one or two gfx950 kernels forward and backward.  C ABI:
``mmfs_pyramid_head_*`` in include/mmfs_msda.h; kernels in csrc/mmfs_pyramid.hip.

``pyramid_head_supported`` tells the module whether the route applies; otherwise the module runs the reference's
framework statement unchanged.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import MultiScaleDeformableAttention as MSDA

_lib = MSDA._lib
_CODE = MSDA._FLOAT_CODE
NCHW, NHWC = 0, 1

# kernel calls since import, for tests and tools that ask which route the module took
launches = {"forward": 0, "backward": 0}


def level_mask(levels):
    """(0, 2, 3) -> the C ABI's bit mask (bit l = level l + 1 of c1, c2, c3, c4)."""
    mask = 0
    for l in levels:
        if not 0 <= int(l) <= 3:
            raise ValueError(f"levels: {l} is not one of 0..3")
        mask |= 1 << int(l)
    return mask


def level_sizes(H, W):
    return ((4 * H, 4 * W), (2 * H, 2 * W), (H, W), (H // 2, W // 2))


def _c1_layout(c1):
    if c1.is_contiguous():
        return NCHW
    return NHWC if c1.is_contiguous(memory_format=torch.channels_last) else None


def pyramid_head_supported(c, xs, c1, pos, H, W, mask):
    """The kernels apply: device tensors of ONE of f32 / f16 / bf16, c [B, 21 HW / 4, C], xs four [B, HW, C], c1
    [B, C, 4H, 4W], ``pos`` None or four fp32 tables [h_l w_l, C], C * element size a multiple of 16, H and W even,
    at least one level in ``mask``.  Inputs of levels that are not selected may be None."""
    if not (c.is_cuda and c.dim() == 3 and c.dtype in _CODE and H > 0 and W > 0):
        return False
    B, N, C = c.shape
    dt, dev = c.dtype, c.device
    if N * 4 != 21 * H * W or not _lib.mmfs_pyramid_head_supported(_CODE[dt], C, H, W, mask):
        return False
    sizes = level_sizes(H, W)
    for l in range(4):
        if not (mask >> l) & 1:
            continue
        x = xs[l]
        if not (x is not None and x.device == dev and x.dtype == dt and tuple(x.shape) == (B, H * W, C)):
            return False
        if pos is not None and not (pos[l].device == dev and pos[l].dtype == torch.float32
                                    and tuple(pos[l].shape) == (sizes[l][0] * sizes[l][1], C)):
            return False
    if mask & 1 and not (c1 is not None and c1.device == dev and c1.dtype == dt
                         and tuple(c1.shape) == (B, C, 4 * H, 4 * W)):
        return False
    return True



class PyramidHeadFunction(Function):
    """(c [B, 21 HW / 4, C], x1, x2, x3, x4 [B, HW, C], up [B, 4HW, 4C], c1 [B, C, 4H, 4W] contiguous or channels_last,
    pos: four fp32 tables or None, H, W, mask) -> the packed pyramid [B, sum of the selected h_l w_l, C]:
    up + c1 + bilinear x4 (x1) | c2 + bilinear x2 (x2) | c3 + x3 | c4 + mean 2x2 (x4), each + its table.  ``up`` is
    ``adapter_up`` as a GEMM on the c2 tokens with columns (di, dj, o).  Inputs of levels outside ``mask`` may be None
    and get no gradient.  Nothing is saved for the backward; its results are bit-reproducible."""

    @staticmethod
    def forward(ctx, c, x1, x2, x3, x4, up, c1, pos, H, W, mask):
        dt, dev = c.dtype, c.device
        B, _, C = c.shape
        on = [(mask >> l) & 1 for l in range(4)]
        xs = [MSDA._aligned(x.contiguous()) if o else None for x, o in zip((x1, x2, x3, x4), on)]
        c = MSDA._aligned(c.contiguous())
        layout = NCHW
        if on[0]:
            layout = _c1_layout(c1)
            if layout is None:
                c1, layout = c1.contiguous(), NCHW
            c1, up = MSDA._aligned(c1), MSDA._aligned(up.contiguous())
            if _c1_layout(c1) != layout:                   # (a clone for alignment is plain contiguous)
                layout = NCHW
        else:
            c1 = up = None
        tabs = [MSDA._aligned(pos[l].contiguous()) if pos is not None and on[l] else None for l in range(4)]
        S = sum(h * w for (h, w), o in zip(level_sizes(H, W), on) if o)
        out = torch.empty((B, S, C), dtype=dt, device=dev)
        MSDA._call("pyramid_fwd", "mmfs_pyramid_head_forward", dev, _CODE[dt], c.data_ptr(), *map(MSDA._ptr, xs),
                   MSDA._ptr(up), MSDA._ptr(c1), *map(MSDA._ptr, tabs), out.data_ptr(), B, H, W, C, mask, layout)
        launches["forward"] += 1
        ctx.conf = (B, H, W, C, mask, layout, c.shape[1], dt, dev)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        B, H, W, C, mask, layout, Nc, dt, dev = ctx.conf
        on = [(mask >> l) & 1 for l in range(4)]
        need = ctx.needs_input_grad                           # (c, x1, x2, x3, x4, up, c1, ...): a gradient nobody needs is not computed
        g = MSDA._aligned(g.to(dt).contiguous())
        gx = [torch.empty((B, H * W, C), dtype=dt, device=dev) if on[l] and need[1 + l] else None for l in range(4)]
        g_up = g_c1 = None
        if on[0] and need[5]:
            g_up = torch.empty((B, 4 * H * W, 4 * C), dtype=dt, device=dev)
        if on[0] and need[6]:
            g_c1 = torch.empty((B, C, 4 * H, 4 * W), dtype=dt, device=dev,
                               memory_format=torch.channels_last if layout == NHWC else torch.contiguous_format)
        if B * C and any(t is not None for t in gx + [g_up, g_c1]):
            MSDA._call("pyramid_bwd", "mmfs_pyramid_head_backward", dev, _CODE[dt], g.data_ptr(), MSDA._ptr(g_up),
                       MSDA._ptr(g_c1), *map(MSDA._ptr, gx), B, H, W, C, mask, layout)
            launches["backward"] += 1
        # the adapter tokens' gradient is levels 2..4 of g itself; a level that was not produced gives none (zeros)
        lo = 16 * H * W if on[0] else 0
        if not need[0]:
            g_c = None
        elif on[1] and on[2] and on[3]:
            g_c = g[:, lo:]
        elif on[1] or on[2] or on[3]:
            g_c = g.new_zeros((B, Nc, C))
            at = 0
            for l, (h, w) in enumerate(level_sizes(H, W)[1:], 1):
                if on[l]:
                    g_c[:, at:at + h * w] = g[:, lo:lo + h * w]
                    lo += h * w
                at += h * w
        else:
            g_c = None
        return (g_c, *gx, g_up, g_c1, None, None, None, None)
