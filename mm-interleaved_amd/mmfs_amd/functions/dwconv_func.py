"""The depthwise 3x3 convolution of the ViT-Adapter's ``ConvFFN`` on the tokens as they lie, with bias and an optional
exact GELU (mm_interleaved/models/encoders/vit_adapter/adapter_modules.py:64-89 between ``fc1`` and ``fc2``: three
transposed copies, three convolutions, three transposes back, a ``cat`` and GELU) as one gfx950 kernel forward and one
pass + a small fixed-order reduction backward.  C ABI: ``mmfs_dwconv_tokens_*`` in include/mmfs_msda.h; kernels in
csrc/msda_dwconv.hip.

``dwconv_tokens_supported`` tells the block whether the route applies; otherwise the block runs the reference's
framework statement unchanged.
"""
import ctypes

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import MultiScaleDeformableAttention as MSDA

_lib = MSDA._lib
_CODE = MSDA._FLOAT_CODE
ACT = {"none": 0, "gelu": 1}

# kernel calls since import, for tests and tools that ask which route a block took
launches = {"forward": 0, "backward": 0}

_host_levels = {}


def _levels(level_hw):
    """((h, w), ...) -> (key, the host array the C ABI reads); one array per table, kept."""
    key = tuple((int(h), int(w)) for h, w in level_hw)
    arr = _host_levels.get(key)
    if arr is None:
        arr = _host_levels[key] = (ctypes.c_int64 * (2 * len(key)))(*[v for hw in key for v in hw])
    return key, arr


def dwconv_tokens_supported(x, weight, bias):
    """The token kernel applies: device tensors of ONE of f32 / f16 / bf16 (input, weight and bias alike), x [B, N, C]
    with C * element size a multiple of 16, weight [C, 1, 3, 3]."""
    return bool(x.is_cuda and x.dim() == 3 and x.dtype in _CODE and weight.is_cuda and weight.dtype == x.dtype
                and tuple(weight.shape) == (x.shape[2], 1, 3, 3)
                and (bias is None or (bias.is_cuda and bias.dtype == x.dtype and tuple(bias.shape) == (x.shape[2],)))
                and _lib.mmfs_dwconv_tokens_supported(_CODE[x.dtype], x.shape[2], 1, 0))


class DWConvTokensFunction(Function):
    """(x [B, N, C], weight [C, 1, 3, 3], bias [C] | None, level_hw ((h, w), ...) with sum h * w == N, act "none" | "gelu")
    -> [B, N, C]: every map convolved as an image (3x3, stride 1, zero padding, depthwise), then -- "gelu" -- the exact
    GELU of the stored pre-activation.  With gradients the pre-activation is kept beside ``x``; the backward returns
    the gradients of x, weight and bias, the last two bit-reproducible."""

    @staticmethod
    def forward(ctx, x, weight, bias, level_hw, act):
        dt, dev = x.dtype, x.device
        B, N, C = x.shape
        key, arr = _levels(level_hw)
        code = ACT[act]
        x = MSDA._aligned(x.contiguous())
        weight = MSDA._aligned(weight.contiguous())
        bias = None if bias is None else MSDA._aligned(bias.contiguous())
        needs_grad = any(ctx.needs_input_grad[:3])
        out = torch.empty((B, N, C), dtype=dt, device=dev)
        pre = torch.empty((B, N, C), dtype=dt, device=dev) if needs_grad and code else None
        MSDA._call("dwconv_fwd", "mmfs_dwconv_tokens_forward", dev, _CODE[dt], x.data_ptr(), weight.data_ptr(),
                   MSDA._ptr(bias), out.data_ptr(), MSDA._ptr(pre), arr, B, N, C, len(key), code)
        launches["forward"] += 1
        if needs_grad:
            ctx.save_for_backward(x, weight, pre)
            ctx.conf = (key, code, bias is not None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, weight, pre = ctx.saved_tensors
        key, code, has_bias = ctx.conf
        dt, dev = x.dtype, x.device
        B, N, C = x.shape
        _, arr = _levels(key)
        g = MSDA._aligned(g.to(dt).contiguous())
        gx = torch.empty_like(x)
        gw = torch.empty_like(weight)
        gb = torch.empty((C,), dtype=dt, device=dev) if has_bias else None
        if x.numel() == 0:
            gw.zero_()
            if gb is not None:
                gb.zero_()
            return gx, gw, gb, None, None
        nbytes = _lib.mmfs_dwconv_tokens_backward_workspace_bytes(_CODE[dt], arr, B, N, C, len(key), code)
        MSDA._check(min(nbytes, 0), "mmfs_dwconv_tokens_backward_workspace_bytes")
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        MSDA._call("dwconv_bwd", "mmfs_dwconv_tokens_backward", dev, _CODE[dt], g.data_ptr(), x.data_ptr(), MSDA._ptr(pre),
                   weight.data_ptr(), gx.data_ptr(), gw.data_ptr(), MSDA._ptr(gb), ws.data_ptr(), arr, B, N, C, len(key),
                   code)
        launches["backward"] += 1
        return gx, gw, gb, None, None
