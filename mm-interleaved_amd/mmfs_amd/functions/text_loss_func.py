"""The text loss on the device (csrc/mmfs_text_loss.hip; C ABI ``mmfs_text_loss_*`` in include/mmfs_msda.h): the
cross-entropy of the text decoder's logits [B, L, V], read once in their storage type, and its gradient, written once
(mm_interleaved/models/mm_interleaved.py:449-476).  Nothing here reads a value back from the device: every call can be
captured into a graph.

``text_loss_supported`` tells ``mmfs_amd.text_loss`` whether the kernels apply; otherwise it states the same mathematics
with framework ops.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import MultiScaleDeformableAttention as MSDA

_lib = MSDA._lib
_CODE = MSDA._FLOAT_CODE
REDUCTION = {"none": 0, "sum": 1, "mean": 2}
MAX_ROWS = 1 << 22

# kernel calls since import, for tests and tools that ask which route the module took
launches = {"forward": 0, "backward": 0}


def text_loss_supported(logits):
    """The kernels apply to ``logits`` [B, L, V]: a device tensor of f32 / f16 / bf16 with B L <= 2^22 rows of any width
    1 <= V <= 2^24, outside autocast."""
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype in _CODE and logits.dim() == 3):
        return False
    if torch.is_autocast_enabled():
        return False
    B, L, V = logits.shape
    return B * L <= MAX_ROWS and bool(_lib.mmfs_text_loss_supported(_CODE[logits.dtype], V))


def _forward(logits, labels, first, ignore_index, code):
    dt, dev = logits.dtype, logits.device
    B, L, V = logits.shape
    n = labels.shape[1]
    x = MSDA._aligned(logits.contiguous())
    lab = labels.contiguous()
    # one allocation: loss | lse | out; and the two counters
    buf = torch.empty(2 * B * n + 1, dtype=torch.float32, device=dev)
    loss, lse, out = buf.split((B * n, B * n, 1))
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    MSDA._call("text_loss_fwd", "mmfs_text_loss_forward", dev, _CODE[dt], x.data_ptr(), lab.data_ptr(), loss.data_ptr(),
               lse.data_ptr(), out.data_ptr(), counts.data_ptr(), B, L, V, first, n, ignore_index, code)
    launches["forward"] += 1
    return x, lab, loss.view(B, n), lse.view(B, n), out.view(()), counts


def row_losses(logits, labels, first, ignore_index):
    """-> (loss [B, n], lse [B, n], counts [2]) of the forward kernels, outside autograd (tests and tools)."""
    with torch.no_grad():
        _, _, loss, lse, _, counts = _forward(logits, labels, first, ignore_index, 0)
    return loss, lse, counts


class TextLossFunction(Function):
    """(logits [B, L, V] of T, labels [B, n] long, first, ignore_index, reduction) -> (out, counts [2] int32): row
    (b, first + j) against labels[b, j] in fp32; ``out`` is [B, n] fp32 ("none", 0 at ignored rows) or a 0-dim fp32 tensor
    ("sum", "mean" over the valid rows); counts = valid rows, rows whose label is outside [0, V) and not ``ignore_index``
    (treated as ignored).  The gradient has the logits' type and shape, every element written.  Bit-reproducible."""

    @staticmethod
    def forward(ctx, logits, labels, first, ignore_index, reduction):
        code = REDUCTION[reduction]
        x, lab, loss, lse, out, counts = _forward(logits, labels, first, ignore_index, code)
        ctx.save_for_backward(x, lab, lse, counts)
        ctx.conf = (*logits.shape, first, labels.shape[1], ignore_index, code, logits.dtype, logits.device)
        ctx.mark_non_differentiable(counts)
        return (loss if code == 0 else out), counts

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_counts):
        x, lab, lse, counts = ctx.saved_tensors
        B, L, V, first, n, ignore_index, code, dt, dev = ctx.conf
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        g = g.to(torch.float32).contiguous()
        grad = torch.empty((B, L, V), dtype=dt, device=dev)
        MSDA._call("text_loss_bwd", "mmfs_text_loss_backward", dev, _CODE[dt], x.data_ptr(), lab.data_ptr(), lse.data_ptr(),
                   g.data_ptr(), counts.data_ptr(), grad.data_ptr(), B, L, V, first, n, ignore_index, code)
        launches["backward"] += 1
        return (grad,) + (None,) * 4
