"""The interleaved sequence on the device (csrc/mmfs_sequence.hip; C ABI ``mmfs_sequence_*`` in include/mmfs_msda.h):
the int32 tables of the special tokens from ``text_ids`` in one launch, the token embeddings with the visual embeddings
and the ``<soi>`` token in place (mm_interleaved/models/mm_interleaved.py:144-171), and the reversed, ragged gather that
makes the image decoder's per-image context (:254-304), each with its backward.  Nothing here reads a value back from
the device: every call can be captured into a graph.

``sequence_supported`` tells ``mmfs_amd.sequence`` whether the kernels apply; otherwise it states the same mathematics
with framework ops.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import MultiScaleDeformableAttention as MSDA

_lib = MSDA._lib
_CODE = MSDA._FLOAT_CODE
MAX_TOKENS = 1 << 22

# kernel calls since import, for tests and tools that ask which route the module took
launches = {"index": 0, "embed_forward": 0, "embed_backward": 0, "context_forward": 0, "context_backward": 0}


def sequence_supported(ref, *others, C=None):
    """The kernels apply to ``ref`` (and to ``others``, tensors or None, which must share its device and type): a device
    tensor of f32 / f16 / bf16 whose rows of ``C`` (default: its last dimension) elements are whole 16-byte vectors, outside
    autocast."""
    if not (isinstance(ref, torch.Tensor) and ref.is_cuda and ref.dtype in _CODE) or torch.is_autocast_enabled():
        return False
    C = ref.shape[-1] if C is None else C
    if not _lib.mmfs_sequence_supported(_CODE[ref.dtype], C):
        return False
    return all(t is None or (t.device == ref.device and t.dtype == ref.dtype) for t in others)



def sequence_index(text_ids, image_token_id, soi_token_id, n_vis, n_images):
    """text_ids [B, L] (long, on the device) -> (img_rank [B L], img_pos [n_vis], soi_row [n_images], soi_col [n_images],
    row_first [B + 1], counts [2]), all int32, in one launch."""
    B, L = text_ids.shape
    dev = text_ids.device
    if max(B * L, n_vis, n_images) > MAX_TOKENS:
        raise ValueError(f"sequence_index: B * L = {B * L}, n_vis = {n_vis}, n_images = {n_images}: at most {MAX_TOKENS} each")
    ids = text_ids.contiguous()
    # one allocation: rank | pos | row | col | first | counts
    sizes = (B * L, n_vis, n_images, n_images, B + 1, 2)
    buf = torch.empty(sum(sizes), dtype=torch.int32, device=dev)
    parts = buf.split(sizes)
    MSDA._call("seq_index", "mmfs_sequence_index", dev, ids.data_ptr(), B, L, int(image_token_id), int(soi_token_id), n_vis,
               n_images, *[p.data_ptr() for p in parts])
    launches["index"] += 1
    return parts


class SequenceEmbedFunction(Function):
    """(text [B, L, C] of T or fp32, vis [n_vis, C] of T, soi_token [.., C] of T, text_ids [B, L], soi_token_id, img_rank,
    img_pos, soi_row, soi_col, counts, n_images) -> [B, L, C] of T: the visual rows in place of the image tokens' rows, the
    text rows cast to T elsewhere, ``soi_token`` added (in T) to every ``<soi>`` row.  The tables are ``sequence_index``'s
    for this ``text_ids`` and n_vis; grad_soi sums the first min(found, n_images) ``<soi>`` rows.  Bit-reproducible."""

    @staticmethod
    def forward(ctx, text, vis, soi_token, text_ids, soi_token_id, img_rank, img_pos, soi_row, soi_col, counts, n_images):
        dt, dev = vis.dtype, vis.device
        B, L, C = text.shape
        n_vis = vis.shape[0]
        text_c = MSDA._aligned(text.contiguous())
        vis_c = MSDA._aligned(vis.contiguous())
        soi_c = MSDA._aligned(soi_token.contiguous())
        ids = text_ids.contiguous()
        out = torch.empty((B, L, C), dtype=dt, device=dev)
        MSDA._call("seq_embed_fwd", "mmfs_sequence_embed_forward", dev, _CODE[dt], _CODE[text.dtype], text_c.data_ptr(),
                   vis_c.data_ptr(), soi_c.data_ptr(), ids.data_ptr(), int(soi_token_id), img_rank.data_ptr(),
                   out.data_ptr(), B * L, C, n_vis)
        launches["embed_forward"] += 1
        ctx.save_for_backward(img_rank, img_pos, soi_row, soi_col, counts)
        ctx.conf = (B, L, C, n_vis, n_images, dt, text.dtype, dev, tuple(soi_token.shape))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        img_rank, img_pos, soi_row, soi_col, counts = ctx.saved_tensors
        B, L, C, n_vis, n_images, dt, text_dt, dev, soi_shape = ctx.conf
        need = ctx.needs_input_grad
        g = MSDA._aligned(g.to(dt).contiguous())
        g_text = torch.empty((B, L, C), dtype=text_dt, device=dev) if need[0] else None
        g_vis = torch.empty((n_vis, C), dtype=dt, device=dev) if need[1] else None
        g_soi = torch.empty(soi_shape, dtype=dt, device=dev) if need[2] else None
        if any(t is not None and t.numel() for t in (g_text, g_vis, g_soi)):
            MSDA._call("seq_embed_bwd", "mmfs_sequence_embed_backward", dev, _CODE[dt], _CODE[text_dt], g.data_ptr(),
                       img_rank.data_ptr(), img_pos.data_ptr(), soi_row.data_ptr(), soi_col.data_ptr(), counts.data_ptr(),
                       MSDA._ptr(g_text), MSDA._ptr(g_vis), MSDA._ptr(g_soi), B * L, L, C, n_vis, n_images)
            launches["embed_backward"] += 1
        return (g_text, g_vis, g_soi) + (None,) * 8


class ContextGatherFunction(Function):
    """(src [B, L, C], pad_row [C] | None, pos [seq_len, C] | None, soi_row, soi_col, row_first, start_idx | None,
    bos_idx | None, n_images, max_len) -> (out [n_images, max_len, C], mask [n_images, max_len] long):
    out[i, j] = src[row_i, col_i - j] + pos[j] inside image i's window, pad_row + pos[j] behind it (include/mmfs_msda.h,
    "The interleaved sequence").  ``src`` and ``pad_row`` get gradients (a gather and a two-stage sum, no atomics);
    ``pos`` is a constant table and gets none."""

    @staticmethod
    def forward(ctx, src, pad_row, pos, soi_row, soi_col, row_first, start_idx, bos_idx, n_images, max_len):
        dt, dev = src.dtype, src.device
        B, L, C = src.shape
        seq_len = pos.shape[0] if pos is not None else max(max_len, L)
        src_c = MSDA._aligned(src.contiguous())
        pad_c = None if pad_row is None else MSDA._aligned(pad_row.contiguous())
        pos_c = None if pos is None else MSDA._aligned(pos.contiguous())
        start_c = None if start_idx is None else start_idx.contiguous()
        bos_c = None if bos_idx is None else bos_idx.contiguous()
        out = torch.empty((n_images, max_len, C), dtype=dt, device=dev)
        mask = torch.empty((n_images, max_len), dtype=torch.long, device=dev)
        MSDA._call("seq_context_fwd", "mmfs_sequence_context_forward", dev, _CODE[dt], src_c.data_ptr(), MSDA._ptr(pad_c),
                   MSDA._ptr(pos_c), soi_row.data_ptr(), soi_col.data_ptr(), MSDA._ptr(start_c), MSDA._ptr(bos_c),
                   out.data_ptr(), mask.data_ptr(), B, L, C, n_images, max_len, seq_len)
        launches["context_forward"] += 1
        ctx.save_for_backward(soi_row, soi_col, row_first, start_c, bos_c)
        ctx.conf = (B, L, C, n_images, max_len, seq_len, dt, dev, pad_row is not None)
        ctx.mark_non_differentiable(mask)
        return out, mask

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_mask):
        soi_row, soi_col, row_first, start_c, bos_c = ctx.saved_tensors
        B, L, C, n_images, max_len, seq_len, dt, dev, has_pad = ctx.conf
        need = ctx.needs_input_grad
        g = MSDA._aligned(g.to(dt).contiguous())
        g_src = torch.empty((B, L, C), dtype=dt, device=dev) if need[0] else None
        g_pad = ws = None
        if has_pad and need[1]:
            g_pad = torch.empty((C,), dtype=dt, device=dev)
            nbytes = _lib.mmfs_sequence_context_backward_workspace_bytes(_CODE[dt], C, n_images)
            MSDA._check(min(nbytes, 0), "mmfs_sequence_context_backward_workspace_bytes")
            ws = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=dev)
        if g_src is not None or g_pad is not None:
            MSDA._call("seq_context_bwd", "mmfs_sequence_context_backward", dev, _CODE[dt], g.data_ptr(), soi_row.data_ptr(),
                       soi_col.data_ptr(), row_first.data_ptr(), MSDA._ptr(start_c), MSDA._ptr(bos_c), MSDA._ptr(g_src),
                       MSDA._ptr(g_pad), MSDA._ptr(ws), B, L, C, n_images, max_len, seq_len)
            launches["context_backward"] += 1
        return (g_src, g_pad) + (None,) * 8
