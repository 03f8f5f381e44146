"""The interleaved sequence between the tokenizer and the two decoders, without Python loops over the batch and without
device->host syncs: step 3 of the reference's ``_prepare_mm_embeds``
(mm_interleaved/models/mm_interleaved.py:144-171) and ``_prepare_context_features_for_image_decoder`` (:254-304).

    tables = sequence_tables(text_ids, image_token_id=.., soi_token_id=.., n_vis=.., n_images=..)
    mm_embeds = assemble_mm_embeds(text_embeds, text_ids, vis_embed, soi_token, image_token_id=.., soi_token_id=..)
    feats, mask = prepare_context_features_for_image_decoder(context, text_ids, context_feat_proj, soi_token_id=..,
                                                             n_images=.., seq_len=.., max_len=77)

The per-image context rests on one identity.  With P = context_feat_proj(context) over the B L tokens that exist,

    out[i, j] = P[row_i, soi_i - j] + pos[j]        j < len_i = soi_i - bos_i + 1
              = bias + pos[j]                       len_i <= j < max_len          (proj(0) = bias)

so the projection runs once per token (``order="project_first"``) and the per-image tensor is a reversed, ragged gather
with an add -- the reference projects every padded row of every image.  One deviation follows: a padded row is
``bias + pos``, not ``0 W + bias + pos``; a non-finite weight does not reach the masked padding.

Device tensors of f32 / f16 / bf16 with rows of whole 16-byte vectors run the gfx950 kernels of csrc/mmfs_sequence.hip
(``functions/sequence_func.py``); host tensors, autocast, other widths and types run the same statements with framework
ops, loop-free and sync-free too.  ``route="kernels"`` / ``"framework"`` forces either; a forced kernel route that does
not apply raises.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from . import levels as _levels

SequenceTables = namedtuple("SequenceTables", "img_rank img_pos soi_row soi_col row_first counts B L n_vis n_images "
                                              "image_token_id soi_token_id")
SequenceTables.__doc__ = """int32 tables of one ``text_ids`` [B, L] (csrc/mmfs_sequence.hip ``seq_index``): img_rank [B L]
the row-major rank of an image token (-1: not one, or rank >= n_vis); img_pos [n_vis] its inverse (-1: no such token);
soi_row / soi_col [n_images] row and column of the k-th ``<soi>`` (-1 past the last); row_first [B + 1] the images of
row b are row_first[b] .. row_first[b + 1] - 1; counts [2] the image and ``<soi>`` tokens found."""

# which route device tensors take when the caller does not say (profiles/sequence.md holds the measurement behind it)
DEFAULT_ROUTE = "kernels"


def _func():
    from .functions import sequence_func            # (loads the native library: host-only callers never need it)
    return sequence_func


def _route(route, ok, what):
    forced = route is not None
    route = route if forced else DEFAULT_ROUTE
    if route not in ("kernels", "framework"):
        raise ValueError(f"route: {route!r} is not 'kernels' or 'framework'")
    if route == "kernels" and not ok():
        if forced:
            raise RuntimeError(f"{what}: route='kernels', but the kernels do not serve these tensors")
        return "framework"
    return route


# --------------------------------------------------------------------------------------------- the tables
def _tables_framework(text_ids, image_token_id, soi_token_id, n_vis, n_images):
    B, L = text_ids.shape
    N, dev = B * L, text_ids.device
    flat = text_ids.reshape(-1)
    at = torch.arange(N, device=dev)

    def ranked(hit, cap):
        """-> (the rank of each hit below ``cap`` or -1 [N], the flat position of the k-th hit or -1 [cap], the running
        count before each token [N])"""
        upto = hit.cumsum(0)
        rank = upto - 1
        placed = hit & (rank < cap)
        # (unplaced tokens all write the spare slot behind the table)
        pos = torch.full((cap + 1,), -1, dtype=torch.long, device=dev).scatter_(0, torch.where(placed, rank, cap), at)
        return torch.where(placed, rank, -1), pos[:cap], upto - hit.long()

    img_rank, img_pos, _ = ranked(flat == image_token_id, n_vis)
    is_soi = flat == soi_token_id
    _, soi_pos, before = ranked(is_soi, n_images)
    found = soi_pos >= 0
    if L:
        soi_row = torch.where(found, soi_pos // L, -1)
        soi_col = torch.where(found, soi_pos % L, -1)
        first = before.view(B, L)[:, 0]
    else:
        soi_row = soi_col = soi_pos
        first = torch.zeros(B, dtype=torch.long, device=dev)
    n_soi = is_soi.sum()
    row_first = torch.cat((first, n_soi[None])).clamp_max(n_images)
    counts = torch.stack(((flat == image_token_id).sum(), n_soi))
    i32 = lambda t: t.to(torch.int32)
    return i32(img_rank), i32(img_pos), i32(soi_row), i32(soi_col), i32(row_first), i32(counts)


def sequence_tables(text_ids, *, image_token_id, soi_token_id, n_vis, n_images, route=None):
    """text_ids [B, L] (long) -> ``SequenceTables``.  ``n_vis``: rows of the visual embeddings (image tokens beyond them
    keep their text embedding); ``n_images``: slots of the per-image tensors (``<soi>`` tokens beyond them are ignored by
    the image decoder's context; slots beyond the last ``<soi>`` are padding).  Host ints, no sync.  On the device: one
    launch of one workgroup (B L <= 2^22)."""
    if text_ids.dim() != 2 or text_ids.dtype != torch.long:
        raise ValueError("text_ids must be a [B, L] long tensor")
    n_vis, n_images = int(n_vis), int(n_images)
    B, L = text_ids.shape
    ok = lambda: text_ids.is_cuda and max(B * L, n_vis, n_images) <= (1 << 22)
    with torch.no_grad():
        if _route(route, ok, "sequence_tables") == "kernels":
            parts = _func().sequence_index(text_ids, image_token_id, soi_token_id, n_vis, n_images)
        else:
            parts = _tables_framework(text_ids, image_token_id, soi_token_id, n_vis, n_images)
    return SequenceTables(*parts, B, L, n_vis, n_images, int(image_token_id), int(soi_token_id))


def _check_tables(tables, text_ids, what, **want):
    if (tables.B, tables.L) != tuple(text_ids.shape) or tables.img_rank.device != text_ids.device:
        raise ValueError(f"{what}: tables were made for another text_ids")
    for k, v in want.items():
        if v is not None and getattr(tables, k) != v:
            raise ValueError(f"{what}: tables were made with {k} = {getattr(tables, k)}, the call has {v}")


# --------------------------------------------------------------------------------------------- the embeddings
def _embed_framework(text_embeds, text_ids, vis, soi_token, tables):
    B, L, C = text_embeds.shape
    text = text_embeds.reshape(B * L, C).to(vis.dtype)
    rank = tables.img_rank.long()
    out = text
    if vis.shape[0]:
        out = torch.where((rank >= 0)[:, None], vis[rank.clamp_min(0)], text)
    is_soi = (text_ids.reshape(-1) == tables.soi_token_id)[:, None]
    out = torch.where(is_soi, out + soi_token.reshape(1, C).to(vis.dtype), out)        # one add, one rounding, in T
    return out.view(B, L, C)


def assemble_mm_embeds(text_embeds, text_ids, vis_embed, soi_token, *, image_token_id, soi_token_id, validate=False,
                       tables=None, route=None):
    """Step 3 of ``_prepare_mm_embeds``: text_embeds [B, L, C], vis_embed [n_vis, C] (or [B_I, l, C]), soi_token [1, C]
    -> mm_embeds [B, L, C] in ``vis_embed``'s type: the k-th image token's row (row-major) is the k-th visual row, every
    other row the text embedding cast to that type, and ``soi_token`` is added to every ``<soi>`` row.

    ``validate=True`` makes the reference's assertion (as many image tokens as visual rows): the one sync, off by
    default.  Without it surplus image tokens keep their text embedding and surplus visual rows get a zero gradient.
    ``tables``: ``sequence_tables`` of this ``text_ids`` with ``n_vis`` = the visual rows, to share them with other
    calls; its ``n_images`` must be at least the number of ``<soi>`` tokens for ``soi_token``'s gradient to be whole
    (without ``tables`` it is B L)."""
    B, L, C = text_embeds.shape
    if tuple(text_ids.shape) != (B, L):
        raise ValueError(f"text_ids {list(text_ids.shape)} does not match text_embeds {list(text_embeds.shape)}")
    vis = vis_embed.reshape(-1, C)
    n_vis = vis.shape[0]
    if tables is None:
        tables = sequence_tables(text_ids, image_token_id=image_token_id, soi_token_id=soi_token_id, n_vis=n_vis,
                                 n_images=B * L, route=route)
    _check_tables(tables, text_ids, "assemble_mm_embeds", n_vis=n_vis, image_token_id=int(image_token_id),
                  soi_token_id=int(soi_token_id))
    if validate:
        found = int(tables.counts[0])
        if found != n_vis:
            raise AssertionError(f"assemble_mm_embeds: {found} image tokens in text_ids, {n_vis} rows in vis_embed")
    ok = lambda: (_func().sequence_supported(vis, soi_token) and text_embeds.device == vis.device
                  and text_embeds.dtype in (vis.dtype, torch.float32) and text_ids.device == vis.device
                  and soi_token.numel() == C and B * L <= (1 << 22) and n_vis <= (1 << 22))
    if _route(route, ok, "assemble_mm_embeds") == "kernels":
        return _func().SequenceEmbedFunction.apply(text_embeds, vis, soi_token, text_ids, tables.soi_token_id,
                                                   tables.img_rank, tables.img_pos, tables.soi_row, tables.soi_col,
                                                   tables.counts, tables.n_images)
    return _embed_framework(text_embeds, text_ids, vis, soi_token, tables)


# --------------------------------------------------------------------------------------------- the sin-cos table
_sincos = {}


def sincos_1d_table(seq_len, C, dtype, device):
    """The reference's 1-d sin-cos position table [seq_len, C] (models/utils/pos_embed.py, positions 0 .. seq_len - 1):
    frequencies 10000^(-k / (C / 2)), the sines in the first half of the channels and the cosines in the second, all of it
    in float32 on the host -- the same operations in the same precision, so the bits are the reference's -- then cast to
    ``dtype``.  Made once per (seq_len, C, dtype, device) and kept; ``mmfs_amd.invalidate_caches()`` drops it."""
    if C % 2:
        raise ValueError("sincos_1d_table: C must be even")
    key = (int(seq_len), int(C), dtype, str(torch.device(device)))
    hit = _sincos.get(key)
    if hit is not None and hit[0] == _levels.cache_epoch():
        return hit[1]
    half = C // 2
    freq = np.arange(half, dtype=np.float32)
    freq /= C / 2.
    freq = np.float32(1.) / np.power(np.float32(10000), freq)
    angle = np.arange(seq_len, dtype=np.float32)[:, None] * freq[None, :]
    host = np.concatenate([np.sin(angle), np.cos(angle)], axis=1)
    assert host.dtype == np.float32
    with torch.inference_mode(False), torch.no_grad():         # (the table outlives the call that made it: levels.py)
        table = torch.from_numpy(host).to(device=device, dtype=dtype)
    _sincos[key] = (_levels.cache_epoch(), table)
    return table


# --------------------------------------------------------------------------------------------- the image decoder's context
def _windows(tables, start_idx, bos_idx, L, cap):
    """-> (row, col, len) [n_images] long: the kernel's window_of (csrc/mmfs_sequence.hip)"""
    row = tables.soi_row.long()
    col = tables.soi_col.long() if start_idx is None else start_idx.long()
    bos = 0 if bos_idx is None else bos_idx.long().clamp_min(0)
    live = (row >= 0) & (col >= 0) & (col < L)
    length = torch.where(live, col - bos + 1, 0).clamp(0, cap)
    return row, col, length


def _gather_framework(src, pad_row, pos, tables, start_idx, bos_idx, max_len):
    B, L, C = src.shape
    n_images = tables.n_images
    row, col, length = _windows(tables, start_idx, bos_idx, L, max_len)
    j = torch.arange(max_len, device=src.device)
    mask = j[None, :] < length[:, None]
    if B * L:
        flat = (row.clamp_min(0) * L)[:, None] + (col[:, None] - j[None, :]).clamp(0, L - 1)
        rows = src.reshape(B * L, C)[flat]
    else:
        rows = src.new_zeros((n_images, max_len, C))
    pad = src.new_zeros(()) if pad_row is None else pad_row.to(src.dtype)
    out = torch.where(mask[..., None], rows, pad)
    if pos is not None:
        out = out + pos[:max_len].to(src.dtype)
    return out, mask.long()


def _gather(src, pad_row, pos, tables, start_idx, bos_idx, max_len, route, what):
    ok = lambda: (_func().sequence_supported(src, pad_row, pos) and tables.soi_row.device == src.device
                  and all(t is None or (t.device == src.device and t.dtype == torch.long) for t in (start_idx, bos_idx))
                  and (pos is None or (pos.shape[0] >= max_len and pos.shape[1] == src.shape[-1]))
                  and max(src.shape[0] * src.shape[1], tables.n_images, max_len) <= (1 << 22))
    if _route(route, ok, what) == "kernels":
        return _func().ContextGatherFunction.apply(src, pad_row, pos, tables.soi_row, tables.soi_col, tables.row_first,
                                                   start_idx, bos_idx, tables.n_images, max_len)
    return _gather_framework(src, pad_row, pos, tables, start_idx, bos_idx, max_len)


def prepare_context_features_for_image_decoder(context_features, text_ids, context_feat_proj, *, soi_token_id, n_images,
                                               seq_len, nearest_bos_idxs=None, image_start_token_idx=None, max_len=None,
                                               order="auto", tables=None, route=None):
    """``_prepare_context_features_for_image_decoder``: context_features [B, L, C], text_ids [B, L], ``context_feat_proj``
    a Linear (``weight`` [C_out, C], ``bias`` or None) -> (features [n_images, max_len, C_out], mask [n_images, max_len]
    long).  Image i is the i-th ``<soi>`` of ``text_ids`` (row-major); its context runs backwards from column
    ``image_start_token_idx[i]`` (default: the ``<soi>``'s own column) to ``nearest_bos_idxs[i]`` (default 0; both
    long tensors [n_images], negative ``<bos>`` entries count as 0), is
    projected, and gets the 1-d sin-cos table of ``seq_len`` positions added; behind it the row is ``bias + pos``.
    Slots beyond the last ``<soi>`` are padding throughout.

    ``max_len=None`` reads the longest context from the device: ONE sync (like ``max_num_image=None`` in ``bank.py``).
    A host int avoids it; contexts longer than ``max_len`` are then CUT at ``max_len`` (their nearest ``max_len``
    tokens remain), shorter ones are padded to it.
    ``order``: "project_first" projects the B L tokens once and gathers; "gather_first" gathers and projects the
    n_images max_len rows (the reference's order, for a batch with few images); "auto" takes project_first iff
    B L <= n_images max_len -- the row counts of the two products, host ints.
    The bias receives the padded rows' gradient through the gather; the weight and the real rows go through autograd's
    ``F.linear``.  The table is a constant."""
    B, L, C = context_features.shape
    if tuple(text_ids.shape) != (B, L):
        raise ValueError(f"text_ids {list(text_ids.shape)} does not match context_features {list(context_features.shape)}")
    n_images, seq_len = int(n_images), int(seq_len)
    if order not in ("auto", "project_first", "gather_first"):
        raise ValueError(f"order: {order!r}")
    if tables is None:
        tables = sequence_tables(text_ids, image_token_id=-1, soi_token_id=soi_token_id, n_vis=0, n_images=n_images,
                                 route=route)
    _check_tables(tables, text_ids, "prepare_context_features_for_image_decoder", n_images=n_images,
                  soi_token_id=int(soi_token_id))
    for name, t in (("nearest_bos_idxs", nearest_bos_idxs), ("image_start_token_idx", image_start_token_idx)):
        if t is not None and (t.dim() != 1 or t.shape[0] != n_images):
            raise ValueError(f"{name} must hold one entry per image slot: [{n_images}], not {list(t.shape)}")
    if max_len is None:
        with torch.no_grad():
            max_len = max(int(_windows(tables, image_start_token_idx, nearest_bos_idxs, L, L)[2].max()), 1) if n_images else 1
    max_len = int(max_len)
    if not 1 <= max_len <= seq_len:
        raise ValueError(f"max_len = {max_len} must lie in [1, seq_len = {seq_len}]")
    weight, bias = context_feat_proj.weight, getattr(context_feat_proj, "bias", None)
    what = "prepare_context_features_for_image_decoder"
    if order == "auto":
        order = "project_first" if B * L <= n_images * max_len else "gather_first"
    if order == "project_first":
        projected = F.linear(context_features, weight, bias)
        pos = sincos_1d_table(seq_len, projected.shape[-1], projected.dtype, projected.device)
        return _gather(projected, bias, pos, tables, image_start_token_idx, nearest_bos_idxs, max_len, route, what)
    rows, mask = _gather(context_features, None, None, tables, image_start_token_idx, nearest_bos_idxs, max_len, route, what)
    projected = F.linear(rows, weight, bias)
    pos = sincos_1d_table(seq_len, projected.shape[-1], projected.dtype, projected.device)
    return projected + pos[None, :max_len], mask
