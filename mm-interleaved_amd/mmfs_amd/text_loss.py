"""The text loss at the end of the training step, without the transposed fp32 copy of the logits, without Python loops
over the batch and without device->host syncs: the reference's ``_prepare_gt_text_ids``
(mm_interleaved/models/mm_interleaved.py:342-406), the two statements that end ``MMInterleaved.forward`` (:449-476)

    text_logits = rearrange(text_logits, "b n c -> b c n").float()
    loss_txt = F.cross_entropy(text_logits[..., :-1].contiguous(), gt_text_ids.contiguous())

and the per-option scores of ``generate_scores`` (:726-737).

    labels = prepare_gt_text_ids(text_ids, attention_mask, bos_token_id=.., soi_token_id=.., image_token_id=..,
                                 pad_token_id=.., ignore_prompt_token_offset=.., ignore_noimage_cond_loss=..)
    loss = text_loss(text_logits, labels)                          # text_logits [B, L, V] as the text decoder returns it
    scores = option_scores(text_logits, options_ids, options_attn_masks, context_offset=..)

Row (b, first + j) of the logits is scored against ``labels[b, j]``; training is ``first=0`` with L - 1 labels.  Device
logits of f32 / f16 / bf16 run the gfx950 kernels of csrc/mmfs_text_loss.hip (``functions/text_loss_func.py``): one read
of the logits forward, one read and one write backward, fp32 arithmetic from the stored values.  Host tensors, autocast,
fp64 and whatever else the kernels refuse run the same statement with framework ops on the logits as they lie (the
labels are padded to [B, L] instead of the logits being permuted and sliced).  ``route="kernels"`` / ``"framework"``
forces either; a forced kernel route that does not apply raises.
"""
import torch
import torch.nn.functional as F

# which route device tensors take when the caller does not say (profiles/text_loss.md holds the measurement behind it:
# forward + backward at [2, 2048, 32003] and [8, 512, 32003], bf16 and f32, against this module's framework route and
# the reference's four lines)
DEFAULT_ROUTE = "kernels"

_NO_IGNORE = -(1 << 63)                 # an ``ignore_index`` no label equals: option_scores scores every token


def _func():
    from .functions import text_loss_func          # (loads the native library: host-only callers never need it)
    return text_loss_func


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


# --------------------------------------------------------------------------------------------- the labels
def _prompt_offsets(offset, B, L, device):
    """-> what ``gt[:, :offset] = -100`` covers, as a column bound: an int, or a long tensor [B, 1]"""
    if isinstance(offset, torch.Tensor):
        if offset.dim() != 1 or offset.shape[0] != B:
            raise ValueError(f"ignore_prompt_token_offset: {list(offset.shape)} entries for a batch of {B}")
        off = offset.to(device=device, dtype=torch.long)
    elif isinstance(offset, int):
        return offset if offset >= 0 else max(L + offset, 0)
    else:
        offset = [int(o) for o in offset]
        if len(offset) != B:
            raise ValueError(f"ignore_prompt_token_offset: {len(offset)} entries for a batch of {B}")
        off = torch.tensor(offset, dtype=torch.long, device=device)
    # (a negative bound of a slice counts from the end)
    return torch.where(off < 0, (off + L).clamp_min(0), off)[:, None]


def prepare_gt_text_ids(text_ids, attention_mask, *, bos_token_id, soi_token_id, image_token_id, pad_token_id,
                        ignore_prompt_token_offset=0, ignore_noimage_cond_loss=False, gt_text_ids=None):
    """``_prepare_gt_text_ids``: text_ids [B, L] long, attention_mask [B, L] -> labels [B, L - 1] long, -100 where a token
    is not scored.  Label j is token j + 1.  Not scored: the first ``ignore_prompt_token_offset`` tokens of a row (an int, a
    sequence of B ints, or a long device tensor [B] -- the form a captured graph can replay); with
    ``ignore_noimage_cond_loss`` (the reference's ``meta["dataset_name"] in dataset_to_ignore_noimage_cond_loss``) every
    token whose nearest ``<soi>`` to the left lies before its nearest ``<bos>`` or does not exist; padding, image and
    ``<bos>`` tokens; tokens whose attention mask is 0; an ``<soi>`` that directly follows a ``<bos>``.  As the reference
    writes it: the nearest ``<bos>`` of a row without one counts as column 0 while the nearest ``<soi>`` stays -1.
    ``gt_text_ids`` [B, L] given: its columns 1 .. L - 1, nothing else.  Framework ops on 16 bytes per token, no loop over
    the batch, no sync."""
    if gt_text_ids is not None:
        return gt_text_ids[..., 1:]
    if text_ids.dim() != 2:
        raise ValueError("text_ids must be a [B, L] tensor")
    B, L = text_ids.shape
    dev = text_ids.device
    col = torch.arange(L, device=dev)[None, :]
    ignored = col < _prompt_offsets(ignore_prompt_token_offset, B, L, dev)
    if ignore_noimage_cond_loss and L:
        minus = col.new_full((), -1)
        bos = torch.where(text_ids == bos_token_id, col, minus).cummax(dim=1).values.clamp(min=0)
        soi = torch.where(text_ids == soi_token_id, col, minus).cummax(dim=1).values
        ignored = ignored | (soi < bos) | (soi == -1)
    ids, before = text_ids[:, 1:], text_ids[:, :-1]
    ignored = ignored[:, 1:] | (ids == pad_token_id) | (ids == image_token_id) | (ids == bos_token_id)
    ignored = ignored | ((before == bos_token_id) & (ids == soi_token_id))
    if attention_mask is not None:
        ignored = ignored | (attention_mask[:, 1:] == 0)
    return ids.masked_fill(ignored, -100)


# --------------------------------------------------------------------------------------------- the loss
def _classes(labels, V, ignore_index):
    """-> (valid, out of range) [B, n] bool"""
    kept = labels != ignore_index
    inside = (labels >= 0) & (labels < V)
    return kept & inside, kept & ~inside


def _loss_framework(logits, labels, reduction, ignore_index, first):
    B, L, V = logits.shape
    n = labels.shape[1]
    valid, bad = _classes(labels, V, ignore_index)
    counts = torch.stack((valid.sum(), bad.sum())).to(torch.int32)
    # the labels grow to [B, L] (8 bytes a row) so that the logits stay where they are: rows outside the window are ignored
    full = labels.new_full((B, L), -100)
    full[:, first:first + n] = torch.where(valid, labels, -100)
    x = logits if logits.dtype == torch.float64 else logits.float()
    rows = F.cross_entropy(x.reshape(B * L, V), full.reshape(B * L), ignore_index=-100,
                           reduction="none" if reduction == "none" else reduction)
    if reduction == "none":
        rows = rows.view(B, L)[:, first:first + n]
    return rows, counts


def _loss_and_counts(text_logits, gt_text_ids, reduction, ignore_index, first, route, what):
    if text_logits.dim() != 3:
        raise ValueError(f"{what}: text_logits must be [B, L, V], not {list(text_logits.shape)}")
    B, L, V = text_logits.shape
    if gt_text_ids.dim() != 2 or gt_text_ids.shape[0] != B or gt_text_ids.dtype != torch.long:
        raise ValueError(f"{what}: labels must be a [B = {B}, n] long tensor, not {list(gt_text_ids.shape)} {gt_text_ids.dtype}")
    if gt_text_ids.device != text_logits.device:
        raise ValueError(f"{what}: labels on {gt_text_ids.device}, logits on {text_logits.device}")
    first, ignore_index, n = int(first), int(ignore_index), gt_text_ids.shape[1]
    if first < 0 or first + n > L:
        raise ValueError(f"{what}: rows first = {first} .. first + n = {first + n} do not lie in [0, L = {L}]")
    if reduction not in ("none", "sum", "mean"):
        raise ValueError(f"reduction: {reduction!r}")
    ok = lambda: _func().text_loss_supported(text_logits)
    if _route(route, ok, what) == "kernels":
        return _func().TextLossFunction.apply(text_logits, gt_text_ids, first, ignore_index, reduction)
    return _loss_framework(text_logits, gt_text_ids, reduction, ignore_index, first)


def text_loss(text_logits, gt_text_ids, *, reduction="mean", ignore_index=-100, first=0, validate=False, route=None):
    """The cross-entropy of text_logits [B, L, V] -- as the text decoder returns them: no transpose, no slice -- against
    gt_text_ids [B, n] long: row (b, first + j) is scored against gt_text_ids[b, j], first + n <= L.  Training is
    ``first=0`` with the L - 1 labels of ``prepare_gt_text_ids``.  fp32 arithmetic from the stored logits (fp64 logits:
    fp64), which is what ``.float()`` followed by ``F.cross_entropy`` computes.

    ``reduction``: "mean" -> a 0-dim fp32 tensor, the sum over the rows whose label is not ``ignore_index`` divided by
    their number, both on the device (no such row: NaN, with a zero gradient); "sum"; "none" -> [B, n] fp32 with 0 at
    ignored rows.  The gradient has the logits' type and shape; rows outside [first, first + n) and ignored rows are exact
    zeros.  A label outside [0, V) that is not ``ignore_index`` never reads outside its row: the row counts as ignored and
    a device counter records it; ``validate=True`` reads the counter -- the one sync, off by default -- and raises
    ``IndexError``."""
    out, counts = _loss_and_counts(text_logits, gt_text_ids, reduction, ignore_index, first, route, "text_loss")
    if validate:
        bad = int(counts[1])
        if bad:
            raise IndexError(f"text_loss: {bad} labels lie outside [0, {text_logits.shape[-1]}) and are not "
                             f"ignore_index = {ignore_index}")
    return out


def option_scores(text_logits, options_ids, options_attn_masks, *, context_offset, route=None):
    """``generate_scores``' score of each option (mm_interleaved.py:726-737): text_logits [n_options, L, V], options_ids and
    options_attn_masks [n_options, n]; token j of an option is predicted by row context_offset - 1 + j.
    -> (log_softmax(text_logits[:, context_offset - 1 : context_offset - 1 + n]).gather(options_ids) * mask).sum(-1),
    [n_options] -- the negative of ``text_loss(reduction="none", first=context_offset - 1)`` with no label ignored, masked
    and summed.  No gradient."""
    with torch.no_grad():
        rows, _ = _loss_and_counts(text_logits, options_ids, "none", _NO_IGNORE, int(context_offset) - 1, route,
                                   "option_scores")
        return (-rows * options_attn_masks).sum(dim=-1)
