"""The LLM's self-attention in generation on the device (csrc/mmfs_llama_attn.hip, csrc/mmfs_llama_prefill.hip; C ABI
``mmfs_llama_attn_*`` in include/mmfs_msda.h): the rotary embedding and the in-place append to a key / value cache in one
launch, the single-token attention over that cache in two (the split walk of the keys, the merge of its partials), and a
prompt's attention over it in one (tiled online softmax, the mask read where it lies).  Inference only:
nothing here is differentiable.  Nothing reads a value back from the device: a step can be captured into a graph.

``mmfs_amd.llama_attn`` holds the cache (``LlamaKVCache``) and the module (``LlamaSelfAttention``) built on these.
"""
import torch

import MultiScaleDeformableAttention as MSDA

_lib = MSDA._lib
_CODE = MSDA._DTYPE_CODE
HEAD_DIM = 128
# how the decode kernel cuts the keys: a wave's, a workgroup's (= a split's): where its paths change
WAVE_KEYS, SPLIT_KEYS = int(_lib.mmfs_llama_attn_decode_keys(0)), int(_lib.mmfs_llama_attn_decode_keys(1))
# how the prefill kernel cuts its work: the query rows of a wave, of a workgroup, the keys of a tile
PREFILL_TILES = MSDA._tiles("mmfs_llama_attn_prefill_tiles", 3)
PREFILL_CAUSAL, PREFILL_VISIT_ALL = 1, 2                # MMFS_LLAMA_PREFILL_*

# kernel launches since import, for tests and tools that ask which route the module took
launches = {"append": 0, "decode": 0, "prefill": 0}


def rope_table(head_dim, max_positions, base=10000, device=None):
    """(cos, sin) [max_positions, head_dim / 2] fp32, computed as the reference's FixedLlamaRotaryEmbedding computes its
    cache (modeling_llama_mmfs.py:126-141): an fp32 ``arange`` times the fp32 ``inv_freq``, on the host, then moved.  The
    reference keeps both halves of ``cat((freqs, freqs))``; they are equal, so one is kept here."""
    inv_freq = 1.0 / (base ** (torch.arange(0, head_dim, 2).float() / head_dim))
    freqs = torch.outer(torch.arange(max_positions, dtype=torch.float32), inv_freq)
    cos, sin = freqs.cos(), freqs.sin()
    if device is not None:
        cos, sin = cos.to(device), sin.to(device)
    return cos.contiguous(), sin.contiguous()


def llama_attn_supported(q, heads, cap):
    """The kernels apply: a device tensor q [B, Lq, H 128] of bf16 or fp16, 1 <= Lq <= cap, outside autocast."""
    return MSDA._attn_supported(q, heads, "mmfs_llama_attn_supported", cap)


_require, _plain = MSDA._require, MSDA._plain


def _check_cache(q, keys, values, length, src_row, what):
    """the cache tensors as the kernels address them: a wrong one would be read out of bounds on the device, so it raises here"""
    dev, dt = q.device, q.dtype
    _require(q.is_cuda and q.dim() == 3 and dt in (torch.float16, torch.bfloat16), f"{what}: q must be a device tensor [B, Lq, H 128] "
             "of bf16 or fp16")
    _require(keys.dim() == 4 and keys.shape == values.shape and keys.shape[0] == q.shape[0] and keys.shape[3] == HEAD_DIM
             and keys.shape[1] * HEAD_DIM == q.shape[2], f"{what}: keys and values must be [B, H, cap, 128] for q {tuple(q.shape)}")
    for name, t in (("keys", keys), ("values", values)):
        _require(t.dtype == dt and t.device == dev and t.is_contiguous(), f"{what}: {name} must be contiguous, of q's type, on q's device")
    _require(length.dtype == torch.int32 and length.device == dev and length.numel() == 1, f"{what}: length must be one int32 on q's device")
    _require(src_row.dtype == torch.int32 and src_row.device == dev and src_row.is_contiguous()
             and tuple(src_row.shape) == (keys.shape[0], keys.shape[2]), f"{what}: src_row must be contiguous int32 [B, cap] on q's device")


def _bias_args(bias, dev, dt):
    """a mask as the kernels read it -> (tensor or None, dtype code, strides of the axes before the keys, keys): of fp32 or
    of the inputs' type where it lies (anything else is cast to fp32), HF's 4-d mask without its head axis, the keys one
    element apart and aligned to an element (else copied); an axis of length 1 has stride 0.  At least 2-d: the prefill
    takes the batch and the query stride, the decode the batch stride alone."""
    if bias is None:
        return None, 0, (0, 0), 0
    t = bias.detach()
    if t.dim() == 4:
        t = t[:, 0]
    if t.dtype not in (torch.float32, dt) or t.device != dev:
        t = t.to(device=dev, dtype=torch.float32)
    if t.stride(-1) != 1 or t.data_ptr() % t.element_size():
        t = t.clone(memory_format=torch.contiguous_format)
    strides = tuple(0 if n == 1 else s for n, s in zip(t.shape[:-1], t.stride()[:-1]))
    return t, _CODE[t.dtype], strides, t.shape[-1]


def llama_rope_append(q, k, v, position_ids, cos, sin, keys, values, length, src_row):
    """q, k, v [B, Lq, H 128] as the Linear layers return them, position_ids [B, Lq] int64, (cos, sin) of ``rope_table``
    on the device; keys, values [B, H, cap, 128]: one layer of a cache, ``length`` [1] and ``src_row`` [B, cap] int32.
    -> q_rot [B, Lq, H 128]; the rotated k and v are written at slots length + j and src_row there.  The caller has
    checked length + Lq <= cap on the host."""
    _check_cache(q, keys, values, length, src_row, "llama_rope_append")
    dev, dt = q.device, q.dtype
    B, Lq, _ = q.shape
    _require(k.shape == q.shape and v.shape == q.shape and k.dtype == dt and v.dtype == dt and k.device == dev and v.device == dev,
             "llama_rope_append: k and v must have q's shape, type and device")
    for name, t in (("cos", cos), ("sin", sin)):
        _require(t.dtype == torch.float32 and t.device == dev and t.is_contiguous() and t.dim() == 2 and t.shape[1] == HEAD_DIM // 2
                 and t.shape == cos.shape, f"llama_rope_append: {name} must be contiguous fp32 [max_pos, 64] on q's device (rope_table)")
    _require(position_ids.numel() in (Lq, B * Lq), "llama_rope_append: position_ids must be [B, Lq] (or [1, Lq])")
    return _rope_append(q, k, v, position_ids, cos, sin, keys, values, length, src_row)


def _rope_append(q, k, v, position_ids, cos, sin, keys, values, length, src_row):
    """``llama_rope_append`` without its argument checks: what LlamaSelfAttention calls with a LlamaKVCache's own tensors"""
    dev, dt = q.device, q.dtype
    B, Lq, C = q.shape
    H, cap = keys.shape[1], keys.shape[2]
    q, k, v = _plain(q), _plain(k), _plain(v)
    pos = position_ids.detach()
    if pos.dtype != torch.int64 or pos.device != dev or not pos.is_contiguous() or tuple(pos.shape) != (B, Lq):
        pos = pos.to(device=dev, dtype=torch.int64).expand(B, Lq).contiguous()
    q_rot = torch.empty((B, Lq, C), dtype=dt, device=dev)
    MSDA._call("llama_rope_append", "mmfs_llama_attn_rope_append", dev, _CODE[dt], q.data_ptr(), k.data_ptr(), v.data_ptr(),
               pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), cos.shape[0], length.data_ptr(), q_rot.data_ptr(),
               keys.data_ptr(), values.data_ptr(), src_row.data_ptr(), B, Lq, H, C // H, cap)
    launches["append"] += 1
    return q_rot


def llama_attn_decode(q_rot, keys, values, length, src_row, bias=None, kv_bound=None):
    """q_rot [B, 1, H 128] -> context [B, 1, H 128]: softmax over the keys t < length + 1 of
    q_rot . keys[src_row[b, t], h, t] / sqrt(128) + bias[b, t], times the values.  ``bias`` [B or 1, kv_len] of fp32 or of
    the inputs' type, read where it lies.  ``kv_bound``: a host upper bound of length + 1 (default: the capacity; the grid
    is cut from it, the result does not depend on it)."""
    _check_cache(q_rot, keys, values, length, src_row, "llama_attn_decode")
    B, Lq, C = q_rot.shape
    _require(Lq == 1, "llama_attn_decode: one new token a row (q_rot [B, 1, H 128])")
    _require(bias is None or (bias.dim() == 2 and bias.shape[0] in (1, B)), "llama_attn_decode: bias must be [B or 1, kv_len]")
    return _attn_decode(q_rot, keys, values, length, src_row, bias, kv_bound)


def _attn_decode(q_rot, keys, values, length, src_row, bias=None, kv_bound=None):
    """``llama_attn_decode`` without its argument checks (see ``_rope_append``)"""
    dev, dt = q_rot.device, q_rot.dtype
    B, _, C = q_rot.shape
    H, cap = keys.shape[1], keys.shape[2]
    kv_bound = cap if kv_bound is None else int(kv_bound)
    q_rot = _plain(q_rot)
    bias_t, code, (stride, *_), blen = _bias_args(bias, dev, dt)
    out = torch.empty((B, 1, C), dtype=dt, device=dev)
    # the partials of the split walk (the caching allocator's, like ``out``: no device allocation in a steady loop)
    ws = torch.empty(max(_lib.mmfs_llama_attn_decode_workspace_bytes(B, H, kv_bound) // 4, 1), dtype=torch.float32, device=dev)
    MSDA._call("llama_attn_decode", "mmfs_llama_attn_decode", dev, _CODE[dt], q_rot.data_ptr(), keys.data_ptr(),
               values.data_ptr(), src_row.data_ptr(), length.data_ptr(), MSDA._ptr(bias_t), code, stride, blen,
               out.data_ptr(), ws.data_ptr(), B, H, C // H, cap, kv_bound)
    launches["decode"] += 2
    return out


def llama_attn_prefill(q_rot, keys, values, length, src_row, bias=None, causal=False):
    """q_rot [B, Lq, H 128] (what ``llama_rope_append`` returned; its keys and values are in the cache) -> context
    [B, Lq, H 128]: softmax over the keys t < length + Lq of q_rot[b, j] . keys[src_row[b, t], h, t] / sqrt(128) +
    bias[b, j, t], times the values.  ``bias`` [B or 1, 1 or Lq, kv] or HF's 4-d mask [B or 1, 1, 1 or Lq, kv], of fp32 or
    of the inputs' type, read where it lies through its strides (an expanded view costs nothing).  ``causal``: key t is
    excluded for query j iff t > length + j, on top of the bias.  A key at or below finfo.min, or excluded, scores
    finfo.min: rows whose keys are all masked are the mean of the values, also where HF's mask holds -Inf."""
    _check_cache(q_rot, keys, values, length, src_row, "llama_attn_prefill")
    B, Lq, _ = q_rot.shape
    _require(1 <= Lq <= keys.shape[2], "llama_attn_prefill: 1 <= Lq <= the capacity")
    if bias is not None:
        _require(isinstance(bias, torch.Tensor) and bias.dim() in (3, 4) and (bias.dim() == 3 or bias.shape[1] == 1)
                 and bias.shape[0] in (1, B) and bias.shape[-2] in (1, Lq) and bias.shape[-1] <= keys.shape[2],
                 "llama_attn_prefill: bias must be [B or 1, 1 or Lq, kv] or [B or 1, 1, 1 or Lq, kv], kv within the capacity")
    return _attn_prefill(q_rot, keys, values, length, src_row, bias, causal)


def _attn_prefill(q_rot, keys, values, length, src_row, bias=None, causal=False, visit_all=False):
    """``llama_attn_prefill`` without its argument checks (see ``_rope_append``); ``visit_all``: no key tile is skipped"""
    dev, dt = q_rot.device, q_rot.dtype
    B, Lq, C = q_rot.shape
    H, cap = keys.shape[1], keys.shape[2]
    q_rot = _plain(q_rot)
    bias_t, code, (batch_stride, query_stride), blen = _bias_args(bias, dev, dt)
    flags = (PREFILL_CAUSAL if causal else 0) | (PREFILL_VISIT_ALL if visit_all else 0)
    out = torch.empty((B, Lq, C), dtype=dt, device=dev)
    MSDA._call("llama_attn_prefill", "mmfs_llama_attn_prefill", dev, _CODE[dt], q_rot.data_ptr(), keys.data_ptr(),
               values.data_ptr(), src_row.data_ptr(), length.data_ptr(), MSDA._ptr(bias_t), code, batch_stride, query_stride,
               blen, flags, out.data_ptr(), B, Lq, H, C // H, cap)
    launches["prefill"] += 1
    return out
