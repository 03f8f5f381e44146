"""The LLM's self-attention in text generation: the reference's ``LlamaAttention``
(mm_interleaved/models/decoders/modeling_llama_mmfs.py:192-280) with its constructor, parameter names (``q_proj``,
``k_proj``, ``v_proj``, ``o_proj``) and forward signature, and a key / value cache that is written in place.

    cache = mmfs_amd.LlamaKVCache(num_layers, batch, heads, cap, 128, torch.bfloat16, device)
    for every generated token:
        for i, layer in enumerate(layers):
            out, _, present = layer.self_attn(h, attention_mask=mask, position_ids=pos, past_key_value=cache[i], use_cache=True)
        cache.advance()                      # once per step, after the last layer
        cache.reorder(beam_idx)              # beam search: in place of _reorder_cache's index_select of every layer

Two routes.  ``"kernels"``: ``past_key_value`` is a handle of a ``LlamaKVCache``; csrc/mmfs_llama_attn.hip rotates q and k,
appends k and v to the cache where it lies and, for a single new token, walks the keys once (no ``torch.cat``, no
[B, H, 1, T] tensor); more than one new token (the prefill into the cache) takes the append kernel and then the prefill
kernel (csrc/mmfs_llama_prefill.hip: tiled online softmax over the cache, the mask read where it lies, no [B, H, Lq, kv]
tensor) from ``PREFILL_KERNEL_MIN_TOKENS`` new tokens on, below it the reference's mathematics in framework ops on the
rotated q and the cache's views; ``module.prefill_kernel = True / False`` forces either, ``module.last_prefill`` says which
ran.  Returns the handle as the present.
``"framework"``: the reference's statement, tuple cache included -- host tensors, fp32, a tuple (or no) cache,
``use_cache=False``, ``output_attentions``, autocast, anything that requires grad, a mask that is not
[B or 1, 1, q_len or 1, kv_len].  The class is a drop-in with or without a ``LlamaKVCache``.  A call that is handed a cache
handle and takes the framework route all the same (``last_reason`` says why) reads the past from the handle's views, writes
its new keys and values INTO the cache with framework ops and returns the handle, so ``cache.advance()`` counts the token on
either route; a cache that cannot take them (another type, device or shape) raises.  Only ``use_cache=False`` appends nothing.
``module.route = "kernels"`` / ``"framework"`` forces either; a forced kernel route that does not apply raises.

Training.  A module in training mode that is handed a 2-D ``attention_mask`` [B, q_len] and no ``past_key_value`` -- the
convention of the reference's ``replace_llama_attn_with_flash_attn()``, whose ``_forward_train`` this is -- rotates q and k,
runs CAUSAL attention, does not read the mask, ignores ``use_cache`` and returns ``(o_proj(context), None, None)``.  Device
bf16 / fp16 tensors with heads of 128 channels outside autocast take csrc/mmfs_llama_train.hip forward and backward (no
[B, H, L, L] tensor, bit-reproducible) from ``TRAIN_KERNEL_MIN_TOKENS`` tokens on; anything else states the same with
framework ops, differentiable by autograd.  ``module.last_train`` says which ran.
"""
import warnings

import torch
from torch import nn

# which route device tensors with a cache handle take when nothing is forced, per shape class (profiles/llama_attn.md
# holds the measurement behind it)
DEFAULT_ROUTE = {"decode": "kernels", "prefill": "kernels"}
# on the kernel route, a prompt of at least this many new tokens takes the prefill kernel behind the append, a shorter one
# the framework ops on the cache's views (2: always; profiles/llama_attn.md holds the measurement behind it)
PREFILL_KERNEL_MIN_TOKENS = 2
# on the training route, a sequence of at least this many tokens takes the training kernels, a shorter one the framework ops
# (1: always -- at B = 4, H = 32, bf16 the kernels' forward + backward took 145 / 324 / 2754 us against the framework
# statement's 729 / 1074 / 10016 at L = 128 / 512 / 2048, more than both spreads apart at each: profiles/llama_attn.md, "Training")
TRAIN_KERNEL_MIN_TOKENS = 1


def _func():
    from .functions import llama_attn_func          # (loads the native library: host-only callers never need it)
    return llama_attn_func


def _train_func():
    from .functions import llama_train_func         # (loads the native library)
    return llama_train_func


def rope_table(head_dim, max_positions, base=10000, device=None):
    """(cos, sin) [max_positions, head_dim / 2] fp32 as the reference's FixedLlamaRotaryEmbedding computes them
    (functions/llama_attn_func.py)"""
    return _func().rope_table(head_dim, max_positions, base=base, device=device)


def rotate_half(x):
    """(x_lo, x_hi) -> (-x_hi, x_lo): the partner of channel i is channel i +- D / 2"""
    lo, hi = x.chunk(2, dim=-1)
    return torch.cat((hi.neg(), lo), dim=-1)


class LlamaKVLayer:
    """One layer of a ``LlamaKVCache``: what ``past_key_value`` is on the kernel route.  ``layer[0]`` / ``layer[1]`` are the
    reference's key / value tensors [B, H, len, D] (views of the cache while no beam reorder has happened, a gather
    through ``src_row`` afterwards), so code that reads ``past_key_values[0][0].shape[2]`` keeps working."""

    def __init__(self, cache, index):
        self.cache, self.index = cache, index
        self.pending = 0                    # tokens appended in this step and not yet counted by cache.advance()

    @property
    def keys(self):
        return self.cache.store[self.index, 0]

    @property
    def values(self):
        return self.cache.store[self.index, 1]

    def __len__(self):
        return 2

    def __iter__(self):
        return iter((self[0], self[1]))

    def __getitem__(self, which):
        if which not in (0, 1, -1, -2):
            raise IndexError(which)
        c = self.cache
        n = c.host_length + self.pending
        full = c.store[self.index, which % 2]
        if c.identity:
            return full[:, :, :n]
        rows = c.src_row[:, :n].long()[:, None, :]
        heads = torch.arange(c.heads, device=full.device)[None, :, None]
        at = torch.arange(n, device=full.device)[None, None, :]
        return full[rows, heads, at]


class LlamaKVCache:
    """The key / value cache of all layers in one allocation [layers, 2, B, H, cap, D], written in place.
    ``length`` (device int32 [1]): the tokens held, the same for every row, as in the reference's padded batch, with a
    host mirror ``host_length``; ``src_row`` (device int32 [B, cap]): the physical batch row that holds logical row b's
    token t.  ``cache[i]`` is layer i's handle."""

    def __init__(self, num_layers, batch, heads, cap, head_dim=128, dtype=torch.bfloat16, device=None):
        if min(num_layers, batch, heads, cap, head_dim) < 1:
            raise ValueError("LlamaKVCache: every size is at least 1")
        self.num_layers, self.batch, self.heads, self.cap, self.head_dim = num_layers, batch, heads, cap, head_dim
        self.store = torch.empty((num_layers, 2, batch, heads, cap, head_dim), dtype=dtype, device=device)
        self.length = torch.zeros(1, dtype=torch.int32, device=device)
        self.src_row = torch.empty((batch, cap), dtype=torch.int32, device=device)
        self.layers = [LlamaKVLayer(self, i) for i in range(num_layers)]
        self.reset()

    dtype = property(lambda self: self.store.dtype)
    device = property(lambda self: self.store.device)

    def __len__(self):
        return self.num_layers

    def __getitem__(self, i):
        return self.layers[i]

    def __iter__(self):
        return iter(self.layers)

    def reset(self):
        """Empty the cache: the length is 0 and every row holds its own tokens again (two fill kernels; the rows
        themselves are not touched -- nothing reads a slot at or behind the length)."""
        self.length.zero_()
        self.src_row.copy_(torch.arange(self.batch, dtype=torch.int32, device=self.src_row.device)[:, None].expand(-1, self.cap))
        self.host_length, self.identity = 0, True
        for layer in self.layers:
            layer.pending = 0

    def set_length(self, n):
        """The cache holds ``n`` tokens a row (filled elsewhere, or a step taken back): the device word and the mirror"""
        if not 0 <= n <= self.cap:
            raise RuntimeError(f"LlamaKVCache: a length of {n} is outside the capacity {self.cap}")
        self.length.fill_(n)
        self.host_length = n
        for layer in self.layers:
            layer.pending = 0

    def reserve(self, layer, n):
        """Layer ``layer`` is about to append ``n`` tokens: checked on the host, from the mirror."""
        if self.host_length + n > self.cap:
            raise RuntimeError(f"LlamaKVCache: {self.host_length} tokens held + {n} new ones exceed the capacity {self.cap}")
        layer.pending = n

    def append_rows(self, layer, keys, values):
        """What the append kernel does, in framework ops: ``keys`` (rotated) and ``values`` [B, H, L, D] go to slots
        length .. length + L of their own physical rows, from the host mirror.  The module's framework route calls it
        when it is handed a cache handle, so that the cache never misses a token whichever route a call takes."""
        want = (self.batch, self.heads, keys.shape[2], self.head_dim)
        if tuple(keys.shape) != want or tuple(values.shape) != want or keys.dtype != self.dtype or keys.device != self.device:
            raise RuntimeError(f"LlamaKVCache: rows of shape {tuple(keys.shape)}, {keys.dtype} on {keys.device} do not go into a "
                               f"cache of [{self.batch}, {self.heads}, cap, {self.head_dim}], {self.dtype} on {self.device}")
        n, count = self.host_length, keys.shape[2]
        self.reserve(layer, count)
        layer.keys[:, :, n:n + count] = keys.detach()
        layer.values[:, :, n:n + count] = values.detach()
        self.src_row[:, n:n + count] = torch.arange(self.batch, dtype=torch.int32, device=self.src_row.device)[:, None]

    def advance(self, n=None):
        """Once per step, after the last layer: the tokens the layers appended now count (an in-place add on the device,
        and the mirror).  ``n`` defaults to what the layers appended."""
        if n is None:
            n = max(layer.pending for layer in self.layers)
        if self.host_length + n > self.cap:
            raise RuntimeError(f"LlamaKVCache: advancing {self.host_length} by {n} exceeds the capacity {self.cap}")
        self.length.add_(n)
        self.host_length += n
        for layer in self.layers:
            layer.pending = 0

    def advance_host(self, n=1):
        """A replay of a captured step advanced the device word by ``n``; the mirror follows here."""
        if self.host_length + n > self.cap:
            raise RuntimeError(f"LlamaKVCache: advancing {self.host_length} by {n} exceeds the capacity {self.cap}")
        self.host_length += n

    def reorder(self, beam_idx):
        """Beam search: logical row b continues beam ``beam_idx[b]`` -- the rows of ``src_row`` (B * cap ints) are permuted
        in place of the reference's ``index_select`` of every layer's keys and values (:913-917)."""
        idx = beam_idx.to(device=self.src_row.device, dtype=torch.long)
        if idx.shape != (self.batch,):
            raise ValueError(f"LlamaKVCache.reorder: beam_idx has shape {tuple(idx.shape)}, not ({self.batch},)")
        self.src_row.copy_(self.src_row.index_select(0, idx))
        self.identity = False


class LlamaSelfAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        heads, hidden = config.num_attention_heads, config.hidden_size
        if hidden % heads != 0:
            raise ValueError(f"LlamaSelfAttention: {hidden} channels do not split into {heads} heads")
        self.config = config
        self.hidden_size, self.num_heads, self.head_dim = hidden, heads, hidden // heads
        self.max_position_embeddings = config.max_position_embeddings
        for name in ("q_proj", "k_proj", "v_proj", "o_proj"):               # the reference's parameter names; no biases
            setattr(self, name, nn.Linear(hidden, hidden, bias=False))
        # the rotary table, fp32, per device: not a buffer (module.to(dtype) would round it; the reference's buffers are
        # not persistent either, so the state dict is the four weights)
        self._tables = {}
        self.route = None                       # None: DEFAULT_ROUTE where the kernels apply
        self.last_route = None                  # what the last forward took (tests, tools)
        self.last_reason = None                 # why it was the framework route
        self.prefill_kernel = None              # None: PREFILL_KERNEL_MIN_TOKENS decides; True / False: the prefill kernel / framework ops
        self.last_prefill = None                # "kernel" / "framework ops": what the last prompt on the kernel route took
        self.last_train = None                  # "kernel" / "framework ops": what the last call on the training route took; else None

    def rope(self, device, positions=0):
        """(cos, sin) [>= positions, head_dim / 2] fp32 on ``device``; grown when a sequence is longer, as the reference's"""
        device = torch.device(device)
        need = max(int(positions), self.max_position_embeddings)
        got = self._tables.get(device)
        if got is None or got[0].shape[0] < need:
            got = rope_table(self.head_dim, need, device=device)
            self._tables[device] = got
        return got

    def _split(self, x):
        """[B, L, H D] -> [B, H, L, D] (a view)"""
        return x.unflatten(-1, (self.num_heads, self.head_dim)).transpose(1, 2)

    # ------------------------------------------------------------------------------------------ routing
    def _kernel_reason(self, hidden_states, q, mask, past_key_value, output_attentions, use_cache):
        """why this call cannot take the kernels, or None"""
        if not isinstance(past_key_value, LlamaKVLayer):
            return "no LlamaKVCache handle as past_key_value"
        if not use_cache:
            return "use_cache=False"
        if output_attentions:
            return "output_attentions"
        cache = past_key_value.cache
        if q.dim() != 3 or not q.is_cuda:
            return "host tensors"
        if torch.is_autocast_enabled():
            return "autocast"
        if torch.is_grad_enabled() and (hidden_states.requires_grad or any(p.requires_grad for p in self.parameters())):
            return "tensors that require grad"
        B, Lq, _ = q.shape
        if cache.dtype != q.dtype or cache.device != q.device or cache.batch != B or cache.heads != self.num_heads or \
                cache.head_dim != self.head_dim:
            return "a cache of another type, device or shape"
        if not _func().llama_attn_supported(q, self.num_heads, cache.cap):
            return "tensors the kernels do not serve"
        if mask is not None:
            kv = cache.host_length + Lq
            # a single token's mask may be wider than kv_len, up to the capacity (a static mask of a captured step): the
            # kernel reads the first length + 1 entries of a row.  A prompt's mask is exact: framework ops add it as it is
            wide = kv <= mask.shape[-1] <= cache.cap if Lq == 1 else mask.shape[-1] == kv
            if mask.dim() != 4 or mask.shape[0] not in (1, B) or mask.shape[1] != 1 or not wide or \
                    mask.shape[2] not in ((1,) if Lq == 1 else (1, Lq)) or mask.device != q.device:
                return "a mask that is not [B or 1, 1, q_len or 1, kv_len]"
        return None

    def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_value=None, output_attentions=False,
                use_cache=False):
        forced = self.route is not None
        if forced and self.route not in ("kernels", "framework"):
            raise ValueError(f"route: {self.route!r} is not 'kernels' or 'framework'")
        if not (self.prefill_kernel is None or isinstance(self.prefill_kernel, bool)):
            raise ValueError(f"prefill_kernel: {self.prefill_kernel!r} is not None, True or False")
        rows, q_len = hidden_states.shape[0], hidden_states.shape[1]
        q, k, v = self.q_proj(hidden_states), self.k_proj(hidden_states), self.v_proj(hidden_states)
        self.last_train = None
        if self.training and past_key_value is None and isinstance(attention_mask, torch.Tensor) and \
                tuple(attention_mask.shape) == (rows, q_len):
            return self._train(q, k, v, position_ids, output_attentions)
        reason = self._kernel_reason(hidden_states, q, attention_mask, past_key_value, output_attentions, use_cache)
        if reason is None and not forced and DEFAULT_ROUTE["decode" if q_len == 1 else "prefill"] != "kernels":
            reason = "the default route of this shape class"
        if self.route == "kernels" and reason is not None:
            raise RuntimeError(f"LlamaSelfAttention: route='kernels', but the call has {reason}")
        if position_ids is None:
            held = 0 if past_key_value is None else past_key_value[0].shape[2]
            position_ids = torch.arange(held, held + q_len, device=hidden_states.device)[None, :].expand(rows, -1)
        if reason is None and self.route != "framework":
            self.last_route, self.last_reason = "kernels", None
            return self._kernels(q, k, v, attention_mask, position_ids, past_key_value)
        self.last_route, self.last_reason = "framework", reason
        return self._framework(q, k, v, attention_mask, position_ids, past_key_value, output_attentions, use_cache)

    # ------------------------------------------------------------------------------------------ the training route
    def _train_reason(self, q):
        """why this training call cannot take the kernels, or None"""
        if q.dim() != 3 or not q.is_cuda:
            return "host tensors"
        if torch.is_autocast_enabled():
            return "autocast"
        if not _train_func().llama_attn_train_supported(q, self.num_heads):
            return "tensors the kernels do not serve"
        return None

    def _train(self, q, k, v, position_ids, output_attentions):
        """the reference's _forward_train: the mask is not read, the attention is causal, nothing is cached"""
        if output_attentions:
            warnings.warn("Output attentions is not supported for patched `LlamaAttention`, returning `None` instead.")
        rows, q_len, _ = q.shape
        reason = self._train_reason(q)
        if reason is None and self.route is None and q_len < TRAIN_KERNEL_MIN_TOKENS:
            reason = "fewer tokens than TRAIN_KERNEL_MIN_TOKENS"
        if self.route == "kernels" and reason is not None:
            raise RuntimeError(f"LlamaSelfAttention: route='kernels', but the call has {reason}")
        if position_ids is None:
            position_ids = torch.arange(q_len, device=q.device)[None, :].expand(rows, -1)
        if reason is None and self.route != "framework":
            self.last_route, self.last_reason, self.last_train = "kernels", None, "kernel"
            capturing = torch.cuda.is_current_stream_capturing()
            cos, sin = self.rope(q.device, 0 if capturing else q_len)
            context = _train_func().llama_attn_train(q, k, v, position_ids, cos, sin, self.num_heads)
            return self.o_proj(context), None, None
        self.last_route, self.last_reason, self.last_train = "framework", reason, "framework ops"
        cos, sin = (torch.cat((t, t), dim=-1).to(q.dtype)[position_ids].unsqueeze(1) for t in self.rope(q.device, q_len))
        query, keys = self._split(q), self._split(k)
        query = query * cos + rotate_half(query) * sin
        keys = keys * cos + rotate_half(keys) * sin
        context, _ = self._attend(query, keys, self._split(v), None, False, causal=True)
        return self.o_proj(context), None, None

    # ------------------------------------------------------------------------------------------ the kernel route
    def _kernels(self, q, k, v, mask, position_ids, layer):
        f = _func()
        cache = layer.cache
        q_len = q.shape[1]
        cache.reserve(layer, q_len)
        # the table covers every position the cache can hold, as the framework route's grows with the sequence (made before a
        # capture: building it is a host-to-device copy)
        capturing = torch.cuda.is_current_stream_capturing()
        cos, sin = self.rope(q.device, 0 if capturing else cache.cap)
        # (the unchecked entries: _kernel_reason has held the cache against q, and its tensors and the table are this package's own)
        q_rot = f._rope_append(q, k, v, position_ids, cos, sin, layer.keys, layer.values, cache.length, cache.src_row)
        if q_len == 1:
            bias = None if mask is None else mask.reshape(mask.shape[0], mask.shape[3])
            # the grid is cut from a host bound of the length: the capacity while a graph is being captured (the replays run
            # at later lengths), the mirror otherwise; the result does not depend on it
            bound = cache.cap if capturing else cache.host_length + 1
            context = f._attn_decode(q_rot, layer.keys, layer.values, cache.length, cache.src_row, bias, bound)
        elif q_len >= PREFILL_KERNEL_MIN_TOKENS if self.prefill_kernel is None else self.prefill_kernel:
            # the mask as it lies: [B or 1, 1, q_len or 1, kv_len], its strides read from the tensor
            context = f._attn_prefill(q_rot, layer.keys, layer.values, cache.length, cache.src_row, mask)
            self.last_prefill = "kernel"
        else:
            context = self._attend(self._split(q_rot), layer[0], layer[1], mask, False)[0]
            self.last_prefill = "framework ops"
        return self.o_proj(context), None, layer

    # ------------------------------------------------------------------------------------------ the framework route
    def _attend(self, query, keys, values, mask, want_weights, causal=False):
        """query [B, H, L, D] (rotated), keys / values [B, H, kv, D], mask broadcastable to [B, 1, L, kv] or None ->
        (context [B, L, H D], probabilities or None).  The reference's order of roundings: the query is scaled before the
        product, the sum with the mask is clamped at finfo.min, the softmax runs in fp32 (wider types keep theirs) and
        is rounded back before the second product.  ``causal``: key t > query j is filled with -Inf (the training route)."""
        scores = (query * self.head_dim ** -0.5) @ keys.transpose(-1, -2)
        if causal:
            future = torch.ones(scores.shape[-2:], dtype=torch.bool, device=scores.device).triu(1)
            scores = scores.masked_fill(future, float("-inf"))
        if mask is not None:
            scores = (scores + mask).clamp_min(torch.finfo(scores.dtype).min)
        probs = scores.softmax(dim=-1, dtype=torch.promote_types(scores.dtype, torch.float32)).to(query.dtype)
        context = (probs @ values).transpose(1, 2).flatten(2)
        return context, (probs if want_weights else None)

    def _framework(self, q, k, v, mask, position_ids, past, want_weights, use_cache):
        rows, q_len, _ = q.shape
        held = 0 if past is None else past[0].shape[2]
        total = held + q_len
        if mask is not None and tuple(mask.shape) != (rows, 1, q_len, total):
            raise ValueError(f"LlamaSelfAttention: the framework route takes a mask of shape {(rows, 1, q_len, total)}, "
                             f"not {tuple(mask.shape)}")
        # the whole table is indexed, not its first ``total`` rows: the same numbers for every position it serves, and a
        # position at or behind ``total`` is no out-of-range index on the device
        cos, sin = (torch.cat((t, t), dim=-1).to(q.dtype)[position_ids].unsqueeze(1) for t in self.rope(q.device, total))
        query, new_keys, new_values = self._split(q), self._split(k), self._split(v)
        query = query * cos + rotate_half(query) * sin
        new_keys = new_keys * cos + rotate_half(new_keys) * sin
        keys = new_keys if past is None else torch.cat((past[0], new_keys), dim=2)
        values = new_values if past is None else torch.cat((past[1], new_values), dim=2)
        present = None
        if use_cache and isinstance(past, LlamaKVLayer):
            past.cache.append_rows(past, new_keys, new_values)             # the cache holds the token on either route
            present = past
        elif use_cache:
            present = (keys, values)
        context, probs = self._attend(query, keys, values, mask, want_weights)
        return self.o_proj(context), probs, present
