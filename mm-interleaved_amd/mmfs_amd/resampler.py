"""The attention of the Perceiver resampler's Q-Former with a LayerNorm over the channels of every head of q and of k
(DESIGN.md 4.16): the class the reference patches over ``Blip2QFormerMultiHeadAttention``
(mm_interleaved/models/utils/monkey_patch/blip2_qknorm_monkey_patch.py), with its constructor, parameter names
(``query``, ``key``, ``value``, ``q_norm``, ``k_norm``) and forward signature, so that the reference's one-line patch can
install it and its checkpoints load:

    import transformers.models.blip_2.modeling_blip_2 as blip2
    blip2.Blip2QFormerMultiHeadAttention = mmfs_amd.QKNormAttention

Two routes.  ``"kernels"``: the three Linear layers, then csrc/mmfs_attn.hip on their outputs as they lie (no permuted
views, no [B, H, Nq, Nk] tensor); returns ``(context, None)`` -- there is no permuted key / value pair to hand on.
``"framework"``: the reference's mathematics in framework ops, returning its full tuple
``(context[, attention_probs], (key_layer, value_layer))``.  The framework route is taken on host tensors, under
autocast, on what ``qk_attn_supported`` refuses (fp32 storage, another head width, more than 128 queries or 8192 keys),
and whenever the call asks for something the kernels do not compute: ``head_mask``, ``past_key_value``,
``output_attentions``, ``save_attention`` on a cross-attention call (the reference saves the map only there: a
self-attention call ignores the flag and stays fused), relative position embeddings, a mask that is not one bias per key
(a 3-D mask, a 4-D mask that varies per query or per head), dropout above 0 in training mode.
``module.route = "kernels"`` / ``"framework"`` forces either; a forced kernel route that does not apply raises.
"""
import math

import torch
from torch import nn

# which route device tensors take when nothing is forced, per shape class (profiles/qk_attn.md holds the measurement
# behind it: each class against the framework route and against LayerNorm + F.scaled_dot_product_attention)
DEFAULT_ROUTE = {"self": "kernels", "cross": "kernels", "cross_long": "kernels"}
LONG_KEYS = 1024                       # "cross_long": cross-attention over at least this many keys


def _func():
    from .functions import qk_attn_func            # (loads the native library: host-only callers never need it)
    return qk_attn_func


class QKNormAttention(nn.Module):
    def __init__(self, config, is_cross_attention=False):
        super().__init__()
        self.config = config
        heads, hidden = config.num_attention_heads, config.hidden_size
        if hidden % heads != 0 and not hasattr(config, "embedding_size"):
            raise ValueError(f"The hidden size ({hidden}) is not a multiple of the number of attention heads ({heads})")
        self.num_attention_heads = heads
        self.attention_head_size = hidden // heads
        self.all_head_size = heads * self.attention_head_size
        source = config.encoder_hidden_size if is_cross_attention else hidden
        self.query = nn.Linear(hidden, self.all_head_size)
        self.key = nn.Linear(source, self.all_head_size)
        self.value = nn.Linear(source, self.all_head_size)
        self.dropout = nn.Dropout(config.attention_probs_dropout_prob)
        self.position_embedding_type = getattr(config, "position_embedding_type", "absolute")
        if self.position_embedding_type in ("relative_key", "relative_key_query"):
            self.max_position_embeddings = config.max_position_embeddings
            self.distance_embedding = nn.Embedding(2 * config.max_position_embeddings - 1, self.attention_head_size)
        self.save_attention = False
        width = self.attention_head_size
        normed = bool(config.qk_normalization)
        self.q_norm = nn.LayerNorm(width, eps=config.layer_norm_eps) if normed else nn.Identity()
        self.k_norm = nn.LayerNorm(width, eps=config.layer_norm_eps) if normed else nn.Identity()
        self.route = None                       # None: DEFAULT_ROUTE where the kernels apply
        self.last_route = None                  # what the last forward took (tests, tools)

    # the reference's hooks for attention maps
    def save_attn_gradients(self, attn_gradients):
        self.attn_gradients = attn_gradients

    def get_attn_gradients(self):
        return self.attn_gradients

    def save_attention_map(self, attention_map):
        self.attention_map = attention_map

    def get_attention_map(self):
        return self.attention_map

    def transpose_for_scores(self, x):
        return x.unflatten(-1, (self.num_attention_heads, self.attention_head_size)).transpose(1, 2)

    # ------------------------------------------------------------------------------------------ routing
    def _key_bias(self, mask, B, Nk):
        """HF's extended mask as one additive bias per key: -> (serves, bias [B, Nk] or None)"""
        if mask is None:
            return True, None
        if mask.dim() != 4 or mask.shape[1] != 1 or mask.shape[2] != 1 or mask.shape[3] != Nk or mask.shape[0] not in (1, B):
            return False, None
        return True, mask.reshape(mask.shape[0], Nk).expand(B, Nk)

    def _fused_reason(self, head_mask, past_key_value, output_attentions, cross):
        """why this call cannot be fused, or None"""
        if head_mask is not None:
            return "head_mask"
        if past_key_value is not None:
            return "past_key_value"
        if output_attentions:
            return "output_attentions"
        if cross and self.save_attention:
            return "save_attention"
        if self.position_embedding_type in ("relative_key", "relative_key_query"):
            return "relative position embeddings"
        if self.training and self.dropout.p > 0:
            return "dropout in training mode"
        return None

    def forward(self, hidden_states, attention_mask=None, head_mask=None, encoder_hidden_states=None,
                encoder_attention_mask=None, past_key_value=None, output_attentions=False):
        cross = encoder_hidden_states is not None
        source = encoder_hidden_states if cross else hidden_states
        mask = encoder_attention_mask if cross else attention_mask
        forced = self.route is not None
        if forced and self.route not in ("kernels", "framework"):
            raise ValueError(f"route: {self.route!r} is not 'kernels' or 'framework'")
        q, k, v = self.query(hidden_states), self.key(source), self.value(source)
        reason = self._fused_reason(head_mask, past_key_value, output_attentions, cross)
        bias = None
        if reason is None and not (q.dim() == 3 and k.dim() == 3):
            reason = "inputs that are not [B, N, C]"
        if reason is None:
            ok, bias = self._key_bias(mask, q.shape[0], k.shape[1])
            if not ok:
                reason = "a mask that is not one bias per key"
        if reason is None and not (q.is_cuda and _func().qk_attn_supported(q, k, v, self.num_attention_heads, bias)):
            reason = "tensors the kernels do not serve"
        if reason is None and not forced:
            kind = ("cross_long" if k.shape[1] >= LONG_KEYS else "cross") if cross else "self"
            if DEFAULT_ROUTE[kind] != "kernels":
                reason = "the default route of this shape class"
        if self.route == "kernels" and reason is not None:
            raise RuntimeError(f"QKNormAttention: route='kernels', but the call has {reason}")
        if reason is None and self.route != "framework":
            self.last_route = "kernels"
            normed = isinstance(self.q_norm, nn.LayerNorm)
            params = (self.q_norm.weight, self.q_norm.bias, self.k_norm.weight, self.k_norm.bias) if normed else (None,) * 4
            eps = self.q_norm.eps if normed else 0.0
            context, _ = _func().QKNormAttentionFunction.apply(q, k, v, *params, eps, bias, self.num_attention_heads)
            return (context, None)
        self.last_route = "framework"
        return self._framework(hidden_states, q, k, v, mask, head_mask, cross, past_key_value, output_attentions)

    # ------------------------------------------------------------------------------------------ the framework route
    def _framework(self, hidden_states, q, k, v, mask, head_mask, cross, past_key_value, output_attentions):
        key_layer = self.k_norm(self.transpose_for_scores(k))
        value_layer = self.transpose_for_scores(v)
        if not cross and past_key_value is not None:
            key_layer = torch.cat((past_key_value[0], key_layer), dim=2)
            value_layer = torch.cat((past_key_value[1], value_layer), dim=2)
        query_layer = self.q_norm(self.transpose_for_scores(q))
        scores = query_layer @ key_layer.transpose(-1, -2)
        if self.position_embedding_type in ("relative_key", "relative_key_query"):
            n = hidden_states.shape[1]
            at = torch.arange(n, dtype=torch.long, device=hidden_states.device)
            table = self.distance_embedding(at[:, None] - at[None, :] + self.max_position_embeddings - 1).to(query_layer.dtype)
            scores = scores + torch.einsum("bhld,lrd->bhlr", query_layer, table)
            if self.position_embedding_type == "relative_key_query":
                scores = scores + torch.einsum("bhrd,lrd->bhlr", key_layer, table)
        scores = scores / math.sqrt(self.attention_head_size)
        if mask is not None and scores.dtype in (torch.bfloat16, torch.float16):
            # A 16-bit sum would round score + bias to the bias's grid (a grid of 1 at a bias of 150 in bf16) and lose the
            # score: the bias is added and the softmax taken in fp32, and the weights are rounded to T once.  With HF's masks
            # (0 and finfo(T).min) these are the sum in T's own bits: score + 0 is the score, and a key at or below
            # finfo(T).min keeps the mask entry as its score, which is what the sum in T leaves of it and the kernels' rule
            # (csrc/mmfs_attn_core.h, score_of).
            # (The masked branch adds score - score.detach(), an exact 0: the gradient passes through a masked key's
            # score as it does through the sum in T.)
            wide, s32 = mask.float(), scores.float()
            scores = torch.where(wide <= torch.finfo(scores.dtype).min, wide + (s32 - s32.detach()), s32 + wide)
            probs = scores.softmax(dim=-1).to(query_layer.dtype)
        else:
            if mask is not None:
                scores = scores + mask
            probs = scores.softmax(dim=-1)
        if cross and self.save_attention:
            self.save_attention_map(probs)
            probs.register_hook(self.save_attn_gradients)
        dropped = self.dropout(probs)
        if head_mask is not None:
            dropped = dropped * head_mask
        context = (dropped @ value_layer).transpose(1, 2).flatten(2)
        outputs = (context, probs) if output_attentions else (context,)
        return outputs + ((key_layer, value_layer),)
