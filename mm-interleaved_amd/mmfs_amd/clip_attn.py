"""The image encoder's self-attention: the reference's ``CLIPXAttention``
(mm_interleaved/models/encoders/vit_adapter/xattn.py:21-141) with its constructor, parameter names (``q_proj``, ``k_proj``,
``v_proj``, ``out_proj``) and forward signature, without xformers.

    mmfs_amd.convert_clip_visual_attn(clip_vision_model)      # every encoder layer's self_attn becomes a CLIPSelfAttention
    context = mmfs_amd.clip_attention(q, k, v, heads)          # the attention alone, q, k, v [B, L, H 64]

Two routes.  ``"kernels"``: csrc/mmfs_clip_attn.hip, forward and backward, no [B H, L, L] tensor, bit-reproducible, with or
without gradients (a checkpointed encoder with frozen weights included) -- device bf16 / fp16 tensors, heads of 64 channels,
outside autocast, no mask, dropout 0 (or eval mode), ``output_attentions=False``.  ``"framework"``: the reference's
mathematical statement, the Hugging Face statement it keeps as a comment (xattn.py:75-135: q scaled, ``bmm``, the masks added,
softmax, dropout, ``bmm``) -- host and fp32 tensors, autocast, any mask (``causal_attention_mask`` included: the reference's
pipeline never converts the text model), dropout in training, ``output_attentions=True`` (it returns the weights).
``module.route = "kernels"`` / ``"framework"`` forces either; a forced kernel route that does not apply raises with the reason.
``module.last_route`` / ``last_reason`` say what the last call took.
"""
import torch
from torch import nn

# which route a call that the kernels can serve takes when nothing is forced, per shape class: "L257" up to 257 tokens (224 px),
# "long" beyond (448 px: 1025).  profiles/clip_attn.md holds the measurement behind it.
DEFAULT_ROUTE = {"L257": "kernels", "long": "kernels"}
HEAD_DIM = 64


def _func():
    from .functions import clip_attn_func           # (loads the native library: host-only callers never need it)
    return clip_attn_func


def clip_attention(q, k, v, heads):
    """q, k, v [B, L, H 64] device tensors of bf16 or fp16 -> context [B, L, H 64] (functions/clip_attn_func.py)"""
    return _func().clip_attention(q, k, v, heads)


def shape_class(tokens):
    return "L257" if tokens <= 257 else "long"


class CLIPSelfAttention(nn.Module):
    def __init__(self, config, _adopt=None):
        super().__init__()
        self.config = config
        self.embed_dim = config.hidden_size
        self.num_heads = config.num_attention_heads
        self.head_dim = self.embed_dim // self.num_heads
        if self.head_dim * self.num_heads != self.embed_dim:
            raise ValueError(f"embed_dim must be divisible by num_heads (got `embed_dim`: {self.embed_dim} and `num_heads`:"
                             f" {self.num_heads}).")
        self.scale = self.head_dim ** -0.5
        self.dropout = config.attention_dropout
        for name in ("k_proj", "v_proj", "q_proj", "out_proj"):              # the reference's names and order; with biases
            setattr(self, name, nn.Linear(self.embed_dim, self.embed_dim) if _adopt is None else getattr(_adopt, name))
        self.route = None                       # None: DEFAULT_ROUTE where the kernels apply
        self.last_route = None                  # what the last forward took (tests, tools)
        self.last_reason = None                 # why it was the framework route

    @classmethod
    def adopt(cls, attn):
        """a CLIPSelfAttention around the four Linear modules of ``attn`` (a Hugging Face ``CLIPAttention``, a
        ``CLIPXAttention``): the modules themselves, so dtype, device, ``requires_grad`` and parameter identity are kept"""
        module = cls(attn.config, _adopt=attn)
        module.train(attn.training)
        return module

    # ------------------------------------------------------------------------------------------ routing
    def _kernel_reason(self, q, attention_mask, causal_attention_mask, output_attentions):
        """why this call cannot take the kernels, or None"""
        if output_attentions:
            return "output_attentions"
        if attention_mask is not None or causal_attention_mask is not None:
            return "a mask"
        if self.training and self.dropout != 0.0:
            return "dropout in training"
        if q.dim() != 3 or not q.is_cuda:
            return "host tensors"
        if torch.is_autocast_enabled():
            return "autocast"
        if self.head_dim != HEAD_DIM or not _func().clip_attn_supported(q, self.num_heads):
            return "tensors the kernels do not serve"
        return None

    def forward(self, hidden_states, attention_mask=None, causal_attention_mask=None, output_attentions=False, **kwargs):
        """Input shape: Batch x Time x Channel -> (out_proj(context), the weights [B, H, L, L] if asked for, else None)"""
        forced = self.route is not None
        if forced and self.route not in ("kernels", "framework"):
            raise ValueError(f"route: {self.route!r} is not 'kernels' or 'framework'")
        q, k, v = self.q_proj(hidden_states), self.k_proj(hidden_states), self.v_proj(hidden_states)
        reason = self._kernel_reason(q, attention_mask, causal_attention_mask, output_attentions)
        if reason is None and not forced and DEFAULT_ROUTE[shape_class(q.shape[1])] != "kernels":
            reason = "the default route of this shape class"
        if self.route == "kernels" and reason is not None:
            raise RuntimeError(f"CLIPSelfAttention: route='kernels', but the call has {reason}")
        if reason is None and self.route != "framework":
            self.last_route, self.last_reason = "kernels", None
            return self.out_proj(_func().clip_attention(q, k, v, self.num_heads)), None
        self.last_route, self.last_reason = "framework", reason
        context, weights = self._framework(q, k, v, attention_mask, causal_attention_mask, output_attentions)
        return self.out_proj(context), weights

    # ------------------------------------------------------------------------------------------ the framework route
    def _framework(self, q, k, v, attention_mask, causal_attention_mask, want_weights):
        """xattn.py:75-135: the query is scaled before the product, the causal mask and then the attention mask (each
        [B, 1, L, L]) are added, the softmax runs in the tensors' type, dropout acts on the weights"""
        bsz, tgt_len, _ = q.shape
        heads = lambda x: x.view(bsz, -1, self.num_heads, self.head_dim).transpose(1, 2).reshape(bsz * self.num_heads, -1, self.head_dim)
        query, keys, values = heads(q * self.scale), heads(k), heads(v)
        src_len = keys.size(1)
        weights = torch.bmm(query, keys.transpose(1, 2))
        for name, mask in (("causal attention mask", causal_attention_mask), ("attention mask", attention_mask)):
            if mask is None:
                continue
            if mask.size() != (bsz, 1, tgt_len, src_len):
                raise ValueError(f"The {name} should be of size {(bsz, 1, tgt_len, src_len)}, but is {tuple(mask.size())}")
            weights = (weights.view(bsz, self.num_heads, tgt_len, src_len) + mask).view(bsz * self.num_heads, tgt_len, src_len)
        weights = nn.functional.softmax(weights, dim=-1)
        shown = weights.view(bsz, self.num_heads, tgt_len, src_len) if want_weights else None
        probs = nn.functional.dropout(weights, p=self.dropout, training=self.training)
        context = torch.bmm(probs, values).view(bsz, self.num_heads, tgt_len, self.head_dim).transpose(1, 2)
        return context.reshape(bsz, tgt_len, self.embed_dim), shown


def convert_clip_visual_attn(model):
    """The reference's function (xattn.py:144-155): every ``model.vision_model.encoder.layers[i].self_attn`` becomes a
    ``CLIPSelfAttention`` that ADOPTS the layer's four Linear modules (nothing is copied).  A ``CLIPVisionModel`` of a
    transformers version that keeps the encoder on the model itself (no ``vision_model`` in between) is taken as it is.  -> model"""
    for layer in getattr(model, "vision_model", model).encoder.layers:
        layer.self_attn = CLIPSelfAttention.adopt(layer.self_attn)
    return model
