"""mmfs_amd -- host-side mirror of the reference's MMFS operator interface, backed
by the hand-written gfx950 kernels of libmmfs_msda.so.

Layout mirrors mm_interleaved/models/utils/ops/ of the reference:
    mmfs_amd.functions   MSDeformAttnFunction, ms_deform_attn_core_pytorch
    mmfs_amd.modules     MMFS, MSDeformAttn
and the callers either side of the op:
    mmfs_amd.blocks      LlamaMMFSAttention, MMFSBlock, MMFSNet; the image encoder's ViT-Adapter blocks
                         (Injector, Extractor, InteractionBlock, InteractionBlockWithCls, deform_inputs)
    mmfs_amd.bank        feature-bank builders + the RCCL all-gather of image features
    mmfs_amd.sequence    the interleaved sequence: embeddings with the visual rows and <soi> in place, the image decoder's
                         per-image context, the special-token tables both read
    mmfs_amd.text_loss   the end of the training step: the labels, the cross-entropy of the text decoder's 16-bit logits and
                         its gradient in three passes over the logits, the per-option scores (the package attribute
                         ``text_loss`` is the function; ``from mmfs_amd.text_loss import ..`` reaches the module)
    mmfs_amd.resampler   QKNormAttention: the Perceiver resampler's Q-Former attention with per-head q/k LayerNorm, fused
    mmfs_amd.llama_attn  LlamaSelfAttention, LlamaKVCache: the LLM's self-attention in text generation -- rotary embedding,
                         a key / value cache written in place (re-indexed, not copied, under beam search), prompt and single-token
                         attention over it; in training, causal attention forward and backward with no L x L tensor
                         (``llama_attn_train``, the module's training route)
    mmfs_amd.clip_attn   CLIPSelfAttention, convert_clip_visual_attn, clip_attention: the image encoder's (CLIP ViT) self-attention,
                         heads of 64 channels, forward and backward with no L x L tensor
"""
from .functions import MSDeformAttnFunction, ms_deform_attn_core_pytorch  # noqa: F401
from .functions import QKNormAttentionFunction, qk_attn_supported  # noqa: F401
from .functions import llama_attn_decode, llama_attn_prefill, llama_attn_supported, llama_rope_append, rope_table  # noqa: F401
from .functions import LlamaAttnTrainFunction, llama_attn_train, llama_attn_train_supported  # noqa: F401
from .functions import ClipAttentionFunction, clip_attn_supported  # noqa: F401
from .clip_attn import CLIPSelfAttention, clip_attention, convert_clip_visual_attn  # noqa: F401
from .levels import invalidate_caches  # noqa: F401
from .llama_attn import LlamaKVCache, LlamaKVLayer, LlamaSelfAttention  # noqa: F401
from .resampler import QKNormAttention  # noqa: F401
from .sequence import (SequenceTables, assemble_mm_embeds, prepare_context_features_for_image_decoder,  # noqa: F401
                       sequence_tables, sincos_1d_table)
from .text_loss import option_scores, prepare_gt_text_ids, text_loss  # noqa: F401

__version__ = "0.1.0"
