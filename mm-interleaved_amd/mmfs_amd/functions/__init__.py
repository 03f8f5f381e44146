# mirrors mm_interleaved/models/utils/ops/functions/__init__.py:9
from .ms_deform_attn_func import MSDeformAttnFunction, ms_deform_attn_core_pytorch  # noqa: F401
from .mmfs_plan_func import MMFSPlanFunction, mmfs_plan_supported  # noqa: F401,E402
from .bank_func import BankGatherFunction, bank_gather_supported  # noqa: F401,E402
from .norm_func import RMSNormFunction, rmsnorm_supported  # noqa: F401,E402
from .deform_plan_func import DeformPlanFunction, deform_plan_supported, deform_sample_forward  # noqa: F401,E402
from .dwconv_func import DWConvTokensFunction, dwconv_tokens_supported  # noqa: F401,E402
from .pyramid_func import PyramidHeadFunction, pyramid_head_supported  # noqa: F401,E402
from .sequence_func import ContextGatherFunction, SequenceEmbedFunction, sequence_supported  # noqa: F401,E402
from .qk_attn_func import QKNormAttentionFunction, qk_attn_supported  # noqa: F401,E402
from .llama_attn_func import llama_attn_decode, llama_attn_prefill, llama_attn_supported, llama_rope_append, rope_table  # noqa: F401,E402
from .llama_train_func import LlamaAttnTrainFunction, llama_attn_train, llama_attn_train_supported  # noqa: F401,E402
from .clip_attn_func import ClipAttentionFunction, clip_attn_supported  # noqa: F401,E402
