"""The callers either side of the op."""
from .llama_mmfs import LlamaMMFSAttention, LlamaMMFSSchedule, MMFSRMSNorm, ProjectedBank  # noqa: F401
from .sd_mmfs import MMFSBlock, MMFSNet  # noqa: F401
from .vit_adapter import (ConvFFN, DWConv, Extractor, Injector, InteractionBlock, InteractionBlockWithCls,  # noqa: F401
                          deform_inputs, get_reference_points)
