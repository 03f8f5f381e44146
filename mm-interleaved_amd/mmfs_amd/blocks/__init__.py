"""The callers either side of the op."""
from .llama_mmfs import LlamaMMFSAttention, LlamaMMFSSchedule, MMFSRMSNorm, ProjectedBank  # noqa: F401
from .sd_mmfs import MMFSBlock, MMFSNet  # noqa: F401
from .vit_adapter import (AdapterPyramidHead, ConvFFN, DWConv, Extractor, Injector, InteractionBlock,  # noqa: F401
                          InteractionBlockWithCls, deform_inputs, get_reference_points, pyramid_pos_tables)
