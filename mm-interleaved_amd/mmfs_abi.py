"""The C ABI of ``libmmfs_msda.so`` as Python sees it: ONE table of signatures, one line per prototype of
include/mmfs_msda.h in the header's order, and ``bind``, which applies it to a ``ctypes.CDLL`` handle.  The shim
(MultiScaleDeformableAttention.py, next to this file) binds the library once; the tests bind their own handle with the
same call.  tests/test_capi.py parses the header and holds this table to it, name by name and argument by argument.
Entries added beside that header keep a table of their own (``CLIP_ATTN_SIGNATURES``: include/mmfs_clip_attn.h), which
``bind`` applies as well.
"""
import ctypes
import re

import torch

# name, return kind, argument kinds.  Kinds: i int, l int64_t, u unsigned, f float, p pointer (any ``*``; c_void_p),
# s ``const char *`` (returns only), v void (returns only).  A digit repeats the letter before it: "p6" is six pointers.
_TABLE = """
mmfs_msda_abi_version                           i
mmfs_msda_build_info                            s
mmfs_msda_status_string                         s  i
mmfs_msda_plan_selfcheck                        i  ll i
mmfs_msda_forward                               i  i p6 l7 p
mmfs_msda_forward_flags                         i  i p6 l7 u p
mmfs_msda_forward_shared                        i  i p6 ll i l6 u p
mmfs_msda_backward_taps_fused                   i  i l7 u
mmfs_msda_backward_workspace_bytes              l  i l7 u
mmfs_msda_backward                              i  i p10 l8 u p
mmfs_msda_backward_checked                      i  i p10 l8 u pp
mmfs_msda_backward_taps                         i  i p8 l7 p
mmfs_msda_backward_value                        i  i p7 l8 p
mmfs_msda_backward_value_prepare                i  i p3 l8 p
mmfs_msda_backward_value_sort                   i  i p3 l8 p
mmfs_msda_backward_value_reduce                 i  i p3 l8 p
mmfs_msda_backward_value_run                    i  i p5 l8 p
mmfs_msda_backward_hybrid_workspace_bytes       l  i pp l7 u
mmfs_msda_backward_hybrid                       i  i p12 l8 uu p
mmfs_msda_backward_sorted_workspace_bytes       l  i l7 u
mmfs_msda_backward_sorted                       i  i p10 l9 uu p
mmfs_msda_cast_from_f32                         i  i pp l p
mmfs_plan_forward                               i  i p11 l9 p
mmfs_plan_backward                              i  i p12 l9 p
mmfs_plan_forward_heads                         i  i pp ll pp ll p7 l9 p
mmfs_plan_backward_heads                        i  i p10 ll i pp l11 p
mmfs_sample_forward                             i  i p12 l11 p
mmfs_sample_forward_token                       i  i p13 l11 p
mmfs_sample_forward_heads                       i  i p5 ll p8 l11 p
mmfs_sample_forward_heads_shared                i  i p5 ll p8 ll i l10 p
mmfs_bank_quantize_fp8                          i  i p l4 p3
mmfs_msda_forward_fp8                           i  i p7 ll i l6 p
mmfs_sample_forward_heads_fp8                   i  i p6 ll p8 ll i l10 p
mmfs_sample_forward_groups                      i  i l4
mmfs_deform_plan_supported                      i  i l4
mmfs_deform_plan_forward                        i  i pp ll p4 l8 p
mmfs_deform_plan_backward                       i  i p7 l10 p
mmfs_deform_sample_forward                      i  i p5 ll pp l10 p
mmfs_dwconv_tokens_supported                    i  i ll i
mmfs_dwconv_tokens_forward                      i  i p6 l4 i p
mmfs_dwconv_tokens_backward_workspace_bytes     l  i p l4 i
mmfs_dwconv_tokens_backward                     i  i p9 l4 i p
mmfs_pyramid_head_supported                     i  i l3 i
mmfs_pyramid_head_forward                       i  i p12 l4 ii p
mmfs_pyramid_head_backward                      i  i p7 l4 ii p
mmfs_sequence_supported                         i  i l
mmfs_sequence_index                             i  p l6 p7
mmfs_sequence_embed_forward                     i  ii p4 l pp l3 p
mmfs_sequence_embed_backward                    i  ii p9 l5 p
mmfs_sequence_context_forward                   i  i p9 l6 p
mmfs_sequence_context_backward_workspace_bytes  l  i ll
mmfs_sequence_context_backward                  i  i p9 l6 p
mmfs_text_loss_supported                        i  i l
mmfs_text_loss_forward                          i  i p6 l6 i p
mmfs_text_loss_backward                         i  i p6 l6 i p
mmfs_qk_attn_supported                          i  i l3
mmfs_qk_attn_forward                            i  i p7 i f p i l p3 l5 p
mmfs_qk_attn_backward                           i  i p7 i f p i l p8 l5 p
mmfs_llama_attn_supported                       i  i l3
mmfs_llama_attn_rope_append                     i  i p6 l p5 l5 p
mmfs_llama_attn_decode_keys                     l  i
mmfs_llama_attn_decode_workspace_bytes          l  l3
mmfs_llama_attn_decode                          i  i p6 i ll pp l5 p
mmfs_llama_attn_prefill                         i  i p6 i l3 u p l5 p
mmfs_llama_attn_prefill_tiles                   l  i
mmfs_llama_attn_train_supported                 i  i ll
mmfs_llama_attn_train_tiles                     l  i
mmfs_llama_attn_train_workspace_bytes           l  l3
mmfs_llama_attn_train_rope                      i  i p5 l pp l4 p
mmfs_llama_attn_train_forward                   i  i p5 l4 p
mmfs_llama_attn_train_backward                  i  i p9 l p4 l4 p
mmfs_bank_gather                                i  ii p4 l3 p
mmfs_bank_scatter                               i  ii p4 l3 p
mmfs_rmsnorm_supported                          i  i l
mmfs_rmsnorm_forward                            i  i p4 ll f p
mmfs_rmsnorm_backward                           i  i p6 ll p
mmfs_rmsnorm_backward_partials_rows             i  l
mmfs_rmsnorm_backward_partials                  i  i p6 ll p
mmfs_query_prep_supported                       i  i ll
mmfs_query_prep                                 i  i p7 l3 f p
mmfs_tokens_add                                 i  i p3 l3 p
mmfs_linear_small_supported                     i  i l3
mmfs_linear_small                               i  i p4 l5 p
mmfs_linear_small_add                           i  i p5 l6 p
mmfs_env_reload                                 v
mmfs_env_knob                                   i  i p3
"""

# include/mmfs_clip_attn.h, in its order: additive entries that live in a header of their own (the ABI version does not move;
# tests/test_clip_attn.py holds this table to that header)
_CLIP_ATTN_TABLE = """
mmfs_clip_attn_supported                        i  i ll
mmfs_clip_attn_tiles                            l  i
mmfs_clip_attn_workspace_bytes                  l  l3
mmfs_clip_attn_forward                          i  i p5 l4 p
mmfs_clip_attn_backward                         i  i p10 l5 p
"""

_KIND = {"i": ctypes.c_int, "l": ctypes.c_int64, "u": ctypes.c_uint, "f": ctypes.c_float, "p": ctypes.c_void_p,
         "s": ctypes.c_char_p, "v": None}


def _parse(table):
    out = {}
    for line in table.strip().splitlines():
        name, ret, *args = line.split()
        out[name] = (ret, re.sub(r"(.)(\d+)", lambda m: m[1] * int(m[2]), "".join(args)))
    return out


# {name: (return kind, argument kinds -- one letter per argument)}, in the header's order
SIGNATURES = _parse(_TABLE)
CLIP_ATTN_SIGNATURES = _parse(_CLIP_ATTN_TABLE)

# the one entry point whose pointers are typed: it hands three strings back
_TYPED = {"mmfs_env_knob": [ctypes.c_int] + [ctypes.POINTER(ctypes.c_char_p)] * 3}

# enum mmfs_dtype (include/mmfs_msda.h): MMFS_F32, MMFS_F16, MMFS_BF16, MMFS_F64 -- and the three that every entry point
# besides the op itself stops at
DTYPE_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.float64: 3}
FLOAT_CODE = {t: c for t, c in DTYPE_CODE.items() if t != torch.float64}


def bind(lib):
    """Give every entry point of the two tables its ``restype`` / ``argtypes`` on ``lib`` (a ``ctypes.CDLL``); -> ``lib``.
    A name the library does not export raises ImportError."""
    for name, (ret, args) in {**SIGNATURES, **CLIP_ATTN_SIGNATURES}.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise ImportError(f"{getattr(lib, '_name', lib)} does not export {name}: rebuild the library") from None
        fn.restype = _KIND[ret]
        fn.argtypes = _TYPED.get(name) or [_KIND[k] for k in args]
    return lib
