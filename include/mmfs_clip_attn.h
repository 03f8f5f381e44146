/* mmfs_clip_attn.h -- the CLIP ViT's self-attention of libmmfs_msda.so (csrc/mmfs_clip_attn.hip).
 *
 * A header of its own beside mmfs_msda.h, whose status codes, dtype codes and conventions it takes: the entries below are
 * additive, MMFS_MSDA_ABI_VERSION stays what it is, and a caller detects them by the symbol.
 *
 * Full (non-causal) self-attention for heads of 64 channels, forward and backward, without a tensor of size L x L: what the
 * reference's CLIPXAttention (encoders/vit_adapter/xattn.py:21-141) asks of xformers.ops.memory_efficient_attention(q, k, v).
 *   q, k, v, out, dout, dq, dk, dv   [B, L, H * 64] of dtype (MMFS_F16 / MMFS_BF16), packed, token-major, as the Linear layers
 *                                    return and take them; 16-byte aligned
 *   lse                              [B, H, L] fp32: ln sum_t exp(q_j . k_t / 8)
 *   out = softmax_t(q_j . k_t / 8) v, P rounded to the storage type before the second product; arithmetic in fp32.
 * No entry reads anything back, allocates, clears or synchronises; no atomics: bit-reproducible, eager or replayed from a graph.
 * mmfs_clip_attn_supported: D == 64, a 16-bit type, 1 <= L <= 2^22; otherwise 0 and the calls return MMFS_E_UNSUPPORTED.
 * mmfs_clip_attn_tiles: level 0 the query rows of a workgroup (forward, dq), 1 the keys of a forward tile, 2 the keys of a dkdv
 *   workgroup, 3 the queries of a dkdv tile, 4 the query rows of a wave; any other level MMFS_E_DIMS.  Host-only.
 * mmfs_clip_attn_workspace_bytes: what the backward's ``workspace`` (16-byte aligned, nothing to clear) holds: delta [B, H, L]
 *   fp32; < 0: MMFS_E_DIMS.  Host-only.
 * mmfs_clip_attn_forward: one launch.  lse may be NULL: it is not written then, and no backward can follow.
 * mmfs_clip_attn_backward: two launches (dq, which also writes delta = rowsum(dout * out) to the workspace; then dk and dv).
 *   Both recompute P = exp(score - lse).
 * Errors come back before any launch: MMFS_E_DTYPE (an unknown code); MMFS_E_DIMS for a negative size, B * H > 2^24 or a grid of
 *   more than 2^31 - 1 workgroups (ceil(L / tiles(0)) * B * H); MMFS_E_UNSUPPORTED for what the query refuses (an empty L is not
 *   refused); then 0 for an empty problem (B, H or L of 0); MMFS_E_NULLPTR for a NULL required pointer or a workspace of fewer
 *   than workspace_bytes(B, H, L) bytes; MMFS_E_ALIGN for tensors and the workspace that are not 16-byte aligned (lse: 4). */
#ifndef MMFS_CLIP_ATTN_H
#define MMFS_CLIP_ATTN_H

#include "mmfs_msda.h"

#ifdef __cplusplus
extern "C" {
#endif

int mmfs_clip_attn_supported(int dtype, int64_t D, int64_t L);
int64_t mmfs_clip_attn_tiles(int level);
int64_t mmfs_clip_attn_workspace_bytes(int64_t B, int64_t H, int64_t L);
int mmfs_clip_attn_forward(int dtype, const void *q, const void *k, const void *v, void *out, float *lse, int64_t B, int64_t L,
                           int64_t H, int64_t D, void *stream);
int mmfs_clip_attn_backward(int dtype, const void *q, const void *k, const void *v, const void *out, const void *dout,
                            const float *lse, void *dq, void *dk, void *dv, float *workspace, int64_t workspace_bytes,
                            int64_t B, int64_t L, int64_t H, int64_t D, void *stream);

#ifdef __cplusplus
}
#endif

#endif
