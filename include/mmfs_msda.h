/*
 * include/mmfs_msda.h -- C ABI of libmmfs_msda.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for the one hot path this repository replaces in
 * OpenGVLab/MM-Interleaved: the native extension ``MultiScaleDeformableAttention``
 * behind the Multi-modal Feature Synchronizer (MMFS).  The reference binds that
 * extension with pybind11 (two functions); each entry point below names the
 * reference interface it replaces.  The Python shim that adapts torch tensors to
 * these raw pointers is mm-interleaved_amd/MultiScaleDeformableAttention.py; the
 * binding a reference maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HIP) unless stated otherwise;
 *   - all tensors are contiguous, row-major, in the layouts of the reference op:
 *       value   [B, S, H, D]          S = sum_l Hl*Wl over all L levels
 *       shapes  [L, 2]  int64 (Hl, Wl)        (device memory, as in the reference,
 *       start   [L]     int64                  ms_deform_attn_cuda.cu:68-69)
 *       loc     [B, Nq, H, L, P, 2]   (x, y) normalised to [0, 1]
 *       attn    [B, Nq, H, L, P]
 *       out     [B, Nq, H*D]
 *   - ``dtype`` selects the storage type of value/loc/attn/out/grad_out; arithmetic
 *     is fp32 for 16-bit storage (the reference's opmath, ms_deform_im2col_cuda.cuh:32);
 *   - ``stream`` is a hipStream_t (NULL = the null stream).  Launches are
 *     asynchronous; the library keeps no state, allocates and frees nothing, and is
 *     re-entrant from any host thread (autograd engine threads, checkpoint re-runs);
 *   - return value: 0 on success; < 0 argument error (MMFS_E_*); > 0 a hipError_t
 *     from the launch.  Unlike the reference, launch errors are returned, not
 *     printed (ms_deform_im2col_cuda.cuh:951-955).
 */
#ifndef MMFS_MSDA_H_
#define MMFS_MSDA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMFS_MSDA_ABI_VERSION 14  /* 14 (additive): + mmfs_llama_attn_train_supported / _train_tiles / _train_workspace_bytes / _train_rope / _train_forward /
                                   *     _train_backward: the same attention in training, causal, forward and backward, see "LLaMA
                                   *     self-attention in training" below
                                   * 14 (additive): + mmfs_llama_attn_prefill / _prefill_tiles, MMFS_LLAMA_PREFILL_*: the same attention over a prompt, see
                                   *     "LLaMA self-attention over a prompt" below
                                   * 14 (additive): + mmfs_llama_attn_supported / _rope_append / _decode_keys / _decode_workspace_bytes / _decode: the LLM's self-attention
                                   *     at decode (rotary embedding, in-place key / value cache, split-key attention), see "LLaMA self-attention at
                                   *     decode" below
                                   * 14 (additive): + mmfs_qk_attn_supported / _forward / _backward: the Q-Former's attention with per-head q/k
                                   *     LayerNorm as one forward and one backward kernel, see "Q-Former attention" below
                                   * 14 (additive): + mmfs_text_loss_supported / _forward / _backward, MMFS_TEXT_LOSS_*: the text loss (cross-entropy of
                                   *     the text decoder's 16-bit logits and its gradient) on the device, see "The text loss" below
                                   * 14 (additive): + mmfs_sequence_supported / _index / _embed_forward / _embed_backward / _context_forward /
                                   *     _context_backward_workspace_bytes / _context_backward: the interleaved sequence (embeddings and the image
                                   *     decoder's context) built on the device, see "The interleaved sequence" below
                                   * 14 (additive): + mmfs_pyramid_head_supported / _forward / _backward: the ViT-Adapter's output pyramid from the
                                   *     tokens, packed for the feature bank, see "The adapter's output pyramid" below
                                   * 14 (additive): + mmfs_dwconv_tokens_supported / _forward / _backward_workspace_bytes / _backward: the depthwise
                                   *     convolution of the ViT-Adapter's ConvFFN in the token layout, see "ConvFFN's depthwise convolution" below
                                   * 14 (additive): + mmfs_deform_plan_supported / _forward / _backward, mmfs_deform_sample_forward: the image
                                   *     encoder's MSDeformAttn front end, see "The image encoder's MSDeformAttn" below
                                   * 14 (additive): + mmfs_bank_quantize_fp8, mmfs_msda_forward_fp8, mmfs_sample_forward_heads_fp8:
                                   *     the inference-only fp8 (e4m3) value bank with fp32 scales, see "fp8 bank" below
                                   * 14: + mmfs_msda_forward_shared, mmfs_sample_forward_heads_shared: one value bank of Bv rows serves
                                   *     B = g * Bv query rows (MMFS_BANK_TILE / MMFS_BANK_INTERLEAVE) without being copied
                                   * 13: + mmfs_msda_backward_sorted (+ _workspace_bytes): the whole backward on the cell-sorted records -- grad_loc / grad_attn
                                   *     from the records the grad_value sort makes (csrc/msda_bwd_taps_sorted.hip), no per-sample value-row gather;
                                   *     GONE: the workgroup-local grad_value of the small levels (csrc/msda_gv_mma.hip: parity-green, slower on every
                                   *     shipped geometry for three rounds) with stage MMFS_HYB_BWD_VALUE_BLOCKS, MMFS_BWD_VALUE_SORTED_ONLY /
                                   *     MMFS_BWD_VALUE_LDS_BLOCKS, mmfs_msda_backward_value_lds_levels, mmfs_msda_debug_value_plan
                                   * 12: + mmfs_env_reload / mmfs_env_knob (the environment knobs are one table, read once); 11: + MMFS_FWD_QUERY_WAVES (the forward's fourth formulation, csrc/msda_fwd_wq.hip: the default for 16-bit
                                   *     heads of 128 channels with one chunk of samples per query -- the north-star shape); every
                                   *     matrix-core forward returns the reference's Inf / NaN element for element (a non-finite sum
                                   *     is recomputed channel by channel)
                                   * 10: + mmfs_sample_forward_groups, mmfs_linear_small_add, mmfs_plan_forward_heads / mmfs_plan_backward_heads; mmfs_sample_forward* serve at most 8 queries per (sample,
                                   *     head) -- a decode step -- with a workgroup per query (same products, another order of
                                   *     the fp32 sums: see there)
                                   * 9: + MMFS_FWD_SLICES (the forward's third formulation, csrc/msda_fwd_q8.hip);
                                   *    mmfs_msda_backward_checked serves a table its device-side check refuses IN THE
                                   *    SAME CALL (float-atomic fallback, csrc/msda_bwd_refused.hip; round 3 returned a
                                   *    zero grad_value for it): the workspace of MMFS_BWD_DEVICE_CHECKED_LEVELS grows by
                                   *    an fp32 image for 16-bit storage
                                   * 8: + stage MMFS_HYB_BWD_VALUE_BLOCKS of mmfs_msda_backward_hybrid (grad_value of the small levels sorted
                                   *      and reduced inside a workgroup, csrc/msda_gv_mma.hip), MMFS_BWD_VALUE_SORTED_ONLY /
                                   *      MMFS_BWD_VALUE_LDS_BLOCKS, mmfs_msda_backward_value_lds_levels
                                   * 7: + mmfs_msda_forward_flags (the forward's two formulations, selectable);
                                   *    + mmfs_msda_backward_checked: a level table the device-side check cannot serve is
                                   *      REPORTED through a status word, no device trap (MMFS_BWD_DEVICE_CHECKED_LEVELS
                                   *      is refused by mmfs_msda_backward, which has nowhere to report)
                                   * 6: + mmfs_sample_forward (plan -> sampler in one kernel)
                                   * 5: + MMFS_BWD_DEVICE_CHECKED_LEVELS; the dense forward / grad_value products
                                   *    (mmfs_msda_forward_hybrid*, MMFS_BWD_DENSE_VALUE) are gone: measured slower than
                                   *    the row-gather forward and the matrix-core tile reduce on every shipped geometry */

enum mmfs_dtype {
    MMFS_F32  = 0,
    MMFS_F16  = 1,
    MMFS_BF16 = 2,   /* new capability: the reference has no bf16 (ms_deform_attn_cuda.cu:65) */
    MMFS_F64  = 3
};

enum mmfs_status {
    MMFS_OK          = 0,
    MMFS_E_DTYPE     = -1,   /* unknown dtype code */
    MMFS_E_DIMS      = -2,   /* negative dim or a product that overflows the kernel's index range */
    MMFS_E_NULLPTR   = -3,   /* required pointer is NULL while the tensor is non-empty */
    MMFS_E_ALIGN     = -4,   /* tensor base not aligned to its element size */
    MMFS_E_UNSUPPORTED = -5
};

/* ABI version of the loaded library (== MMFS_MSDA_ABI_VERSION at build time). */
int mmfs_msda_abi_version(void);

/* Static description of the build, e.g. "gfx950 hipcc <ver>".  Host string. */
const char *mmfs_msda_build_info(void);

/* Text for a status returned by any entry point.  Host string, never NULL. */
const char *mmfs_msda_status_string(int status);

/* Host-only self-check of the sorted backward's tiling rules for one H x W level cut into at least
 * ``nt_min`` sort tiles (the functions the device plan uses, run on the host): 0 when the tiles cover every
 * cell exactly once and every 4x4 block of the level is planned exactly once, -1 when the level owns no
 * tile (empty, or an extent >= 65536), else a count of violations.  No reference counterpart: test hook. */
int mmfs_msda_plan_selfcheck(int64_t H, int64_t W, int nt_min);

/*
 * Forward.  Replaces ``ms_deform_attn_forward`` of the reference extension
 *   mm_interleaved/models/utils/ops/src/vision.cpp:14
 *   -> src/ms_deform_attn.h:20-39 -> src/cuda/ms_deform_attn_cuda.cu:21-81
 *   -> kernel src/cuda/ms_deform_im2col_cuda.cuh:240-302.
 * Writes every element of ``out`` (no pre-zeroing needed).  One launch covers the
 * whole batch; ``im2col_step`` of the reference has no effect on results and is
 * not part of this ABI.
 */
int mmfs_msda_forward(int dtype,
                      const void *value, const int64_t *shapes, const int64_t *start,
                      const void *loc, const void *attn, void *out,
                      int64_t B, int64_t S, int64_t H, int64_t D,
                      int64_t L, int64_t Nq, int64_t P, void *stream);

/*
 * The same forward with the formulation chosen by the caller (tests, measurements; mmfs_msda_forward is
 * flags = 0).  Two kernels implement it:
 *   row gather   (csrc/msda_fwd.hip)      every sample's four pixel rows through the vector-memory path;
 *                any storage type, any head width;
 *   LDS levels   (csrc/msda_fwd_mma.hip)  16-bit storage, D in {64, 128}, L <= 64: the levels of the pyramid
 *                that fit in the CU's LDS (smallest first, decided on the device from the table) are copied
 *                there once per workgroup and sampled by the matrix cores, the others by row gather.
 * flags = 0 (rounds 3-4) picked LDS levels for heads of 128 channels when a (b, h) slab has at least 64 queries and 4096 samples;
 * round 5: such shapes with at most 16 samples per query take "query waves" (below), longer sample lists keep LDS levels -- both only
 * in launches that give every CU two runs of (256, 128 or 64) queries, else the row gather, which fills the chip better -- (heads of
 * 64 channels measured no faster that way and stay on the row gather / the slices unless MMFS_FWD_LDS_LEVELS asks).
 * MMFS_FWD_LDS_LEVELS on a shape that does not allow it returns MMFS_E_UNSUPPORTED.
 */
#define MMFS_FWD_ROW_GATHER 1u
#define MMFS_FWD_LDS_LEVELS 2u
/*   slices       csrc/msda_fwd_q8.hip (round 4): 16-bit storage, head widths that are multiples of 32 channels, L <= 64.
 *                A workgroup owns a 32-channel SLICE of one (batch, head); every level whose slice fits in LDS (32x32 +
 *                16x16 + 8x8: 101 KB) is sampled by the matrix cores in tiles of 8 queries, the rest by row gather.
 * MMFS_FWD_SLICES on a shape that does not allow it returns MMFS_E_UNSUPPORTED. */
#define MMFS_FWD_SLICES 4u
/*   query waves  csrc/msda_fwd_wq.hip (round 5): 16-bit storage, D = 128, L <= 64.  A wave works on one query at a time;
 *                a sample's four pixel rows -- one wave-wide load, from memory or from the LDS image of the levels that
 *                fit -- are the B operand of ONE matrix-core product whose A operand carries the four bilinear weights
 *                on a diagonal (no unpack, no multiply-add in the vector ALU).  The default for that shape.
 * MMFS_FWD_QUERY_WAVES on a shape that does not allow it returns MMFS_E_UNSUPPORTED. */
#define MMFS_FWD_QUERY_WAVES 8u
int mmfs_msda_forward_flags(int dtype,
                            const void *value, const int64_t *shapes, const int64_t *start,
                            const void *loc, const void *attn, void *out,
                            int64_t B, int64_t S, int64_t H, int64_t D,
                            int64_t L, int64_t Nq, int64_t P, unsigned flags, void *stream);

/*
 * Shared bank.  Classifier-free guidance doubles the feature bank (torch.cat([bank] * 2)) and beam search repeats it per beam
 * (bank.repeat_interleave(num_beams, 0)): g query rows then read identical banks.  Here ``value`` holds the bank ONCE,
 * [Bv, S, H, D], and serves the B = g * Bv query rows of loc / attn / out (Bv > 0, B % Bv == 0):
 *     query row b reads bank row  vrow(b) = (b / div) % Bv
 *   MMFS_BANK_TILE        div = 1   the order of torch.cat([bank] * g)        (classifier-free guidance)
 *   MMFS_BANK_INTERLEAVE  div = g   the order of bank.repeat_interleave(g, 0) (beam search)
 * Bv = B is the identity (every existing entry is that call with MMFS_BANK_TILE).  The result is, bit for bit, the same
 * call on the expanded bank: only the (b, h) slab a query row reads from changes.  loc / attn / out keep the batch B.
 * mmfs_msda_forward_shared: mmfs_msda_forward_flags with a shared bank (same routing, decided for the B query rows).
 * MMFS_E_DIMS for Bv <= 0 or B % Bv != 0, MMFS_E_UNSUPPORTED for another layout code.  Forward only: a backward on a shared
 * bank is the backward on the expanded bank with grad_value summed over the copies (the Python shim does that).
 */
#define MMFS_BANK_TILE 0
#define MMFS_BANK_INTERLEAVE 1
int mmfs_msda_forward_shared(int dtype,
                             const void *value, const int64_t *shapes, const int64_t *start,
                             const void *loc, const void *attn, void *out,
                             int64_t B, int64_t Bv, int layout, int64_t S, int64_t H, int64_t D,
                             int64_t L, int64_t Nq, int64_t P, unsigned flags, void *stream);

/* Flags of mmfs_msda_backward(). */
#define MMFS_BWD_CANONICAL_LEVELS 1u
/*   The caller guarantees the level table is the canonical packing the reference's
 *   callers build (modeling_llama_mmfs.py:303-305, sd_mmfs.py:35-37):
 *       start[l] == sum_{k<l} H_k*W_k   and   sum_l H_l*W_l == S.
 *   (The table lives in device memory, so the library cannot check it without a
 *   device->host sync.)  With the guarantee every grad_value pixel has one owner level
 *   and the pixel-stationary kernel applies; without it the library falls back to
 *   float-atomic accumulation, which is also correct for gapped or overlapping levels. */
#define MMFS_BWD_FORCE_ATOMIC 2u      /* testing/measurement: always take the atomic path */
#define MMFS_BWD_DENSE_TAPS   4u      /* mmfs_msda_backward_hybrid: small levels' grad_loc / grad_attn by MFMA */
/* The caller does not read grad_attn (nor grad_loc, which is 0 anyway) of samples whose attention
 * weight is exactly 0: they may be written as 0 without reading the value rows.  True for MMFS: the
 * weights come out of its masked softmax (mmfs.py:203-231), whose backward multiplies every
 * incoming gradient by the weight itself, and images a token cannot see have weight exactly 0.
 * Honoured by mmfs_msda_backward and mmfs_msda_backward_hybrid (row-gather kernel); a hint. */
#define MMFS_BWD_LAZY_ZERO_ATTN 16u
/* The caller has NOT looked at the level table (it lives in device memory, and the reference's callers
 * rebuild it on every call: modeling_llama_mmfs.py:298-308, sd_mmfs.py:31-41) and does not want to pay a
 * device->host copy per backward to find out whether MMFS_BWD_CANONICAL_LEVELS holds.  The sorted
 * backward is taken and the table is checked ON THE DEVICE: any table whose levels do not overlap is
 * served (rows that belong to no level are zero-filled, like the reference's zero-initialised output).
 * Overlapping, out-of-range or >= 65536-wide levels cannot be served by the sorted backward: the SAME call then
 * computes grad_value as the reference does, with float atomics into a zero-filled fp32 image and a cast
 * (cuh:128-155, .cu:122-165; csrc/msda_bwd_refused.hip -- three launches that read the plan's verdict on the
 * device and return at once for any table the sorted backward served), and ORs 1 into the caller's status word
 * (mmfs_msda_backward_checked) so that the caller can learn it took the slow path.  The workspace of such a call
 * is larger by that image for 16-bit storage (mmfs_msda_backward_workspace_bytes with this flag says how much).
 * Only mmfs_msda_backward_checked takes this flag. */
#define MMFS_BWD_DEVICE_CHECKED_LEVELS 32u
/* grad_loc / grad_attn have two formulations (tests, measurements; default: the library chooses):
 *   row gather   csrc/msda_bwd.hip, plus -- mmfs_msda_backward_hybrid only -- levels of <= 256 pixels as a DENSE
 *                matrix-core product over all their pixels (csrc/msda_dense.hip);
 *   LDS levels   csrc/msda_taps_mma.hip: one kernel for all levels, 16-bit storage, D = 128, L <= 64; the levels that
 *                fit in the CU's LDS (decided on the device) are contracted on the matrix cores from GATHERED rows,
 *                the others by row gather.  Default from 64 queries and 4096 samples per (b, h) slab on.
 * MMFS_BWD_TAPS_LDS_LEVELS on a shape that does not allow it returns MMFS_E_UNSUPPORTED. */
#define MMFS_BWD_TAPS_ROW_GATHER 64u
#define MMFS_BWD_TAPS_LDS_LEVELS 128u
/* 1 when, for these arguments, grad_loc / grad_attn of ALL levels come from the one LDS-levels kernel (the staged
 * hybrid backward's MMFS_HYB_BWD_TAPS_COARSE stage then has nothing to launch), else 0.  Host-only. */
int mmfs_msda_backward_taps_fused(int dtype, int64_t B, int64_t S, int64_t H, int64_t D,
                                  int64_t L, int64_t Nq, int64_t P, unsigned flags);

/*
 * Scratch the backward needs for these arguments (0 when none).  Host-only computation.
 * Pixel-stationary path: re-packed copies of loc/attn (3*pts elements, pts = B*Nq*H*L*P), one
 * cursor per (b, h, level), a {first, count} run table per (b, h, pixel) and the pixel-sorted
 * {query, weight} records (4*pts * 8 bytes);
 * atomic path with 16-bit storage: an fp32 image of grad_value.
 */
int64_t mmfs_msda_backward_workspace_bytes(int dtype, int64_t B, int64_t S, int64_t H, int64_t D,
                                           int64_t L, int64_t Nq, int64_t P, unsigned flags);

/*
 * Backward.  Replaces ``ms_deform_attn_backward`` of the reference extension
 *   src/vision.cpp:15 -> src/ms_deform_attn.h:42-61
 *   -> src/cuda/ms_deform_attn_cuda.cu:84-166
 *   -> kernels src/cuda/ms_deform_im2col_cuda.cuh:304-923.
 *
 *   grad_out    [B, Nq, H*D]          storage dtype
 *   grad_value  [B, S, H, D]          storage dtype, fully overwritten (no pre-zeroing)
 *   grad_loc    [B, Nq, H, L, P, 2]   storage dtype, fully overwritten
 *   grad_attn   [B, Nq, H, L, P]      storage dtype, fully overwritten
 *   workspace   device scratch of at least mmfs_msda_backward_workspace_bytes(...)
 *               bytes (may be NULL when that is 0); contents irrelevant on entry
 *
 * grad_value is accumulated in fp32 (fp64 for MMFS_F64) and rounded once at the end,
 * the reference's semantics (ms_deform_attn_cuda.cu:122-129, 156-165).  Two
 * implementations, chosen by the library (see flags):
 *   pixel-stationary (no atomics; msda_bwd_value.hip) and float-atomic scatter
 *   (msda_bwd.hip; zero-fills and casts through ``workspace`` itself).
 */
int mmfs_msda_backward(int dtype,
                       const void *value, const int64_t *shapes, const int64_t *start,
                       const void *loc, const void *attn, const void *grad_out,
                       void *grad_value, void *grad_loc, void *grad_attn,
                       void *workspace, int64_t workspace_bytes,
                       int64_t B, int64_t S, int64_t H, int64_t D,
                       int64_t L, int64_t Nq, int64_t P, unsigned flags, void *stream);

/*
 * The same backward for callers that pass MMFS_BWD_DEVICE_CHECKED_LEVELS: ``table_status`` points at an int32
 * the device can write (device memory or mapped host memory), owned and zero-initialised by the caller.  When
 * the device-side check finds a table the sorted backward cannot serve, the sorted launches find nothing to do,
 * the float-atomic fallback at the end of the sequence computes grad_value as the reference does, and bit 0 of
 * *table_status is set (information only: every output of the call is correct; MMFS_BWD_FORCE_ATOMIC, or no flag,
 * takes the float-atomic path directly and faster).
 * Without the flag ``table_status`` is ignored (may be NULL) and the call is mmfs_msda_backward.
 */
int mmfs_msda_backward_checked(int dtype,
                               const void *value, const int64_t *shapes, const int64_t *start,
                               const void *loc, const void *attn, const void *grad_out,
                               void *grad_value, void *grad_loc, void *grad_attn,
                               void *workspace, int64_t workspace_bytes,
                               int64_t B, int64_t S, int64_t H, int64_t D,
                               int64_t L, int64_t Nq, int64_t P, unsigned flags,
                               int32_t *table_status, void *stream);

/*
 * The two stages of the pixel-stationary backward as separate launches (what
 * mmfs_msda_backward runs back to back when MMFS_BWD_CANONICAL_LEVELS applies); exported so
 * a caller can time or overlap them.  Same tensors and conventions as above.
 *   _taps  : grad_loc and grad_attn only (reads value)            -- kernel msda_bwd_vec<.., false>
 *   _value : grad_value only, canonical level table REQUIRED      -- kernel msda_bwd_value_tiled
 * Both return MMFS_E_UNSUPPORTED when the head width has no vector path
 * (D*sizeof(dtype) must be 16 bytes * 2^k, k <= 6; MMFS_F64 never): use mmfs_msda_backward.
 */
int mmfs_msda_backward_taps(int dtype,
                            const void *value, const int64_t *shapes, const int64_t *start,
                            const void *loc, const void *attn, const void *grad_out,
                            void *grad_loc, void *grad_attn,
                            int64_t B, int64_t S, int64_t H, int64_t D,
                            int64_t L, int64_t Nq, int64_t P, void *stream);
int mmfs_msda_backward_value(int dtype,
                             const int64_t *shapes, const int64_t *start,
                             const void *loc, const void *attn, const void *grad_out,
                             void *grad_value,
                             void *workspace, int64_t workspace_bytes,   /* as for mmfs_msda_backward */
                             int64_t B, int64_t S, int64_t H, int64_t D,
                             int64_t L, int64_t Nq, int64_t P, void *stream);

/* mmfs_msda_backward_value == _prepare (re-pack loc/attn into the workspace, clear the level
 * cursors), then _sort, then _reduce (_run == _sort + _reduce); exported separately so each kernel
 * can be timed / profiled on its own.  Two generations answer to _sort / _reduce:
 *   block-stationary (csrc/msda_bwd_block.hip; default for L <= 128 and head rows of 64..512 bytes):
 *     _sort keys every SAMPLE by the cell of its top-left corner (kernel msda_bwd_cell_sort, one
 *     16-byte record per sample); _reduce lets a lane group own a 2x2 pixel block and walk the 9
 *     cell runs that touch it (kernel msda_bwd_block_reduce: 2.25 instead of 4 grad_out row reads
 *     per sample), queues the lists of hot blocks whole and finishes them with
 *     msda_bwd_block_overflow / msda_bwd_block_ovf_store;
 *   pixel-stationary (csrc/msda_bwd_value.hip; the fallback, or MMFS_VALUE_ALGO=pixel): _sort writes
 *     one record per tap corner sorted by pixel (kernel msda_bwd_value_sort), _reduce lets a lane
 *     group own one pixel (kernel msda_bwd_value_reduce). */
int mmfs_msda_backward_value_prepare(int dtype, const void *loc, const void *attn,
                                     void *workspace, int64_t workspace_bytes,
                                     int64_t B, int64_t S, int64_t H, int64_t D,
                                     int64_t L, int64_t Nq, int64_t P, void *stream);
int mmfs_msda_backward_value_sort(int dtype, const int64_t *shapes, const int64_t *start,
                                  void *workspace, int64_t workspace_bytes,
                                  int64_t B, int64_t S, int64_t H, int64_t D,
                                  int64_t L, int64_t Nq, int64_t P, void *stream);
int mmfs_msda_backward_value_reduce(int dtype, const void *grad_out, void *grad_value,
                                    void *workspace, int64_t workspace_bytes,
                                    int64_t B, int64_t S, int64_t H, int64_t D,
                                    int64_t L, int64_t Nq, int64_t P, void *stream);
int mmfs_msda_backward_value_run(int dtype, const int64_t *shapes, const int64_t *start,
                                 const void *grad_out, void *grad_value,
                                 void *workspace, int64_t workspace_bytes,
                                 int64_t B, int64_t S, int64_t H, int64_t D,
                                 int64_t L, int64_t Nq, int64_t P, void *stream);

/* ------------------------------------------------------------------------------------------
 * Hybrid backward (no counterpart in the reference; same results within the storage type's
 * rounding).  On MI355X the row gathers of this op are bound by the vector-memory path, not by
 * HBM, and every level receives the same number of taps whatever its size.  When the caller can
 * hand over a HOST copy of the level table (``host_shapes`` [L, 2], ``host_start`` [L]: int64 in
 * host memory, equal to the device tables), grad_loc / grad_attn of levels of at most
 * min(256, 64*P) pixels are evaluated as a dense product on the matrix cores
 * (csrc/msda_dense.hip, kernel msda_taps_coarse):
 *     dot = grad_out . V_l^T    [queries x pixels], then 4 look-ups per sample
 * and the other levels run through the row-gather kernel of the plain entry point, restricted to
 * those levels.  grad_value always takes the sorted path of mmfs_msda_backward.
 * Applies to MMFS_F16 / MMFS_BF16, D in {32, 64, 128}, L <= 64, Nq >= 32, at least one such level,
 * MMFS_BWD_CANONICAL_LEVELS and MMFS_BWD_DENSE_TAPS in ``flags``; otherwise the *_workspace_bytes
 * query returns 0 and the call MMFS_E_UNSUPPORTED: use mmfs_msda_backward.
 * One behavioural difference, inherent to a dense product: a NON-FINITE value element inside a
 * dense level propagates (0 * Inf = NaN) to grad_loc / grad_attn of every query of its (b, h),
 * not only to the queries that sample it.  Environment MMFS_HYBRID=0 disables the routing.
 *
 * ``stages`` selects which launches a call issues (OR of the bits; all of them = the whole
 * pass, in this order), so each kernel can be timed on its own.  The stages of one pass share the
 * workspace and run in this order: VALUE_PREPARE also plans the sort (level rows, tiles) and may tell
 * the sort to read ``loc`` / ``attn`` where they are instead of re-packing them, so VALUE_SORT needs
 * the VALUE_PREPARE of THIS entry point on the same workspace, and ``loc`` / ``attn`` unchanged until
 * the sort has run.
 */
#define MMFS_HYB_BWD_TAPS_FINE      1u
#define MMFS_HYB_BWD_TAPS_COARSE    2u
#define MMFS_HYB_BWD_VALUE_PREPARE  4u
#define MMFS_HYB_BWD_VALUE_SORT     8u
#define MMFS_HYB_BWD_VALUE_REDUCE  16u
#define MMFS_HYB_BWD_ALL           31u
int64_t mmfs_msda_backward_hybrid_workspace_bytes(int dtype,
                                                  const int64_t *host_shapes, const int64_t *host_start,
                                                  int64_t B, int64_t S, int64_t H, int64_t D,
                                                  int64_t L, int64_t Nq, int64_t P, unsigned flags);
int mmfs_msda_backward_hybrid(int dtype,
                              const void *value, const int64_t *shapes, const int64_t *start,
                              const int64_t *host_shapes, const int64_t *host_start,
                              const void *loc, const void *attn, const void *grad_out,
                              void *grad_value, void *grad_loc, void *grad_attn,
                              void *workspace, int64_t workspace_bytes,
                              int64_t B, int64_t S, int64_t H, int64_t D,
                              int64_t L, int64_t Nq, int64_t P,
                              unsigned flags, unsigned stages, void *stream);

/* ------------------------------------------------------------------------------------------
 * The whole backward on the CELL-SORTED records (round 6; replaces ms_deform_attn_backward, vision.cpp:15,
 * ms_deform_attn_cuda.cu:84-166, ms_deform_im2col_cuda.cuh:90-162 + 304-923, like mmfs_msda_backward).
 * The grad_value half sorts the samples by the cell of their top-left corner anyway; a sample's four corners are the four
 * pixels around that cell.  Here grad_loc / grad_attn are computed from the same records (csrc/msda_bwd_taps_sorted.hip):
 * a wave per 4x4 block of cells holds the block's 5x5 value rows as one matrix-core operand and multiplies them with the
 * records' grad_out rows -- no value row is gathered per sample (the gather kernels: 4 rows per sample through the
 * vector-memory path).  Same results within the storage type's rounding (same products, fp32 sums in another order).
 * Applies to MMFS_F16 / MMFS_BF16, D in {32, 64, 128}, P a power of two with Nq * P <= 65536, a level table the HOST has
 * verified (MMFS_BWD_CANONICAL_LEVELS in ``flags``), a value slab S * H * D * 2 of less than 2 GiB and shapes whose sort
 * keeps its samples in registers (Nq <= 4096 per vector group); otherwise *_workspace_bytes returns 0 and the call MMFS_E_UNSUPPORTED: use mmfs_msda_backward[_hybrid].
 * MMFS_BWD_LAZY_ZERO_ATTN as there.  ``stages``: OR of the bits, all of them = the whole pass, in this order (each stage
 * needs the ones before it on the same workspace, and ``loc`` / ``attn`` unchanged until the sort has run).
 */
#define MMFS_SRT_BWD_PREPARE  1u   /* clear the cursors, plan (level rows, tiles) */
#define MMFS_SRT_BWD_SORT     2u   /* cell sort; also writes the zero grad_loc / grad_attn of samples that get no record */
#define MMFS_SRT_BWD_TAPS     4u   /* grad_loc / grad_attn from the records */
#define MMFS_SRT_BWD_REDUCE   8u   /* grad_value from the records (the matrix-core tile reduce) */
#define MMFS_SRT_BWD_ALL     15u
int64_t mmfs_msda_backward_sorted_workspace_bytes(int dtype, int64_t B, int64_t S, int64_t H, int64_t D,
                                                  int64_t L, int64_t Nq, int64_t P, unsigned flags);
/* blocks4: the number of 4x4 pixel blocks of all levels when the caller knows the level table on the host (exact grids),
 * else 0 (a bound is launched). */
int mmfs_msda_backward_sorted(int dtype,
                              const void *value, const int64_t *shapes, const int64_t *start,
                              const void *loc, const void *attn, const void *grad_out,
                              void *grad_value, void *grad_loc, void *grad_attn,
                              void *workspace, int64_t workspace_bytes,
                              int64_t B, int64_t S, int64_t H, int64_t D,
                              int64_t L, int64_t Nq, int64_t P, int64_t blocks4,
                              unsigned flags, unsigned stages, void *stream);

/*
 * dst[i] = (dtype) src[i], round-to-nearest-even.  Replaces the trailing
 * ``grad_value.to(torch::kHalf)`` of the reference backward (ms_deform_attn_cuda.cu:156-165);
 * used internally by the atomic path and exported for callers that keep fp32 buffers.
 * ``dtype`` must be MMFS_F16 or MMFS_BF16 (MMFS_F32 copies).
 */
int mmfs_msda_cast_from_f32(int dtype, const float *src, void *dst, int64_t n, void *stream);

/* ------------------------------------------------------------------------------------------
 * MMFS sampling plan: everything the reference's MMFS.forward does
 * between its Linear layers and the op, mm_interleaved/models/utils/ops/modules/mmfs.py:181-265
 * (relative-position term, per-level offset scaling, visibility penalty, constant sink logit,
 * softmax over all n*L*(P+1) logits, offsets -> normalised locations), in ONE kernel each way.
 * The linear heads are evaluated by the caller as head(W q) (off_q, att_q) plus table rows
 * head.weight @ query_relpos[m] (off_tab, att_tab); see mmfs_amd/modules/mmfs.py.
 *
 *   off_q   [N, Lq, H, P, 2]       att_q   [N, Lq, H, L, P]            (storage dtype)
 *   off_tab [M, H, P, 2]           att_tab [M, H, L, P]                (storage dtype)
 *           (point columns only: the head's (P+1)-th "sink" column is a constant, mmfs.py:225)
 *   relpos  [N, Lr, n] int64   image's rank among the visible ones, 0 = not visible; Lr = 1 or Lq
 *   ref     [Nr, Lq, 2] fp32   reference point (x, y) per query; Nr = 1 or N
 *   shapes  [n*L, 2] int64 (H_l, W_l);   ratios [L] fp32 (spatial_shape / base_spatial_shape)
 *   loc     [N, Lq, H, n*L, P, 2]  attn [N, Lq, H, n*L, P]  (storage dtype)   sink [N, Lq, H] fp32
 * Limits: P in {4, 8, 16}, n*L <= 64 (else MMFS_E_UNSUPPORTED: use the framework ops).
 * Backward: d_off_q / d_att_q are fully written (fp32, shaped like off_q / att_q); d_off_tab /
 * d_att_tab (fp32, shaped like the tables) are ACCUMULATED into and must be zero-filled by the
 * caller; grad_sink may be NULL (the sink weights feed nothing trainable in the reference).
 */
int mmfs_plan_forward(int dtype, const void *off_q, const void *att_q, const void *off_tab,
                      const void *att_tab, const int64_t *relpos, const float *ref,
                      const int64_t *shapes, const float *ratios, void *loc, void *attn, float *sink,
                      int64_t N, int64_t Lq, int64_t H, int64_t L, int64_t P, int64_t n, int64_t M,
                      int64_t Lr, int64_t Nr, void *stream);
int mmfs_plan_backward(int dtype, const void *grad_loc, const void *grad_attn, const float *grad_sink,
                       const void *attn, const float *sink, const int64_t *relpos,
                       const int64_t *shapes, const float *ratios,
                       float *d_off_q, float *d_att_q, float *d_off_tab, float *d_att_tab,
                       int64_t N, int64_t Lq, int64_t H, int64_t L, int64_t P, int64_t n, int64_t M,
                       int64_t Lr, int64_t Nr, void *stream);

/* The two calls for a caller that evaluates both query heads as ONE GEMM (their weights stacked: both read the same
 * activations, mmfs.py:174-176) and both tables as one: ``off_q`` / ``att_q`` are two column ranges of one
 * [N*Lq, H*2P + H*L*P] matrix -- token rows ``ld_off`` / ``ld_att`` elements apart (0 = packed) --, ``off_tab`` / ``att_tab``
 * likewise of one [M, ...] matrix (``ld_toff`` / ``ld_tatt``); the backward writes the gradients in the same layout, the
 * query-side ones in the storage type when ``q_grads_in_storage_type`` (one rounding of the fp32 sums, what a caller's cast
 * of the fp32 tensors does) -- so the gradient of the stacked GEMM's result is ONE tensor, made by this kernel. */
int mmfs_plan_forward_heads(int dtype, const void *off_q, const void *att_q, int64_t ld_off, int64_t ld_att,
                            const void *off_tab, const void *att_tab, int64_t ld_toff, int64_t ld_tatt,
                            const int64_t *relpos, const float *ref,
                            const int64_t *shapes, const float *ratios, void *loc, void *attn, float *sink,
                            int64_t N, int64_t Lq, int64_t H, int64_t L, int64_t P, int64_t n, int64_t M,
                            int64_t Lr, int64_t Nr, void *stream);
int mmfs_plan_backward_heads(int dtype, const void *grad_loc, const void *grad_attn, const float *grad_sink,
                             const void *attn, const float *sink, const int64_t *relpos,
                             const int64_t *shapes, const float *ratios,
                             void *d_off_q, void *d_att_q, int64_t ld_off, int64_t ld_att, int q_grads_in_storage_type,
                             float *d_off_tab, float *d_att_tab, int64_t ld_toff, int64_t ld_tatt,
                             int64_t N, int64_t Lq, int64_t H, int64_t L, int64_t P, int64_t n, int64_t M,
                             int64_t Lr, int64_t Nr, void *stream);

/*
 * The plan feeding the sampler (second half): mmfs_plan_forward followed by
 * mmfs_msda_forward as ONE kernel -- the locations and weights [N, Lq, H, n*L, P(, 2)] never exist in
 * memory.  Same inputs as mmfs_plan_forward plus the op's value / level tables (``shapes`` / ``start``
 * have n*L rows), same arithmetic (the plan's numbers are rounded to the storage type before use), so
 * ``out`` [N, Lq, H*D] is bit-identical to the two calls (more than 8 queries per (sample, head); fewer: see
 * mmfs_sample_forward_groups).  ``sink`` [N, Lq, H] fp32 may be NULL.
 * Forward only -- the backward needs loc / attn as tensors (a training step keeps the two calls).
 * MMFS_E_UNSUPPORTED (use the two calls) for P = 16, head rows that are not 16 bytes x 2^k (k <= 6), value
 * slabs of 2 GiB or more.
 */
int mmfs_sample_forward(int dtype, const void *value, const int64_t *shapes, const int64_t *start,
                        const void *off_q, const void *att_q, const void *off_tab, const void *att_tab,
                        const int64_t *relpos, const float *ref, const float *ratios, void *out, float *sink,
                        int64_t N, int64_t S, int64_t Lq, int64_t H, int64_t D, int64_t L, int64_t P, int64_t n,
                        int64_t M, int64_t Lr, int64_t Nr, void *stream);
/* The same with MMFS's ignore-token term folded into the store (mmfs.py:236-241, 274: ``out + ignore_token * sink``;
 * three framework kernels and a full-size temporary per block otherwise): ``token`` [H, D] of the storage type, 16-byte
 * aligned, or NULL (= mmfs_sample_forward).  Roundings as the framework statement's: the sampled output, the sink
 * weight and their product are each rounded to the storage type before the sum -- bit-identical to the three kernels. */
int mmfs_sample_forward_token(int dtype, const void *value, const int64_t *shapes, const int64_t *start,
                              const void *off_q, const void *att_q, const void *off_tab, const void *att_tab,
                              const int64_t *relpos, const float *ref, const float *ratios, const void *token,
                              void *out, float *sink,
                              int64_t N, int64_t S, int64_t Lq, int64_t H, int64_t D, int64_t L, int64_t P, int64_t n,
                              int64_t M, int64_t Lr, int64_t Nr, void *stream);
/* The same with the two query heads as COLUMNS of wider matrices: token row t of ``off_q`` starts ``ld_off`` elements
 * after row t - 1 (``ld_att`` for ``att_q``; 0 = packed, H*2P / H*L*P).  What a caller that evaluates
 * sampling_offsets and attention_weights as ONE GEMM (their weights stacked: both read the same activations,
 * mmfs.py:174-176) hands over: two column ranges of its [N*Lq, H*2P + H*L*P] result, no copies. */
int mmfs_sample_forward_heads(int dtype, const void *value, const int64_t *shapes, const int64_t *start,
                              const void *off_q, const void *att_q, int64_t ld_off, int64_t ld_att,
                              const void *off_tab, const void *att_tab,
                              const int64_t *relpos, const float *ref, const float *ratios, const void *token,
                              void *out, float *sink,
                              int64_t N, int64_t S, int64_t Lq, int64_t H, int64_t D, int64_t L, int64_t P, int64_t n,
                              int64_t M, int64_t Lr, int64_t Nr, void *stream);

/* The same with a shared bank (see mmfs_msda_forward_shared): ``value`` [Nv, S, H, D] serves the N = g * Nv query rows of
 * off_q / att_q / relpos / out / sink (and ref when it is batched) in the ``layout`` order, MMFS_BANK_TILE or
 * MMFS_BANK_INTERLEAVE; MMFS_E_DIMS for Nv <= 0 or N % Nv != 0.  ``out`` is bit-identical to the call on the expanded bank.
 * The launch order is the unshared call's: launching the g query rows of one bank row next to each other measured no faster
 * (DESIGN.md 4.9). */
int mmfs_sample_forward_heads_shared(int dtype, const void *value, const int64_t *shapes, const int64_t *start,
                                     const void *off_q, const void *att_q, int64_t ld_off, int64_t ld_att,
                                     const void *off_tab, const void *att_tab,
                                     const int64_t *relpos, const float *ref, const float *ratios, const void *token,
                                     void *out, float *sink,
                                     int64_t N, int64_t Nv, int layout, int64_t S, int64_t Lq, int64_t H, int64_t D, int64_t L,
                                     int64_t P, int64_t n, int64_t M, int64_t Lr, int64_t Nr, void *stream);

/*
 * fp8 bank (inference only).  A value bank read many times over (a generation's kept projections) may be stored at 8 bits:
 * ``q`` [Bv, S, H, D] OCP e4m3 (e4m3fn: bias 7, max 448, 0x7f / 0xff NaN, no infinities -- NOT the fnuz format) and
 * ``scale`` [Bv, H*D] fp32, one per (bank row, channel); element (b, s, h, d) stands for  float(q) * scale[b, h*D + d].
 * The kernels sum  w * float(q)  in fp32 and multiply by the scale once per output channel at the store.
 *
 * mmfs_bank_quantize_fp8: x [nbanks, Bv, R, C] of ``dtype`` (MMFS_F32 / MMFS_F16 / MMFS_BF16; R = rows per bank row, n*S;
 * C = H*D, a multiple of 16) -> q [nbanks, Bv, R, C] e4m3, scale [nbanks, Bv, C] fp32.  nbanks independent banks, one call.
 *     amax[b, c] = max |x| over the FINITE elements of bank row b, column c;   scale = amax / 448  (fp32 division)
 *     q = e4m3(RNE(clamp(x / scale, -448, 448)));   scale == 0 -> q = 0 (+0);   x not finite -> q = 0x7f (NaN)
 * Deterministic (the column maxima are order-independent).  x, q and scale 16-byte aligned.
 *
 * mmfs_msda_forward_fp8: mmfs_msda_forward_shared on an fp8 bank (pass Bv = B, MMFS_BANK_TILE for an unshared one); ``dtype``
 * is the type of loc / attn / out (MMFS_F32 / MMFS_F16 / MMFS_BF16).  The row gather only.  D = 16 * 2^k, k <= 4, else
 * MMFS_E_UNSUPPORTED (dequantise and use the 16-bit entries).
 * mmfs_sample_forward_heads_fp8: mmfs_sample_forward_heads_shared on an fp8 bank plus its ``scale``; the ignore-token term
 * and its roundings stay in ``dtype``.  The same D rule.  For the lane groups it uses (mmfs_sample_forward_groups), ask
 * with MMFS_BF16 and D / 2: 16 channels per lane, the lanes of a bf16 bank of half the width.
 * Argument errors come back before any launch, as for the shared entries.
 */
int mmfs_bank_quantize_fp8(int dtype, const void *x, int64_t nbanks, int64_t Bv, int64_t R, int64_t C,
                           void *q, float *scale, void *stream);
int mmfs_msda_forward_fp8(int dtype, const void *q, const float *scale, const int64_t *shapes, const int64_t *start,
                          const void *loc, const void *attn, void *out,
                          int64_t B, int64_t Bv, int layout, int64_t S, int64_t H, int64_t D,
                          int64_t L, int64_t Nq, int64_t P, void *stream);
int mmfs_sample_forward_heads_fp8(int dtype, const void *q, const float *scale, const int64_t *shapes, const int64_t *start,
                                  const void *off_q, const void *att_q, int64_t ld_off, int64_t ld_att,
                                  const void *off_tab, const void *att_tab,
                                  const int64_t *relpos, const float *ref, const float *ratios, const void *token,
                                  void *out, float *sink,
                                  int64_t N, int64_t Nv, int layout, int64_t S, int64_t Lq, int64_t H, int64_t D, int64_t L,
                                  int64_t P, int64_t n, int64_t M, int64_t Lr, int64_t Nr, void *stream);

/* How many lane groups share ONE query's samples in mmfs_sample_forward* for this shape (``nL`` = n * L level rows):
 * 1 = the samples are summed in their order, ``out`` bit-identical to mmfs_plan_forward + mmfs_msda_forward;
 * > 1 (at most 8 queries per (sample, head): a decode step; csrc/mmfs_plan.hip ``mmfs_sample_decode``) = every row of
 * a query is requested at once and the groups' fp32 partial sums are added in a fixed tree: the same products, equal to
 * the two calls within one rounding of the storage type, deterministic.  0 for shapes mmfs_sample_forward refuses. */
int mmfs_sample_forward_groups(int dtype, int64_t Lq, int64_t D, int64_t nL, int64_t P);

/* ---------------------------------------------------------------------------------------------
 * The image encoder's MSDeformAttn (ViT-Adapter): its sampling plan (csrc/msda_deform_plan.hip; additive at ABI 14).
 * Replaces what mm_interleaved/models/encoders/vit_adapter/ops/modules/ms_deform_attn.py:108-127 runs between its two
 * Linear heads and the op -- softmax, division by the level extent, add of the reference point, cast, two copies:
 *   off    [N, Lq, H, L, P, 2]  sampling_offsets(query)       storage type ``dtype`` (MMFS_F32 / MMFS_F16 / MMFS_BF16);
 *   logit  [N, Lq, H, L, P]     attention_weights(query)      token rows ``ld_off`` / ``ld_att`` ELEMENTS apart (0 = packed,
 *                                                             H*L*P*2 / H*L*P): both may be column ranges of one GEMM result
 *   ref    [Nr, Lq, Lref, R]    fp32; Nr = 1 or N, Lref = 1 or L (broadcast over the batch / the levels), R = 2 or 4
 *   shapes [L, 2]               int64 (H_l, W_l), device memory
 *   attn = softmax of the L*P logits of (n, q, h);   R = 2: loc = ref + off / (W_l, H_l);
 *   R = 4: loc = ref[:2] + off / P * ref[2:] * 0.5.   fp32 arithmetic, ONE rounding to the storage type at the store.
 * mmfs_deform_plan_forward  -> loc [N, Lq, H, L, P, 2], attn [N, Lq, H, L, P] (packed, 16-byte aligned), every element written.
 * mmfs_deform_plan_backward -> grad_off / grad_logit in the storage type, written with the forward's leading dimensions (one
 *   stacked gradient tensor feeds one GEMM backward): grad_logit_i = a_i (g_i - sum_j a_j g_j) from the saved ``attn``;
 *   grad_off = grad_loc * (1/W_l, 1/H_l) (R = 2) or * ref[2:] * 0.5 / P (R = 4).  Every element has one writer: no atomics,
 *   nothing to clear.  There is no gradient for ``ref``.
 * mmfs_deform_sample_forward: the plan feeding mmfs_msda_forward's row gather in ONE kernel, for calls without gradients --
 *   loc / attn never reach memory.  They are rounded to the storage type inside the kernel before use, with the plan kernel's
 *   own arithmetic and reduction order: ``out`` [N, Lq, H*D] is a function of the same numbers the two calls see.  value
 *   [N, S, H, D] and out 16-byte aligned.  MMFS_E_UNSUPPORTED (run the two calls) unless D * sizeof(T) is 32 .. 512 bytes,
 *   a power of two, and a value slab is below 2 GiB.
 * mmfs_deform_plan_supported: bit 0 = the plan kernels serve (dtype, L, P, R): P in {2, 4, 8}, L <= 8; bit 1 = the fused
 *   sampler serves head rows of D elements as well (D = 0 asks about the plan only).  Host only.
 * Errors come back before any launch: MMFS_E_DTYPE; MMFS_E_DIMS for a negative dimension, Nr / Lref / R outside the sets above
 * or a leading dimension below the packed one; MMFS_E_UNSUPPORTED for P / L / D outside the kernels' range; MMFS_E_NULLPTR
 * for a NULL tensor of a non-empty problem; MMFS_E_ALIGN for rows the vector accesses cannot take.  N * Lq == 0 returns 0. */
int mmfs_deform_plan_supported(int dtype, int64_t L, int64_t P, int64_t R, int64_t D);
int mmfs_deform_plan_forward(int dtype, const void *off, const void *logit, int64_t ld_off, int64_t ld_att,
                             const float *ref, const int64_t *shapes, void *loc, void *attn,
                             int64_t N, int64_t Lq, int64_t H, int64_t L, int64_t P, int64_t Nr, int64_t Lref, int64_t R,
                             void *stream);
int mmfs_deform_plan_backward(int dtype, const void *grad_loc, const void *grad_attn, const void *attn,
                              const float *ref, const int64_t *shapes, void *grad_off, void *grad_logit,
                              int64_t ld_off, int64_t ld_att,
                              int64_t N, int64_t Lq, int64_t H, int64_t L, int64_t P, int64_t Nr, int64_t Lref, int64_t R,
                              void *stream);
int mmfs_deform_sample_forward(int dtype, const void *value, const int64_t *shapes, const int64_t *start,
                               const void *off, const void *logit, int64_t ld_off, int64_t ld_att,
                               const float *ref, void *out,
                               int64_t N, int64_t S, int64_t Lq, int64_t H, int64_t D, int64_t L, int64_t P,
                               int64_t Nr, int64_t Lref, int64_t R, void *stream);

/* ---------------------------------------------------------------------------------------------
 * ConvFFN's depthwise convolution (ViT-Adapter) in the token layout (csrc/msda_dwconv.hip; additive at ABI 14).
 * Replaces what mm_interleaved/models/encoders/vit_adapter/adapter_modules.py:64-89 runs between fc1 and fc2: three
 * transposed copies into [B, C, h, w], three depthwise 3x3 convolutions, three transposes back, a concatenation and GELU.
 *   x        [B, N, C]      storage type ``dtype`` (MMFS_F32 / MMFS_F16 / MMFS_BF16): L maps packed one after the other, level l =
 *                           h_l x w_l tokens, row-major, N = sum h_l * w_l
 *   weight   [C, 1, 3, 3]   nn.Conv2d's, read where it lies;   bias [C] or NULL
 *   level_hw [2 * L]        HOST array (h_0, w_0, h_1, w_1, ...): the extents travel to the kernels by value -- no device table,
 *                           no allocation, no synchronisation, so the launches can be captured into a graph
 *   y[b, p, c] = bias[c] + sum_{ky,kx} weight[c, ky, kx] x[b, p + (ky-1, kx-1), c]: stride 1, zero padding; a tap outside its own
 *   map is skipped (never multiplied by 0: a non-finite input reaches exactly the outputs whose window covers it).  fp32
 *   arithmetic, ONE rounding to the storage type: y_T.
 *   act = MMFS_DWCONV_ACT_NONE: out = y_T.   act = MMFS_DWCONV_ACT_GELU: out = gelu(y_T), the exact (erf) GELU of the ROUNDED
 *   pre-activation, so that calls with and without ``pre`` return the same bits and the backward differentiates the number the
 *   forward used.
 * mmfs_dwconv_tokens_forward: out [B, N, C]; ``pre`` [B, N, C] or NULL: y_T, written only for MMFS_DWCONV_ACT_GELU (what the
 *   backward needs).  Every element written.
 * mmfs_dwconv_tokens_backward: from grad_out (the gradient of ``out``), x and -- MMFS_DWCONV_ACT_GELU -- pre:
 *   g_y = grad_out * (Phi(y_T) + y_T phi(y_T)) (MMFS_DWCONV_ACT_NONE: grad_out);  grad_x[p] = sum_d w[d] g_y[p - d];
 *   grad_weight[d] = sum_{b,p} x[p] g_y[p - d] ([C, 1, 3, 3]);  grad_bias = sum g_y ([C], or NULL), all in the storage type.
 *   One pass over the tensors; the weight / bias gradients are a two-stage reduction through ``workspace``
 *   (mmfs_dwconv_tokens_backward_workspace_bytes bytes, 16-byte aligned; every byte the second stage reads is written by the
 *   first: nothing to clear) added in a fixed order -- no float atomics, bit-reproducible.
 * mmfs_dwconv_tokens_backward_workspace_bytes: >= 0, or an MMFS_E_* of the list below.  Host only.
 * mmfs_dwconv_tokens_supported: 1 when the kernels serve (dtype, C, L, act): C * sizeof(T) a multiple of 16, 1 <= L <= 8.  Host only.
 * Errors come back before any launch: MMFS_E_DTYPE (an unknown code, MMFS_F64); MMFS_E_DIMS for a negative B, N or C, a
 * non-positive level extent or sum h_l * w_l != N; MMFS_E_UNSUPPORTED for L outside [1, 8], C * sizeof(T) not a multiple of 16 or
 * an unknown ``act``; MMFS_E_NULLPTR for a NULL required pointer of a non-empty problem (``level_hw`` included); MMFS_E_ALIGN for
 * tensors not 16-byte aligned.  B * N * C == 0 returns 0 without a launch. */
enum mmfs_dwconv_act {
    MMFS_DWCONV_ACT_NONE = 0,
    MMFS_DWCONV_ACT_GELU = 1
};
int mmfs_dwconv_tokens_supported(int dtype, int64_t C, int64_t L, int act);
int mmfs_dwconv_tokens_forward(int dtype, const void *x, const void *weight, const void *bias, void *out, void *pre,
                               const int64_t *level_hw, int64_t B, int64_t N, int64_t C, int64_t L, int act, void *stream);
int64_t mmfs_dwconv_tokens_backward_workspace_bytes(int dtype, const int64_t *level_hw, int64_t B, int64_t N, int64_t C,
                                                    int64_t L, int act);
int mmfs_dwconv_tokens_backward(int dtype, const void *grad_out, const void *x, const void *pre, const void *weight,
                                void *grad_x, void *grad_weight, void *grad_bias, void *workspace,
                                const int64_t *level_hw, int64_t B, int64_t N, int64_t C, int64_t L, int act, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The adapter's output pyramid (ViT-Adapter) from the tokens, packed token-major (csrc/mmfs_pyramid.hip; additive at ABI 14).
 * Replaces the tail of mm_interleaved/models/encoders/vit_adapter/vit_adapter_hf.py:137-153 (transposed copies of the adapter's
 * tokens and the four ViT maps, adapter_up, three bilinear resizes, five adds), the position add of encoders/visual_tokenizer.py:
 * 74-82 and the transposition back into the bank's layout.  H x W is the ViT map, both even.
 *   c     [B, 21 H W / 4, C]  the adapter's tokens c2 (2H x 2W) | c3 (H x W) | c4 (H/2 x W/2), storage type ``dtype``
 *   x1..x4 [B, H W, C]        the ViT's tokens after each interaction block
 *   up    [B, 4 H W, 4 C]     adapter_up as a GEMM on the c2 tokens, bias included: columns (di, dj, o); output pixel
 *                             (2i + di, 2j + dj) of level 1 reads row (i, j), column block (di, dj)
 *   c1    [B, C, 4H, 4W]      the spatial prior's first map: MMFS_PYRAMID_C1_NCHW contiguous, MMFS_PYRAMID_C1_NHWC channels_last
 *                             memory (i.e. [B, 4H, 4W, C])
 *   pos1..pos4 [h_l w_l, C]   fp32 tables, each or NULL
 *   levels                    bit l - 1 selects level l; the packed row holds the selected levels only, in order
 *   out   [B, S, C]           S = sum of the selected h_l w_l, (h_l, w_l) = (4H, 4W), (2H, 2W), (H, W), (H/2, W/2):
 *     level 1 = up + c1 + bilinear x4 (x1) + pos1;  level 2 = c2 + bilinear x2 (x2) + pos2;  level 3 = c3 + x3 + pos3;
 *     level 4 = c4 + mean 2x2 (x4) + pos4.   The resizes are F.interpolate's (bilinear, align_corners = False).  fp32 arithmetic,
 *     ONE rounding to the storage type.  A tap of weight 0 (the second tap of the clamped first rows / columns) is not read: a
 *     non-finite input reaches exactly the outputs that hold it under a non-zero weight.  Every element written.
 * mmfs_pyramid_head_backward: from grad_out [B, S, C]: grad_up [B, 4HW, 4C] and grad_c1 (c1's layout) are level 1's rows
 *   permuted; grad_x1 / grad_x2 are gathered by their owner from at most 8 x 8 / 4 x 4 gradient pixels; grad_x3 is level 3's
 *   rows; grad_x4[i, j] = 0.25 grad_4[i / 2, j / 2].  No atomics, nothing to clear, bit-reproducible.  The gradient of ``c`` is
 *   levels 2..4 of grad_out itself and is left to the caller.  An output pointer that is NULL is a gradient nobody needs: it
 *   is not computed.  Pointers of levels that are not selected are not looked at, by either call (alignment included).
 * mmfs_pyramid_head_supported: 1 when the kernels serve (dtype, C, H, W, levels): f32 / f16 / bf16, C * sizeof(T) a multiple
 *   of 16, H and W even and >= 2, 1 <= levels <= 15.  Host only.
 * Errors come back before any launch: MMFS_E_DTYPE (an unknown code, MMFS_F64); MMFS_E_DIMS for a negative B, H, W or C or
 * extents beyond the index range (H, W > 4096); MMFS_E_UNSUPPORTED for what the query refuses or an unknown ``c1_layout``;
 * MMFS_E_NULLPTR for a NULL input (or ``out`` / ``grad_out``) of a selected level; MMFS_E_ALIGN for tensors of selected levels
 * that are not 16-byte aligned.  B * C == 0 returns 0 without a launch. */
enum mmfs_pyramid_c1_layout {
    MMFS_PYRAMID_C1_NCHW = 0,
    MMFS_PYRAMID_C1_NHWC = 1
};
int mmfs_pyramid_head_supported(int dtype, int64_t C, int64_t H, int64_t W, int levels);
int mmfs_pyramid_head_forward(int dtype, const void *c, const void *x1, const void *x2, const void *x3, const void *x4,
                              const void *up, const void *c1, const float *pos1, const float *pos2, const float *pos3,
                              const float *pos4, void *out, int64_t B, int64_t H, int64_t W, int64_t C, int levels,
                              int c1_layout, void *stream);
int mmfs_pyramid_head_backward(int dtype, const void *grad_out, void *grad_up, void *grad_c1, void *grad_x1, void *grad_x2,
                               void *grad_x3, void *grad_x4, int64_t B, int64_t H, int64_t W, int64_t C, int levels,
                               int c1_layout, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The interleaved sequence (csrc/mmfs_sequence.hip; additive at ABI 14).  Replaces step 3 of _prepare_mm_embeds
 * (mm_interleaved/models/mm_interleaved.py:144-171: two nonzero(), a cast, a scatter, a scatter_add) and
 * _prepare_context_features_for_image_decoder (:254-304: two nonzero(), a Python loop over the images that slices with device
 * scalars, a projection of every padded row, a sin-cos table built on the host per call).  No entry reads anything back, allocates
 * or synchronises: all of them can be captured into a graph.  T is the storage type ``dtype`` (MMFS_F32 / MMFS_F16 / MMFS_BF16),
 * C * sizeof(T) a multiple of 16 and C > 0 (mmfs_sequence_supported; otherwise MMFS_E_UNSUPPORTED and the caller keeps the
 * framework's statements).  Arithmetic is fp32 with ONE rounding; copies move bits.
 *
 * mmfs_sequence_index: text_ids [B, L] int64 -> int32 tables, one launch (B * L, n_vis, n_images <= 2^22 each):
 *   img_rank [B L]       the row-major rank of an image token; -1 for another token and for a rank >= n_vis
 *   img_pos  [n_vis]     the flat position of the k-th image token; -1 where there is none
 *   soi_row, soi_col [n_images]   row and column of the k-th <soi>, row-major; -1 past the last one
 *   row_first [B + 1]    the images of row b are row_first[b] .. row_first[b + 1] - 1 (entries at most n_images)
 *   counts   [2]         image tokens and <soi> tokens found (not clamped: the caller's optional validation)
 * mmfs_sequence_embed_forward: out [rows, C] of T, rows = B L:  out[r] = img_rank[r] >= 0 ? vis[img_rank[r]] : T(text[r]);
 *   ``text`` [rows, C] is stored as ``text_dtype``: ``dtype`` or MMFS_F32.  A row with text_ids[r] == soi_token_id then becomes
 *   round_T(float(out[r]) + float(soi_token)).  vis [n_vis, C], soi_token [C] of T; the tables must come from an index call with
 *   this n_vis.
 * mmfs_sequence_embed_backward: from grad [rows, C] of T: grad_text[r] = img_rank[r] >= 0 ? 0 : grad[r] (``text_dtype``);
 *   grad_vis[k] = img_pos[k] >= 0 ? grad[img_pos[k]] : 0;  grad_soi = the sum of grad over the first min(counts[1], n_images) <soi>
 *   rows in ascending order.  Every element of an output is written; a NULL output is a gradient nobody needs.
 * mmfs_sequence_context_forward: image i < n_images has the window row_i = soi_row[i], col_i = start_idx[i] (or soi_col[i] when
 *   start_idx is NULL), bos_i = max(bos_idx[i], 0) (or 0), len_i = col_i - bos_i + 1 -- 0 when row_i < 0 or col_i is outside
 *   [0, L) -- clamped to [0, max_len]:
 *     out [n_images, max_len, C]:  out[i, j] = round_T(float(src[row_i, col_i - j]) + float(pos[j]))  for j < len_i,
 *                                             round_T(float(pad_row) + float(pos[j]))                elsewhere
 *     mask [n_images, max_len] int64: j < len_i
 *   src [B, L, C], pad_row [C] or NULL (= 0), pos [seq_len, C] or NULL (the value is then copied, not added), all of T.
 * mmfs_sequence_context_backward: from grad_out [n_images, max_len, C]: grad_src [B, L, C], token (b, t) the sum over the images
 *   of row b (row_first) whose window covers it, ascending; grad_pad [C] the sum of the padded rows, per image in ascending j into
 *   ``workspace`` (mmfs_sequence_context_backward_workspace_bytes, 16-byte aligned, every element written) and then over the
 *   images in ascending order.  Either output may be NULL.  No atomics, nothing to clear, bit-reproducible.
 * Errors come back before any launch: MMFS_E_DTYPE (an unknown code, MMFS_F64); MMFS_E_DIMS for a negative size, max_len < 1,
 * max_len > seq_len or a size beyond 2^22; MMFS_E_UNSUPPORTED for what mmfs_sequence_supported refuses or a ``text_dtype`` that
 * is neither ``dtype`` nor MMFS_F32; MMFS_E_NULLPTR for a NULL required pointer of a non-empty problem; MMFS_E_ALIGN for a
 * tensor of T that is not 16-byte aligned (tables: their element size). */
int mmfs_sequence_supported(int dtype, int64_t C);
int mmfs_sequence_index(const int64_t *text_ids, int64_t B, int64_t L, int64_t image_token_id, int64_t soi_token_id,
                        int64_t n_vis, int64_t n_images, int32_t *img_rank, int32_t *img_pos, int32_t *soi_row,
                        int32_t *soi_col, int32_t *row_first, int32_t *counts, void *stream);
int mmfs_sequence_embed_forward(int dtype, int text_dtype, const void *text, const void *vis, const void *soi_token,
                                const int64_t *text_ids, int64_t soi_token_id, const int32_t *img_rank, void *out,
                                int64_t rows, int64_t C, int64_t n_vis, void *stream);
int mmfs_sequence_embed_backward(int dtype, int text_dtype, const void *grad, const int32_t *img_rank, const int32_t *img_pos,
                                 const int32_t *soi_row, const int32_t *soi_col, const int32_t *counts, void *grad_text,
                                 void *grad_vis, void *grad_soi, int64_t rows, int64_t L, int64_t C, int64_t n_vis,
                                 int64_t n_images, void *stream);
int mmfs_sequence_context_forward(int dtype, const void *src, const void *pad_row, const void *pos, const int32_t *soi_row,
                                  const int32_t *soi_col, const int64_t *start_idx, const int64_t *bos_idx, void *out,
                                  int64_t *mask, int64_t B, int64_t L, int64_t C, int64_t n_images, int64_t max_len,
                                  int64_t seq_len, void *stream);
int64_t mmfs_sequence_context_backward_workspace_bytes(int dtype, int64_t C, int64_t n_images);
int mmfs_sequence_context_backward(int dtype, const void *grad_out, const int32_t *soi_row, const int32_t *soi_col,
                                   const int32_t *row_first, const int64_t *start_idx, const int64_t *bos_idx, void *grad_src,
                                   void *grad_pad, void *workspace, int64_t B, int64_t L, int64_t C, int64_t n_images,
                                   int64_t max_len, int64_t seq_len, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The text loss (csrc/mmfs_text_loss.hip; additive at ABI 14).  Replaces the last statement of the training step
 * (mm_interleaved/models/mm_interleaved.py:449-476: a cast of the logits to fp32, "b n c -> b c n", a sliced copy and
 * F.cross_entropy, and the same passes backwards) by one read of the logits forward and one read and one write backward.  No
 * entry reads anything back, allocates or synchronises: all of them can be captured into a graph.  T is the storage type
 * ``dtype`` (MMFS_F32 / MMFS_F16 / MMFS_BF16) of logits [B, L, V] and grad [B, L, V]; 1 <= V <= 2^24, any V: a row need not be a
 * whole number of 16-byte vectors (mmfs_text_loss_supported; otherwise MMFS_E_UNSUPPORTED and the caller keeps the framework's
 * statement).  Arithmetic is fp32 from the stored logits.
 *
 * Row (b, first + j), j < n, is scored against labels [B, n] int64; first + n <= L.  A label equal to ``ignore_index`` is
 * ignored; a label outside [0, V) that is not ``ignore_index`` is OUT OF RANGE: its row counts as ignored, nothing is read
 * through it, and it is counted.  ``reduction``: MMFS_TEXT_LOSS_NONE / _SUM / _MEAN.
 * mmfs_text_loss_forward: two launches.
 *   lse  [B, n] fp32     log sum_i exp(logits[b, first + j, i]) of a valid row, 0 of any other row (which is not read)
 *   loss [B, n] fp32     lse - logits[b, first + j, label] of a valid row, 0 of any other row
 *   out  [1]    fp32     the sum of loss in a fixed order (_SUM), divided by the number of valid rows (_MEAN: NaN when there is
 *                        none); not written and may be NULL for _NONE
 *   counts [2]  int32    valid rows, out-of-range rows
 * mmfs_text_loss_backward: one launch; EVERY element of grad is written.  A valid row:
 *     grad[b, first + j, i] = round_T((exp(logits[b, first + j, i] - lse[b, j]) - (i == label)) * g)
 *   with g = upstream[b, j] (_NONE), upstream[0] (_SUM) or upstream[0] / counts[0] (_MEAN), all fp32 on the device; every other
 *   row, the rows outside [first, first + n) included, is zeros.  grad leaves with the non-temporal hint.
 * Errors come back before any launch: MMFS_E_DTYPE (an unknown code, MMFS_F64); MMFS_E_DIMS for a negative size, first + n > L,
 * B * L > 2^22 or V > 2^24; MMFS_E_UNSUPPORTED for V = 0 with rows to score or an unknown ``reduction``; MMFS_E_NULLPTR for
 * a NULL required pointer of a non-empty problem (``counts`` always; ``out`` unless _NONE); MMFS_E_ALIGN for logits or grad that
 * are not 16-byte aligned (the other tensors: their element size). */
enum mmfs_text_loss_reduction { MMFS_TEXT_LOSS_NONE = 0, MMFS_TEXT_LOSS_SUM = 1, MMFS_TEXT_LOSS_MEAN = 2 };
int mmfs_text_loss_supported(int dtype, int64_t V);
int mmfs_text_loss_forward(int dtype, const void *logits, const int64_t *labels, float *loss, float *lse, float *out,
                           int32_t *counts, int64_t B, int64_t L, int64_t V, int64_t first, int64_t n, int64_t ignore_index,
                           int reduction, void *stream);
int mmfs_text_loss_backward(int dtype, const void *logits, const int64_t *labels, const float *lse, const float *upstream,
                            const int32_t *counts, void *grad, int64_t B, int64_t L, int64_t V, int64_t first, int64_t n,
                            int64_t ignore_index, int reduction, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Q-Former attention with per-head q/k LayerNorm (csrc/mmfs_attn.hip; additive at ABI 14).  Replaces, between the three Linear
 * layers of the reference's patched Blip2QFormerMultiHeadAttention and its output
 * (mm_interleaved/models/utils/monkey_patch/blip2_qknorm_monkey_patch.py:76-147), the three permuted views, the LayerNorm over
 * the 64 channels of every head of q and of k, q k^T / 8 + mask, the softmax over a [B, H, Nq, Nk] tensor, p v and the permuted
 * copy back.  No entry reads anything back, allocates, clears or synchronises: all of them can be captured into a graph.
 *   q [B, Nq, H * 64], k, v [B, Nk, H * 64] of T (MMFS_F16 / MMFS_BF16), packed, as the Linear layers return them
 *   q_norm_weight, q_norm_bias, k_norm_weight, k_norm_bias [64] of ``norm_dtype`` (MMFS_F32 or ``dtype``) with ``eps``: all
 *       four or none (no normalisation)
 *   key_bias [B, Nk] (``bias_stride`` = Nk) or [Nk] shared by the batch (``bias_stride`` = 0) of ``bias_dtype`` (MMFS_F32 or
 *       ``dtype``), or NULL: added to the scaled scores (HF's extended mask [B, 1, 1, Nk]); not differentiated.  A bias at or
 *       below finfo(T).min marks a masked key: its score IS the bias, as the framework's sum in T leaves it
 * mmfs_qk_attn_supported: D == 64, 1 <= Nq <= 128, 1 <= Nk <= 8192, a 16-bit type; otherwise 0, the calls return
 * MMFS_E_UNSUPPORTED and the caller keeps the framework's statement (fp32 storage, other head widths, more queries).
 * mmfs_qk_attn_forward: one launch, B * H workgroups.
 *   context [B, Nq, H * 64] of T    softmax_k(q^ . k^ / 8 + key_bias) v, q^ / k^ the normalised rows rounded to T; every element
 *                                   written once.  Keys at finfo(T).min only: the uniform average; at -Inf only: NaN
 *   lse   [B, H, Nq]    fp32        log sum_k exp(score)
 *   stats [B, H, Nq, 2] fp32        (row maximum m, l = sum_k exp(score - m)): what the backward reads
 * mmfs_qk_attn_backward: one launch (two with the LayerNorms).  grad_q, grad_k, grad_v of T: every element written exactly once,
 *   no atomics: bit-reproducible.  partials [B * H, 4, 64] fp32 (workspace, every element written) and grad_params [4, 64] fp32 =
 *   d(q_norm_weight), d(q_norm_bias), d(k_norm_weight), d(k_norm_bias), summed over the workgroups in ascending order; both
 *   unused and may be NULL without the LayerNorms.
 * Errors come back before any launch: MMFS_E_DTYPE (an unknown code; a ``norm_dtype`` / ``bias_dtype`` of a given tensor that is
 * neither MMFS_F32 nor ``dtype``); MMFS_E_DIMS for a negative size, B * H > 2^24 or a ``bias_stride`` that is neither 0 nor Nk;
 * MMFS_E_UNSUPPORTED for what the query refuses; MMFS_E_NULLPTR for a NULL required pointer of a non-empty problem or some but
 * not all of the four LayerNorm pointers; MMFS_E_ALIGN for q, k, v, context and the gradients that are not 16-byte aligned
 * (the small tensors and the fp32 ones: their element size). */
int mmfs_qk_attn_supported(int dtype, int64_t D, int64_t Nq, int64_t Nk);
int mmfs_qk_attn_forward(int dtype, const void *q, const void *k, const void *v, const void *q_norm_weight,
                         const void *q_norm_bias, const void *k_norm_weight, const void *k_norm_bias, int norm_dtype, float eps,
                         const void *key_bias, int bias_dtype, int64_t bias_stride, void *context, float *lse, float *stats,
                         int64_t B, int64_t H, int64_t D, int64_t Nq, int64_t Nk, void *stream);
int mmfs_qk_attn_backward(int dtype, const void *q, const void *k, const void *v, const void *q_norm_weight,
                          const void *q_norm_bias, const void *k_norm_weight, const void *k_norm_bias, int norm_dtype, float eps,
                          const void *key_bias, int bias_dtype, int64_t bias_stride, const void *context,
                          const void *grad_context, const float *stats, void *grad_q, void *grad_k, void *grad_v,
                          float *partials, float *grad_params, int64_t B, int64_t H, int64_t D, int64_t Nq, int64_t Nk,
                          void *stream);

/* ---------------------------------------------------------------------------------------------
 * LLaMA self-attention at decode (csrc/mmfs_llama_attn.hip; additive at ABI 14).  Replaces, between the three Linear layers of the
 * reference's LlamaAttention and its o_proj (mm_interleaved/models/decoders/modeling_llama_mmfs.py:217-280), the rotary embedding
 * (:165-172), the torch.cat that grows the cache (:241-242), the [B, H, 1, T] scores, their clamp, softmax and second product
 * (:246-264), and under beam search the index_select of the whole cache (:913-917).  No entry reads anything back, allocates,
 * clears or synchronises: all of them can be captured into a graph.
 *   k_cache, v_cache [B, H, cap, 128] of T (MMFS_F16 / MMFS_BF16): one layer's keys (rotated) and values, written in place
 *   length   [1] int32      device word: the tokens the cache holds, the same for every row; the CALLER adds to it after the last
 *                           layer of a step (the entries read it, none writes it)
 *   src_row  [B, cap] int32 the physical batch row that holds logical row b's token t: the append writes b; a beam reorder
 *                           permutes its rows (B * cap ints) in place of the cache
 * mmfs_llama_attn_supported: D == 128, a 16-bit type, 1 <= Lq <= cap <= 2^22; otherwise 0, the calls return MMFS_E_UNSUPPORTED
 * and the caller keeps the framework's statement.
 * mmfs_llama_attn_rope_append: one launch.  q, k, v [B, Lq, H * 128] of T, packed, as the Linear layers return them; position_ids
 *   [B, Lq] int64; cos_table, sin_table [max_pos, 64] fp32 (host-made, as FixedLlamaRotaryEmbedding makes them).
 *   q_rot [B, Lq, H * 128] = q cos + rotate_half(q) sin (channel pairs (i, i + 64), fp32, one rounding); the same of k and v as it
 *   is go to slots length + j, j < Lq, of physical row b, and src_row[b, length + j] = b.  A position outside [0, max_pos) reads no
 *   table entry and makes that token's q and k NaN.  The caller guarantees length + Lq <= cap; a slot outside the cache is not
 *   written.
 * mmfs_llama_attn_decode: Lq = 1, two launches (the split walk of the keys, the merge of its partials in ascending order).
 *   context [B, 1, H * 128] of T = softmax_t(q_rot . K[src_row[b, t], h, t] / sqrt(128) + bias[b, t]) V over the keys
 *   t < length + 1 (the slot the append of this step wrote included).
 *   bias [B, bias_len] with rows ``bias_stride`` apart, or one shared row (``bias_stride`` = 0), of ``bias_dtype`` (MMFS_F32 or
 *       ``dtype``), or NULL: HF's extended mask [B, 1, 1, kv_len] without its broadcast axes; keys at or behind bias_len have
 *       none.  A bias at or below finfo(T).min marks a masked key: its score IS the bias, as the reference's sum and clamp in T
 *       leave it; keys that are all masked give the uniform average of their values
 *   kv_bound  a HOST upper bound of length + 1, <= cap: the grid is cut from it (256 keys a workgroup), never from the device
 *       word, and workgroups behind the length return at once, so a step captured at one length replays at any later length
 *       up to kv_bound.  Results do not depend on it.  A length + 1 outside [1, kv_bound] gives NaN
 *   workspace  mmfs_llama_attn_decode_workspace_bytes(B, H, kv_bound) bytes (< 0: MMFS_E_DIMS), 16-byte aligned: the partials;
 *       nothing in it needs clearing
 *   No atomics: bit-reproducible, eager or replayed.
 * Errors come back before any launch: MMFS_E_DTYPE (an unknown code; a ``bias_dtype`` of a given bias that is neither MMFS_F32 nor
 * ``dtype``); MMFS_E_DIMS for a negative size, B * H > 2^24, kv_bound outside [1, cap], a bias_stride that is neither 0 nor at
 * least bias_len; MMFS_E_UNSUPPORTED for what the query refuses; MMFS_E_NULLPTR for a NULL required pointer of a non-empty
 * problem; MMFS_E_ALIGN for q, k, v, q_rot, the caches, the tables, context and the workspace that are not 16-byte aligned
 * (position_ids, length, src_row and the bias: their element size). */
int mmfs_llama_attn_supported(int dtype, int64_t D, int64_t Lq, int64_t cap);
int mmfs_llama_attn_rope_append(int dtype, const void *q, const void *k, const void *v, const int64_t *position_ids,
                                const float *cos_table, const float *sin_table, int64_t max_pos, const int32_t *length,
                                void *q_rot, void *k_cache, void *v_cache, int32_t *src_row, int64_t B, int64_t Lq, int64_t H,
                                int64_t D, int64_t cap, void *stream);
/* the decode walk's cut of the keys, for callers and tests that want its edges: level 0 the keys of a wave, level 1 the keys of a
 * workgroup, which is a split; any other level MMFS_E_DIMS.  Host-only. */
int64_t mmfs_llama_attn_decode_keys(int level);
int64_t mmfs_llama_attn_decode_workspace_bytes(int64_t B, int64_t H, int64_t kv_bound);
int mmfs_llama_attn_decode(int dtype, const void *q_rot, const void *k_cache, const void *v_cache, const int32_t *src_row,
                           const int32_t *length, const void *bias, int bias_dtype, int64_t bias_stride, int64_t bias_len,
                           void *context, float *workspace, int64_t B, int64_t H, int64_t D, int64_t cap, int64_t kv_bound,
                           void *stream);

/* LLaMA self-attention over a prompt from the same cache (csrc/mmfs_llama_prefill.hip; additive at ABI 14): Lq new tokens a row,
 * one launch, after mmfs_llama_attn_rope_append has written their slots.  Reads the cache, src_row and length; writes context.
 *   context [B, Lq, H * 128] of T = softmax_t(q_rot[b, j] . K[src_row[b, t], h, t] / sqrt(128) + bias(b, j, t)) V over the keys
 *   t < length + Lq (``length``: the tokens held BEFORE the call; the grid comes from (B, H, Lq), the key walk's end from the
 *   device word).  Slots at or behind length + Lq never enter a product.
 *   bias  HF's extended mask read where it lies, of ``bias_dtype`` (MMFS_F32 or ``dtype``), or NULL: entry (b, j, t) lies at
 *       b * bias_batch_stride + j * bias_query_stride + t elements (a stride of 0: one shared batch row / one row for all
 *       queries); keys at or behind bias_len have none.  Only element-size alignment is assumed.
 *   flags MMFS_LLAMA_PREFILL_CAUSAL: key t is excluded for query j iff t > length + j (the reference's _make_causal_mask on top
 *       of the bias); MMFS_LLAMA_PREFILL_VISIT_ALL: no key tile is skipped (the results are the same bits; for tests).
 *   A key whose bias is at or below finfo(T).min, or which the causal flag excludes, has the score max(bias, finfo(T).min): the
 *   reference's clamp, which brings HF's finfo.min + finfo.min = -Inf entries of a left-padded prompt back, so a padded query row
 *   is the finite average of all values (mmfs_llama_attn_decode keeps a -Inf bias as it is).
 *   No atomics: bit-reproducible, eager or replayed.
 * mmfs_llama_attn_prefill_tiles: level 0 the query rows of a wave, 1 of a workgroup, 2 the keys of a tile; any other level
 *   MMFS_E_DIMS.  Host-only.
 * Errors come back before any launch, as mmfs_llama_attn_decode's; MMFS_E_DIMS also for unknown flag bits, a bias_query_stride
 * that is neither 0 nor at least bias_len, a bias_batch_stride that is neither 0 nor at least what a batch row's queries span
 * ((Lq - 1) * bias_query_stride + bias_len).  B * H == 0 returns 0. */
#define MMFS_LLAMA_PREFILL_CAUSAL 1u
#define MMFS_LLAMA_PREFILL_VISIT_ALL 2u
int mmfs_llama_attn_prefill(int dtype, const void *q_rot, const void *k_cache, const void *v_cache, const int32_t *src_row,
                            const int32_t *length, const void *bias, int bias_dtype, int64_t bias_batch_stride,
                            int64_t bias_query_stride, int64_t bias_len, unsigned flags, void *context, int64_t B, int64_t Lq,
                            int64_t H, int64_t D, int64_t cap, void *stream);
int64_t mmfs_llama_attn_prefill_tiles(int level);

/* LLaMA self-attention in training (csrc/mmfs_llama_train.hip; additive at ABI 14): what the reference's _forward_train
 * (models/utils/monkey_patch/llama_flash_attn_train_monkey_patch.py:35-82) asks of flash_attn_func(q, k, v, 0.0, None, causal=True),
 * forward and backward, with no tensor of size L x L.  No cache, no bias; the mask is causal, always: key t is live for query j
 * iff t <= j.  q, k, v, q_rot, k_rot, context, grad_context, grad_q, grad_k, grad_v [B, L, H * 128] of T (MMFS_F16 / MMFS_BF16),
 * packed, token-major; lse [B, H, L] fp32; position_ids [B, L] int64; cos_table, sin_table [max_pos, 64] fp32 as for
 * mmfs_llama_attn_rope_append.  No entry reads anything back, allocates, clears or synchronises; no atomics: bit-reproducible,
 * eager or replayed.  A masked score is selected, never added to: a NaN in token t's k or v reaches no query j < t.
 * mmfs_llama_attn_train_supported: D == 128, a 16-bit type, 1 <= L <= 2^22; otherwise 0 and the calls return MMFS_E_UNSUPPORTED.
 * mmfs_llama_attn_train_tiles: level 0 the query rows of a workgroup (forward, dq), 1 the keys of a forward tile, 2 the keys of
 *   a dkdv workgroup, 3 the queries of a dkdv tile, 4 the query rows of a wave; any other level MMFS_E_DIMS.  Host-only.
 * mmfs_llama_attn_train_workspace_bytes: what the backward's ``workspace`` (16-byte aligned, nothing to clear) holds: delta
 *   [B, H, L] fp32; < 0: MMFS_E_DIMS.  Host-only.
 * mmfs_llama_attn_train_rope: one launch.  q_rot = q cos + rotate_half(q) sin, k_rot alike (fp32, one rounding); a position outside
 *   [0, max_pos) makes that token's q_rot and k_rot NaN.
 * mmfs_llama_attn_train_forward: one launch.  context = softmax_t(q_rot[b, j] . k_rot[b, t] / sqrt(128)) v over t <= j, P rounded
 *   to T before the second product; lse = ln sum_t exp(score).
 * mmfs_llama_attn_train_backward: two launches (dq, which also writes delta = rowsum(grad_context * context) to the workspace;
 *   then dk and dv).  Both recompute P = exp(score - lse).  grad_q and grad_k are the gradients of the UNROTATED q and k: the
 *   inverse rotation runs on the fp32 sums, one rounding.
 * Errors come back before any launch: MMFS_E_DTYPE (an unknown code); MMFS_E_DIMS for a negative size, B * H > 2^24, a max_pos
 * outside [0, 2^40]; MMFS_E_UNSUPPORTED for what the query refuses (an empty L is not refused); then 0 for an empty problem (B, H
 * or L of 0); MMFS_E_NULLPTR for a NULL required pointer; MMFS_E_ALIGN for tensors, tables and the workspace that are not 16-byte
 * aligned (position_ids: 8, lse: 4). */
int mmfs_llama_attn_train_supported(int dtype, int64_t D, int64_t L);
int64_t mmfs_llama_attn_train_tiles(int level);
int64_t mmfs_llama_attn_train_workspace_bytes(int64_t B, int64_t H, int64_t L);
int mmfs_llama_attn_train_rope(int dtype, const void *q, const void *k, const int64_t *position_ids, const float *cos_table,
                               const float *sin_table, int64_t max_pos, void *q_rot, void *k_rot, int64_t B, int64_t L,
                               int64_t H, int64_t D, void *stream);
int mmfs_llama_attn_train_forward(int dtype, const void *q_rot, const void *k_rot, const void *v, void *context, float *lse,
                                  int64_t B, int64_t L, int64_t H, int64_t D, void *stream);
int mmfs_llama_attn_train_backward(int dtype, const void *q_rot, const void *k_rot, const void *v, const void *context,
                                   const void *grad_context, const float *lse, const int64_t *position_ids,
                                   const float *cos_table, const float *sin_table, int64_t max_pos, void *grad_q, void *grad_k,
                                   void *grad_v, float *workspace, int64_t B, int64_t L, int64_t H, int64_t D, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-image feature bank: MMFS's ``input_flatten`` built in one pass.
 * Replaces the Python loops of mm_interleaved/models/mm_interleaved.py:223-250 (zero-filled
 * [B, n, C, h, w] buffers per level, per-sequence slice copies, "b n c h w -> b n (h w) c", concatenation
 * over levels) and the rearrange + concatenation of decoders/sd_mmfs.py:241-245.
 *   level_ptrs [n_levels]  HOST array of DEVICE pointers: level l is [n_img, C, hw_l] (channel-major,
 *                          contiguous), storage dtype;   level_hw [n_levels]  HOST array: hw_l = h_l * w_l
 *   src_index  [n_slots]   device int64: the image a bank slot shows; < 0 or >= n_img -> a zero slot
 *   bank       [n_slots, sum_l hw_l, C]   token-major, levels in list order, fully written
 * mmfs_bank_scatter is the adjoint (needed when the image encoder is trained):
 *   grad_level_ptrs[l] [n_img, C, hw_l] = sum over the slots s with src_index[s] == image of
 *   grad_bank[s] (fp32 accumulation, slots in ascending order, rounded once); fully written, images
 *   no slot shows get zeros.  No atomics: bit-reproducible.
 * Limits: n_levels <= 8, n_slots <= 65535 (gather) / n_img <= 65535 (scatter); dtypes f32, f16, bf16.
 */
int mmfs_bank_gather(int dtype, int n_levels, const void *const *level_ptrs, const int64_t *level_hw,
                     const int64_t *src_index, void *bank, int64_t n_img, int64_t C, int64_t n_slots,
                     void *stream);
int mmfs_bank_scatter(int dtype, int n_levels, void *const *grad_level_ptrs, const int64_t *level_hw,
                      const int64_t *src_index, const void *grad_bank, int64_t n_img, int64_t C,
                      int64_t n_slots, void *stream);

/*
 * RMS normalisation of the LLM-side block (``LlamaRMSNorm``, mm_interleaved/models/decoders/modeling_llama_mmfs.py:53-70,
 * applied at :352-353 to the token stream and to the feature bank), one pass each way instead of the reference's
 * chain of seven framework kernels.  x, y, grad_y, grad_x: [rows, C] contiguous, ``weight`` [C], all of storage type
 * ``dtype`` (MMFS_F32 / MMFS_F16 / MMFS_BF16), 16-byte aligned; ``rstd`` [rows] fp32 (forward: written when not
 * NULL; backward: read).  y = weight * round(x * rsqrt(mean(x^2) + eps)), the rounding to the storage type between
 * the two products exactly where the reference has its ``.to(weight.dtype)``.  Backward: ``grad_weight_f32`` [C] fp32
 * is ACCUMULATED into (atomics): zero it first; cast it to the storage type afterwards.
 * mmfs_rmsnorm_supported: C a multiple of the 16-byte vector and at most 1024 vectors (8192 channels of 16 bits).
 */
int mmfs_rmsnorm_supported(int dtype, int64_t C);
int mmfs_rmsnorm_forward(int dtype, const void *x, const void *weight, void *y, float *rstd,
                         int64_t rows, int64_t C, float eps, void *stream);
int mmfs_rmsnorm_backward(int dtype, const void *grad_y, const void *x, const void *weight, const float *rstd,
                          void *grad_x, float *grad_weight_f32, int64_t rows, int64_t C, void *stream);
/* The same backward without atomics: workgroup g leaves ITS sum of the gain gradient in row g of
 * ``grad_weight_partials`` [mmfs_rmsnorm_backward_partials_rows(rows), C] fp32 (every element written: no zeroing), and
 * the caller adds the rows up (one framework reduction).  2 M float atomics on C addresses from hundreds of workgroups on
 * 8 XCDs were 150 of mmfs_rmsnorm_backward's 180 us at 8192 x 4096; what the Python operator package calls. */
int mmfs_rmsnorm_backward_partials_rows(int64_t rows);
int mmfs_rmsnorm_backward_partials(int dtype, const void *grad_y, const void *x, const void *weight, const float *rstd,
                                   void *grad_x, float *grad_weight_partials, int64_t rows, int64_t C, void *stream);

/* ---- the two layout changes around the image decoder's synchronizer block (csrc/mmfs_query.hip) ----------------------
 * MMFSBlock (mm_interleaved/models/decoders/sd_mmfs.py:121-146) gets a UNet residual [B, C, H, W] and works on tokens:
 *   mmfs_query_prep:  q[b, p, :] = round(LayerNorm_C(x[b, :, p]) * gamma + beta) + pos[p, :]      (sd_mmfs.py:124-131)
 *                     x [B, C, HW] -> q [B, HW, C]; statistics in fp32; ``pos`` [HW, C] may be NULL (no second term);
 *                     ``mean`` / ``rstd`` [B * HW] fp32, both or neither: what a LayerNorm backward needs.
 *   mmfs_tokens_add:  y[b, c, p] = round(tok[b, p, c] + res[b, c, p])     (the rearrange back + the caller's residual add,
 *                     sd_mmfs.py:146, 262-270); tok [B, HW, C], res and y [B, C, HW].
 * One read of the input and one write of the output each (a transposing tile in LDS) instead of a copy, a normalisation
 * and two adds.  16-bit storage types, C % 8 == 0, C <= 2048, HW % 8 == 0 (mmfs_query_prep_supported); else
 * MMFS_E_UNSUPPORTED and the caller keeps the framework's kernels. */
int mmfs_query_prep_supported(int dtype, int64_t C, int64_t HW);
int mmfs_query_prep(int dtype, const void *x, const void *gamma, const void *beta, const void *pos, void *q,
                    float *mean, float *rstd, int64_t B, int64_t C, int64_t HW, float eps, void *stream);
int mmfs_tokens_add(int dtype, const void *tok, const void *res, void *y, int64_t B, int64_t C, int64_t HW, void *stream);

/* ---- a Linear layer for a handful of tokens (csrc/mmfs_linear.hip) -----------------------------------------------------
 * y[m, :] = x[m, :] W^T + bias for M <= 8 token rows -- what an MMFS layer's Linear layers (mmfs.py:174-176, 274) are in a
 * decode step: each weight row is read once and meets M activations.  x [M, K] with rows ``ldx`` elements apart, W [N, K]
 * packed (nn.Linear's layout), bias [N] or NULL, y [M, N] with rows ``ldy`` apart; fp32 accumulation, bias added in fp32,
 * one rounding to the storage type.  16-bit storage types, K % 8 == 0, M * K * 2 bytes <= 64 KB (rounded up to 4 or 8
 * rows); else MMFS_E_UNSUPPORTED (mmfs_linear_small_supported) and the caller keeps its BLAS call. */
int mmfs_linear_small_supported(int dtype, int64_t M, int64_t N, int64_t K);
int mmfs_linear_small(int dtype, const void *x, const void *weight, const void *bias, void *y,
                      int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldy, void *stream);
/* The same followed by ``+ residual`` [M, N] (rows ``ldr`` apart; NULL = mmfs_linear_small): the decoder layer's
 * ``hidden_states = residual + hidden_states`` (modeling_llama_mmfs.py:700-717) in the projection's store -- the result is
 * rounded to the storage type, THEN added and rounded again: the bits of the framework's two kernels. */
int mmfs_linear_small_add(int dtype, const void *x, const void *weight, const void *bias, const void *residual, void *y,
                          int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldy, int64_t ldr, void *stream);

/* ---- the library's environment knobs (csrc/msda_env.h) --------------------------------------------------------------------
 * Every MMFS_* variable the library reads is a tuning / test hook (which formulation runs, how a launch is cut; none changes a
 * result).  They are ONE table, read once at the first use; no launch path calls getenv().  (The reference has no counterpart:
 * its extension reads no environment, ops/src/vision.cpp:14-15.)
 *   mmfs_env_reload: read the environment again (a test that flips a knob inside one process says so).
 *   mmfs_env_knob:   entry ``index`` of the table (0 ... until MMFS_E_DIMS): its name, one line of documentation, and the value
 *                    the library holds for it (NULL: unset).  Any of the three pointers may be NULL. */
void mmfs_env_reload(void);
int mmfs_env_knob(int index, const char **name, const char **doc, const char **value);

#ifdef __cplusplus
}
#endif
#endif /* MMFS_MSDA_H_ */
