// mmfs_attn_core.h -- what the attention kernels share (mmfs_attn.hip: the Q-Former, D = 64; mmfs_llama_attn.hip: decode,
// mmfs_llama_prefill.hip: prefill, mmfs_llama_train.hip: training, D = 128; mmfs_clip_attn.hip: the CLIP ViT, D = 64;
// mmfs_text_loss.hip takes exp_hw alone): exp by the hardware's exp2, finfo(T).min
// and the masked-key rule, the fragment helpers of the 16x16x32 matrix products, and on the host side the checks that the
// LLaMA entries make alike.  The online-softmax tile step of qk_attn_fwd and llama_attn_prefill is NOT here: each kernel
// keeps its loop (profiles/attn_core.md says what a shared routine measured).  The two TRAINING attentions (mmfs_llama_train.hip,
// mmfs_clip_attn.hip) do share their three tile walks: mmfs_attn_train.h (attn_train_fwd, attn_train_dq, attn_train_dkdv), on
// top of this file.
#pragma once
#include "msda_host.h"
#include "msda_mma_common.h"
#include <math.h>

namespace mmfs {
namespace attn {

using mma::f32x4;
using mma::s16x4;
using mma::s16x8;

constexpr float kLog2e = 1.44269504088896340736f;

__device__ __forceinline__ float exp_hw(float d) { return __builtin_amdgcn_exp2f(d * kLog2e); }

// finfo(T).min, and a word of two NaNs of T
template <typename T> struct Lowest;
template <> struct Lowest<bf16_t> { static constexpr float value = -3.3895313892515355e38f; static constexpr uint32_t nan2 = 0x7fc07fc0u; };
template <> struct Lowest<half_t> { static constexpr float value = -65504.f; static constexpr uint32_t nan2 = 0x7e007e00u; };

// 1 / sqrt(D) for a head of D channels.  score_of takes D, not the factor: handed over as an argument, the factor gave the
// same bits but another compare / select order in every caller (profiles/attn_core.md)
template <int D> struct HeadScale;
template <> struct HeadScale<64> { static constexpr float value = 0.125f; };
template <> struct HeadScale<128> { static constexpr float value = 0.08838834764831845f; };

// A key whose bias is at or below finfo(T).min is a MASKED key and its score is the bias itself -- what the framework's sum
// in T leaves of score + finfo(T).min (bf16: fp32 absorbs the score as well; fp16: -65504 + score would not).
// Where the two part, in fp16: the framework's sum is -65504 only while |score| < 16 (half a unit of 65504); at
// score >= 16 it is -65472 (or above) while the key stays at -65504 here: a masked key 32 units above its masked
// neighbours, visible only in a row whose keys are all masked.  At score <= -16 the sum rounds to -Inf.  The Q-Former's
// statement has no clamp: the key is excluded there and a row of such keys is NaN -- out of reach with qk-norm at any sane
// scale (|q^ . k^| / 8 of a few units), reachable without it.  The LLaMA statement has the reference's max(., finfo.min),
// which brings the sum BACK to -65504, so only score >= 16 parts.
template <typename T, int D> __device__ __forceinline__ float score_of(float dot, float bias)
{
    return bias <= Lowest<T>::value ? bias : dot * HeadScale<D>::value + bias;
}

__device__ __forceinline__ s16x8 lds8(const uint16_t *p) { return *reinterpret_cast<const s16x8 *>(p); }

// elements 0..3 at p, 4..7 at p + 16: the k order of an accumulator pair used as the other operand
__device__ __forceinline__ s16x8 lds4x2(const uint16_t *p)
{
    const s16x4 a = *reinterpret_cast<const s16x4 *>(p), b = *reinterpret_cast<const s16x4 *>(p + 16);
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

// registers 0..3 of two accumulators, rounded to T: k-slots 0..3 and 4..7 of the lane's fragment
template <typename T> __device__ __forceinline__ s16x8 pack_pair(const float (&a)[4], const float (&b)[4])
{
    const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    const uint4 w = Vec16<T>::pack(v);
    return __builtin_bit_cast(s16x8, w);
}

template <typename T> __device__ __forceinline__ void store4(T *p, const float (&v)[4])
{
    uint2 w;
    w.x = Vec16<T>::pk(v[0], v[1]);
    w.y = Vec16<T>::pk(v[2], v[3]);
    *reinterpret_cast<uint2 *>(p) = w;
}

// ---- host side: what the entries check alike

// the type of a small fp32-or-T vector (LayerNorm parameters, a bias): 1 fp32, 0 T, < 0 neither (it is aligned to 4 or 2 bytes)
inline int small_f32(int small_dtype, int dtype) { return small_dtype == MMFS_F32 ? 1 : small_dtype == dtype ? 0 : -1; }

// what every attention entry asks of its dtype code, batch and heads; of its other dimensions (a, b, c) only the sign
inline int batch_heads_check(int dtype, int64_t B, int64_t H, int64_t a, int64_t b, int64_t c)
{
    if (dtype != MMFS_F32 && dtype != MMFS_F16 && dtype != MMFS_BF16 && dtype != MMFS_F64) return MMFS_E_DTYPE;
    if (B < 0 || H < 0 || a < 0 || b < 0 || c < 0) return MMFS_E_DIMS;
    if (B > (1 << 20) || H > (1 << 20) || B * H > (1 << 24)) return MMFS_E_DIMS;
    return MMFS_OK;
}

// the LLaMA entries (decode, prefill, the append): a cache [B, H, cap, 128], Lq new tokens a row
constexpr int kLlamaD = 128;
constexpr int64_t kLlamaMaxCap = 1 << 22;           // decode: splits <= 16384 (grid.y)

inline bool llama_supported(int dtype, int64_t D, int64_t Lq, int64_t cap)
{
    return (dtype == MMFS_F16 || dtype == MMFS_BF16) && D == kLlamaD && cap >= 1 && cap <= kLlamaMaxCap && Lq >= 1 && Lq <= cap;
}

inline int llama_check(int dtype, int64_t B, int64_t H, int64_t D, int64_t Lq, int64_t cap)
{
    if (const int rc = batch_heads_check(dtype, B, H, D, Lq, cap)) return rc;
    return llama_supported(dtype, D, Lq, cap) ? MMFS_OK : MMFS_E_UNSUPPORTED;
}

// the training entries (mmfs_llama_train.hip): no cache, L tokens a row; an empty problem (B, H or L of 0) is no error
constexpr int64_t kLlamaTrainMaxL = 1 << 22;

inline bool llama_train_supported(int dtype, int64_t D, int64_t L)
{
    return (dtype == MMFS_F16 || dtype == MMFS_BF16) && D == kLlamaD && L >= 1 && L <= kLlamaTrainMaxL;
}

inline int llama_train_check(int dtype, int64_t B, int64_t H, int64_t D, int64_t L)
{
    if (const int rc = batch_heads_check(dtype, B, H, D, L, 0)) return rc;
    return llama_train_supported(dtype, D, L ? L : 1) ? MMFS_OK : MMFS_E_UNSUPPORTED;
}

// the LLaMA entries' bias argument: -> status and the type flag (fp32 without a bias); the strides are the entry's own to judge
inline int llama_bias(const void *bias, int bias_dtype, int dtype, int64_t bias_len, int &bias_f32)
{
    bias_f32 = bias ? small_f32(bias_dtype, dtype) : 1;
    if (bias_f32 < 0) return MMFS_E_DTYPE;
    if (bias && (bias_len < 0 || bias_len > kLlamaMaxCap)) return MMFS_E_DIMS;
    return MMFS_OK;
}

// the CLIP ViT entries (mmfs_clip_attn.hip): plain self-attention, heads of 64 channels, L tokens a row; an empty problem
// (B, H or L of 0) is no error
constexpr int kClipD = 64;
constexpr int64_t kClipMaxL = 1 << 22;

inline bool clip_supported(int dtype, int64_t D, int64_t L)
{
    return (dtype == MMFS_F16 || dtype == MMFS_BF16) && D == kClipD && L >= 1 && L <= kClipMaxL;
}

inline int clip_check(int dtype, int64_t B, int64_t H, int64_t D, int64_t L)
{
    if (const int rc = batch_heads_check(dtype, B, H, D, L, 0)) return rc;
    return clip_supported(dtype, D, L ? L : 1) ? MMFS_OK : MMFS_E_UNSUPPORTED;
}

}  // namespace attn
}  // namespace mmfs
