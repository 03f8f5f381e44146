// mmfs_llama_attn.hip -- the LLM's self-attention at decode: between the three Linear layers of the
// reference's LlamaAttention and its o_proj (mm_interleaved/models/decoders/modeling_llama_mmfs.py:217-280), the rotary
// embedding (:165-172), the growth of the key / value cache (:241-242) and softmax(q K^T / sqrt(128) + mask) V (:246-264),
// on a cache that is written in place and, under beam search, re-indexed instead of copied (:913-917).
//
// Cache of a layer: K and V [B, H, cap, 128] of T (bf16 / fp16): the keys of one (row, head) are one stream of 256-byte
// rows.  Per cache (all layers share them): ``length``, one device int32 -- the tokens already held, the same for every
// row -- and ``src_row`` [B, cap] int32: the PHYSICAL batch row that holds logical row b's token t.  Arithmetic is fp32.
//
//   llama_rope_append   q, k, v [B, Lq, H 128] as the Linear layers return them, position_ids [B, Lq] int64, cos / sin
//                       [max_pos, 64] fp32 (made on the host as the reference makes them: no trigonometry here).  8 lanes a
//                       (token, head): a lane holds channels 8 i .. 8 i + 7 and their partners 64 further on, six 16-byte
//                       loads of q / k / v and four of the table:
//                           out[c] = x[c] cos[c] - x[c + 64] sin[c],   out[c + 64] = x[c + 64] cos[c] + x[c] sin[c]
//                       (x cos + rotate_half(x) sin), fp32, rounded to T once.  q goes to q_rot [B, Lq, H 128]; k (rotated)
//                       and v (as it is) go to slot length + j of physical row b, and src_row[b, length + j] = b.  A position
//                       outside [0, max_pos) reads no table entry: that token's q and k are NaN.  ``length`` is read from
//                       the device word; a slot outside [0, cap) is not written (the host refuses it from its mirror).
//   llama_attn_decode   Lq = 1.  Grid (B H, splits): workgroup (bh, s) of 8 waves owns keys [256 s, 256 s + 256), wave w
//                       the 32 of them from 32 w.  n = length + 1 keys are live (the append wrote slot ``length``; the
//                       cache advances after the last layer).  A workgroup behind n returns at once: the grid comes from a
//                       HOST bound of n, never from the device word, so a captured step replays at any later length up
//                       to that bound.  A key row is 16 lanes x 16 bytes; one load instruction fetches 4 rows.  A wave
//                       requests its 8 K loads and 8 V loads (16 KB) straight to VGPRs, nothing through LDS, with no
//                       branch round any of them (how many are in flight together: "Resources" below); src_row and the bias of its 32 keys are one coalesced load each, handed round by
//                       lane shuffles.  score = q . k / sqrt(128) + bias, or the bias itself at a masked key (below);
//                       m = max, p = exp(score - m), l = sum p, o = sum p v: sums over 16 lanes by shuffles, in a fixed
//                       order.  The eight waves meet in LDS in ascending order and the workgroup leaves one partial
//                       (m, l, o[128]) in fp32.
//   llama_attn_merge    16 lanes a (b, h), 8 channels a lane: the live partials in ascending order,
//                           M = max m_j,  L = sum l_j exp(m_j - M),  context = sum o_j exp(m_j - M) / L   -> T, one rounding.
//                       n < 1 or n above the host bound (keys nobody visited) gives NaN, so the error shows.
// No atomics, no flags between workgroups, no host read-back, nothing allocated, no memset node: the three launches can
// be captured, and every sum has a fixed order that depends on n alone (not on the grid): results are bit-reproducible,
// eager or replayed.
//
// Masked keys, the rule of mmfs_attn_core.h's score_of: ``bias`` ([B, kv_len] or one shared row, fp32 or T, read where it
// lies) is HF's extended mask without its broadcast axes; a bias at or below finfo(T).min IS the key's score -- what the
// reference's ``+ mask`` followed by ``max(., finfo.min)`` leaves in T.  Keys that are all masked give the uniform average
// of v, as the reference does; a row of -Inf biases gives NaN, as softmax(-Inf ..) does.  Where fp16 parts from this
// (a masked key whose product is at or above 16) is said there.  In bf16 finfo.min absorbs every fp32 score.
//
// Resources (make asm, gfx950; no spills, no scratch):
//                               VGPRs  AGPRs  LDS bytes  waves / SIMD
//   llama_rope_append  bf16      60     0      0          8
//   llama_rope_append  fp16      60     0      0          8
//   llama_attn_decode  bf16      93     0      4160       4
//   llama_attn_decode  fp16      92     0      4160       4
//   llama_attn_merge   bf16      30     0      0          8
//   llama_attn_merge   fp16      30     0      0          8
// The decode kernel asks for 4 waves per SIMD (amdgpu_waves_per_eu; two workgroups a CU).  What the compiler makes of the 16
// row loads (make asm): the fp16 build requests all 16 and then waits for them one by one; the bf16 build -- the measured
// type -- requests the q row and 10 rows, waits for all of them (vmcnt(0)), computes the scores it can, and only then
// requests the last 6 rows (V rows): 10 KB, then 6 KB in flight a wave, 16 waves a CU.  A scheduling barrier behind the loads
// (__builtin_amdgcn_sched_barrier(0): all 16 rows requested first in both builds, 112 / 106 VGPRs) was built and measured:
// 38.0 against 36.5 us replayed at B H = 128 and 2048 keys, 130.4 against 130.1 at B H = 640 -- no gain, so the compiler's
// schedule stays.  Against the first build (4 waves of 64 keys, 162 VGPRs, 2 waves per SIMD): the same at B H = 640,
// 39 -> 35 us per layer-step at B H = 128 and 2048 keys (profiles/llama_attn.md).
//
// Error bounds (tests/llama_attn_refs.py evaluates them element by element; the GPU tests hold the kernels AND the
// framework route in T to them against fp64 on the same stored inputs: a bound the reference's own statement misses is a
// wrong bound, so each counts the roundings of whichever route rounds more).  u = T's unit roundoff, half the spacing of its numbers
// at 1 (2^-8 bf16, 2^-11 fp16), t = T's smallest normal, e = 2^-24.
//   rope     r = x c - y s exactly (c, s the fp32 table entries), A = |x c| + |y s|.  The framework rounds c and s to T,
//            each product and the sum: (2 u + 3 u^2) A + u |r|.  Here: two fp32 products and a sum, one rounding: 4 e A + u |r|.
//                E_rope = (2 u + 3 u^2 + 4 e) A + u |r| + t;     NaN exactly where the position is outside the table
//            v and src_row are copies: bit-equal.
//   s        s0 = q . k / sqrt(128) on the STORED q_rot and K,  s = s0 + bias,  A = |q| . |k| / sqrt(128).  The framework rounds
//            q / sqrt(128) to T (the factor is no power of two), the product and the sum with the mask:
//            (u + 2 u^2) A + u |s0| + u |s|, and |s| <= |s0| + |bias|.  128 fp32 accumulations, the scaling and the bias in
//            either route: c_n e (A + |s0| + |bias|), c_n = 160.
//                E_s = (u + 2 u^2) A + 2 u |s0| + u |bias| + c_n e (A + |s0| + |bias|)
//                      [+ (E_q . |k| + |q| . E_k) / sqrt(128) when q and K are themselves known to E_q, E_k only: the module
//                      against the reference's fp64 tensors];   0 at a masked key (its score is the bias)
//   p        |dp_k| <= p_k (E_s,k + sum_j p_j E_s,j); v_exp_f32 with the product by log2 e, the sums over n keys in three
//            levels (lanes, waves, splits) and the rescaling of the partials: c_e e, c_e = 256 + n.  The framework rounds its
//            fp32 softmax to T: u.
//                E_p = p (E_s + sum_j p_j E_s,j + u + c_e e)
//   context  |context - ref| <= E_p |v| + c_e e p |v| + 2 u |ref| + t     (to T; the framework rounds p v once more)
//   Measured worst ratios |got - ref| / bound are kept in profiles/llama_attn.md.
//
// Offsets are 64-bit.
#include "mmfs_attn_core.h"
#include <hip/hip_runtime.h>

namespace mmfs {

namespace {

using namespace attn;

constexpr int kD = kLlamaD;             // channels of a head
constexpr int kHalf = 64;               // a channel's rotary partner is kHalf further on
constexpr int kThreads = 256;          // llama_rope_append
constexpr int kWaves = 8;               // llama_attn_decode: waves of a workgroup
constexpr int kDecodeThreads = kWaves * 64;
constexpr int kWaveKeys = 32;           // keys of a wave: 8 loads of 4 rows
constexpr int kLoads = kWaveKeys / 4;
constexpr int kSplitKeys = kWaves * kWaveKeys;      // keys of a workgroup = of a split: 256
constexpr int kPartial = 4 + kD;        // floats of a partial: m, l, two unused, o[128] (16-byte rows)
constexpr int kMergeThreads = 128;      // 8 (b, h) pairs of 16 lanes

__device__ __forceinline__ void load8f(const float *p, float (&o)[8])
{
    const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
llama_rope_append(const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v, const int64_t *__restrict__ pos,
                  const float *__restrict__ cos_t, const float *__restrict__ sin_t, const int64_t max_pos,
                  const int32_t *__restrict__ length, T *__restrict__ q_rot, T *__restrict__ kc, T *__restrict__ vc,
                  int32_t *__restrict__ src_row, const int64_t total, const int Lq, const int H, const int64_t cap)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;         // ((b Lq + j) H + h) 8 + part
    if (i >= total) return;
    const int part = (int)(i & 7);
    const int64_t r = i >> 3, tok = r / H;
    const int h = (int)(r - tok * H);
    const int64_t b = tok / Lq;
    const int j = (int)(tok - b * Lq);
    const int64_t p = pos[tok];
    const bool ok = p >= 0 && p < max_pos;
    const int64_t in = r * kD + part * 8;
    float c[8], s[8], ql[8], qh[8], kl[8], kh[8];
    if (ok) {
        load8f(cos_t + p * kHalf + part * 8, c);
        load8f(sin_t + p * kHalf + part * 8, s);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) c[e] = s[e] = __builtin_nanf("");
    }
    load_vec<T, 8>(q + in, ql);
    load_vec<T, 8>(q + in + kHalf, qh);
    load_vec<T, 8>(k + in, kl);
    load_vec<T, 8>(k + in + kHalf, kh);
    const uint4 vl = *reinterpret_cast<const uint4 *>(v + in), vh = *reinterpret_cast<const uint4 *>(v + in + kHalf);
    float ol[8], oh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { ol[e] = ql[e] * c[e] - qh[e] * s[e]; oh[e] = qh[e] * c[e] + ql[e] * s[e]; }
    store_vec<T, 8, false>(q_rot + in, ol);
    store_vec<T, 8, false>(q_rot + in + kHalf, oh);
    const int64_t slot = (int64_t)length[0] + j;
    if (slot < 0 || slot >= cap) return;                                    // (the host refuses this from its mirror)
#pragma unroll
    for (int e = 0; e < 8; ++e) { ol[e] = kl[e] * c[e] - kh[e] * s[e]; oh[e] = kh[e] * c[e] + kl[e] * s[e]; }
    const int64_t out = ((b * H + h) * cap + slot) * kD + part * 8;
    store_vec<T, 8, false>(kc + out, ol);
    store_vec<T, 8, false>(kc + out + kHalf, oh);
    *reinterpret_cast<uint4 *>(vc + out) = vl;
    *reinterpret_cast<uint4 *>(vc + out + kHalf) = vh;
    if (h == 0 && part == 0) src_row[b * cap + slot] = (int32_t)b;
}

// the live keys: length + 1, at most the host's bound (llama_attn_merge reports a length beyond it)
__device__ __forceinline__ int live_keys(const int32_t *length, int kv_bound)
{
    const int64_t n = (int64_t)length[0] + 1;
    return (int)(n < 0 ? 0 : n > kv_bound ? kv_bound : n);
}

template <typename T>
__global__ void __launch_bounds__(kDecodeThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
llama_attn_decode(const T *__restrict__ q_rot, const T *__restrict__ kc, const T *__restrict__ vc,
                  const int32_t *__restrict__ src_row, const int32_t *__restrict__ length, const void *__restrict__ bias,
                  const int bias_f32, const int64_t bias_stride, const int bias_len, float *__restrict__ partials, const int B,
                  const int H, const int64_t cap, const int kv_bound)
{
    __shared__ __attribute__((aligned(16))) float sO[kWaves][kD];
    __shared__ float sM[kWaves], sL[kWaves];
    const int n = live_keys(length, kv_bound);
    const int split = blockIdx.y, k0 = split * kSplitKeys;
    if (k0 >= n) return;                                                    // (workgroup-uniform)
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int w0 = k0 + wave * kWaveKeys;

    float m = -INFINITY, l = 0.f, o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
    if (w0 < n) {                                                           // (wave-uniform)
        // this lane's key of the wave's (lanes 0 .. 31): its physical row and its bias, handed round below
        const int mine = w0 + lane;
        int row_l = 0;
        float bias_l = 0.f;
        if (mine < n && lane < kWaveKeys) {
            row_l = src_row[(int64_t)b * cap + mine];
            if (bias && mine < bias_len) {
                const int64_t at = (int64_t)b * bias_stride + mine;
                bias_l = bias_f32 ? static_cast<const float *>(bias)[at] : to_f32(static_cast<const T *>(bias)[at]);
            }
            if ((unsigned)row_l >= (unsigned)B) {                           // a slot nobody wrote: never dereferenced,
                row_l = 0;                                                  // and its NaN score shows the error
                bias_l = __builtin_nanf("");
            }
        }
        // a key behind n reads the row of key n - 1 again (no branch round a load: all 32 are in flight together) and gets p = 0
        const T *kb = kc + (int64_t)h * cap * kD + c * 8;                   // row 0, head h, this lane's channels
        const T *vb = vc + (int64_t)h * cap * kD + c * 8;
        const int64_t row_stride = (int64_t)H * cap * kD;
        uint4 kr[kLoads], vr[kLoads];
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            const int t = min(w0 + 4 * i + g, n - 1);
            const int64_t at = __shfl(row_l, t - w0, 64) * row_stride + (int64_t)t * kD;
            kr[i] = *reinterpret_cast<const uint4 *>(kb + at);
            vr[i] = *reinterpret_cast<const uint4 *>(vb + at);
        }
        float qf[8];
        load_vec<T, 8>(q_rot + (int64_t)bh * kD + c * 8, qf);
        float s[kLoads];
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            float kf[8];
            Vec16<T>::unpack(kr[i], kf);
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) d += qf[e] * kf[e];
            d = group_add<16>(d);
            const float bs = __shfl(bias_l, 4 * i + g, 64);
            s[i] = w0 + 4 * i + g < n ? score_of<T, kD>(d, bs) : -INFINITY;
            m = fmaxf(m, s[i]);
        }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        const float base = m == -INFINITY ? 0.f : m;
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            const float p = exp_hw(s[i] - base);
            l += p;
            float vf[8];
            Vec16<T>::unpack(vr[i], vf);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] += p * vf[e];
        }
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            o[e] += __shfl_xor(o[e], 16, 64);
            o[e] += __shfl_xor(o[e], 32, 64);
        }
    }
    if (g == 0) {
        *reinterpret_cast<float4 *>(&sO[wave][c * 8]) = make_float4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<float4 *>(&sO[wave][c * 8 + 4]) = make_float4(o[4], o[5], o[6], o[7]);
    }
    if (lane == 0) { sM[wave] = m; sL[wave] = l; }
    __syncthreads();
    if (tid < kD) {
        // the waves in ascending order (a wave behind n holds (-Inf, 0, 0))
        float M = sM[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) M = fmaxf(M, sM[w]);
        const float base = M == -INFINITY ? 0.f : M;
        float L = 0.f, O = 0.f;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const float a = exp_hw(sM[w] - base);
            L += sL[w] * a;
            O += sO[w][tid] * a;
        }
        float *P = partials + ((int64_t)bh * gridDim.y + split) * kPartial;
        if (tid == 0) { P[0] = M; P[1] = L; }
        P[4 + tid] = O;
    }
}

template <typename T>
__global__ void __launch_bounds__(kMergeThreads)
llama_attn_merge(const float *__restrict__ partials, const int32_t *__restrict__ length, T *__restrict__ ctx, const int BH,
                 const int splits, const int kv_bound)
{
    const int bh = blockIdx.x * (kMergeThreads / 16) + (threadIdx.x >> 4), c = threadIdx.x & 15;
    if (bh >= BH) return;
    const int64_t len1 = (int64_t)length[0] + 1;
    const int n = live_keys(length, kv_bound);
    const int ns = (n + kSplitKeys - 1) / kSplitKeys;                      // <= splits: the grid came from kv_bound
    const float *P = partials + (int64_t)bh * splits * kPartial;
    float M = -INFINITY;
    for (int j = 0; j < ns; ++j) M = fmaxf(M, P[(int64_t)j * kPartial]);
    const float base = M == -INFINITY ? 0.f : M;
    float L = 0.f, O[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) O[e] = 0.f;
    for (int j = 0; j < ns; ++j) {
        const float *Pj = P + (int64_t)j * kPartial;
        const float a = exp_hw(Pj[0] - base);
        L += Pj[1] * a;
        float oj[8];
        load8f(Pj + 4 + c * 8, oj);
#pragma unroll
        for (int e = 0; e < 8; ++e) O[e] += oj[e] * a;
    }
    const bool wrong = len1 < 1 || len1 > kv_bound;                         // keys nobody visited: the error must show
#pragma unroll
    for (int e = 0; e < 8; ++e) O[e] = wrong ? __builtin_nanf("") : O[e] / L;
    store_vec<T, 8, false>(ctx + (int64_t)bh * kD + c * 8, O);
}

int64_t splits_of(int64_t kv_bound) { return (kv_bound + kSplitKeys - 1) / kSplitKeys; }

}  // namespace
}  // namespace mmfs

extern "C" {

int mmfs_llama_attn_supported(int dtype, int64_t D, int64_t Lq, int64_t cap)
{
    return mmfs::attn::llama_supported(dtype, D, Lq, cap);
}

int mmfs_llama_attn_rope_append(int dtype, const void *q, const void *k, const void *v, const int64_t *position_ids,
                                const float *cos_table, const float *sin_table, int64_t max_pos, const int32_t *length,
                                void *q_rot, void *k_cache, void *v_cache, int32_t *src_row, int64_t B, int64_t Lq, int64_t H,
                                int64_t D, int64_t cap, void *stream)
{
    using namespace mmfs;
    const int rc = llama_check(dtype, B, H, D, Lq, cap);
    if (rc) return rc;
    if (max_pos < 0 || max_pos > (1LL << 40) || B * Lq > (1LL << 32) || B * Lq * H > (1LL << 34)) return MMFS_E_DIMS;
    if (B * H == 0) return MMFS_OK;
    const bool rope = max_pos != 0;
    if (const int rt = check_tensors({{q, 16}, {k, 16}, {v, 16}, {position_ids, 8}, {length, 4}, {q_rot, 16}, {k_cache, 16},
                                      {v_cache, 16}, {src_row, 4}, {cos_table, 16, rope}, {sin_table, 16, rope}}))
        return rt;
    const int64_t total = B * Lq * H * 8;
    return by_half_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(llama_rope_append<T>, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                           (hipStream_t)stream, (const T *)q, (const T *)k, (const T *)v, position_ids, cos_table, sin_table,
                           max_pos, length, (T *)q_rot, (T *)k_cache, (T *)v_cache, src_row, total, (int)Lq, (int)H, cap);
        return (int)hipGetLastError();
    });
}

int64_t mmfs_llama_attn_decode_keys(int level)
{
    return level == 0 ? mmfs::kWaveKeys : level == 1 ? mmfs::kSplitKeys : MMFS_E_DIMS;
}

int64_t mmfs_llama_attn_decode_workspace_bytes(int64_t B, int64_t H, int64_t kv_bound)
{
    using namespace mmfs;
    if (B < 0 || H < 0 || kv_bound < 1 || kv_bound > kLlamaMaxCap || B > (1 << 20) || H > (1 << 20) || B * H > (1 << 24))
        return MMFS_E_DIMS;
    return B * H * splits_of(kv_bound) * kPartial * (int64_t)sizeof(float);
}

int mmfs_llama_attn_decode(int dtype, const void *q_rot, const void *k_cache, const void *v_cache, const int32_t *src_row,
                           const int32_t *length, const void *bias, int bias_dtype, int64_t bias_stride, int64_t bias_len,
                           void *context, float *workspace, int64_t B, int64_t H, int64_t D, int64_t cap, int64_t kv_bound,
                           void *stream)
{
    using namespace mmfs;
    int rc = llama_check(dtype, B, H, D, 1, cap);
    if (rc) return rc;
    if (kv_bound < 1 || kv_bound > cap) return MMFS_E_DIMS;
    int bias_f32;
    rc = llama_bias(bias, bias_dtype, dtype, bias_len, bias_f32);
    if (rc) return rc;
    if (bias && ((bias_stride != 0 && bias_stride < bias_len) || bias_stride > kLlamaMaxCap)) return MMFS_E_DIMS;
    if (B * H == 0) return MMFS_OK;
    if ((rc = check_tensors({{q_rot, 16}, {k_cache, 16}, {v_cache, 16}, {src_row, 4}, {length, 4}, {context, 16}, {workspace, 16},
                             maybe(bias, bias_f32 ? 4 : 2)})))
        return rc;
    const int64_t splits = splits_of(kv_bound);
    return by_half_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(llama_attn_decode<T>, dim3((unsigned)(B * H), (unsigned)splits), dim3(kDecodeThreads), 0,
                           (hipStream_t)stream, (const T *)q_rot, (const T *)k_cache, (const T *)v_cache, src_row, length, bias,
                           bias_f32, bias_stride, (int)bias_len, workspace, (int)B, (int)H, cap, (int)kv_bound);
        const int e = (int)hipGetLastError();
        if (e) return e;
        const int per = kMergeThreads / 16;
        hipLaunchKernelGGL(llama_attn_merge<T>, dim3((unsigned)((B * H + per - 1) / per)), dim3(kMergeThreads), 0,
                           (hipStream_t)stream, workspace, length, (T *)context, (int)(B * H), (int)splits, (int)kv_bound);
        return (int)hipGetLastError();
    });
}

}  // extern "C"
