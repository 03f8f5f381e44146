// mmfs_attn.hip -- the Q-Former's attention with a LayerNorm over the 64 channels of every head of q and of k
// (DESIGN.md 4.16): the statement of the reference's patched Blip2QFormerMultiHeadAttention
// (mm_interleaved/models/utils/monkey_patch/blip2_qknorm_monkey_patch.py:76-147) between its three Linear layers and
// its output, as one forward kernel and one backward kernel (+ a 256-lane sum of the LayerNorm parameter gradients).
//
// q [B, Nq, H 64], k, v [B, Nk, H 64] of T (bf16 / fp16) are read as the Linear layers return them: token-major, the
// heads side by side in a row; nothing is permuted.  Optional: the two LayerNorms' weight and bias [64] with eps, and a
// per-key additive bias [B, Nk] or [1, Nk] (HF's extended mask [B, 1, 1, Nk] without its broadcast axes); both of fp32 or
// of T, read as they lie: the module's parameters and mask need no cast, so a call is its kernels and nothing else.
// D = 64, 1 <= Nq <= 128, 1 <= Nk <= 8192.  Arithmetic is fp32; q^, k^ (the normalised rows), p and ds are rounded to T
// where they enter a matrix product (v_mfma_f32_16x16x32_{bf16,f16}), as the framework's LayerNorm and softmax hand
// them to its products.
//
//   qk_attn_fwd      one workgroup of 4 waves per (b, h).  q^ [Nq, 64] is staged once (LDS, row-major), then key tiles
//                    of 64: k^ row-major, v TRANSPOSED ([channel][key]).  A row is normalised as it is staged: 8 lanes a
//                    row, mean and centred variance in fp32.  Wave w owns the 16-query blocks w and w + 4.  It forms
//                    S^T = k^ q^T (key on the accumulator's rows, query on the lane: a lane holds 16 scores of ONE
//                    query), s = S / 8 + bias, and keeps one running pair (m, l) per lane:
//                        m' = max(m, tile max);  base = m' == -Inf ? 0 : m';  a = exp(m - base)
//                        p = exp(s - base);  l = l a + sum p;  O^T = O^T a + v^T p^T
//                    m starts at -Inf and l at 0, so the first tile's maximum IS the first maximum and exp(m - m) = 1
//                    exactly: keys that are all at finfo(T).min give p = 1 each, a uniform average, as the reference
//                    has it (a bias at or below finfo(T).min IS the key's score: score_of).  ``base`` keeps -Inf out of
//                    the subtractions: a tile whose keys are all at -Inf leaves (m, l, O) = (-Inf, 0, 0) or the pair it
//                    found, and a row of -Inf alone ends as 0 / 0 = NaN in every channel, as softmax(-Inf ..) v gives it.
//                    Keys behind Nk carry -Inf and zero v rows.
//                    The S^T accumulators ARE the B operand of O^T = v^T p^T (cdna_hip_programming.md 3, "An
//                    accumulator tile as the next MFMA's operand"): registers of two 16-key blocks, packed to T, are
//                    k-slots 8g + j of lane group g, and the A operand reads v^T at the same keys
//                    (32 ks + 4 g + j, 32 ks + 16 + 4 g + j - 4).  No trip through LDS.
//                    context [B, Nq, H 64] is written once, 4 channels a lane; lse = m + log l and the pair (m, l)
//                    ([B, H, Nq] and [B, H, Nq, 2], fp32) are kept.  The backward reads (m, l), not lse: next to
//                    m = finfo.min, log l is lost in the sum.
//   qk_attn_bwd      one workgroup per (b, h) walks the key tiles again.  Resident: q^ and dO row-major AND transposed,
//                    delta = rowsum(dO O), m, 1 / l.  Per tile: k^ row-major and transposed, v row-major.  Wave w owns
//                    the tile's 16-key block w: S = q^ k^T and dP = dO v^T with the QUERY on the rows and the key on
//                    the lane, p = exp(s - m) / l, ds = p (dP - delta); those accumulators are the B operands of
//                    dV^T = dO^T p and dK^^T = q^^T ds (sums over the query), which are complete when the tile is
//                    done: dv is stored, dk^ / 8 goes through the LayerNorm backward and is stored.  ds crosses LDS once
//                    ([query][key], T) for dQ^ += ds k^, query blocks w and w + 4 of wave w, held in registers for the
//                    whole walk; after it, dq^ / 8 goes through the LayerNorm backward and is stored.
//                        dx = rstd (g - mean(g) - x^ mean(g x^)),  g = dy gamma,  x^ = (x - mean) rstd  (fp32, from x)
//                    Every element of dq, dk, dv is written exactly once; no atomics, no clears.  The workgroup's
//                    d(gamma_q), d(beta_q), d(gamma_k), d(beta_k) go to partials [B H, 4, 64].
//   qk_attn_params   256 lanes: lane t adds partials[.., t] over the B H workgroups in ascending order: one serial chain
//                    of B H coalesced loads a lane -- 128 and 384 at the pipeline's shapes, a few microseconds; it grows
//                    linearly with B H (the entry allows up to 2^24), where a fixed-order tree would be the thing to build.
// All sums have a fixed order: results are bit-reproducible.  No host read-back, nothing allocated or cleared: the
// launches can be captured.
//
// Resources (make asm, gfx950; no spills, no scratch):
//                              VGPRs  AGPRs  LDS bytes  waves / SIMD
//   qk_attn_fwd  qk-norm        120    32     37120      3
//   qk_attn_fwd  plain          112    32     37120      3
//   qk_attn_bwd  qk-norm fp16   201    68     125184     1
//   qk_attn_bwd  qk-norm bf16   203    64     125184     1
//   qk_attn_bwd  plain   fp16   120    64     119552     1
//   qk_attn_bwd  plain   bf16   124    64     119552     1
//   qk_attn_params              5      0      0          8
// The backward's workgroup holds the whole query side of its (b, h) in LDS: one workgroup per CU, one wave per SIMD.
//
// Error bounds (tests/qk_attn_refs.py evaluates them element by element; the tests hold BOTH routes to them against fp64
// on the stored q, k, v: a bound the reference's own statement misses is a wrong bound, so where the framework's
// statement in T rounds more often than the kernels, the bound counts its roundings).  u = T's unit roundoff (2^-9 bf16,
// 2^-12 fp16), t = T's smallest normal, e = 2^-24.  First order; |x| of a matrix is taken element by element.
//   q^, k^   the fp32 LayerNorm, one rounding to T: relative u each (0 without qk-norm: the stored rows enter the product)
//   s        s0 = q^ . k^ / 8,  A = |q^| . |k^| / 8.  Rounded operands: 2 u A.  64 fp32 accumulations, the LayerNorms' fp32
//            arithmetic, the scaling and the bias: c_n e (A + |s0|), c_n = 96.  The framework rounds the product, the
//            quotient and the sum with the mask to T: 3 u |s0|.
//                E_s = 2 u A [qk-norm] + 3 u |s0| + c_n e (A + |s0|);   0 at a masked key (its score is the bias)
//   p        softmax: |dp_k| <= p_k (E_s,k + sum_j p_j E_s,j).  v_exp_f32 with the product by log2 e, (2.5 |s - m| + 2) e at
//            |s - m| <= 88, and the fp32 chains of the sums over Nq or Nk terms: c_e e, c_e = 256 + Nq + Nk.  To T: u.
//                E_p = p (E_s + sum_j p_j E_s,j + u + c_e e)
//   context  |context - ref| <= E_p |v| + c_e e p |v| + 2 u |ref| + t       (to T; the framework rounds p v once more)
//   lse      |lse - ref| <= sum_j p_j E_s,j + c_e e (1 + |lse|)             (the framework route has no lse)
//   delta    rowsum(dO O) from the rounded context (the framework: sum_k p dP from the rounded p and dP):
//                E_delta = sum_d |dO_d| W_d,   W = (E_p + (2 u + c_e e) p) |v| + t
//   ds       p (dP - delta); the framework rounds dP, ds and ds / 8 to T, the kernels ds once:
//                E_ds = E_p |dP - delta| + p (u |dP| + E_delta) + 3 u |ds|
//   dv       p^T dO:   |dv - ref| <= E_p^T |dO| + c_e e p^T |dO| + 2 u |ref| + t
//   dq^      ds k^ / 8 (dk^ = ds^T q^ / 8 alike):   G = (E_ds |k^| + (u [qk-norm] + c_e e) |ds| |k^|) / 8 + u |dq^|
//            without qk-norm that is dq:   |dq - ref| <= G + u |ref| + t
//   LayerNorm backward  dx = rstd (g - mean g - x^ mean(g x^)), g = dy gamma, dy known to G:
//                |dx - ref| <= rstd (|gamma| G + mean(|gamma| G) + |x^| mean(|gamma| G |x^|))
//                              + c_e e rstd (|g| + mean |g| + |x^| mean |g x^|) + 2 u |ref| + t
//                d(gamma) = sum_rows dy x^:  sum_rows G |x^| + c_e e sum_rows |dy x^| + 2 u |ref| + t;   d(beta): without x^
//   (d(beta_k) is 0 in exact arithmetic: a constant added to every key's score leaves the softmax alone.)
//   Measured worst ratios |got - ref| / bound are kept in profiles/qk_attn.md.
//
// Offsets are 64-bit.
#include "mmfs_attn_core.h"
#include <hip/hip_runtime.h>
#include <type_traits>

namespace mmfs {

namespace {

using namespace attn;

constexpr int kD = 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxNq = 128;
constexpr int kMaxNk = 8192;
constexpr int kKT = 64;                 // keys of a tile
constexpr int kLd = 72;                 // elements between rows of a row-major image [row][64 channels + 8]: 144 bytes
constexpr int kLdKt = 72;               // transposed key tile [channel][64 keys + 8]
constexpr int kLdQt = 136;              // transposed query-side image [channel][128 queries + 8]
constexpr float kScale = HeadScale<kD>::value;

// a small vector of fp32 or of T read by index (the LayerNorm parameters, the key bias); ``f32`` is uniform
template <typename T> struct Small {
    const void *p;
    int f32;
    __device__ __forceinline__ float operator[](int64_t i) const
    {
        return f32 ? static_cast<const float *>(p)[i] : to_f32(static_cast<const T *>(p)[i]);
    }
};

template <typename T> __device__ __forceinline__ uint16_t bits_of(float x) { return __builtin_bit_cast(uint16_t, (T)x); }

// rows [r0, r0 + R) of a head's slice src[row * ld + 0 .. 63] -> LDS, rounded to T: row-major (``rows``, stride kLd) and /
// or transposed (``trans`` [channel][row], stride tld).  8 lanes a row, 8 channels a lane; R * 8 is a multiple of the
// workgroup.  NORM: the per-head LayerNorm; rows at or behind N are zeros either way.  mean_out / rstd_out: [R] or null.
template <typename T, bool NORM>
__device__ __forceinline__ void stage_rows(const T *__restrict__ src, int64_t ld, int r0, int N, int R,
                                           const Small<T> gamma, const Small<T> beta, float eps,
                                           uint16_t *rows, uint16_t *trans, int tld, float *mean_out, float *rstd_out, int tid)
{
    for (int i = tid; i < R * 8; i += kThreads) {
        const int r = i >> 3, c0 = (i & 7) * 8;
        const bool live = r0 + r < N;
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = 0.f;
        if (live) load_vec<T, 8>(src + (int64_t)(r0 + r) * ld + c0, x);
        if constexpr (NORM) {
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) s += x[e];
            const float mean = group_add<8>(s) * (1.f / kD);
            float ss = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) { x[e] -= mean; ss += x[e] * x[e]; }
            const float rstd = 1.f / sqrtf(group_add<8>(ss) * (1.f / kD) + eps);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = live ? x[e] * rstd * gamma[c0 + e] + beta[c0 + e] : 0.f;
            if (mean_out && (i & 7) == 0) { mean_out[r] = mean; rstd_out[r] = rstd; }
        }
        const uint4 w = Vec16<T>::pack(x);
        if (rows) *reinterpret_cast<uint4 *>(rows + r * kLd + c0) = w;
        if (trans) {
            uint16_t hw[8];
            __builtin_memcpy(hw, &w, 16);
#pragma unroll
            for (int e = 0; e < 8; ++e) trans[(c0 + e) * tld + r] = hw[e];
        }
    }
}

template <typename T> __device__ __forceinline__ void load4(const T *p, float (&v)[4])
{
    T t[4];
    __builtin_memcpy(t, __builtin_assume_aligned(p, 8), 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = to_f32(t[e]);
}

template <typename T, bool NORM>
__global__ void __launch_bounds__(kThreads)
qk_attn_fwd(const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v, const void *__restrict__ qn_w_,
            const void *__restrict__ qn_b_, const void *__restrict__ kn_w_, const void *__restrict__ kn_b_, const int norm_f32,
            const float eps, const void *__restrict__ bias_, const int bias_f32, const int bias_stride, T *__restrict__ ctx,
            float *__restrict__ lse, float *__restrict__ stats, const int H, const int Nq, const int Nk)
{
    const Small<T> qn_w = {qn_w_, norm_f32}, qn_b = {qn_b_, norm_f32}, kn_w = {kn_w_, norm_f32}, kn_b = {kn_b_, norm_f32};
    const Small<T> bias = {bias_, bias_f32}, none = {nullptr, 1};
    __shared__ __attribute__((aligned(16))) uint16_t sQ[kMaxNq * kLd];
    __shared__ __attribute__((aligned(16))) uint16_t sK[kKT * kLd];
    __shared__ __attribute__((aligned(16))) uint16_t sVt[kD * kLdKt];
    __shared__ __attribute__((aligned(16))) float sBias[kKT];
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int64_t ld = (int64_t)H * kD;
    const T *qb = q + (int64_t)b * Nq * ld + h * kD;
    const T *kb = k + (int64_t)b * Nk * ld + h * kD;
    const T *vb = v + (int64_t)b * Nk * ld + h * kD;
    const int Rq = (Nq + 31) & ~31, nqb = (Nq + 15) >> 4;

    stage_rows<T, NORM>(qb, ld, 0, Nq, Rq, qn_w, qn_b, eps, sQ, nullptr, 0, nullptr, nullptr, tid);
    __syncthreads();

    s16x8 fq[2][2];
    float m[2], l[2];
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int blk = wave + kWaves * i;
        const int row = (blk < nqb ? blk : 0) * 16 + c;
#pragma unroll
        for (int st = 0; st < 2; ++st) fq[i][st] = lds8(sQ + row * kLd + 32 * st + 8 * g);
        m[i] = -INFINITY;
        l[i] = 0.f;
#pragma unroll
        for (int db = 0; db < 4; ++db) acc[i][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int k0 = 0; k0 < Nk; k0 += kKT) {
        stage_rows<T, NORM>(kb, ld, k0, Nk, kKT, kn_w, kn_b, eps, sK, nullptr, 0, nullptr, nullptr, tid);
        stage_rows<T, false>(vb, ld, k0, Nk, kKT, none, none, 0.f, nullptr, sVt, kLdKt, nullptr, nullptr, tid);
        if (tid < kKT) sBias[tid] = k0 + tid < Nk ? (bias.p ? bias[(int64_t)b * bias_stride + k0 + tid] : 0.f) : -INFINITY;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (wave + kWaves * i >= nqb) continue;                         // (wave-uniform)
            float s[4][4];
            float tm = -INFINITY;
#pragma unroll
            for (int kb16 = 0; kb16 < 4; ++kb16) {
                f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int st = 0; st < 2; ++st)
                    a = mma::FwdMma<T>::run(lds8(sK + (kb16 * 16 + c) * kLd + 32 * st + 8 * g), fq[i][st], a);
                const float4 bs = *reinterpret_cast<const float4 *>(sBias + kb16 * 16 + 4 * g);
                s[kb16][0] = score_of<T, kD>(a[0], bs.x); s[kb16][1] = score_of<T, kD>(a[1], bs.y);
                s[kb16][2] = score_of<T, kD>(a[2], bs.z); s[kb16][3] = score_of<T, kD>(a[3], bs.w);
#pragma unroll
                for (int r = 0; r < 4; ++r) tm = fmaxf(tm, s[kb16][r]);
            }
            tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
            tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
            const float mn = fmaxf(m[i], tm), base = mn == -INFINITY ? 0.f : mn;
            const float alpha = exp_hw(m[i] - base);
            float ps = 0.f;
#pragma unroll
            for (int kb16 = 0; kb16 < 4; ++kb16)
#pragma unroll
                for (int r = 0; r < 4; ++r) { s[kb16][r] = exp_hw(s[kb16][r] - base); ps += s[kb16][r]; }
            ps += __shfl_xor(ps, 16, 64);
            ps += __shfl_xor(ps, 32, 64);
            l[i] = l[i] * alpha + ps;
            m[i] = mn;
#pragma unroll
            for (int db = 0; db < 4; ++db) acc[i][db] *= alpha;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const s16x8 fp = pack_pair<T>(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
                for (int db = 0; db < 4; ++db)
                    acc[i][db] = mma::FwdMma<T>::run(lds4x2(sVt + (db * 16 + c) * kLdKt + 32 * ks + 4 * g), fp, acc[i][db]);
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int qi = (wave + kWaves * i) * 16 + c;
        if (qi >= Nq) continue;
        T *o = ctx + ((int64_t)b * Nq + qi) * ld + h * kD;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            const float out[4] = {acc[i][db][0] / l[i], acc[i][db][1] / l[i], acc[i][db][2] / l[i], acc[i][db][3] / l[i]};
            store4<T>(o + db * 16 + 4 * g, out);
        }
        if (g == 0) {
            const int64_t at = (int64_t)bh * Nq + qi;
            lse[at] = m[i] + logf(l[i]);
            stats[2 * at] = m[i];
            stats[2 * at + 1] = l[i];
        }
    }
}

template <typename T, bool NORM>
__global__ void __launch_bounds__(kThreads)
qk_attn_bwd(const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v, const void *__restrict__ qn_w_,
            const void *__restrict__ qn_b_, const void *__restrict__ kn_w_, const void *__restrict__ kn_b_, const int norm_f32,
            const float eps, const void *__restrict__ bias_, const int bias_f32, const int bias_stride,
            const T *__restrict__ ctx, const T *__restrict__ dctx, const float *__restrict__ stats, T *__restrict__ dq,
            T *__restrict__ dk, T *__restrict__ dv, float *__restrict__ partials, const int H, const int Nq, const int Nk)
{
    const Small<T> qn_w = {qn_w_, norm_f32}, qn_b = {qn_b_, norm_f32}, kn_w = {kn_w_, norm_f32}, kn_b = {kn_b_, norm_f32};
    const Small<T> bias = {bias_, bias_f32}, none = {nullptr, 1};
    __shared__ __attribute__((aligned(16))) uint16_t sQ[kMaxNq * kLd];
    __shared__ __attribute__((aligned(16))) uint16_t sQt[kD * kLdQt];
    __shared__ __attribute__((aligned(16))) uint16_t sO[kMaxNq * kLd];       // dO
    __shared__ __attribute__((aligned(16))) uint16_t sOt[kD * kLdQt];
    __shared__ __attribute__((aligned(16))) uint16_t sK[kKT * kLd];
    __shared__ __attribute__((aligned(16))) uint16_t sKt[kD * kLdKt];
    __shared__ __attribute__((aligned(16))) uint16_t sV[kKT * kLd];
    __shared__ __attribute__((aligned(16))) uint16_t sS[kMaxNq * kLd];       // ds [query][key of the tile]
    __shared__ float sM[kMaxNq], sRl[kMaxNq], sDelta[kMaxNq], sQmean[kMaxNq], sQrstd[kMaxNq];
    __shared__ float sBias[kKT], sKmean[kKT], sKrstd[kKT];
    __shared__ float sRed[kWaves][4][kD];
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int64_t ld = (int64_t)H * kD;
    const int64_t qoff = (int64_t)b * Nq * ld + h * kD, koff = (int64_t)b * Nk * ld + h * kD;
    const int Rq = (Nq + 31) & ~31;

    stage_rows<T, NORM>(q + qoff, ld, 0, Nq, Rq, qn_w, qn_b, eps, sQ, sQt, kLdQt, sQmean, sQrstd, tid);
    stage_rows<T, false>(dctx + qoff, ld, 0, Nq, Rq, none, none, 0.f, sO, sOt, kLdQt, nullptr, nullptr, tid);
    for (int i = tid; i < Rq * 8; i += kThreads) {
        const int r = i >> 3, c0 = (i & 7) * 8;
        float d = 0.f;
        if (r < Nq) {
            float a[8], o[8];
            load_vec<T, 8>(dctx + qoff + (int64_t)r * ld + c0, a);
            load_vec<T, 8>(ctx + qoff + (int64_t)r * ld + c0, o);
#pragma unroll
            for (int e = 0; e < 8; ++e) d += a[e] * o[e];
        }
        d = group_add<8>(d);
        if ((i & 7) == 0) {
            sDelta[r] = d;
            sM[r] = r < Nq ? stats[2 * ((int64_t)bh * Nq + r)] : 0.f;
            sRl[r] = r < Nq ? 1.f / stats[2 * ((int64_t)bh * Nq + r) + 1] : 0.f;
        }
    }

    f32x4 dqa[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int db = 0; db < 4; ++db) dqa[i][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    float gk[4][4], bk[4][4];               // d(gamma_k), d(beta_k) of channel db * 16 + 4 g + r, this lane's keys
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int r = 0; r < 4; ++r) gk[db][r] = bk[db][r] = 0.f;

    for (int k0 = 0; k0 < Nk; k0 += kKT) {
        stage_rows<T, NORM>(k + koff, ld, k0, Nk, kKT, kn_w, kn_b, eps, sK, sKt, kLdKt, sKmean, sKrstd, tid);
        stage_rows<T, false>(v + koff, ld, k0, Nk, kKT, none, none, 0.f, sV, nullptr, 0, nullptr, nullptr, tid);
        if (tid < kKT) sBias[tid] = k0 + tid < Nk && bias.p ? bias[(int64_t)b * bias_stride + k0 + tid] : 0.f;
        __syncthreads();

        const int kl = wave * 16 + c, key = k0 + kl;                // this lane's key
        const bool key_ok = key < Nk;
        const float bias_c = sBias[kl];
        // bf16: a key whose bias lies far below the row maxima has weights at or below fp32's smallest normal, where
        // v_exp_f32 returns 0; its column of P and dS is carried times 2^-ex (ex <= 0, an exact power of two, 0 for every
        // key within 22 of the maxima: the same bits as without it) and dv, dk and the stored dS are scaled back by ldexp.
        // p <= 1 keeps the scaled weight at or below 2^64.  fp16 has no such weights (they are 0 in T) and no such range.
        float ex = 0.f;
        if constexpr (std::is_same<T, bf16_t>::value)
            ex = fminf(0.f, fmaxf(-64.f, rintf((bias_c - sM[0]) * kLog2e) + 32.f));
        const int exi = (int)ex;
        s16x8 fk[2], fv[2];
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            fk[st] = lds8(sK + kl * kLd + 32 * st + 8 * g);
            fv[st] = lds8(sV + kl * kLd + 32 * st + 8 * g);
        }
        f32x4 dvt[4], dkt[4];
#pragma unroll
        for (int db = 0; db < 4; ++db) dvt[db] = dkt[db] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int qp = 0; qp * 32 < Nq; ++qp) {
            float p[2][4], ds[2][4];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int q0 = (2 * qp + hf) * 16;
                f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    s = mma::FwdMma<T>::run(lds8(sQ + (q0 + c) * kLd + 32 * st + 8 * g), fk[st], s);
                    dp = mma::FwdMma<T>::run(lds8(sO + (q0 + c) * kLd + 32 * st + 8 * g), fv[st], dp);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int qi = q0 + 4 * g + r;
                    const float x = score_of<T, kD>(s[r], bias_c);
                    const float pr = key_ok && qi < Nq ? __builtin_amdgcn_exp2f((x - sM[qi]) * kLog2e - ex) * sRl[qi] : 0.f;
                    p[hf][r] = pr;
                    ds[hf][r] = key_ok && qi < Nq ? pr * (dp[r] - sDelta[qi]) : 0.f;
                    sS[qi * kLd + kl] = bits_of<T>(ldexpf(ds[hf][r], exi));
                }
            }
            const s16x8 fp = pack_pair<T>(p[0], p[1]), fds = pack_pair<T>(ds[0], ds[1]);
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                dvt[db] = mma::FwdMma<T>::run(lds4x2(sOt + (db * 16 + c) * kLdQt + 32 * qp + 4 * g), fp, dvt[db]);
                dkt[db] = mma::FwdMma<T>::run(lds4x2(sQt + (db * 16 + c) * kLdQt + 32 * qp + 4 * g), fds, dkt[db]);
            }
        }
        // this lane: dV^T, dK^^T [channel db * 16 + 4 g + r][key]
        {
            const int64_t row = koff + (int64_t)key * ld;
            float dy[4][4], xh[4][4];
            float sg = 0.f, sgx = 0.f;
            const float mean = sKmean[kl], rstd = sKrstd[kl];
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const int d0 = db * 16 + 4 * g;
                if (key_ok) {
                    const float o[4] = {ldexpf(dvt[db][0], exi), ldexpf(dvt[db][1], exi), ldexpf(dvt[db][2], exi),
                                        ldexpf(dvt[db][3], exi)};
                    store4<T>(dv + row + d0, o);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) dy[db][r] = ldexpf(dkt[db][r] * kScale, exi);
                if constexpr (NORM) {
                    float x[4] = {0.f, 0.f, 0.f, 0.f};
                    if (key_ok) load4<T>(k + row + d0, x);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        xh[db][r] = key_ok ? (x[r] - mean) * rstd : 0.f;
                        if (!key_ok) dy[db][r] = 0.f;
                        gk[db][r] += dy[db][r] * xh[db][r];
                        bk[db][r] += dy[db][r];
                        dy[db][r] *= kn_w[d0 + r];
                        sg += dy[db][r];
                        sgx += dy[db][r] * xh[db][r];
                    }
                }
            }
            if constexpr (NORM) {
                sg += __shfl_xor(sg, 16, 64); sg += __shfl_xor(sg, 32, 64);
                sgx += __shfl_xor(sgx, 16, 64); sgx += __shfl_xor(sgx, 32, 64);
                sg *= 1.f / kD;
                sgx *= 1.f / kD;
#pragma unroll
                for (int db = 0; db < 4; ++db)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dy[db][r] = rstd * (dy[db][r] - sg - xh[db][r] * sgx);
            }
            if (key_ok) {
#pragma unroll
                for (int db = 0; db < 4; ++db) store4<T>(dk + row + db * 16 + 4 * g, dy[db]);
            }
        }
        __syncthreads();
        // dQ^ += ds k^: query blocks wave, wave + 4
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q0 = (wave + kWaves * i) * 16;
            if (q0 >= Nq) continue;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const s16x8 fs = lds8(sS + (q0 + c) * kLd + 32 * ks + 8 * g);
#pragma unroll
                for (int db = 0; db < 4; ++db)
                    dqa[i][db] = mma::FwdMma<T>::run(fs, lds8(sKt + (db * 16 + c) * kLdKt + 32 * ks + 8 * g), dqa[i][db]);
            }
        }
        __syncthreads();
    }

    // dq: this lane holds dQ^ [query q0 + 4 g + r][channel db * 16 + c]
    float gq[4], bq[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) gq[db] = bq[db] = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q0 = (wave + kWaves * i) * 16;
        if (q0 >= Nq) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qi = q0 + 4 * g + r;
            const bool ok = qi < Nq;
            const int64_t row = qoff + (int64_t)qi * ld;
            float dy[4], xh[4];
            float sg = 0.f, sgx = 0.f;
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                dy[db] = ok ? dqa[i][db][r] * kScale : 0.f;
                if constexpr (NORM) {
                    xh[db] = ok ? (to_f32(q[row + db * 16 + c]) - sQmean[qi]) * sQrstd[qi] : 0.f;
                    gq[db] += dy[db] * xh[db];
                    bq[db] += dy[db];
                    dy[db] *= qn_w[db * 16 + c];
                    sg += dy[db];
                    sgx += dy[db] * xh[db];
                }
            }
            if constexpr (NORM) {
                sg = group_add<16>(sg) * (1.f / kD);
                sgx = group_add<16>(sgx) * (1.f / kD);
                const float rstd = sQrstd[qi];
#pragma unroll
                for (int db = 0; db < 4; ++db) dy[db] = rstd * (dy[db] - sg - xh[db] * sgx);
            }
            if (ok) {
#pragma unroll
                for (int db = 0; db < 4; ++db) dq[row + db * 16 + c] = (T)dy[db];
            }
        }
    }
    if constexpr (NORM) {
        // d(gamma_q), d(beta_q): channel db * 16 + c, summed over the lane groups; d(gamma_k), d(beta_k): channel
        // db * 16 + 4 g + r, summed over the 16 lanes of a group; then the four waves in ascending order
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            gq[db] += __shfl_xor(gq[db], 16, 64); gq[db] += __shfl_xor(gq[db], 32, 64);
            bq[db] += __shfl_xor(bq[db], 16, 64); bq[db] += __shfl_xor(bq[db], 32, 64);
            if (g == 0) { sRed[wave][0][db * 16 + c] = gq[db]; sRed[wave][1][db * 16 + c] = bq[db]; }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float a = group_add<16>(gk[db][r]), bb = group_add<16>(bk[db][r]);
                if (c == 0) { sRed[wave][2][db * 16 + 4 * g + r] = a; sRed[wave][3][db * 16 + 4 * g + r] = bb; }
            }
        }
        __syncthreads();
        const int which = tid >> 6, d = tid & 63;
        float t = sRed[0][which][d];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) t += sRed[w][which][d];
        partials[((int64_t)bh * 4 + which) * kD + d] = t;
    }
}

// out [4, 64] = sum over the n workgroups of partials [n, 4, 64], ascending
__global__ void __launch_bounds__(4 * kD) qk_attn_params(const float *__restrict__ partials, float *__restrict__ out, const int n)
{
    const int t = threadIdx.x;
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += partials[(int64_t)i * 4 * kD + t];
    out[t] = s;
}

bool supported(int dtype, int64_t D, int64_t Nq, int64_t Nk)
{
    return (dtype == MMFS_F16 || dtype == MMFS_BF16) && D == kD && Nq >= 1 && Nq <= kMaxNq && Nk >= 1 && Nk <= kMaxNk;
}

int check(int dtype, int64_t B, int64_t H, int64_t D, int64_t Nq, int64_t Nk)
{
    if (const int rc = batch_heads_check(dtype, B, H, D, Nq, Nk)) return rc;
    return supported(dtype, D, Nq, Nk) ? MMFS_OK : MMFS_E_UNSUPPORTED;
}

// the four LayerNorm pointers: all or none
int norm_of(const void *a, const void *b, const void *c, const void *d)
{
    const int n = (a != nullptr) + (b != nullptr) + (c != nullptr) + (d != nullptr);
    return n == 4 ? 1 : n == 0 ? 0 : -1;
}

}  // namespace
}  // namespace mmfs

extern "C" {

int mmfs_qk_attn_supported(int dtype, int64_t D, int64_t Nq, int64_t Nk) { return mmfs::supported(dtype, D, Nq, Nk); }

namespace {

// what the two entries check alike, before any launch; -> status, norm (0 / 1), the two type flags
struct QkAttnArgs { int norm, norm_f32, bias_f32; };

int qk_attn_check(int dtype, const void *q, const void *k, const void *v, const void *qw, const void *qb, const void *kw,
                  const void *kb, int norm_dtype, const void *key_bias, int bias_dtype, int64_t bias_stride, int64_t B,
                  int64_t H, int64_t D, int64_t Nq, int64_t Nk, QkAttnArgs &a)
{
    using namespace mmfs;
    const int rc = check(dtype, B, H, D, Nq, Nk);
    if (rc) return rc;
    a.norm = norm_of(qw, qb, kw, kb);
    if (a.norm < 0) return MMFS_E_NULLPTR;
    a.norm_f32 = a.norm ? small_f32(norm_dtype, dtype) : 1;
    a.bias_f32 = key_bias ? small_f32(bias_dtype, dtype) : 1;
    if (a.norm_f32 < 0 || a.bias_f32 < 0) return MMFS_E_DTYPE;
    if (key_bias && bias_stride != 0 && bias_stride != Nk) return MMFS_E_DIMS;
    const bool any = B * H != 0;
    const int na = a.norm_f32 ? 4 : 2, ba = a.bias_f32 ? 4 : 2;
    return check_tensors({{q, 16, any}, {k, 16, any}, {v, 16, any}, maybe(qw, na), maybe(qb, na), maybe(kw, na), maybe(kb, na),
                          maybe(key_bias, ba)});
}

}  // namespace

int mmfs_qk_attn_forward(int dtype, const void *q, const void *k, const void *v, const void *q_norm_weight,
                         const void *q_norm_bias, const void *k_norm_weight, const void *k_norm_bias, int norm_dtype, float eps,
                         const void *key_bias, int bias_dtype, int64_t bias_stride, void *context, float *lse, float *stats,
                         int64_t B, int64_t H, int64_t D, int64_t Nq, int64_t Nk, void *stream)
{
    using namespace mmfs;
    QkAttnArgs a;
    const int rc = qk_attn_check(dtype, q, k, v, q_norm_weight, q_norm_bias, k_norm_weight, k_norm_bias, norm_dtype, key_bias,
                                 bias_dtype, bias_stride, B, H, D, Nq, Nk, a);
    if (rc) return rc;
    if (B * H == 0) return MMFS_OK;
    if (const int rt = check_tensors({{context, 16}, {lse, 4}, {stats, 4}})) return rt;
    return by_half_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        auto kernel = a.norm ? qk_attn_fwd<T, true> : qk_attn_fwd<T, false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)(B * H)), dim3(kThreads), 0, (hipStream_t)stream, (const T *)q, (const T *)k,
                           (const T *)v, q_norm_weight, q_norm_bias, k_norm_weight, k_norm_bias, a.norm_f32, eps, key_bias,
                           a.bias_f32, (int)bias_stride, (T *)context, lse, stats, (int)H, (int)Nq, (int)Nk);
        return (int)hipGetLastError();
    });
}

int mmfs_qk_attn_backward(int dtype, const void *q, const void *k, const void *v, const void *q_norm_weight,
                          const void *q_norm_bias, const void *k_norm_weight, const void *k_norm_bias, int norm_dtype, float eps,
                          const void *key_bias, int bias_dtype, int64_t bias_stride, const void *context,
                          const void *grad_context, const float *stats, void *grad_q, void *grad_k, void *grad_v,
                          float *partials, float *grad_params, int64_t B, int64_t H, int64_t D, int64_t Nq, int64_t Nk,
                          void *stream)
{
    using namespace mmfs;
    QkAttnArgs a;
    const int rc = qk_attn_check(dtype, q, k, v, q_norm_weight, q_norm_bias, k_norm_weight, k_norm_bias, norm_dtype, key_bias,
                                 bias_dtype, bias_stride, B, H, D, Nq, Nk, a);
    if (rc) return rc;
    if (const int rt = check_tensors({{partials, 4, a.norm != 0}, {grad_params, 4, a.norm != 0}})) return rt;
    if (B * H == 0) {
        // no workgroup: the parameter gradients are the empty sum
        if (!a.norm) return MMFS_OK;
        hipLaunchKernelGGL(qk_attn_params, dim3(1), dim3(4 * kD), 0, (hipStream_t)stream, partials, grad_params, 0);
        return (int)hipGetLastError();
    }
    if (const int rt = check_tensors({{context, 16}, {grad_context, 16}, {stats, 4}, {grad_q, 16}, {grad_k, 16}, {grad_v, 16}}))
        return rt;
    return by_half_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        auto kernel = a.norm ? qk_attn_bwd<T, true> : qk_attn_bwd<T, false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)(B * H)), dim3(kThreads), 0, (hipStream_t)stream, (const T *)q, (const T *)k,
                           (const T *)v, q_norm_weight, q_norm_bias, k_norm_weight, k_norm_bias, a.norm_f32, eps, key_bias,
                           a.bias_f32, (int)bias_stride, (const T *)context, (const T *)grad_context, stats, (T *)grad_q,
                           (T *)grad_k, (T *)grad_v, partials, (int)H, (int)Nq, (int)Nk);
        const int e = (int)hipGetLastError();
        if (e || !a.norm) return e;
        hipLaunchKernelGGL(qk_attn_params, dim3(1), dim3(4 * kD), 0, (hipStream_t)stream, partials, grad_params, (int)(B * H));
        return (int)hipGetLastError();
    });
}

}  // extern "C"
