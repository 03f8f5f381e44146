// mmfs_clip_attn.hip -- the CLIP ViT's self-attention: what the reference's CLIPXAttention
// (mm_interleaved/models/encoders/vit_adapter/xattn.py:21-141) asks of xformers.ops.memory_efficient_attention(q, k, v)
// between the three Linear layers and out_proj, forward and backward, without a tensor of size L x L.  Full (non-causal)
// attention, no mask, no bias, no dropout: q, k, v, dO and every output are token-major [B, L, H 64] of T (bf16 / fp16) as
// the Linear layers produce and consume them; arithmetic is fp32; D = 64.
//     s(j, t)    = q[b, j, h] . k[b, t, h] / 8
//     context    = softmax_t(s) v,   lse = ln sum_t exp s  (fp32, [B, H, L])            (clip_attn_fwd)
//     dq, dk, dv                                                                        (clip_attn_dq, clip_attn_dkdv)
// This is mmfs_llama_train.hip without the rotation and without the diagonal: every (query, key) pair in front of L is
// live, so every second product is a plain matrix product and there is nothing like diag_fma here.
//
//   clip_attn_fwd    Workgroup of 4 waves = 128 query rows of one (b, h), a wave owns 32 of them as two 16-query blocks;
//                    grid ceil(L / 128) x B H.  Key tiles of 64 through LDS: K row-major [key][64 + 8], V transposed
//                    [channel][64 + 4].  S^T = K q^T (key on the accumulator's rows, query on the lane), online softmax with
//                    one running (m, l) a lane, P rounded to T; the packed S^T accumulators are the B operand of
//                    O^T += V^T P^T.  context and lse = m + ln l are written once; lse may be NULL (no backward follows).
//   clip_attn_dq     query-stationary, the forward's grid and tiles.  A wave first forms delta[b, h, j] = sum_c dO O (fp32,
//                    16 channels a lane, then the four lane groups in a fixed order) for its rows and writes it to the
//                    workspace; q and dO fragments stay in registers.  Per key tile: K row-major AND transposed, V
//                    row-major.  S'^T = K q^T - 8 lse and dP'^T = V dO^T - delta come out of their chains ready (the row
//                    constants are the initial accumulators); P = exp(S' / 8), dS^T = P (dP'), rounded to T where it enters
//                    dQ^T += K^T dS^T.  dq = dQ / 8, rounded once.
//   clip_attn_dkdv   key-stationary, launched behind dq (it reads delta).  Workgroup of 4 waves = 128 keys of one (b, h), a
//                    wave owns 32 of them as two 16-key blocks and keeps their k and v fragments and dK^T, dV^T (64
//                    accumulator registers) while the workgroup sweeps ALL query tiles of 64: Q and dO row-major and
//                    transposed, -8 lse and -delta.  S' and dP' with the KEY ON THE LANE: their packed accumulators are
//                    the B operands of dV^T += dO^T P and dK^T += Q^T dS.  Grid ceil(L / 128) x B H.
//   Partial tiles    A key at or behind L scores -Inf by SELECTION (forward; p = ds = 0 by selection backward) and its v / k
//                    row is staged as zeros; a 16-key block wholly behind L is not computed at all.  A query row at or behind L
//                    is staged as zeros, its p and ds are selected to 0 in dkdv, and it is never stored.  Key 0 is live for every
//                    row, so the running maximum is finite from the first tile on (the online-softmax step says where it relies
//                    on that).
//   Tile sizes       128 query rows / 64 keys (fwd, dq), 128 keys / 64 queries (dkdv): mmfs_llama_train.hip's, taken over so
//                    that the two files read alike.  NOBODY HAS MEASURED ANOTHER CHOICE.  What was weighed: at L = 257 the
//                    third query tile holds one live row; its three idle waves and its second block skip every product, so the
//                    tile costs its share of staging (5 key tiles) and one block's products -- a third of the workgroups, a
//                    17th of the work.  A 64-row tile would leave a fifth of the workgroups so and stage K and V five times
//                    a head instead of three.  The last key tile at L = 257 holds one live key: one 16-key block of four is
//                    computed.  At L = 257 a head's whole K and V (2 x 33 KB) would fit in LDS and the walk would need no
//                    barrier but the first; not done here: the staged tile is what the L = 1025 shape needs anyway, and one
//                    organisation serves both.  profiles/clip_attn.md holds what was measured.
//   Staging          A tile goes global memory -> registers (load_tile) -> LDS (put_tile), and the NEXT tile's loads are issued
//                    right behind the barrier that publishes the current one, so they are in flight while it is multiplied:
//                    16 registers a lane (dkdv: 18, with -8 lse and -delta).  Measured against staging each tile where it is
//                    used: forward 37.7 -> 36.1 / 105.9 -> 95.9 us, backward 117.6 -> 103.6 / 331.5 -> 276.4 us at
//                    (B, L) = (32, 257) / (8, 1025), H = 16, bf16; the same bits (profiles/clip_attn.md).
//   Seven products   S and dP are computed in both backward kernels, as in mmfs_llama_train.hip and for its reason: no float
//                    atomics, no hand-off between workgroups.
// No float atomics, no flags between workgroups, nothing allocated, cleared or read back; every sum's order depends on L
// alone: results are bit-reproducible, eager or replayed from a graph.  The workspace is delta alone: B H L floats.
// The grid is one-dimensional, tiles x B H <= 2^31 - 1, else MMFS_E_DIMS: never a truncated grid.
//
// Resources (make asm, gfx950; no spills, no scratch; the compiler's own choice of waves per SIMD):
//                              VGPRs  AGPRs  LDS bytes  waves / SIMD
//   clip_attn_fwd    bf16       134    32     17920      3
//   clip_attn_fwd    fp16       134    32     17920      3
//   clip_attn_dq     bf16       132    36     27136      3
//   clip_attn_dq     fp16       133    32     27136      3
//   clip_attn_dkdv   bf16       188    64     36352      2
//   clip_attn_dkdv   fp16       190    64     36352      2
// What bounds each kernel: profiles/clip_attn.md.
//
// Error bounds (tests/clip_attn_refs.py, clip64, evaluates them element by element against fp64 on the STORED q, k, v, dO;
// it builds on tests/qk_attn_refs.py, attention64(norm=None), whose bounds these are; the framework's statement in T is held
// to the same bounds, so each counts the roundings of whichever rounds more).  u = HALF a unit in the last place of T (2^-9
// bf16, 2^-12 fp16), t = T's smallest normal, e = 2^-24, c_e = 256 + 2 L, c_n = 96; A(j, t) = |q_j| . |k_t| / 8.
//   s              E_s = 3 u |s| + c_n e (A + |s|)       (2 matrix-core steps of 32 fp32 accumulations and the scaling here;
//                  the framework rounds q / 8, the score and the softmax's input)
//   p              E_p = p (E_s + sum_t p E_s + u + c_e e)
//   context        |context - ref| <= E_p |v| + c_e e p |v| + 2 u |ref| + t
//   lse            |lse - ref| <= sum_t p E_s + c_e e (1 + |lse|)
//   delta          rowsum(dO O) from the rounded context, fp32:   E_delta = sum_c |dO_c| W_c,   W = (E_p + (2 u + c_e e) p) |v| + t
//   ds             p (dP - delta), rounded once:   E_ds = E_p |dP - delta| + p (u |dP| + E_delta) + 3 u |ds|
//   dv             P^T dO:   |dv - ref| <= E_p^T |dO| + c_e e p^T |dO| + 2 u |ref| + t
//   dq             ds k / 8:   |dq - ref| <= (E_ds |k| + c_e e |ds| |k|) / 8 + 2 u |ref| + t          (dk alike, with q)
//   These bounds add absolute values where the errors of 64 channels and up to L keys largely cancel.  The tests therefore hold
//   the context and the gradients to a second, tight measure as well: a row's error in the 2-norm within 8 (2 u) of the row's
//   norm plus the share of delta's rounding (tests/clip_attn_refs.py, row_error; tests/llama_train_refs.py derives the factor).
//   Measured worst ratios of both are kept in profiles/clip_attn.md.
//
// Offsets are 64-bit.
#include "mmfs_attn_core.h"
#include "../../include/mmfs_clip_attn.h"
#include <hip/hip_runtime.h>

namespace mmfs {

namespace {

using namespace attn;

constexpr int kD = kClipD;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kWaveRows = 32;           // fwd, dq: query rows of a wave: two blocks of 16
constexpr int kRows = kWaves * kWaveRows;           // of a workgroup
constexpr int kKT = 64;                 // fwd, dq: keys of a tile
constexpr int kWaveKeys = 32;           // dkdv: keys of a wave: two blocks of 16
constexpr int kKeys = kWaves * kWaveKeys;           // of a workgroup
constexpr int kQT = 64;                 // dkdv: queries of a tile
constexpr int kLdR = kD + 8;            // elements between rows of a row-major image [row][64 + 8]
constexpr int kLdT = 64 + 4;            // of a transposed image [channel][64 + 4]
constexpr int kDB = kD / 16;            // 16-channel blocks of a head
constexpr int kST = kD / 32;            // matrix-core steps of a score
constexpr float kScale = HeadScale<kD>::value;
constexpr float kInvScale = 8.f;        // sqrt(64)

template <typename T> __device__ __forceinline__ float bits_f32(uint32_t h) { return to_f32(__builtin_bit_cast(T, (uint16_t)h)); }

// A tile is staged in two halves, so that the next tile's loads are in flight while the current one is multiplied.
// load_tile: rows r0 .. r0 + 63 of one head's token-major slice (``src`` at the head's channel 0 of row 0, rows ``ld``
// elements apart) -> registers: a lane holds 8 channels of 2 neighbouring rows; a row at or behind L is zeros.
template <typename T>
__device__ __forceinline__ void load_tile(const T *__restrict__ src, const int64_t ld, const int r0, const int L, uint4 (&vr)[2],
                                          const int tid)
{
    const int cg = tid & 7, kq = tid >> 3;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int row = r0 + 2 * kq + e;
        vr[e] = make_uint4(0u, 0u, 0u, 0u);
        if (row < L) vr[e] = *reinterpret_cast<const uint4 *>(src + (int64_t)row * ld + 8 * cg);
    }
}

// put_tile: those registers -> LDS, row-major (``rows``) and / or transposed (``trans``), either may be null (the transposed
// image takes a lane's share as 8 x 4 bytes)
__device__ __forceinline__ void put_tile(const uint4 (&vr)[2], uint16_t *rows, uint16_t *trans, const int tid)
{
    const int cg = tid & 7, kq = tid >> 3;
    if (rows) {
#pragma unroll
        for (int e = 0; e < 2; ++e) *reinterpret_cast<uint4 *>(rows + (2 * kq + e) * kLdR + 8 * cg) = vr[e];
    }
    if (trans) {
        const uint32_t w[2][4] = {{vr[0].x, vr[0].y, vr[0].z, vr[0].w}, {vr[1].x, vr[1].y, vr[1].z, vr[1].w}};
#pragma unroll
        for (int pr = 0; pr < 4; ++pr) {                                    // channels 2 pr (low halves), 2 pr + 1 (high halves)
            const uint32_t lo = (w[0][pr] & 0xffffu) | (w[1][pr] << 16);
            const uint32_t hi = (w[0][pr] >> 16) | (w[1][pr] & 0xffff0000u);
            *reinterpret_cast<uint32_t *>(trans + (8 * cg + 2 * pr) * kLdT + 2 * kq) = lo;
            *reinterpret_cast<uint32_t *>(trans + (8 * cg + 2 * pr + 1) * kLdT + 2 * kq) = hi;
        }
    }
}

// the 16 channels 32 st + 8 g .. + 7 (st < 2) of one token's head as the fragments of a matrix product; zeros when not ``live``
template <typename T> __device__ __forceinline__ void load_frags(const T *p, const bool live, const int g, s16x8 (&f)[kST])
{
#pragma unroll
    for (int st = 0; st < kST; ++st)
        f[st] = live ? *reinterpret_cast<const s16x8 *>(p + 32 * st + 8 * g) : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
}

// a lane's share of rowsum(a b): the 16 channels of its two fragments, in ascending order
template <typename T> __device__ __forceinline__ float frag_dot(const s16x8 (&a)[kST], const s16x8 (&b)[kST])
{
    float d = 0.f;
#pragma unroll
    for (int st = 0; st < kST; ++st)
#pragma unroll
        for (int e = 0; e < 8; ++e) d += bits_f32<T>((uint16_t)a[st][e]) * bits_f32<T>((uint16_t)b[st][e]);
    return d;
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
clip_attn_fwd(const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v, T *__restrict__ ctx,
              float *__restrict__ lse, const int L, const int H, const int BH)
{
    __shared__ __attribute__((aligned(16))) uint16_t sK[kKT * kLdR];
    __shared__ __attribute__((aligned(16))) uint16_t sVt[kD * kLdT];
    const int qt = blockIdx.x / BH, bh = blockIdx.x - qt * BH, b = bh / H, h = bh - b * H;
    const int q0 = qt * kRows;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int64_t ld = (int64_t)H * kD, off = (int64_t)b * L * ld + (int64_t)h * kD;

    // this lane's query of block i: row q0 + 32 wave + 16 i + c (zeros at or behind L)
    s16x8 fq[2][kST];
    float m[2], l[2];
    f32x4 acc[2][kDB];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int j = q0 + wave * kWaveRows + 16 * i + c;
        load_frags<T>(q + off + (int64_t)min(j, L - 1) * ld, j < L, g, fq[i]);
        m[i] = -INFINITY;
        l[i] = 0.f;
#pragma unroll
        for (int db = 0; db < kDB; ++db) acc[i][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    uint4 rk[2], rv[2];                     // the next key tile, on its way
    load_tile<T>(k + off, ld, 0, L, rk, tid);
    load_tile<T>(v + off, ld, 0, L, rv, tid);
    for (int k0 = 0; k0 < L; k0 += kKT) {
        put_tile(rk, sK, nullptr, tid);
        put_tile(rv, nullptr, sVt, tid);
        __syncthreads();
        if (k0 + kKT < L) {
            load_tile<T>(k + off, ld, k0 + kKT, L, rk, tid);
            load_tile<T>(v + off, ld, k0 + kKT, L, rv, tid);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r0 = q0 + wave * kWaveRows + 16 * i;
            if (r0 >= L) continue;                                          // no row (wave-uniform)
            float s[4][4];
            float tm = -INFINITY;
#pragma unroll
            for (int kb16 = 0; kb16 < 4; ++kb16) {
                const int t0 = k0 + kb16 * 16;
                if (t0 >= L) {                                              // a block wholly behind L (wave-uniform)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[kb16][r] = -INFINITY;
                    continue;
                }
                f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int st = 0; st < kST; ++st)
                    a = mma::FwdMma<T>::run(lds8(sK + (kb16 * 16 + c) * kLdR + 32 * st + 8 * g), fq[i][st], a);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[kb16][r] = t0 + 4 * g + r < L ? a[r] * kScale : -INFINITY;
                    tm = fmaxf(tm, s[kb16][r]);
                }
            }
            tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
            tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
            // Key 0 is live for every row, so from the first tile on mn is finite wherever the row's scores are numbers: no
            // guard against -Inf - -Inf.  (A row whose scores are all NaN keeps mn = -Inf, fmaxf passes NaN over, and
            // -Inf - -Inf makes it NaN, which is what such a row is.)
            const float mn = fmaxf(m[i], tm);
            const float alpha = exp_hw(m[i] - mn);
            float ps = 0.f;
#pragma unroll
            for (int kb16 = 0; kb16 < 4; ++kb16)
#pragma unroll
                for (int r = 0; r < 4; ++r) { s[kb16][r] = exp_hw(s[kb16][r] - mn); ps += s[kb16][r]; }
            ps += __shfl_xor(ps, 16, 64);
            ps += __shfl_xor(ps, 32, 64);
            l[i] = l[i] * alpha + ps;
            m[i] = mn;
#pragma unroll
            for (int db = 0; db < kDB; ++db) acc[i][db] *= alpha;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (k0 + 32 * ks >= L) continue;                            // both blocks behind L: P = 0 (wave-uniform)
                const s16x8 fp = pack_pair<T>(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
                for (int db = 0; db < kDB; ++db)
                    acc[i][db] = mma::FwdMma<T>::run(lds4x2(sVt + (db * 16 + c) * kLdT + 32 * ks + 4 * g), fp, acc[i][db]);
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int qi = q0 + wave * kWaveRows + 16 * i + c;
        if (qi >= L) continue;
        T *o = ctx + off + (int64_t)qi * ld;
#pragma unroll
        for (int db = 0; db < kDB; ++db) {
            const float out[4] = {acc[i][db][0] / l[i], acc[i][db][1] / l[i], acc[i][db][2] / l[i], acc[i][db][3] / l[i]};
            store4<T>(o + db * 16 + 4 * g, out);
        }
        if (lse && g == 0) lse[(int64_t)bh * L + qi] = m[i] + logf(l[i]);
    }
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
clip_attn_dq(const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v, const T *__restrict__ ctx,
             const T *__restrict__ dctx, const float *__restrict__ lse, T *__restrict__ dq, float *__restrict__ delta,
             const int L, const int H, const int BH)
{
    __shared__ __attribute__((aligned(16))) uint16_t sK[kKT * kLdR];
    __shared__ __attribute__((aligned(16))) uint16_t sKt[kD * kLdT];
    __shared__ __attribute__((aligned(16))) uint16_t sV[kKT * kLdR];
    const int qt = blockIdx.x / BH, bh = blockIdx.x - qt * BH, b = bh / H, h = bh - b * H;
    const int q0 = qt * kRows;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int64_t ld = (int64_t)H * kD, off = (int64_t)b * L * ld + (int64_t)h * kD;

    s16x8 fq[2][kST], fdo[2][kST];
    float nl[2], nd[2];                     // -8 lse and -delta of this lane's query
    f32x4 acc[2][kDB];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int j = q0 + wave * kWaveRows + 16 * i + c;
        const bool live = j < L;
        const int64_t row = off + (int64_t)min(j, L - 1) * ld;
        load_frags<T>(q + row, live, g, fq[i]);
        load_frags<T>(dctx + row, live, g, fdo[i]);
        s16x8 fo[kST];
        load_frags<T>(ctx + row, live, g, fo);
        float d = frag_dot<T>(fdo[i], fo);
        d += __shfl_xor(d, 16, 64);
        d += __shfl_xor(d, 32, 64);
        if (live && g == 0) delta[(int64_t)bh * L + j] = d;
        nd[i] = -d;
        nl[i] = live ? -lse[(int64_t)bh * L + j] * kInvScale : 0.f;
#pragma unroll
        for (int db = 0; db < kDB; ++db) acc[i][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    uint4 rk[2], rv[2];                     // the next key tile, on its way
    load_tile<T>(k + off, ld, 0, L, rk, tid);
    load_tile<T>(v + off, ld, 0, L, rv, tid);
    for (int k0 = 0; k0 < L; k0 += kKT) {
        put_tile(rk, sK, sKt, tid);
        put_tile(rv, sV, nullptr, tid);
        __syncthreads();
        if (k0 + kKT < L) {
            load_tile<T>(k + off, ld, k0 + kKT, L, rk, tid);
            load_tile<T>(v + off, ld, k0 + kKT, L, rv, tid);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r0 = q0 + wave * kWaveRows + 16 * i;
            if (r0 >= L) continue;                                          // (wave-uniform)
            float ds[4][4];
#pragma unroll
            for (int kb16 = 0; kb16 < 4; ++kb16) {
                const int t0 = k0 + kb16 * 16;
                if (t0 >= L) {                                              // a block wholly behind L (wave-uniform)
#pragma unroll
                    for (int r = 0; r < 4; ++r) ds[kb16][r] = 0.f;
                    continue;
                }
                f32x4 a = {nl[i], nl[i], nl[i], nl[i]}, dp = {nd[i], nd[i], nd[i], nd[i]};
#pragma unroll
                for (int st = 0; st < kST; ++st) {
                    a = mma::FwdMma<T>::run(lds8(sK + (kb16 * 16 + c) * kLdR + 32 * st + 8 * g), fq[i][st], a);
                    dp = mma::FwdMma<T>::run(lds8(sV + (kb16 * 16 + c) * kLdR + 32 * st + 8 * g), fdo[i][st], dp);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = exp_hw(a[r] * kScale);
                    const float x = p * dp[r];
                    ds[kb16][r] = t0 + 4 * g + r < L ? x : 0.f;
                }
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (k0 + 32 * ks >= L) continue;                            // (wave-uniform)
                const s16x8 fs = pack_pair<T>(ds[2 * ks], ds[2 * ks + 1]);
#pragma unroll
                for (int db = 0; db < kDB; ++db)
                    acc[i][db] = mma::FwdMma<T>::run(lds4x2(sKt + (db * 16 + c) * kLdT + 32 * ks + 4 * g), fs, acc[i][db]);
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int qi = q0 + wave * kWaveRows + 16 * i + c;
        if (qi >= L) continue;
        T *o = dq + off + (int64_t)qi * ld;
#pragma unroll
        for (int db = 0; db < kDB; ++db) {
            const float out[4] = {acc[i][db][0] * kScale, acc[i][db][1] * kScale, acc[i][db][2] * kScale, acc[i][db][3] * kScale};
            store4<T>(o + db * 16 + 4 * g, out);
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
clip_attn_dkdv(const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v, const T *__restrict__ dctx,
               const float *__restrict__ lse, const float *__restrict__ delta, T *__restrict__ dk, T *__restrict__ dv,
               const int L, const int H, const int BH)
{
    __shared__ __attribute__((aligned(16))) uint16_t sQ[kQT * kLdR];
    __shared__ __attribute__((aligned(16))) uint16_t sQt[kD * kLdT];
    __shared__ __attribute__((aligned(16))) uint16_t sO[kQT * kLdR];         // dO
    __shared__ __attribute__((aligned(16))) uint16_t sOt[kD * kLdT];
    __shared__ __attribute__((aligned(16))) float sNl[kQT], sNd[kQT];        // -8 lse, -delta
    const int kt = blockIdx.x / BH, bh = blockIdx.x - kt * BH, b = bh / H, h = bh - b * H;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int64_t ld = (int64_t)H * kD, off = (int64_t)b * L * ld + (int64_t)h * kD;
    const int kw0 = kt * kKeys + wave * kWaveKeys;                          // the wave's first key

    s16x8 fk[2][kST], fv[2][kST];
    f32x4 dkt[2][kDB], dvt[2][kDB];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int t = kw0 + 16 * i + c;
        const int64_t row = off + (int64_t)min(t, L - 1) * ld;
        load_frags<T>(k + row, t < L, g, fk[i]);
        load_frags<T>(v + row, t < L, g, fv[i]);
#pragma unroll
        for (int db = 0; db < kDB; ++db) dkt[i][db] = dvt[i][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    uint4 rq[2], ro[2];                     // the next query tile, on its way, with its -8 lse and -delta (lanes < kQT)
    float rl = 0.f, rd = 0.f;
    const auto load_rows = [&](const int q0) {
        load_tile<T>(q + off, ld, q0, L, rq, tid);
        load_tile<T>(dctx + off, ld, q0, L, ro, tid);
        const bool live = tid < kQT && q0 + tid < L;
        rl = live ? -lse[(int64_t)bh * L + q0 + tid] * kInvScale : 0.f;
        rd = live ? -delta[(int64_t)bh * L + q0 + tid] : 0.f;
    };
    load_rows(0);
    for (int q0 = 0; q0 < L; q0 += kQT) {
        put_tile(rq, sQ, sQt, tid);
        put_tile(ro, sO, sOt, tid);
        if (tid < kQT) {
            sNl[tid] = rl;
            sNd[tid] = rd;
        }
        __syncthreads();
        if (q0 + kQT < L) load_rows(q0 + kQT);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int t0 = kw0 + 16 * i;                                    // the key block
            if (t0 >= L) continue;                                          // no key (wave-uniform)
            float p[4][4], ds[4][4];
#pragma unroll
            for (int qs = 0; qs < 4; ++qs) {
                const int j0 = q0 + 16 * qs;
                if (j0 >= L) {                                              // a block wholly behind L (wave-uniform)
#pragma unroll
                    for (int r = 0; r < 4; ++r) p[qs][r] = ds[qs][r] = 0.f;
                    continue;
                }
                const float4 l4 = *reinterpret_cast<const float4 *>(sNl + 16 * qs + 4 * g);
                const float4 d4 = *reinterpret_cast<const float4 *>(sNd + 16 * qs + 4 * g);
                f32x4 a = {l4.x, l4.y, l4.z, l4.w}, dp = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int st = 0; st < kST; ++st) {
                    a = mma::FwdMma<T>::run(lds8(sQ + (16 * qs + c) * kLdR + 32 * st + 8 * g), fk[i][st], a);
                    dp = mma::FwdMma<T>::run(lds8(sO + (16 * qs + c) * kLdR + 32 * st + 8 * g), fv[i][st], dp);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool live = j0 + 4 * g + r < L;                   // (a dead query's row is zeros: exp(0) = 1, not 0)
                    const float pr = exp_hw(a[r] * kScale);
                    const float x = pr * dp[r];
                    p[qs][r] = live ? pr : 0.f;
                    ds[qs][r] = live ? x : 0.f;
                }
            }
#pragma unroll
            for (int qp = 0; qp < 2; ++qp) {
                if (q0 + 32 * qp >= L) continue;                            // (wave-uniform)
                const s16x8 fp = pack_pair<T>(p[2 * qp], p[2 * qp + 1]), fds = pack_pair<T>(ds[2 * qp], ds[2 * qp + 1]);
#pragma unroll
                for (int db = 0; db < kDB; ++db) {
                    dvt[i][db] = mma::FwdMma<T>::run(lds4x2(sOt + (db * 16 + c) * kLdT + 32 * qp + 4 * g), fp, dvt[i][db]);
                    dkt[i][db] = mma::FwdMma<T>::run(lds4x2(sQt + (db * 16 + c) * kLdT + 32 * qp + 4 * g), fds, dkt[i][db]);
                }
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int t = kw0 + 16 * i + c;
        if (t >= L) continue;
        T *ok = dk + off + (int64_t)t * ld, *ov = dv + off + (int64_t)t * ld;
#pragma unroll
        for (int db = 0; db < kDB; ++db) {
            const float gv[4] = {dvt[i][db][0], dvt[i][db][1], dvt[i][db][2], dvt[i][db][3]};
            const float gk[4] = {dkt[i][db][0] * kScale, dkt[i][db][1] * kScale, dkt[i][db][2] * kScale, dkt[i][db][3] * kScale};
            store4<T>(ov + db * 16 + 4 * g, gv);
            store4<T>(ok + db * 16 + 4 * g, gk);
        }
    }
}

// every entry's checks of (dtype, B, H, D, L); ``empty``: OK without a launch
int entry_check(int dtype, int64_t B, int64_t H, int64_t D, int64_t L, bool &empty)
{
    empty = false;
    const int rc = clip_check(dtype, B, H, D, L);
    if (rc) return rc;
    // the grid is tiles x B H in one dimension (kRows == kKeys: the same count for the three kernels)
    const int64_t tiles = (L + kRows - 1) / kRows;
    if (tiles * B * H > ((int64_t)1 << 31) - 1 || B * L > (1LL << 32) || B * L * H > (1LL << 34)) return MMFS_E_DIMS;
    empty = B * H * L == 0;
    return MMFS_OK;
}

static_assert(kRows == kKeys, "entry_check counts one grid for the three kernels");

}  // namespace
}  // namespace mmfs

extern "C" {

int mmfs_clip_attn_supported(int dtype, int64_t D, int64_t L) { return mmfs::attn::clip_supported(dtype, D, L); }

int64_t mmfs_clip_attn_tiles(int level)
{
    using namespace mmfs;
    return level == 0 ? kRows : level == 1 ? kKT : level == 2 ? kKeys : level == 3 ? kQT : level == 4 ? kWaveRows : MMFS_E_DIMS;
}

int64_t mmfs_clip_attn_workspace_bytes(int64_t B, int64_t H, int64_t L)
{
    using namespace mmfs;
    if (attn::batch_heads_check(MMFS_F16, B, H, L, 0, 0) || L > attn::kClipMaxL) return MMFS_E_DIMS;       // (no dtype to ask about)
    return B * H * L * (int64_t)sizeof(float);                             // delta
}

int mmfs_clip_attn_forward(int dtype, const void *q, const void *k, const void *v, void *out, float *lse, int64_t B, int64_t L,
                           int64_t H, int64_t D, void *stream)
{
    using namespace mmfs;
    bool empty;
    const int rc = entry_check(dtype, B, H, D, L, empty);
    if (rc || empty) return rc;
    if (const int rt = check_tensors({{q, 16}, {k, 16}, {v, 16}, {out, 16}, maybe(lse, 4)})) return rt;
    const int64_t tiles = (L + kRows - 1) / kRows;
    return by_half_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(clip_attn_fwd<T>, dim3((unsigned)(tiles * B * H)), dim3(kThreads), 0, (hipStream_t)stream,
                           (const T *)q, (const T *)k, (const T *)v, (T *)out, lse, (int)L, (int)H, (int)(B * H));
        return (int)hipGetLastError();
    });
}

int mmfs_clip_attn_backward(int dtype, const void *q, const void *k, const void *v, const void *out, const void *dout,
                            const float *lse, void *dq, void *dk, void *dv, float *workspace, int64_t workspace_bytes,
                            int64_t B, int64_t L, int64_t H, int64_t D, void *stream)
{
    using namespace mmfs;
    bool empty;
    const int rc = entry_check(dtype, B, H, D, L, empty);
    if (rc || empty) return rc;
    if (const int rt = check_tensors({{q, 16}, {k, 16}, {v, 16}, {out, 16}, {dout, 16}, {lse, 4}, {dq, 16}, {dk, 16}, {dv, 16}}))
        return rt;
    if (const int rw = check_workspace(workspace, workspace_bytes, B * H * L * (int64_t)sizeof(float))) return rw;
    const int64_t tiles = (L + kRows - 1) / kRows;
    return by_half_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(clip_attn_dq<T>, dim3((unsigned)(tiles * B * H)), dim3(kThreads), 0, (hipStream_t)stream,
                           (const T *)q, (const T *)k, (const T *)v, (const T *)out, (const T *)dout, lse, (T *)dq, workspace,
                           (int)L, (int)H, (int)(B * H));
        const int e = (int)hipGetLastError();
        if (e) return e;
        hipLaunchKernelGGL(clip_attn_dkdv<T>, dim3((unsigned)(tiles * B * H)), dim3(kThreads), 0, (hipStream_t)stream,
                           (const T *)q, (const T *)k, (const T *)v, (const T *)dout, lse, (const float *)workspace, (T *)dk,
                           (T *)dv, (int)L, (int)H, (int)(B * H));
        return (int)hipGetLastError();
    });
}

}  // extern "C"
