// mmfs_attn_train.h -- the tile walks of the two training attentions, written once: mmfs_clip_attn.hip (the CLIP ViT: full
// attention, D = 64) and mmfs_llama_train.hip (the LLM: causal attention of rotated q and k, D = 128;
// DESIGN.md 4.17) instantiate the three kernels below with a traits type each and keep what only they have.  q, k, v, dO and
// every output are token-major [B, L, H D] of T (bf16 / fp16) as the Linear layers produce and consume them; arithmetic is
// fp32; nothing of size L x L exists.  sc = 1 / sqrt(D).
//
//   attn_train_fwd   Workgroup of 4 waves = 128 query rows of one (b, h), a wave owns 32 of them as two 16-query blocks;
//                    grid ceil(L / 128) x B H.  Key tiles of 64 through LDS: K row-major [key][D + 8], V transposed
//                    [channel][64 + 4].  S^T = K q^T (key on the accumulator's rows, query on the lane), online softmax with
//                    one running (m, l) a lane, P rounded to T; the packed S^T accumulators are the B operand of
//                    O^T += V^T P^T.  context and lse = m + ln l (fp32, [B, H, L]) are written once.
//   attn_train_dq    query-stationary, the forward's grid and tiles.  A wave first forms delta[b, h, j] = sum_c dO O (fp32,
//                    D / 4 channels a lane, then the four lane groups in a fixed order) for its rows and writes it to the
//                    workspace; q and dO fragments stay in registers.  Per key tile: K row-major AND transposed, V
//                    row-major.  S'^T = K q^T - lse sqrt(D) and dP'^T = V dO^T - delta come out of their chains ready (the
//                    row constants are the initial accumulators: cdna_hip_programming.md, Appendix B); P = exp(S' sc),
//                    dS^T = P (dP'), rounded to T where it enters dQ^T += K^T dS^T: D / 2 accumulator registers a block for
//                    the whole walk.  The family's epilogue stores dq = dQ sc.
//   attn_train_dkdv  key-stationary, launched behind dq (it reads delta).  Workgroup of 4 waves = 128 keys of one (b, h), a
//                    wave owns 32 of them as two 16-key blocks and keeps their k and v fragments and dK^T, dV^T (D
//                    accumulator registers) while the workgroup sweeps the query tiles of 64: Q and dO row-major and
//                    transposed, -lse sqrt(D) and -delta.  S' and dP' with the KEY ON THE LANE: their packed accumulators
//                    are the B operands of dV^T += dO^T P and dK^T += Q^T dS.  Grid ceil(L / 128) x B H.
//   Partial tiles    A masked score is SELECTED (to -Inf forward, p = ds = 0 backward), never added to.  A key at or behind L
//                    has its v / k row staged as zeros; a 16-key block wholly behind L (or beyond the diagonal) is not
//                    computed at all.  A query row at or behind L is staged as zeros, its p and ds are selected to 0 in dkdv,
//                    and it is never stored.
//   Seven products   S and dP are computed in both backward kernels: 7 matrix products a (query tile, key tile) pair against
//                    the 5 of a single key-stationary kernel: 40 % more matrix-core work.  The five-product form sums dQ
//                    across key blocks with float atomics (not reproducible) or with an ordered hand-off between resident
//                    workgroups that spin on each other; this library uses neither.  Nobody has measured either form here.
// No float atomics, no flags between workgroups, nothing allocated, cleared or read back; every sum's order depends on L
// alone: results are bit-reproducible, eager or replayed from a graph.  The workspace is delta alone: B H L floats.
// The grid is one-dimensional, tiles x B H <= 2^31 - 1, else MMFS_E_DIMS: never a truncated grid.  Offsets are 64-bit.
//
// A family F states its five differences and nothing else:
//   kD               channels of a head, 64 or 128: the scale (HeadScale<D>, a compile-time property: profiles/attn_core.md),
//                    sqrt(D), the row pitch D + 8, D / 32 matrix-core steps a score and D / 16 channel blocks follow.
//   kCausal          the mask.  false: every key in front of L is live for every row.  true: key t is live for query j iff
//                    t <= j.  It decides where the key walk ends (dkdv: where the query walk begins), which 16-blocks are
//                    skipped, the per-element live test, whether a second product is a plain matrix product or keeps the
//                    blocks on the live side of the diagonal and adds the diagonal block by diag_fma, and the forward's guard
//                    against a row that has seen no live key yet.
//   kAhead, TileRegs, load, put
//                    staging.  put<T>(base, off, ld, r0, L, regs, rows, trans, tid) leaves rows r0 .. r0 + 63 of the head's
//                    slice at base + off in LDS, row-major and / or transposed (either may be null), a row at or behind L as
//                    zeros.  kAhead: the family holds the NEXT tile in registers (TileRegs) while the current one is
//                    multiplied: load<T>(base, off, ld, r0, L, regs, tid) issues its loads -- before the walk for the first
//                    tile, then right behind the barrier that publishes the current one -- and put only stores the registers.
//                    Otherwise put loads and stores and there is no load.  dkdv's -lse sqrt(D) / -delta rows ride along in
//                    the same way (two registers ahead, or fetched where they are stored).
//   Epi...           the backward epilogues: without arguments a scaled store (dq = dQ sc, dk = dK sc, dv = dV); with the
//                    rotary arguments (RopeArgs's members, in its order) the inverse rotation (unrotate_store) with the
//                    position lookup, dkdv forming its per-lane pointers BEFORE the walk.  They are kernel parameters of their
//                    own so that a family without them has the parent's argument block.
//   kHeavyFirst, kWaves
//                    dispatch: forward and dq take the last query tiles (the most keys under a causal mask) first, or index
//                    order; amdgpu_waves_per_eu of {fwd, dq, dkdv}, 0 = the compiler's choice.
//   kLseOptional     the forward's lse may be NULL (no backward follows).
// The device code of both families is, instruction for instruction, what their separate kernels compiled to
// (tools/asm_kernel_diff.py; profiles/attn_train_core.md), and the text below is shaped by that:
//   - the kernels are the __global__ templates themselves: wrapped as a __device__ function behind a thin kernel, the same body
//     got another register allocation;
//   - the epilogues and the row constants stand IN the kernels under ``if constexpr``, not behind the family: a routine is
//     optimised by itself before it is inlined, and there the rotation's null test and its address arithmetic came out
//     differently (other flags, one instruction more or less);
//   - the registers of a tile are a plain array and load / put static functions: as members of one object they were split and
//     numbered differently;
//   - dkdv issues its loads from one closure (load_rows) that captures by reference, as the CLIP kernel always did: what that
//     hides from the interprocedural passes is part of how put compiled.  It is empty for a family that is not kAhead.
#pragma once
#include "mmfs_attn_core.h"
#include <hip/hip_runtime.h>

namespace mmfs {
namespace attn {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kWaveRows = 32;           // fwd, dq: query rows of a wave: two blocks of 16
constexpr int kRows = kWaves * kWaveRows;           // of a workgroup
constexpr int kKT = 64;                 // fwd, dq: keys of a tile
constexpr int kWaveKeys = 32;           // dkdv: keys of a wave: two blocks of 16
constexpr int kKeys = kWaves * kWaveKeys;           // of a workgroup
constexpr int kQT = 64;                 // dkdv: queries of a tile
constexpr int kLdT = 64 + 4;            // elements between rows of a transposed image [channel][64 + 4]
template <int D> constexpr int kLdRows = D + 8;     // of a row-major image [row][D + 8]
template <int D> constexpr float kSqrtD = D == 64 ? 8.f : 11.313708498984761f;

static_assert(kRows == kKeys, "entry_check counts one grid for the three kernels");

template <typename T> __device__ __forceinline__ float bits_f32(uint32_t h) { return to_f32(__builtin_bit_cast(T, (uint16_t)h)); }

// the D / 4 channels 32 st + 8 g .. + 7 (st < D / 32) of one token's head as the fragments of a matrix product; zeros when
// not ``live``
template <typename T, int ST> __device__ __forceinline__ void load_frags(const T *p, const bool live, const int g, s16x8 (&f)[ST])
{
#pragma unroll
    for (int st = 0; st < ST; ++st)
        f[st] = live ? *reinterpret_cast<const s16x8 *>(p + 32 * st + 8 * g) : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
}

// a lane's share of rowsum(a b): the D / 4 channels of its fragments, in ascending order
template <typename T, int ST> __device__ __forceinline__ float frag_dot(const s16x8 (&a)[ST], const s16x8 (&b)[ST])
{
    float d = 0.f;
#pragma unroll
    for (int st = 0; st < ST; ++st)
#pragma unroll
        for (int e = 0; e < 8; ++e) d += bits_f32<T>((uint16_t)a[st][e]) * bits_f32<T>((uint16_t)b[st][e]);
    return d;
}

// ---- the causal mask's second products (mmfs_llama_train.hip, "The diagonal")

// elements 0..3 at p (kept iff keep0), 4..7 at p + 16 (kept iff keep1), zeros otherwise: lds4x2 with the halves that a
// diagonal or dead 16-row block must not bring into the product
__device__ __forceinline__ s16x8 lds4x2_keep(const uint16_t *p, const bool keep0, const bool keep1)
{
    const s16x4 z = {0, 0, 0, 0};
    const s16x4 a = keep0 ? *reinterpret_cast<const s16x4 *>(p) : z, b = keep1 ? *reinterpret_cast<const s16x4 *>(p + 16) : z;
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

// the other operand of a second product: all of it under the full mask (a dead row is zeros, a dead weight 0)
template <bool CAUSAL> __device__ __forceinline__ s16x8 lds4x2_mask(const uint16_t *p, const bool keep0, const bool keep1)
{
    if constexpr (CAUSAL) return lds4x2_keep(p, keep0, keep1);
    else return lds4x2(p);
}

// The diagonal block's share of a second product.  acc[db][r] is (channel 16 db + 4 g + r, column c); ``w`` are this lane's
// four weights of column c, rows 4 g + r of the block (what pack_pair would hand the matrix product); xt points at the
// block's first row in a transposed image [channel][kLdT].  Adds sum over the block's rows i of w(i, c) x(i, channel) for the
// live pairs alone -- LOWER: i <= c (row = key, column = query), else i >= c (row = query, column = key) -- ascending in i;
// a masked pair's product is dropped by a select behind the multiplication, so nothing of it arrives.
template <typename T, bool LOWER, int DB>
__device__ __forceinline__ void diag_fma(f32x4 (&acc)[DB], const float (&w)[4], const uint16_t *xt, const int c, const int g)
{
    float wt[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) wt[i] = __shfl(to_f32((T)w[i & 3]), c + 16 * (i >> 2), 64);
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint16_t *p = xt + (db * 16 + 4 * g + r) * kLdT;
            float a = acc[db][r];
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4) {
                const uint2 raw = *reinterpret_cast<const uint2 *>(p + 4 * i4);
                const float x[4] = {bits_f32<T>(raw.x & 0xffffu), bits_f32<T>(raw.x >> 16), bits_f32<T>(raw.y & 0xffffu),
                                    bits_f32<T>(raw.y >> 16)};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * i4 + e;
                    const float prod = wt[i] * x[e];
                    a += (LOWER ? i <= c : i >= c) ? prod : 0.f;
                }
            }
            acc[db][r] = a;
        }
}

// w[which] of four register rows, ``which`` wave-uniform: selects, so that the rows stay registers
__device__ __forceinline__ void pick_block(const float (&w)[4][4], const int which, float (&o)[4])
{
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = which == 0 ? w[0][r] : which == 1 ? w[1][r] : which == 2 ? w[2][r] : w[3][r];
}

// ---- the inverse rotation of the LLM's backward epilogues (mmfs_llama_train.hip, "Inverse rotation"): D = 128

constexpr int kHalf = 64;               // a channel's rotary partner is kHalf further on

// what attn_train_dq and attn_train_dkdv are handed for it (Epi...), by name
struct RopeArgs {
    const int64_t *pos;                     // [B, L]
    const float *cos_t, *sin_t;             // [max_pos, kHalf]
    int64_t max_pos;
};

__device__ __forceinline__ void load4f(const float *p, float (&o)[4])
{
    const float4 a = *reinterpret_cast<const float4 *>(p);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
}

// acc[db][r] is the gradient of the ROTATED channel 16 db + 4 g + r of one token's head before the factor 1 / sqrt(128);
// -> the gradient of the unrotated row, rounded once, 8 stores of 4 channels.
// cs, sn: the token's row of the tables at this lane's channel 4 g, or null for a position outside [0, max_pos): NaN, as the
// forward made that token's rotated row.  out: the token's row of the head at channel 4 g.
template <typename T>
__device__ __forceinline__ void unrotate_store(const f32x4 (&acc)[8], const float *cs_row, const float *sn_row, T *out)
{
    constexpr float kScale = HeadScale<2 * kHalf>::value;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
        float cs[4], sn[4];
        if (cs_row) {
            load4f(cs_row + db * 16, cs);
            load4f(sn_row + db * 16, sn);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) cs[r] = sn[r] = __builtin_nanf("");
        }
        float lo[4], hi[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float gl = acc[db][r] * kScale, gh = acc[db + 4][r] * kScale;
            lo[r] = gl * cs[r] + gh * sn[r];
            hi[r] = gh * cs[r] - gl * sn[r];
        }
        store4<T>(out + db * 16, lo);
        store4<T>(out + kHalf + db * 16, hi);
    }
}

template <typename T, typename F>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(F::kWaves[0], F::kWaves[0])))
attn_train_fwd(const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v, T *__restrict__ ctx,
               float *__restrict__ lse, const int L, const int H, const int BH)
{
    constexpr int D = F::kD, kST = D / 32, kDB = D / 16, kLdR = kLdRows<D>;
    constexpr bool CAUSAL = F::kCausal;
    constexpr float kScale = HeadScale<D>::value;
    __shared__ __attribute__((aligned(16))) uint16_t sK[kKT * kLdR];
    __shared__ __attribute__((aligned(16))) uint16_t sVt[D * kLdT];
    const int nqt = (L + kRows - 1) / kRows;
    const int rank = blockIdx.x / BH, bh = blockIdx.x - rank * BH, b = bh / H, h = bh - b * H;
    const int q0 = (F::kHeavyFirst ? nqt - 1 - rank : rank) * kRows;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int64_t ld = (int64_t)H * D, off = (int64_t)b * L * ld + (int64_t)h * D;

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

    const int kend = CAUSAL ? min(q0 + kRows, L) : L;                       // keys behind the workgroup's last row are live for nobody
    typename F::TileRegs rk, rv;                                            // a family that holds tiles ahead: the next one, on its way
    if constexpr (F::kAhead) {
        F::template load<T>(k, off, ld, 0, L, rk, tid);
        F::template load<T>(v, off, ld, 0, L, rv, tid);
    }
    for (int k0 = 0; k0 < kend; k0 += kKT) {
        F::template put<T>(k, off, ld, k0, L, rk, sK, nullptr, tid);
        F::template put<T>(v, off, ld, k0, L, rv, nullptr, sVt, tid);
        __syncthreads();
        if constexpr (F::kAhead) {
            if (k0 + kKT < kend) {
                F::template load<T>(k, off, ld, k0 + kKT, L, rk, tid);
                F::template load<T>(v, off, ld, k0 + kKT, L, rv, tid);
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r0 = q0 + wave * kWaveRows + 16 * i;
            if (r0 >= L || (CAUSAL && k0 > r0)) continue;                   // no row, or a tile beyond the block's diagonal (wave-uniform)
            const int jq = r0 + c;
            float s[4][4];
            float tm = -INFINITY;
#pragma unroll
            for (int kb16 = 0; kb16 < 4; ++kb16) {
                const int t0 = k0 + kb16 * 16;
                if (CAUSAL ? t0 > r0 : t0 >= L) {                           // beyond the diagonal, or wholly behind L (wave-uniform)
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
                    const int t = t0 + 4 * g + r;
                    s[kb16][r] = (CAUSAL ? t <= jq : t < L) ? a[r] * kScale : -INFINITY;
                    tm = fmaxf(tm, s[kb16][r]);
                }
            }
            tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
            tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
            // Under the causal mask a block's row may have met no live key yet (mn = -Inf): base keeps -Inf - -Inf out.
            // Under the full mask key 0 is live for every row, so from the first tile on mn is finite wherever the row's
            // scores are numbers: no guard.  (A row whose scores are all NaN keeps mn = -Inf, fmaxf passes NaN over, and
            // -Inf - -Inf makes it NaN, which is what such a row is.)
            const float mn = fmaxf(m[i], tm), base = CAUSAL && mn == -INFINITY ? 0.f : mn;
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
            for (int db = 0; db < kDB; ++db) acc[i][db] *= alpha;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int t0 = k0 + 32 * ks;
                const bool keep0 = t0 < r0, keep1 = t0 + 16 < r0;          // causal: 16-key blocks wholly before the diagonal block
                if (CAUSAL ? keep0 : t0 < L) {                              // else P = 0 (wave-uniform)
                    const s16x8 fp = pack_pair<T>(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
                    for (int db = 0; db < kDB; ++db)
                        acc[i][db] = mma::FwdMma<T>::run(lds4x2_mask<CAUSAL>(sVt + (db * 16 + c) * kLdT + 32 * ks + 4 * g, keep0, keep1),
                                                         fp, acc[i][db]);
                }
            }
            if constexpr (CAUSAL) {
                if (r0 < k0 + kKT) {                                        // the tile holds the block's diagonal block (wave-uniform)
                    float pd[4];
                    pick_block(s, (r0 - k0) >> 4, pd);
                    diag_fma<T, true>(acc[i], pd, sVt + (r0 - k0), c, g);
                }
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
        if ((!F::kLseOptional || lse) && g == 0) lse[(int64_t)bh * L + qi] = m[i] + logf(l[i]);
    }
}

template <typename T, typename F, typename... Epi>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(F::kWaves[1], F::kWaves[1])))
attn_train_dq(const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v, const T *__restrict__ ctx,
              const T *__restrict__ dctx, const float *__restrict__ lse, const Epi... epi, T *__restrict__ dq,
              float *__restrict__ delta, const int L, const int H, const int BH)
{
    constexpr int D = F::kD, kST = D / 32, kDB = D / 16, kLdR = kLdRows<D>;
    constexpr bool CAUSAL = F::kCausal, ROPE = sizeof...(Epi) != 0;
    static_assert(!ROPE || D == 2 * kHalf, "the inverse rotation is written for heads of 128 channels");
    constexpr float kScale = HeadScale<D>::value;
    __shared__ __attribute__((aligned(16))) uint16_t sK[kKT * kLdR];
    __shared__ __attribute__((aligned(16))) uint16_t sKt[D * kLdT];
    __shared__ __attribute__((aligned(16))) uint16_t sV[kKT * kLdR];
    const int nqt = (L + kRows - 1) / kRows;
    const int rank = blockIdx.x / BH, bh = blockIdx.x - rank * BH, b = bh / H, h = bh - b * H;
    const int q0 = (F::kHeavyFirst ? nqt - 1 - rank : rank) * kRows;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int64_t ld = (int64_t)H * D, off = (int64_t)b * L * ld + (int64_t)h * D;

    s16x8 fq[2][kST], fdo[2][kST];
    float nl[2], nd[2];                     // -lse sqrt(D) and -delta of this lane's query
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
        nl[i] = live ? -lse[(int64_t)bh * L + j] * kSqrtD<D> : 0.f;
#pragma unroll
        for (int db = 0; db < kDB; ++db) acc[i][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    const int kend = CAUSAL ? min(q0 + kRows, L) : L;
    typename F::TileRegs rk, rv;                                            // a family that holds tiles ahead: the next one, on its way
    if constexpr (F::kAhead) {
        F::template load<T>(k, off, ld, 0, L, rk, tid);
        F::template load<T>(v, off, ld, 0, L, rv, tid);
    }
    for (int k0 = 0; k0 < kend; k0 += kKT) {
        F::template put<T>(k, off, ld, k0, L, rk, sK, sKt, tid);
        F::template put<T>(v, off, ld, k0, L, rv, sV, nullptr, tid);
        __syncthreads();
        if constexpr (F::kAhead) {
            if (k0 + kKT < kend) {
                F::template load<T>(k, off, ld, k0 + kKT, L, rk, tid);
                F::template load<T>(v, off, ld, k0 + kKT, L, rv, tid);
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r0 = q0 + wave * kWaveRows + 16 * i;
            if (r0 >= L || (CAUSAL && k0 > r0)) continue;                   // (wave-uniform)
            const int jq = r0 + c;
            float ds[4][4];
#pragma unroll
            for (int kb16 = 0; kb16 < 4; ++kb16) {
                const int t0 = k0 + kb16 * 16;
                if (CAUSAL ? t0 > r0 : t0 >= L) {                           // beyond the diagonal, or wholly behind L (wave-uniform)
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
                    const int t = t0 + 4 * g + r;
                    ds[kb16][r] = (CAUSAL ? t <= jq : t < L) ? x : 0.f;
                }
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int t0 = k0 + 32 * ks;
                const bool keep0 = t0 < r0, keep1 = t0 + 16 < r0;
                if (CAUSAL ? keep0 : t0 < L) {                              // (wave-uniform)
                    const s16x8 fs = pack_pair<T>(ds[2 * ks], ds[2 * ks + 1]);
#pragma unroll
                    for (int db = 0; db < kDB; ++db)
                        acc[i][db] = mma::FwdMma<T>::run(lds4x2_mask<CAUSAL>(sKt + (db * 16 + c) * kLdT + 32 * ks + 4 * g, keep0, keep1),
                                                         fs, acc[i][db]);
                }
            }
            if constexpr (CAUSAL) {
                if (r0 < k0 + kKT) {                                        // the tile holds the block's diagonal block (wave-uniform)
                    float dd[4];
                    pick_block(ds, (r0 - k0) >> 4, dd);
                    diag_fma<T, true>(acc[i], dd, sKt + (r0 - k0), c, g);
                }
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int qi = q0 + wave * kWaveRows + 16 * i + c;
        if (qi >= L) continue;
        if constexpr (ROPE) {
            const RopeArgs rope{epi...};
            const int64_t ps = rope.pos[(int64_t)b * L + qi];
            const bool ok = ps >= 0 && ps < rope.max_pos;
            unrotate_store<T>(acc[i], ok ? rope.cos_t + ps * kHalf + 4 * g : nullptr, ok ? rope.sin_t + ps * kHalf + 4 * g : nullptr,
                              dq + off + (int64_t)qi * ld + 4 * g);
        } else {
            T *o = dq + off + (int64_t)qi * ld;
#pragma unroll
            for (int db = 0; db < kDB; ++db) {
                const float out[4] = {acc[i][db][0] * kScale, acc[i][db][1] * kScale, acc[i][db][2] * kScale, acc[i][db][3] * kScale};
                store4<T>(o + db * 16 + 4 * g, out);
            }
        }
    }
}

template <typename T, typename F, typename... Epi>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(F::kWaves[2], F::kWaves[2])))
attn_train_dkdv(const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v, const T *__restrict__ dctx,
                const float *__restrict__ lse, const float *__restrict__ delta, const Epi... epi, T *__restrict__ dk,
                T *__restrict__ dv, const int L, const int H, const int BH)
{
    constexpr int D = F::kD, kST = D / 32, kDB = D / 16, kLdR = kLdRows<D>;
    constexpr bool CAUSAL = F::kCausal, ROPE = sizeof...(Epi) != 0;
    static_assert(!ROPE || D == 2 * kHalf, "the inverse rotation is written for heads of 128 channels");
    constexpr float kScale = HeadScale<D>::value;
    __shared__ __attribute__((aligned(16))) uint16_t sQ[kQT * kLdR];
    __shared__ __attribute__((aligned(16))) uint16_t sQt[D * kLdT];
    __shared__ __attribute__((aligned(16))) uint16_t sO[kQT * kLdR];         // dO
    __shared__ __attribute__((aligned(16))) uint16_t sOt[D * kLdT];
    __shared__ __attribute__((aligned(16))) float sNl[kQT], sNd[kQT];        // -lse sqrt(D), -delta
    // index order; under the causal mask the heaviest key blocks (the first ones: the most queries) are so dispatched first
    const int kt = blockIdx.x / BH, bh = blockIdx.x - kt * BH, b = bh / H, h = bh - b * H;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int64_t ld = (int64_t)H * D, off = (int64_t)b * L * ld + (int64_t)h * D;
    const int kw0 = kt * kKeys + wave * kWaveKeys;                          // the wave's first key

    s16x8 fk[2][kST], fv[2][kST];
    f32x4 dkt[2][kDB], dvt[2][kDB];
    // ROPE: what the epilogue needs of this lane's keys, formed here and held in vector registers: its scalar inputs (five
    // pointers, the table's length) then do not live through the walk, where the scalar registers are short
    const float *cs_row[2], *sn_row[2];
    T *dk_row[2], *dv_row[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int t = kw0 + 16 * i + c;
        const int64_t row = off + (int64_t)min(t, L - 1) * ld;
        if constexpr (ROPE) {
            const RopeArgs rope{epi...};
            const int64_t ps = rope.pos[(int64_t)b * L + min(t, L - 1)];
            const bool ok = ps >= 0 && ps < rope.max_pos;
            cs_row[i] = ok ? rope.cos_t + ps * kHalf + 4 * g : nullptr;
            sn_row[i] = ok ? rope.sin_t + ps * kHalf + 4 * g : nullptr;
            dk_row[i] = dk + row + 4 * g;
            dv_row[i] = dv + row + 4 * g;
            asm volatile("" : "+v"(cs_row[i]), "+v"(sn_row[i]), "+v"(dk_row[i]), "+v"(dv_row[i]));
        }
        load_frags<T>(k + row, t < L, g, fk[i]);
        load_frags<T>(v + row, t < L, g, fv[i]);
#pragma unroll
        for (int db = 0; db < kDB; ++db) dkt[i][db] = dvt[i][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    const int qbeg = CAUSAL ? kt * kKeys : 0;                               // queries before the workgroup's first key see none of its keys
    typename F::TileRegs rq, ro;
    // the row constants -lse sqrt(D) and -delta of row q0 + tid (lanes < kQT; 0 at or behind L) ride along with the tiles
    float rl = 0.f, rd = 0.f;
    // kAhead: the next query tile, on its way.  (A closure that captures by reference, empty otherwise: the header's comment
    // says what that is to the compiler.)
    const auto load_rows = [&](const int q0) {
        if constexpr (F::kAhead) {
            F::template load<T>(q, off, ld, q0, L, rq, tid);
            F::template load<T>(dctx, off, ld, q0, L, ro, tid);
            const bool live = tid < kQT && q0 + tid < L;
            rl = live ? -lse[(int64_t)bh * L + q0 + tid] * kSqrtD<D> : 0.f;
            rd = live ? -delta[(int64_t)bh * L + q0 + tid] : 0.f;
        }
    };
    load_rows(qbeg);
    for (int q0 = qbeg; q0 < L; q0 += kQT) {
        F::template put<T>(q, off, ld, q0, L, rq, sQ, sQt, tid);
        F::template put<T>(dctx, off, ld, q0, L, ro, sO, sOt, tid);
        if (tid < kQT) {
            if constexpr (F::kAhead) {
                sNl[tid] = rl;
                sNd[tid] = rd;
            } else {
                const bool live = q0 + tid < L;
                sNl[tid] = live ? -lse[(int64_t)bh * L + q0 + tid] * kSqrtD<D> : 0.f;
                sNd[tid] = live ? -delta[(int64_t)bh * L + q0 + tid] : 0.f;
            }
        }
        __syncthreads();
        if (q0 + kQT < L) load_rows(q0 + kQT);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int t0 = kw0 + 16 * i;                                    // the key block
            if (t0 >= L || (CAUSAL && q0 + kQT <= t0)) continue;            // no key, or a tile before the block's diagonal (wave-uniform)
            const int tk = t0 + c;
            float p[4][4], ds[4][4];
#pragma unroll
            for (int qs = 0; qs < 4; ++qs) {
                const int j0 = q0 + 16 * qs;
                if (CAUSAL ? j0 < t0 : j0 >= L) {                           // before the diagonal, or wholly behind L (wave-uniform)
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
                    const int j = j0 + 4 * g + r;
                    const bool live = (!CAUSAL || tk <= j) && j < L;        // (a dead query's row is zeros: exp(0) = 1, not 0)
                    const float pr = exp_hw(a[r] * kScale);
                    const float x = pr * dp[r];
                    p[qs][r] = live ? pr : 0.f;
                    ds[qs][r] = live ? x : 0.f;
                }
            }
#pragma unroll
            for (int qp = 0; qp < 2; ++qp) {
                const int j0 = q0 + 32 * qp;
                const bool keep0 = j0 > t0, keep1 = j0 + 16 > t0;           // causal: 16-query blocks wholly behind the diagonal block
                if (CAUSAL ? keep1 : j0 < L) {                              // (wave-uniform)
                    const s16x8 fp = pack_pair<T>(p[2 * qp], p[2 * qp + 1]), fds = pack_pair<T>(ds[2 * qp], ds[2 * qp + 1]);
#pragma unroll
                    for (int db = 0; db < kDB; ++db) {
                        dvt[i][db] = mma::FwdMma<T>::run(lds4x2_mask<CAUSAL>(sOt + (db * 16 + c) * kLdT + 32 * qp + 4 * g, keep0, keep1),
                                                         fp, dvt[i][db]);
                        dkt[i][db] = mma::FwdMma<T>::run(lds4x2_mask<CAUSAL>(sQt + (db * 16 + c) * kLdT + 32 * qp + 4 * g, keep0, keep1),
                                                         fds, dkt[i][db]);
                    }
                }
            }
            if constexpr (CAUSAL) {
                if (t0 >= q0) {                                             // the tile holds the block's diagonal block (wave-uniform)
                    float pd[4], dd[4];
                    pick_block(p, (t0 - q0) >> 4, pd);
                    pick_block(ds, (t0 - q0) >> 4, dd);
                    diag_fma<T, false>(dvt[i], pd, sOt + (t0 - q0), c, g);
                    diag_fma<T, false>(dkt[i], dd, sQt + (t0 - q0), c, g);
                }
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int t = kw0 + 16 * i + c;
        if (t >= L) continue;
        if constexpr (ROPE) {
#pragma unroll
            for (int db = 0; db < kDB; ++db) {
                const float out[4] = {dvt[i][db][0], dvt[i][db][1], dvt[i][db][2], dvt[i][db][3]};
                store4<T>(dv_row[i] + db * 16, out);
            }
            unrotate_store<T>(dkt[i], cs_row[i], sn_row[i], dk_row[i]);
        } else {
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
}

// ---- host side: what the two families' entries do alike

// every entry's checks behind the family's own (``rc``: clip_check, llama_train_check) and of the rotary table's length (0
// where there is none); ``empty``: OK without a launch
inline int train_entry_check(int rc, int64_t B, int64_t H, int64_t L, int64_t max_pos, bool &empty)
{
    empty = false;
    if (rc) return rc;
    if (max_pos < 0 || max_pos > (1LL << 40)) return MMFS_E_DIMS;
    // the grid is tiles x B H in one dimension (kRows == kKeys: the same count for the three kernels)
    if ((L + kRows - 1) / kRows * B * H > ((int64_t)1 << 31) - 1 || B * L > (1LL << 32) || B * L * H > (1LL << 34)) return MMFS_E_DIMS;
    empty = B * H * L == 0;
    return MMFS_OK;
}

// *_tiles(level): how the kernels cut their work
inline int64_t train_tiles(int level)
{
    return level == 0 ? kRows : level == 1 ? kKT : level == 2 ? kKeys : level == 3 ? kQT : level == 4 ? kWaveRows : MMFS_E_DIMS;
}

// *_workspace_bytes: delta
inline int64_t train_workspace_bytes(int64_t B, int64_t H, int64_t L, int64_t max_L)
{
    if (batch_heads_check(MMFS_F16, B, H, L, 0, 0) || L > max_L) return MMFS_E_DIMS;       // (no dtype to ask about)
    return B * H * L * (int64_t)sizeof(float);
}

}  // namespace attn
}  // namespace mmfs
