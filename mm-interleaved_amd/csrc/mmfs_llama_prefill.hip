// mmfs_llama_prefill.hip -- the LLM's self-attention over a prompt: what mmfs_llama_attn.hip's decode
// kernel is to one new token, for Lq new tokens a row, read from the same in-place key / value cache.  Inference only.
//
// llama_rope_append has already written slots length .. length + Lq - 1; this kernel only reads the cache, ``src_row`` and
// the device word ``length`` (the tokens held BEFORE the call).  For query j < Lq of row b, head h, n = length + Lq:
//     context[b, j, h] = softmax_t( s(j, t) ) . V[src_row[b, t], h, t]                 over keys t < n
//     s(j, t) = q_rot[b, j, h] . K[src_row[b, t], h, t] / sqrt(128) + bias(b, j, t)
// q_rot and context [B, Lq, H 128] token-major, the cache of a layer [B, H, cap, 128], T = bf16 / fp16, arithmetic in fp32,
// p rounded to T where it enters the second matrix product (v_mfma_f32_16x16x32_{bf16,f16}), one launch.
//
// Mask.  ``bias`` is HF's extended mask read where it lies: fp32 or T, a batch stride (0: one shared batch row), a query
// stride (0: one row for all queries), ``bias_len`` (keys at or behind it carry no bias); only element-size alignment is
// assumed: every entry is its own load, 64 neighbours a wave -- unless every row happens to start 4 elements aligned (the
// pointer and both strides), when a lane loads 4 neighbouring keys at once.  Flag CAUSAL adds the reference's _make_causal_mask: key t is
// excluded for query j iff t > length + j, so a [B, 1, 1, kv] padding row gives HF's whole prompt mask without an Lq x kv
// tensor.
// Masked keys: a key whose bias is at or below finfo(T).min, or which the causal flag excludes, has the score
// max(bias, finfo(T).min) = finfo(T).min; the product is not used.  The max is what the reference's
// ``max(scores + mask, finfo.min)`` does to HF's prompt mask, which is ``expanded + causal`` in T and holds
// finfo.min + finfo.min = -Inf at the pad-key x future-key entries of a left-padded row: a padded query row is the FINITE
// uniform average of all n value rows, not NaN.  (The decode kernel keeps a -Inf bias as the score: a row of them is NaN
// there, as softmax(-Inf ..) is.  A single token's mask is a padding row alone and never holds such a sum.)  In fp16 the
// framework's -65504 + s parts from this at s >= 16 exactly as score_of's comment in mmfs_attn_core.h says.
// Slots at or behind n are never live: their K and V rows are REPLACED by zeros as a tile is staged (their score is -Inf,
// p = 0) -- a NaN there reaches no product.  A src_row entry outside [0, B) is never dereferenced: that key's K and V are
// NaN, so the error shows.  Query rows at or behind Lq in the last tile repeat row Lq - 1 and are not stored.
//
//   llama_attn_prefill   Workgroup of 4 waves = 128 query rows of one (b, h); a wave owns 32 of them as two 16-query
//                        blocks.  Grid: ceil(Lq / 128) x B H workgroups, from (B, H, Lq) alone, the heaviest (last) query
//                        tiles first; the key loop's end comes from the device word, so the launch can be captured.
//                        q fragments come straight from global memory once.  Key tiles of 64 through LDS, shared by the
//                        workgroup: the tile's 64 src_row entries are one coalesced load a wave, handed round by shuffles;
//                        K row-major [key][128 + 8], V TRANSPOSED [channel][64 + 4] (a lane loads 8 channels of 4
//                        neighbouring keys and writes 8 x 8 bytes), the bias tile in fp32 ([128][64 + 4], or one row when
//                        the query stride is 0; with a row per query it is staged BEFORE K and V, so that a tile the mask
//                        excludes for every row -- the upper triangle of HF's prompt mask -- is dropped for the price of its
//                        mask entries and one barrier).  A wave forms S^T = K q^T (key on the accumulator's rows, query on the
//                        lane: a lane holds 16 scores of ONE query) and keeps one running (m, l) per lane and O^T in 64
//                        accumulator registers a block, as mmfs_attn.hip does:
//                            m' = max(m, tile max);  base = m' == -Inf ? 0 : m';  a = exp(m - base)
//                            p = exp(s - base);  l = l a + sum p;  O^T = O^T a + V^T p^T
//                        m starts at -Inf and l at 0; ``base`` keeps -Inf out of the subtractions, so a row whose first
//                        tiles hold no live key at all is still right.  The S^T accumulators, packed to T, ARE the B
//                        operand of V^T p^T (cdna_hip_programming.md 3); no trip through LDS.
//   Tile skipping        Every masked score is exactly finfo(T).min, so a tile whose entries are masked for every row of
//                        the workgroup needs no product if every p would be 0: decided from the tile's largest effective
//                        bias (finfo.min at a masked entry, +Inf at a NaN; reduced as the tile is staged, no extra
//                        barrier) and the smallest running m of the workgroup's rows (one word a wave, written behind the
//                        tile's products): the tile is skipped iff that largest bias is finfo.min and
//                        min m - finfo.min >= 1024: then alpha = exp(0) = 1 and p = exp2(<= -1477) = 0 exactly in fp32,
//                        (m, l, O) would not move by a bit.  A row with m == finfo.min (masked throughout so far) or
//                        m == -Inf forbids the skip.  With CAUSAL, tiles wholly beyond the diagonal of the workgroup's last
//                        row take this decision before anything is read, and end the walk.  Flag VISIT_ALL turns all of it
//                        off (tests).
// No atomics, no flags between workgroups, nothing allocated, cleared or read back; every sum has a fixed order that
// depends on (length, Lq) alone: results are bit-reproducible, eager or replayed.
//
// Resources (make asm, gfx950; no spills, no scratch):
//                                VGPRs  AGPRs  LDS bytes  waves / SIMD
//   llama_attn_prefill  bf16      217    0      69680      2
//   llama_attn_prefill  fp16      217    0      69680      2
// The kernel asks for 2 waves per SIMD (amdgpu_waves_per_eu; two workgroups a CU, which is also what the LDS allows): left
// alone the compiler takes 210 VGPRs + 64 AGPRs for one.  The wide bias path's row loop stays rolled: unrolled, its 8 row
// addresses are hoisted out of the key walk and 14 registers spill.
//
// Error bounds: mmfs_llama_attn.hip's E_s, E_p and context bound with n = length + Lq (tests/llama_attn_refs.py, attend64,
// evaluates them; it is handed the mask clamped at finfo(T).min).  The order of roundings here adds nothing they lack:
// s is 4 matrix-core steps of 32 fp32 accumulations, the scaling and the bias (c_n = 160 covers 128 + 2); p is rounded
// to T before the second product as the framework's softmax is (the u in E_p); the sums over n keys run in tiles of 64
// with one rescaling a tile: at most n / 64 + 1 further roundings a row on top of the n additions, inside c_e = 256 + n.
//
// Offsets are 64-bit.
#include "mmfs_attn_core.h"
#include <hip/hip_runtime.h>

namespace mmfs {

namespace {

using namespace attn;

constexpr int kD = kLlamaD;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kWaveRows = 32;           // query rows of a wave: two blocks of 16
constexpr int kRows = kWaves * kWaveRows;           // of a workgroup
constexpr int kKT = 64;                 // keys of a tile
constexpr int kLdK = kD + 8;            // elements between rows of the key tile [key][128 + 8]
constexpr int kLdV = kKT + 4;           // of the transposed value tile [channel][64 + 4]
constexpr int kLdB = kKT + 4;           // floats between rows of the bias tile
constexpr float kScale = HeadScale<kD>::value;
constexpr float kSkipMargin = 1024.f;   // m - finfo.min at or above it: exp2((finfo.min - m) log2 e) is exactly 0
constexpr unsigned kCausal = MMFS_LLAMA_PREFILL_CAUSAL, kVisitAll = MMFS_LLAMA_PREFILL_VISIT_ALL;

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}

template <typename T>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
llama_attn_prefill(const T *__restrict__ q_rot, const T *__restrict__ kc, const T *__restrict__ vc,
                   const int32_t *__restrict__ src_row, const int32_t *__restrict__ length, const void *__restrict__ bias,
                   const int bias_f32, const int bias_wide_, const int64_t bias_bs, const int64_t bias_qs, const int bias_len,
                   const unsigned flags,
                   T *__restrict__ ctx, const int B, const int Lq, const int H, const int64_t cap, const int BH)
{
    __shared__ __attribute__((aligned(16))) uint16_t sK[kKT * kLdK];
    __shared__ __attribute__((aligned(16))) uint16_t sVt[kD * kLdV];
    __shared__ __attribute__((aligned(16))) float sB[kRows * kLdB];
    __shared__ float sMax[2][kWaves], sMin[kWaves];
    constexpr float low = Lowest<T>::value;
    // the heaviest query tiles (the last ones: the most keys under a causal mask) are dispatched first
    const int nqt = (Lq + kRows - 1) / kRows;
    const int rank = blockIdx.x / BH, bh = blockIdx.x - rank * BH, b = bh / H, h = bh - b * H;
    const int q0 = (nqt - 1 - rank) * kRows, qlast = min(q0 + kRows, Lq) - 1;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int64_t len = length[0];
    const int64_t n64 = len + Lq;
    const int n = (int)(n64 < 0 ? 0 : n64 > cap ? cap : n64);               // the live keys
    const bool causal = flags & kCausal, visit_all = flags & kVisitAll, per_query = bias && bias_qs != 0;
    const bool bias_wide = per_query && bias_wide_;

    // this lane's query of block i: row q0 + 32 wave + 16 i + c (a row at or behind Lq repeats row Lq - 1)
    s16x8 fq[2][4];
    int jq[2];
    bool active[2];
    float m[2], l[2];
    f32x4 acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r0 = q0 + wave * kWaveRows + 16 * i;
        active[i] = r0 < Lq;                                                // (wave-uniform)
        jq[i] = min(r0 + c, Lq - 1);
        const T *qp = q_rot + (((int64_t)b * Lq + jq[i]) * H + h) * kD + 8 * g;
#pragma unroll
        for (int st = 0; st < 4; ++st) fq[i][st] = *reinterpret_cast<const s16x8 *>(qp + 32 * st);
        m[i] = -INFINITY;
        l[i] = 0.f;
#pragma unroll
        for (int db = 0; db < 8; ++db) acc[i][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // the smallest running m of a wave's rows; a wave without rows forbids nothing
    if (lane == 0) sMin[wave] = active[0] ? -INFINITY : INFINITY;
    __syncthreads();

    const int cg = tid & 15, kq = tid >> 4;                                 // staging: channels 8 cg .. + 7 of keys 4 kq .. + 3
    const T *kb = kc + (int64_t)h * cap * kD + 8 * cg;
    const T *vb = vc + (int64_t)h * cap * kD + 8 * cg;
    const int64_t row_stride = (int64_t)H * cap * kD;

    // K row-major and V transposed of keys k0 .. k0 + 63: src_row is one coalesced load a wave, handed round by shuffles
    auto stage_kv = [&](const int k0) {
        const int mine = k0 + lane;
        int row_l = -1;                                                     // -1: behind n (zeros), -2: no valid row (NaN)
        if (mine < n) {
            row_l = src_row[(int64_t)b * cap + mine];
            if ((unsigned)row_l >= (unsigned)B) row_l = -2;
        }
        uint4 vr[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int key = 4 * kq + e;
            const int r = __shfl(row_l, key, 64);
            uint4 kw = make_uint4(0u, 0u, 0u, 0u), vw = kw;
            if (r >= 0) {
                const int64_t at = r * row_stride + (int64_t)(k0 + key) * kD;
                kw = *reinterpret_cast<const uint4 *>(kb + at);
                vw = *reinterpret_cast<const uint4 *>(vb + at);
            } else if (r == -2) {
                kw = vw = make_uint4(Lowest<T>::nan2, Lowest<T>::nan2, Lowest<T>::nan2, Lowest<T>::nan2);
            }
            *reinterpret_cast<uint4 *>(sK + key * kLdK + 8 * cg) = kw;
            vr[e] = vw;
        }
        const uint32_t w[4][4] = {{vr[0].x, vr[0].y, vr[0].z, vr[0].w}, {vr[1].x, vr[1].y, vr[1].z, vr[1].w},
                                  {vr[2].x, vr[2].y, vr[2].z, vr[2].w}, {vr[3].x, vr[3].y, vr[3].z, vr[3].w}};
#pragma unroll
        for (int pr = 0; pr < 4; ++pr) {                                    // channels 2 pr (low halves), 2 pr + 1 (high halves)
            uint2 lo, hi;
            lo.x = (w[0][pr] & 0xffffu) | (w[1][pr] << 16);
            lo.y = (w[2][pr] & 0xffffu) | (w[3][pr] << 16);
            hi.x = (w[0][pr] >> 16) | (w[1][pr] & 0xffff0000u);
            hi.y = (w[2][pr] >> 16) | (w[3][pr] & 0xffff0000u);
            *reinterpret_cast<uint2 *>(sVt + (8 * cg + 2 * pr) * kLdV + 4 * kq) = lo;
            *reinterpret_cast<uint2 *>(sVt + (8 * cg + 2 * pr + 1) * kLdV + 4 * kq) = hi;
        }
    };
    // the bias tile (lane = key, a wave takes every fourth row, 8 loads in flight), and its largest effective entry: finfo.min
    // where the key is masked (for the shared row: for every row of the workgroup), +Inf at a NaN
    auto stage_bias = [&](const int k0, float *sMaxT) {
        const int t = k0 + lane;
        const bool read = bias && t < bias_len && t < n;
        float tmax = -INFINITY;
        auto fetch = [&](int j) {
            const int64_t at = (int64_t)b * bias_bs + (per_query ? (int64_t)j * bias_qs : 0) + t;
            return !read ? 0.f : bias_f32 ? static_cast<const float *>(bias)[at] : to_f32(static_cast<const T *>(bias)[at]);
        };
        auto keep = [&](int row, int j, float val) {
            sB[row * kLdB + lane] = val;
            if (t < n) {
                const bool masked = val <= low || (causal && t > len + j);
                tmax = fmaxf(tmax, val != val ? INFINITY : masked ? low : val);
            }
        };
        if (bias_wide) {
            // rows that start 4 elements aligned: a lane loads 4 neighbouring keys at once (8 or 16 bytes), 16 lanes a row,
            // 4 rows a wave and load; a group of 4 that crosses the end of the bias or of the live keys goes key by key
            const int rg = lane >> 4, c4 = 4 * (lane & 15), t4 = k0 + c4, lim = min(bias_len, n);
            const bool whole = t4 + 3 < lim;
            auto row_of = [&](int u) { return 16 * u + 4 * wave + rg; };
            auto at_of = [&](int row) { return (int64_t)b * bias_bs + (int64_t)min(q0 + row, Lq - 1) * bias_qs + t4; };
            auto keep4 = [&](int row, int64_t at, float (&val)[4]) {
                const int j = min(q0 + row, Lq - 1);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (!whole)
                        val[e] = t4 + e >= lim ? 0.f : bias_f32 ? static_cast<const float *>(bias)[at + e]
                                                                : to_f32(static_cast<const T *>(bias)[at + e]);
                    if (t4 + e < n) {
                        const bool masked = val[e] <= low || (causal && t4 + e > len + j);
                        tmax = fmaxf(tmax, val[e] != val[e] ? INFINITY : masked ? low : val[e]);
                    }
                }
                *reinterpret_cast<float4 *>(sB + row * kLdB + c4) = make_float4(val[0], val[1], val[2], val[3]);
            };
            if (bias_f32) {
#pragma unroll 1
                for (int u0 = 0; u0 < 8; u0 += 2) {                         // (rolled: unrolled, the 8 row addresses live through the key walk)
                    float4 raw[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        raw[u] = whole ? *reinterpret_cast<const float4 *>(static_cast<const float *>(bias) + at_of(row_of(u0 + u)))
                                       : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        float val[4] = {raw[u].x, raw[u].y, raw[u].z, raw[u].w};
                        keep4(row_of(u0 + u), at_of(row_of(u0 + u)), val);
                    }
                }
            } else {
#pragma unroll 1
                for (int u0 = 0; u0 < 8; u0 += 4) {
                    uint2 raw[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        raw[u] = whole ? *reinterpret_cast<const uint2 *>(static_cast<const T *>(bias) + at_of(row_of(u0 + u)))
                                       : make_uint2(0u, 0u);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        float val[4] = {to_f32(__builtin_bit_cast(T, (uint16_t)(raw[u].x & 0xffffu))),
                                        to_f32(__builtin_bit_cast(T, (uint16_t)(raw[u].x >> 16))),
                                        to_f32(__builtin_bit_cast(T, (uint16_t)(raw[u].y & 0xffffu))),
                                        to_f32(__builtin_bit_cast(T, (uint16_t)(raw[u].y >> 16)))};
                        keep4(row_of(u0 + u), at_of(row_of(u0 + u)), val);
                    }
                }
            }
        } else if (per_query) {
            for (int r0 = wave; r0 < kRows; r0 += 8 * kWaves) {
                float val[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) val[u] = fetch(min(q0 + r0 + kWaves * u, Lq - 1));
#pragma unroll
                for (int u = 0; u < 8; ++u) keep(r0 + kWaves * u, min(q0 + r0 + kWaves * u, Lq - 1), val[u]);
            }
        } else if (wave == 0) {
            keep(0, qlast, fetch(0));
        }
        tmax = wave_max(tmax);
        if (lane == 0) sMaxT[wave] = tmax;
    };

    for (int k0 = 0; k0 < n; k0 += kKT) {
        const float min_m = fminf(fminf(sMin[0], sMin[1]), fminf(sMin[2], sMin[3]));
        const bool may_skip = !visit_all && min_m - low >= kSkipMargin;     // (workgroup-uniform; false at -Inf, finfo.min, NaN)
        if (causal && k0 > len + qlast && may_skip) break;                  // beyond the diagonal: so is every later tile

        // ---- stage the tile.  A bias of one row for all queries costs nothing next to K and V: everything is staged, then
        // the tile's largest bias decides.  A bias with a row per query is staged FIRST: a tile it masks for every row (the
        // upper triangle of HF's prompt mask) is dropped before its K and V are read, for one more barrier.
        float *const sMaxT = sMax[(k0 / kKT) & 1];                          // (two sets: a skipped tile has no closing barrier)
        if (per_query) {
            stage_bias(k0, sMaxT);
            __syncthreads();
            if (may_skip && fmaxf(fmaxf(sMaxT[0], sMaxT[1]), fmaxf(sMaxT[2], sMaxT[3])) <= low) continue;
            stage_kv(k0);
            __syncthreads();
        } else {
            stage_kv(k0);
            stage_bias(k0, sMaxT);
            __syncthreads();
            if (may_skip && fmaxf(fmaxf(sMaxT[0], sMaxT[1]), fmaxf(sMaxT[2], sMaxT[3])) <= low) continue;
        }
        {
            float wmin = INFINITY;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (!active[i]) continue;                                   // (wave-uniform)
                const float *brow = sB + (per_query ? (wave * kWaveRows + 16 * i + c) * kLdB : 0);
                float s[4][4];
                float tm = -INFINITY;
#pragma unroll
                for (int kb16 = 0; kb16 < 4; ++kb16) {
                    f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int st = 0; st < 4; ++st)
                        a = mma::FwdMma<T>::run(lds8(sK + (kb16 * 16 + c) * kLdK + 32 * st + 8 * g), fq[i][st], a);
                    const float4 bs4 = *reinterpret_cast<const float4 *>(brow + kb16 * 16 + 4 * g);
                    const float bs[4] = {bs4.x, bs4.y, bs4.z, bs4.w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int t = k0 + kb16 * 16 + 4 * g + r;
                        const bool masked = bs[r] <= low || (causal && t > len + jq[i]);
                        s[kb16][r] = t >= n ? -INFINITY : masked ? low : a[r] * kScale + bs[r];
                        tm = fmaxf(tm, s[kb16][r]);
                    }
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
                wmin = mn != mn ? -INFINITY : fminf(wmin, mn);               // (a NaN forbids the skip as -Inf does)
#pragma unroll
                for (int db = 0; db < 8; ++db) acc[i][db] *= alpha;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const s16x8 fp = pack_pair<T>(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
                    for (int db = 0; db < 8; ++db)
                        acc[i][db] = mma::FwdMma<T>::run(lds4x2(sVt + (db * 16 + c) * kLdV + 32 * ks + 4 * g), fp, acc[i][db]);
                }
            }
            wmin = -wave_max(-wmin);
            if (lane == 0) sMin[wave] = wmin;
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int qi = q0 + wave * kWaveRows + 16 * i + c;
        if (qi >= Lq) continue;
        T *o = ctx + (((int64_t)b * Lq + qi) * H + h) * kD;
#pragma unroll
        for (int db = 0; db < 8; ++db) {
            const float out[4] = {acc[i][db][0] / l[i], acc[i][db][1] / l[i], acc[i][db][2] / l[i], acc[i][db][3] / l[i]};
            store4<T>(o + db * 16 + 4 * g, out);
        }
    }
}

}  // namespace
}  // namespace mmfs

extern "C" {

int64_t mmfs_llama_attn_prefill_tiles(int level)
{
    return level == 0 ? mmfs::kWaveRows : level == 1 ? mmfs::kRows : level == 2 ? mmfs::kKT : MMFS_E_DIMS;
}

int mmfs_llama_attn_prefill(int dtype, const void *q_rot, const void *k_cache, const void *v_cache, const int32_t *src_row,
                            const int32_t *length, const void *bias, int bias_dtype, int64_t bias_batch_stride,
                            int64_t bias_query_stride, int64_t bias_len, unsigned flags, void *context, int64_t B, int64_t Lq,
                            int64_t H, int64_t D, int64_t cap, void *stream)
{
    using namespace mmfs;
    int rc = llama_check(dtype, B, H, D, Lq, cap);
    if (rc) return rc;
    if (flags & ~(kCausal | kVisitAll)) return MMFS_E_DIMS;
    int bias_f32;
    rc = llama_bias(bias, bias_dtype, dtype, bias_len, bias_f32);
    if (rc) return rc;
    if (bias) {
        constexpr int64_t kMaxStride = (int64_t)1 << 40;
        if (bias_query_stride != 0 && (bias_query_stride < bias_len || bias_query_stride > kMaxStride)) return MMFS_E_DIMS;
        // what the queries of one batch row span
        const int64_t extent = bias_query_stride ? (Lq - 1) * bias_query_stride + bias_len : bias_len;
        if (bias_batch_stride != 0 && (bias_batch_stride < extent || bias_batch_stride > kMaxStride)) return MMFS_E_DIMS;
    }
    const int64_t tiles = (Lq + kRows - 1) / kRows;
    if (tiles * B * H > ((int64_t)1 << 31) - 1) return MMFS_E_DIMS;
    if (B * H == 0) return MMFS_OK;
    if ((rc = check_tensors({{q_rot, 16}, {k_cache, 16}, {v_cache, 16}, {src_row, 4}, {length, 4}, {context, 16},
                             maybe(bias, bias_f32 ? 4 : 2)})))
        return rc;
    // a bias with a row per query whose rows all start 4 elements aligned is read 4 keys a lane
    const int bias_wide = bias && bias_query_stride && (uintptr_t)bias % (bias_f32 ? 16 : 8) == 0 && bias_query_stride % 4 == 0 &&
                          bias_batch_stride % 4 == 0;
    return by_half_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(llama_attn_prefill<T>, dim3((unsigned)(tiles * B * H)), dim3(kThreads), 0, (hipStream_t)stream,
                           (const T *)q_rot, (const T *)k_cache, (const T *)v_cache, src_row, length, bias, bias_f32,
                           bias_wide, bias_batch_stride, bias_query_stride, (int)bias_len, flags, (T *)context, (int)B, (int)Lq, (int)H, cap,
                           (int)(B * H));
        return (int)hipGetLastError();
    });
}

}  // extern "C"
