// mmfs_llama_train.hip -- the LLM's self-attention in TRAINING: what the reference's _forward_train
// (mm_interleaved/models/utils/monkey_patch/llama_flash_attn_train_monkey_patch.py:35-82) asks of flash_attn_func(q, k, v,
// 0.0, softmax_scale=None, causal=True) between the three Linear layers and o_proj, forward and backward, without a tensor
// of size L x L.  No cache, no src_row, no bias: q, k, v, dO and every output are token-major [B, L, H 128] of T (bf16 /
// fp16) as the Linear layers produce and consume them; arithmetic is fp32; D = 128.
//     q_rot, k_rot = rope(q), rope(k)                                        (llama_train_rope)
//     s(j, t)      = q_rot[b, j, h] . k_rot[b, t, h] / sqrt(128)             key t is live for query j iff t <= j
//     context      = softmax_t(s) v,   lse = ln sum_t exp s                  (llama_train_fwd)
//     dq, dk, dv   of the UNROTATED q, k and of v                            (llama_train_dq, llama_train_dkdv)
// A masked score is SELECTED (to -Inf forward, p = ds = 0 backward), never added to, and a product over a 16 x 16 block
// that the diagonal crosses is not a matrix product at all (below): a NaN in token t's k or v reaches no query j < t, a NaN
// in query j's dO reaches no dk, dv of a key t > j.  Rows at or behind L in a partial tile are staged as zeros and never stored.
//
//   llama_train_rope    llama_rope_append's rotation without the cache: 8 lanes a (token, head), fp32, one rounding;
//                       a position outside [0, max_pos) makes that token's q_rot and k_rot NaN.
//   llama_train_fwd     llama_attn_prefill's organisation.  Workgroup of 4 waves = 128 query rows of one (b, h), a wave owns
//                       32 of them as two 16-query blocks; grid ceil(L / 128) x B H, the heaviest (last) query tiles first.
//                       Key tiles of 64 through LDS up to the diagonal only: K row-major [key][128 + 8], V transposed
//                       [channel][64 + 4].  S^T = K q^T (key on the accumulator's rows, query on the lane), online softmax
//                       with one running (m, l) a lane, P rounded to T; the packed S^T accumulators are the B operand of
//                       O^T += V^T P^T.  context and lse = m + ln l (fp32, [B, H, L]) are written once.
//   llama_train_dq      query-stationary, the forward's grid and tiles.  A wave first forms delta[b, h, j] = sum_c dO O (fp32,
//                       32 channels a lane, then the four lane groups in a fixed order) for its rows and writes it to the
//                       workspace; q_rot and dO fragments stay in registers.  Per key tile: K row-major AND transposed, V
//                       row-major.  S'^T = K q^T - lse sqrt(128) and dP'^T = V dO^T - delta come out of their chains ready
//                       (the row constants are the initial accumulators: cdna_hip_programming.md, Appendix B);
//                       P = exp(S' / sqrt(128)), dS^T = P (dP'), rounded to T where it enters dQ^T += K^T dS^T: 64
//                       accumulator registers a block for the whole walk.
//   llama_train_dkdv    key-stationary, launched behind dq (it reads delta).  Workgroup of 4 waves = 128 keys of one (b, h),
//                       a wave owns 32 of them as two 16-key blocks and keeps their k_rot and v fragments and dK^T, dV^T
//                       (128 accumulator registers) while the workgroup sweeps the query tiles of 64 from its own to the
//                       end: Q and dO row-major and transposed, -lse sqrt(128) and -delta.  S' and dP' with the KEY ON THE
//                       LANE: their packed accumulators are the B operands of dV^T += dO^T P and dK^T += Q^T dS.  Grid
//                       ceil(L / 128) x B H, the heaviest (first) key blocks first.
//   The diagonal        A 16 x 16 block of (query, key) pairs that the diagonal crosses holds live and masked pairs, and a
//                       matrix product over it would multiply a masked pair's 0 with whatever the other operand holds
//                       (0 x NaN).  So in the second products (V^T P^T; K^T dS^T; dO^T P, Q^T dS) the other operand's 16
//                       rows of such a block -- and of every block beyond the diagonal -- are replaced by zeros, and the
//                       block's own share is added by diag_fma: 16 lane shuffles hand a lane the 16 weights of its
//                       column (rounded to T, as the matrix product takes them), and it adds the products of the live
//                       pairs alone in ascending order, 512 selected multiply-adds a lane and block.  One such block a
//                       query block (fwd, dq) or key block (dkdv) and launch.  In dq this covers k as well: a NaN in token
//                       t's k reaches no dq of a query j < t.
//   Inverse rotation    RoPE is orthogonal: dq = R^T dq_rot = g cos - rotate_half(g) sin.  A lane holds channel
//                       16 db + 4 g + r and its partner 64 further on (db + 4) of one token, so both kernels rotate their fp32
//                       accumulators (times 1 / sqrt(128)) in the epilogue and round ONCE; there is no third kernel and no
//                       fp32 dq_rot / dk_rot in memory.  The workspace is delta alone: B H L floats.
//   Seven products      S and dP are computed in both backward kernels: 7 matrix products a (query tile, key tile) pair,
//                       14 B H L^2 128 / 2 FLOPs under the causal mask, against the 5 (10 ..) of a single key-stationary
//                       kernel: 40 % more matrix-core work.  The five-product form sums dQ across key blocks with float
//                       atomics (not reproducible) or with an ordered hand-off between resident workgroups that spin on
//                       each other; this library uses neither.  Nobody has measured either form here.
// No float atomics, no flags between workgroups, nothing allocated, cleared or read back; every sum's order depends on L
// alone: results are bit-reproducible, eager or replayed from a graph.
//
// Resources (make asm, gfx950; no spills, no scratch):
//                                VGPRs  AGPRs  LDS bytes  waves / SIMD
//   llama_train_rope   bf16       62     0      0          8
//   llama_train_rope   fp16       78     0      0          6
//   llama_train_fwd    bf16       182    0      34816      2
//   llama_train_fwd    fp16       182    0      34816      2
//   llama_train_dq     bf16       174    84     52224      1
//   llama_train_dq     fp16       174    84     52224      1
//   llama_train_dkdv   bf16       244    136    70144      1
//   llama_train_dkdv   fp16       244    136    70144      1
// The forward asks for 2 waves per SIMD as the prefill kernel does, the two backward kernels for 1 (amdgpu_waves_per_eu): left
// alone the compiler aimed dkdv at 2 and put 784 bytes a lane into scratch.  dkdv forms its epilogue's per-lane pointers before
// the walk and holds them in vector registers: with the kernel's ten pointers live through the walk, 6 scalar registers were
// spilled (to lanes of a vector register).
// What bounds each kernel: profiles/llama_attn.md, "Training".
//
// Error bounds (tests/llama_train_refs.py, train64, evaluates them element by element against fp64 on the STORED q, k, v,
// dO; the framework's statement in T is held to the same bounds, so each counts the roundings of whichever rounds more).
// u = T's unit roundoff (2^-8 bf16, 2^-11 fp16), t = T's smallest normal, e = 2^-24, n = j + 1 live keys of row j,
// c_e = 256 + L; c_n = 160 is E_s's count of the fp32 steps of a score (mmfs_llama_attn.hip; C_NORM of
// tests/llama_attn_refs.py, which train64 takes from there); sc = 1 / sqrt(128).
//   q_rot, k_rot   E_rope of mmfs_llama_attn.hip (two fp32 products, a sum, one rounding): they are known to E_q, E_k.
//   s, p, context  mmfs_llama_attn.hip's E_s with its [E_q . |k| + |q| . E_k] sc term, E_p and the context bound; a masked
//                  score is exactly -Inf, p = 0, E_s = 0 there.  Here s is 4 matrix-core steps of 32 fp32 accumulations and
//                  the scaling; the sums over n keys run in tiles of 64, one rescaling a tile, the diagonal block by fp32
//                  multiply-adds: inside c_e.
//   lse            |lse - ref| <= sum_t p E_s + c_e e (1 + |lse|)
//   delta          rowsum(dO O) from the rounded context, fp32 (the framework: sum_t p dP from its rounded dP):
//                      E_delta = sum_c |dO_c| W_c,   W = (E_p + (2 u + c_e e) p) |v| + t
//   p (backward)   exp(s - lse) recomputed from the same rounded operands: E_p again (the lse's error is inside it: it is the
//                  row term sum p E_s and c_e e).
//   ds             p (dP - delta); dP = dO . v is 128 fp32 accumulations on top of -delta; the kernels round ds once, the
//                  framework dP, ds and ds sc:   E_ds = E_p |dP - delta| + p (u |dP| + E_delta) + 3 u |ds|
//   dv             P^T dO:   |dv - ref| <= E_p^T |dO| + c_e e p^T |dO| + 2 u |ref| + t
//   dq_rot         g = sc ds k_rot, k_rot known to E_k (dk_rot = sc ds^T q_rot alike, with E_q):
//                      G = sc (E_ds |k| + |ds| E_k + (u + c_e e) |ds| |k|) + u |g|
//                  (u |ds| |k|: the framework rounds q sc before its product; u |g|: it rounds g, the kernels keep fp32)
//   dq, dk         x = g cos + g' sin (g' the partner channel, its sign with the half): two fp32 products, one sum, one
//                  rounding here; the framework rounds cos, sin, both products and the sum.  A = |g cos| + |g' sin|:
//                      |dq - ref| <= G |cos| + G' |sin| + (2 u + 3 u^2 + 4 e) A + u |ref| + t
//   These bounds add absolute values where the errors of 128 channels and up to L keys largely cancel; on dq and dk they are
//   wider than the gradient at unit-normal rows.  The tests therefore hold the context and the gradients to a second, tight
//   measure as well: a row's error in the 2-norm within 8 u of the row's norm (plus the share of delta's rounding, which does
//   not shrink with the row's gradient); tests/llama_train_refs.py, row_error, derives the factor from the rounding points above.
//   Measured worst ratios of both are kept in profiles/llama_attn.md.
//
// Offsets are 64-bit.
#include "mmfs_attn_core.h"
#include <hip/hip_runtime.h>

namespace mmfs {

namespace {

using namespace attn;

constexpr int kD = kLlamaD;
constexpr int kHalf = 64;               // a channel's rotary partner is kHalf further on
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kWaveRows = 32;           // fwd, dq: query rows of a wave: two blocks of 16
constexpr int kRows = kWaves * kWaveRows;           // of a workgroup
constexpr int kKT = 64;                 // fwd, dq: keys of a tile
constexpr int kWaveKeys = 32;           // dkdv: keys of a wave: two blocks of 16
constexpr int kKeys = kWaves * kWaveKeys;           // of a workgroup
constexpr int kQT = 64;                 // dkdv: queries of a tile
constexpr int kLdR = kD + 8;            // elements between rows of a row-major image [row][128 + 8]
constexpr int kLdT = 64 + 4;            // of a transposed image [channel][64 + 4]
constexpr float kScale = HeadScale<kD>::value;
constexpr float kInvScale = 11.313708498984761f;    // sqrt(128)

template <typename T> __device__ __forceinline__ float bits_f32(uint32_t h) { return to_f32(__builtin_bit_cast(T, (uint16_t)h)); }

// rows r0 .. r0 + 63 of one head's token-major slice (``src`` at the head's channel 0 of row 0, rows ``ld`` elements apart)
// -> LDS, row-major (``rows``) and / or transposed (``trans``), either may be null; a row at or behind L is zeros.  A lane
// loads 8 channels of 4 neighbouring rows (the transposed image takes them as 8 x 8 bytes).
template <typename T>
__device__ __forceinline__ void stage_tile(const T *__restrict__ src, const int64_t ld, const int r0, const int L,
                                           uint16_t *rows, uint16_t *trans, const int tid)
{
    const int cg = tid & 15, kq = tid >> 4;
    uint4 vr[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int row = 4 * kq + e;
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (r0 + row < L) w = *reinterpret_cast<const uint4 *>(src + (int64_t)(r0 + row) * ld + 8 * cg);
        if (rows) *reinterpret_cast<uint4 *>(rows + row * kLdR + 8 * cg) = w;
        vr[e] = w;
    }
    if (trans) {
        const uint32_t w[4][4] = {{vr[0].x, vr[0].y, vr[0].z, vr[0].w}, {vr[1].x, vr[1].y, vr[1].z, vr[1].w},
                                  {vr[2].x, vr[2].y, vr[2].z, vr[2].w}, {vr[3].x, vr[3].y, vr[3].z, vr[3].w}};
#pragma unroll
        for (int pr = 0; pr < 4; ++pr) {                                    // channels 2 pr (low halves), 2 pr + 1 (high halves)
            uint2 lo, hi;
            lo.x = (w[0][pr] & 0xffffu) | (w[1][pr] << 16);
            lo.y = (w[2][pr] & 0xffffu) | (w[3][pr] << 16);
            hi.x = (w[0][pr] >> 16) | (w[1][pr] & 0xffff0000u);
            hi.y = (w[2][pr] >> 16) | (w[3][pr] & 0xffff0000u);
            *reinterpret_cast<uint2 *>(trans + (8 * cg + 2 * pr) * kLdT + 4 * kq) = lo;
            *reinterpret_cast<uint2 *>(trans + (8 * cg + 2 * pr + 1) * kLdT + 4 * kq) = hi;
        }
    }
}

// the 32 channels 32 st + 8 g .. + 7 (st < 4) of one token's head as the fragments of a matrix product; zeros when not ``live``
template <typename T> __device__ __forceinline__ void load_frags(const T *p, const bool live, const int g, s16x8 (&f)[4])
{
#pragma unroll
    for (int st = 0; st < 4; ++st)
        f[st] = live ? *reinterpret_cast<const s16x8 *>(p + 32 * st + 8 * g) : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
}

// elements 0..3 at p (kept iff keep0), 4..7 at p + 16 (kept iff keep1), zeros otherwise: lds4x2 with the halves that a
// diagonal or dead 16-row block must not bring into the product
__device__ __forceinline__ s16x8 lds4x2_keep(const uint16_t *p, const bool keep0, const bool keep1)
{
    const s16x4 z = {0, 0, 0, 0};
    const s16x4 a = keep0 ? *reinterpret_cast<const s16x4 *>(p) : z, b = keep1 ? *reinterpret_cast<const s16x4 *>(p + 16) : z;
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

// The diagonal block's share of a second product.  acc[db][r] is (channel 16 db + 4 g + r, column c); ``w`` are this lane's
// four weights of column c, rows 4 g + r of the block (what pack_pair would hand the matrix product); xt points at the
// block's first row in a transposed image [channel][kLdT].  Adds sum over the block's rows i of w(i, c) x(i, channel) for the
// live pairs alone -- LOWER: i <= c (row = key, column = query), else i >= c (row = query, column = key) -- ascending in i;
// a masked pair's product is dropped by a select behind the multiplication, so nothing of it arrives.
template <typename T, bool LOWER>
__device__ __forceinline__ void diag_fma(f32x4 (&acc)[8], const float (&w)[4], const uint16_t *xt, const int c, const int g)
{
    float wt[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) wt[i] = __shfl(to_f32((T)w[i & 3]), c + 16 * (i >> 2), 64);
#pragma unroll
    for (int db = 0; db < 8; ++db)
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

__device__ __forceinline__ void load4f(const float *p, float (&o)[4])
{
    const float4 a = *reinterpret_cast<const float4 *>(p);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
}

// Epilogue of the two backward kernels: acc[db][r] is the gradient of the ROTATED channel 16 db + 4 g + r of one token's
// head before the factor 1 / sqrt(128); -> the gradient of the unrotated row, rounded once, 8 stores of 4 channels.
// cs, sn: the token's row of the tables at this lane's channel 4 g, or null for a position outside [0, max_pos): NaN, as the
// forward made that token's rotated row.  out: the token's row of the head at channel 4 g.
template <typename T>
__device__ __forceinline__ void unrotate_store(const f32x4 (&acc)[8], const float *cs_row, const float *sn_row, T *out)
{
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

template <typename T>
__global__ void __launch_bounds__(kThreads)
llama_train_rope(const T *__restrict__ q, const T *__restrict__ k, const int64_t *__restrict__ pos,
                 const float *__restrict__ cos_t, const float *__restrict__ sin_t, const int64_t max_pos,
                 T *__restrict__ q_rot, T *__restrict__ k_rot, const int64_t total, const int H)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;         // ((b L + j) H + h) 8 + part
    if (i >= total) return;
    const int part = (int)(i & 7);
    const int64_t r = i >> 3, tok = r / H;
    const int64_t p = pos[tok];
    const bool ok = p >= 0 && p < max_pos;
    const int64_t in = r * kD + part * 8;
    float c[8], s[8], ql[8], qh[8], kl[8], kh[8];
    if (ok) {
        load4f(cos_t + p * kHalf + part * 8, reinterpret_cast<float (&)[4]>(c[0]));
        load4f(cos_t + p * kHalf + part * 8 + 4, reinterpret_cast<float (&)[4]>(c[4]));
        load4f(sin_t + p * kHalf + part * 8, reinterpret_cast<float (&)[4]>(s[0]));
        load4f(sin_t + p * kHalf + part * 8 + 4, reinterpret_cast<float (&)[4]>(s[4]));
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) c[e] = s[e] = __builtin_nanf("");
    }
    load_vec<T, 8>(q + in, ql);
    load_vec<T, 8>(q + in + kHalf, qh);
    load_vec<T, 8>(k + in, kl);
    load_vec<T, 8>(k + in + kHalf, kh);
    float ol[8], oh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { ol[e] = ql[e] * c[e] - qh[e] * s[e]; oh[e] = qh[e] * c[e] + ql[e] * s[e]; }
    store_vec<T, 8, false>(q_rot + in, ol);
    store_vec<T, 8, false>(q_rot + in + kHalf, oh);
#pragma unroll
    for (int e = 0; e < 8; ++e) { ol[e] = kl[e] * c[e] - kh[e] * s[e]; oh[e] = kh[e] * c[e] + kl[e] * s[e]; }
    store_vec<T, 8, false>(k_rot + in, ol);
    store_vec<T, 8, false>(k_rot + in + kHalf, oh);
}

template <typename T>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
llama_train_fwd(const T *__restrict__ q_rot, const T *__restrict__ k_rot, const T *__restrict__ v, T *__restrict__ ctx,
                float *__restrict__ lse, const int L, const int H, const int BH)
{
    __shared__ __attribute__((aligned(16))) uint16_t sK[kKT * kLdR];
    __shared__ __attribute__((aligned(16))) uint16_t sVt[kD * kLdT];
    // the heaviest query tiles (the last ones: the most keys) are dispatched first
    const int nqt = (L + kRows - 1) / kRows;
    const int rank = blockIdx.x / BH, bh = blockIdx.x - rank * BH, b = bh / H, h = bh - b * H;
    const int q0 = (nqt - 1 - rank) * kRows;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int64_t ld = (int64_t)H * kD, off = (int64_t)b * L * ld + (int64_t)h * kD;

    // this lane's query of block i: row q0 + 32 wave + 16 i + c (zeros at or behind L)
    s16x8 fq[2][4];
    float m[2], l[2];
    f32x4 acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int j = q0 + wave * kWaveRows + 16 * i + c;
        load_frags<T>(q_rot + off + (int64_t)min(j, L - 1) * ld, j < L, g, fq[i]);
        m[i] = -INFINITY;
        l[i] = 0.f;
#pragma unroll
        for (int db = 0; db < 8; ++db) acc[i][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    const int kend = min(q0 + kRows, L);                                    // keys behind the workgroup's last row are live for nobody
    for (int k0 = 0; k0 < kend; k0 += kKT) {
        stage_tile<T>(k_rot + off, ld, k0, L, sK, nullptr, tid);
        stage_tile<T>(v + off, ld, k0, L, nullptr, sVt, tid);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r0 = q0 + wave * kWaveRows + 16 * i;
            if (r0 >= L || k0 > r0) continue;                               // no row, or a tile beyond the block's diagonal (wave-uniform)
            const int jq = r0 + c;
            float s[4][4];
            float tm = -INFINITY;
#pragma unroll
            for (int kb16 = 0; kb16 < 4; ++kb16) {
                const int t0 = k0 + kb16 * 16;
                if (t0 > r0) {                                              // beyond the diagonal (wave-uniform)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[kb16][r] = -INFINITY;
                    continue;
                }
                f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int st = 0; st < 4; ++st)
                    a = mma::FwdMma<T>::run(lds8(sK + (kb16 * 16 + c) * kLdR + 32 * st + 8 * g), fq[i][st], a);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[kb16][r] = t0 + 4 * g + r <= jq ? a[r] * kScale : -INFINITY;
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
#pragma unroll
            for (int db = 0; db < 8; ++db) acc[i][db] *= alpha;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int t0 = k0 + 32 * ks;
                const bool keep0 = t0 < r0, keep1 = t0 + 16 < r0;          // 16-key blocks wholly before the diagonal block
                if (keep0) {
                    const s16x8 fp = pack_pair<T>(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
                    for (int db = 0; db < 8; ++db)
                        acc[i][db] = mma::FwdMma<T>::run(lds4x2_keep(sVt + (db * 16 + c) * kLdT + 32 * ks + 4 * g, keep0, keep1), fp,
                                                         acc[i][db]);
                }
            }
            if (r0 < k0 + kKT) {                                            // the tile holds the block's diagonal block (wave-uniform)
                float pd[4];
                pick_block(s, (r0 - k0) >> 4, pd);
                diag_fma<T, true>(acc[i], pd, sVt + (r0 - k0), c, g);
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
        for (int db = 0; db < 8; ++db) {
            const float out[4] = {acc[i][db][0] / l[i], acc[i][db][1] / l[i], acc[i][db][2] / l[i], acc[i][db][3] / l[i]};
            store4<T>(o + db * 16 + 4 * g, out);
        }
        if (g == 0) lse[(int64_t)bh * L + qi] = m[i] + logf(l[i]);
    }
}

// a lane's share of rowsum(a b): the 32 channels of its four fragments, in ascending order
template <typename T> __device__ __forceinline__ float frag_dot(const s16x8 (&a)[4], const s16x8 (&b)[4])
{
    float d = 0.f;
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
        for (int e = 0; e < 8; ++e) d += bits_f32<T>((uint16_t)a[st][e]) * bits_f32<T>((uint16_t)b[st][e]);
    return d;
}

template <typename T>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(1, 1)))
llama_train_dq(const T *__restrict__ q_rot, const T *__restrict__ k_rot, const T *__restrict__ v, const T *__restrict__ ctx,
               const T *__restrict__ dctx, const float *__restrict__ lse, const int64_t *__restrict__ pos,
               const float *__restrict__ cos_t, const float *__restrict__ sin_t, const int64_t max_pos, T *__restrict__ dq,
               float *__restrict__ delta, const int L, const int H, const int BH)
{
    __shared__ __attribute__((aligned(16))) uint16_t sK[kKT * kLdR];
    __shared__ __attribute__((aligned(16))) uint16_t sKt[kD * kLdT];
    __shared__ __attribute__((aligned(16))) uint16_t sV[kKT * kLdR];
    const int nqt = (L + kRows - 1) / kRows;
    const int rank = blockIdx.x / BH, bh = blockIdx.x - rank * BH, b = bh / H, h = bh - b * H;
    const int q0 = (nqt - 1 - rank) * kRows;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int64_t ld = (int64_t)H * kD, off = (int64_t)b * L * ld + (int64_t)h * kD;

    s16x8 fq[2][4], fdo[2][4];
    float nl[2], nd[2];                     // -lse sqrt(128) and -delta of this lane's query
    f32x4 acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int j = q0 + wave * kWaveRows + 16 * i + c;
        const bool live = j < L;
        const int64_t row = off + (int64_t)min(j, L - 1) * ld;
        load_frags<T>(q_rot + row, live, g, fq[i]);
        load_frags<T>(dctx + row, live, g, fdo[i]);
        s16x8 fo[4];
        load_frags<T>(ctx + row, live, g, fo);
        float d = frag_dot<T>(fdo[i], fo);
        d += __shfl_xor(d, 16, 64);
        d += __shfl_xor(d, 32, 64);
        if (live && g == 0) delta[(int64_t)bh * L + j] = d;
        nd[i] = -d;
        nl[i] = live ? -lse[(int64_t)bh * L + j] * kInvScale : 0.f;
#pragma unroll
        for (int db = 0; db < 8; ++db) acc[i][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    const int kend = min(q0 + kRows, L);
    for (int k0 = 0; k0 < kend; k0 += kKT) {
        stage_tile<T>(k_rot + off, ld, k0, L, sK, sKt, tid);
        stage_tile<T>(v + off, ld, k0, L, sV, nullptr, tid);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r0 = q0 + wave * kWaveRows + 16 * i;
            if (r0 >= L || k0 > r0) continue;                               // (wave-uniform)
            const int jq = r0 + c;
            float ds[4][4];
#pragma unroll
            for (int kb16 = 0; kb16 < 4; ++kb16) {
                const int t0 = k0 + kb16 * 16;
                if (t0 > r0) {                                              // beyond the diagonal (wave-uniform)
#pragma unroll
                    for (int r = 0; r < 4; ++r) ds[kb16][r] = 0.f;
                    continue;
                }
                f32x4 a = {nl[i], nl[i], nl[i], nl[i]}, dp = {nd[i], nd[i], nd[i], nd[i]};
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    a = mma::FwdMma<T>::run(lds8(sK + (kb16 * 16 + c) * kLdR + 32 * st + 8 * g), fq[i][st], a);
                    dp = mma::FwdMma<T>::run(lds8(sV + (kb16 * 16 + c) * kLdR + 32 * st + 8 * g), fdo[i][st], dp);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = exp_hw(a[r] * kScale);
                    const float x = p * dp[r];
                    ds[kb16][r] = t0 + 4 * g + r <= jq ? x : 0.f;
                }
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int t0 = k0 + 32 * ks;
                const bool keep0 = t0 < r0, keep1 = t0 + 16 < r0;
                if (keep0) {
                    const s16x8 fs = pack_pair<T>(ds[2 * ks], ds[2 * ks + 1]);
#pragma unroll
                    for (int db = 0; db < 8; ++db)
                        acc[i][db] = mma::FwdMma<T>::run(lds4x2_keep(sKt + (db * 16 + c) * kLdT + 32 * ks + 4 * g, keep0, keep1), fs,
                                                         acc[i][db]);
                }
            }
            if (r0 < k0 + kKT) {                                            // the tile holds the block's diagonal block (wave-uniform)
                float dd[4];
                pick_block(ds, (r0 - k0) >> 4, dd);
                diag_fma<T, true>(acc[i], dd, sKt + (r0 - k0), c, g);
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int qi = q0 + wave * kWaveRows + 16 * i + c;
        if (qi >= L) continue;
        const int64_t ps = pos[(int64_t)b * L + qi];
        const bool ok = ps >= 0 && ps < max_pos;
        unrotate_store<T>(acc[i], ok ? cos_t + ps * kHalf + 4 * g : nullptr, ok ? sin_t + ps * kHalf + 4 * g : nullptr,
                          dq + off + (int64_t)qi * ld + 4 * g);
    }
}

template <typename T>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(1, 1)))
llama_train_dkdv(const T *__restrict__ q_rot, const T *__restrict__ k_rot, const T *__restrict__ v, const T *__restrict__ dctx,
                 const float *__restrict__ lse, const float *__restrict__ delta, const int64_t *__restrict__ pos,
                 const float *__restrict__ cos_t, const float *__restrict__ sin_t, const int64_t max_pos, T *__restrict__ dk,
                 T *__restrict__ dv, const int L, const int H, const int BH)
{
    __shared__ __attribute__((aligned(16))) uint16_t sQ[kQT * kLdR];
    __shared__ __attribute__((aligned(16))) uint16_t sQt[kD * kLdT];
    __shared__ __attribute__((aligned(16))) uint16_t sO[kQT * kLdR];         // dO
    __shared__ __attribute__((aligned(16))) uint16_t sOt[kD * kLdT];
    __shared__ __attribute__((aligned(16))) float sNl[kQT], sNd[kQT];        // -lse sqrt(128), -delta
    // the heaviest key blocks (the first ones: the most queries) are dispatched first
    const int kt = blockIdx.x / BH, bh = blockIdx.x - kt * BH, b = bh / H, h = bh - b * H;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int64_t ld = (int64_t)H * kD, off = (int64_t)b * L * ld + (int64_t)h * kD;
    const int kw0 = kt * kKeys + wave * kWaveKeys;                          // the wave's first key

    s16x8 fk[2][4], fv[2][4];
    f32x4 dkt[2][8], dvt[2][8];
    // what the epilogue needs of this lane's keys, formed here and held in vector registers: its scalar inputs (five
    // pointers, the table's length) then do not live through the walk, where the scalar registers are short
    const float *cs_row[2], *sn_row[2];
    T *dk_row[2], *dv_row[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int t = kw0 + 16 * i + c;
        const int64_t row = off + (int64_t)min(t, L - 1) * ld;
        const int64_t ps = pos[(int64_t)b * L + min(t, L - 1)];
        const bool ok = ps >= 0 && ps < max_pos;
        cs_row[i] = ok ? cos_t + ps * kHalf + 4 * g : nullptr;
        sn_row[i] = ok ? sin_t + ps * kHalf + 4 * g : nullptr;
        dk_row[i] = dk + row + 4 * g;
        dv_row[i] = dv + row + 4 * g;
        asm volatile("" : "+v"(cs_row[i]), "+v"(sn_row[i]), "+v"(dk_row[i]), "+v"(dv_row[i]));
        load_frags<T>(k_rot + row, t < L, g, fk[i]);
        load_frags<T>(v + row, t < L, g, fv[i]);
#pragma unroll
        for (int db = 0; db < 8; ++db) dkt[i][db] = dvt[i][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int q0 = kt * kKeys; q0 < L; q0 += kQT) {
        stage_tile<T>(q_rot + off, ld, q0, L, sQ, sQt, tid);
        stage_tile<T>(dctx + off, ld, q0, L, sO, sOt, tid);
        if (tid < kQT) {
            const bool live = q0 + tid < L;
            sNl[tid] = live ? -lse[(int64_t)bh * L + q0 + tid] * kInvScale : 0.f;
            sNd[tid] = live ? -delta[(int64_t)bh * L + q0 + tid] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int t0 = kw0 + 16 * i;                                    // the key block
            if (t0 >= L || q0 + kQT <= t0) continue;                        // no key, or a tile before the block's diagonal (wave-uniform)
            const int tk = t0 + c;
            float p[4][4], ds[4][4];
#pragma unroll
            for (int qs = 0; qs < 4; ++qs) {
                const int j0 = q0 + 16 * qs;
                if (j0 < t0) {                                              // before the diagonal (wave-uniform)
#pragma unroll
                    for (int r = 0; r < 4; ++r) p[qs][r] = ds[qs][r] = 0.f;
                    continue;
                }
                const float4 l4 = *reinterpret_cast<const float4 *>(sNl + 16 * qs + 4 * g);
                const float4 d4 = *reinterpret_cast<const float4 *>(sNd + 16 * qs + 4 * g);
                f32x4 a = {l4.x, l4.y, l4.z, l4.w}, dp = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    a = mma::FwdMma<T>::run(lds8(sQ + (16 * qs + c) * kLdR + 32 * st + 8 * g), fk[i][st], a);
                    dp = mma::FwdMma<T>::run(lds8(sO + (16 * qs + c) * kLdR + 32 * st + 8 * g), fv[i][st], dp);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = j0 + 4 * g + r;
                    const bool live = tk <= j && j < L;
                    const float pr = exp_hw(a[r] * kScale);
                    const float x = pr * dp[r];
                    p[qs][r] = live ? pr : 0.f;
                    ds[qs][r] = live ? x : 0.f;
                }
            }
#pragma unroll
            for (int qp = 0; qp < 2; ++qp) {
                const int j0 = q0 + 32 * qp;
                const bool keep0 = j0 > t0, keep1 = j0 + 16 > t0;           // 16-query blocks wholly behind the diagonal block
                if (keep1) {
                    const s16x8 fp = pack_pair<T>(p[2 * qp], p[2 * qp + 1]), fds = pack_pair<T>(ds[2 * qp], ds[2 * qp + 1]);
#pragma unroll
                    for (int db = 0; db < 8; ++db) {
                        dvt[i][db] = mma::FwdMma<T>::run(lds4x2_keep(sOt + (db * 16 + c) * kLdT + 32 * qp + 4 * g, keep0, keep1), fp,
                                                         dvt[i][db]);
                        dkt[i][db] = mma::FwdMma<T>::run(lds4x2_keep(sQt + (db * 16 + c) * kLdT + 32 * qp + 4 * g, keep0, keep1), fds,
                                                         dkt[i][db]);
                    }
                }
            }
            if (t0 >= q0) {                                                 // the tile holds the block's diagonal block (wave-uniform)
                float pd[4], dd[4];
                pick_block(p, (t0 - q0) >> 4, pd);
                pick_block(ds, (t0 - q0) >> 4, dd);
                diag_fma<T, false>(dvt[i], pd, sOt + (t0 - q0), c, g);
                diag_fma<T, false>(dkt[i], dd, sQt + (t0 - q0), c, g);
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int t = kw0 + 16 * i + c;
        if (t >= L) continue;
#pragma unroll
        for (int db = 0; db < 8; ++db) {
            const float out[4] = {dvt[i][db][0], dvt[i][db][1], dvt[i][db][2], dvt[i][db][3]};
            store4<T>(dv_row[i] + db * 16, out);
        }
        unrotate_store<T>(dkt[i], cs_row[i], sn_row[i], dk_row[i]);
    }
}

// every entry's checks of (dtype, B, H, D, L) and of the rotary table's length (the forward has none: 0); ``empty``: OK
// without a launch
int train_check(int dtype, int64_t B, int64_t H, int64_t D, int64_t L, int64_t max_pos, bool &empty)
{
    empty = false;
    const int rc = llama_train_check(dtype, B, H, D, L);
    if (rc) return rc;
    if (max_pos < 0 || max_pos > (1LL << 40)) return MMFS_E_DIMS;
    const int64_t tiles = (L + kRows - 1) / kRows;
    if (tiles * B * H > ((int64_t)1 << 31) - 1 || B * L > (1LL << 32) || B * L * H > (1LL << 34)) return MMFS_E_DIMS;
    empty = B * H * L == 0;
    return MMFS_OK;
}

}  // namespace
}  // namespace mmfs

extern "C" {

int mmfs_llama_attn_train_supported(int dtype, int64_t D, int64_t L) { return mmfs::attn::llama_train_supported(dtype, D, L); }

int64_t mmfs_llama_attn_train_tiles(int level)
{
    using namespace mmfs;
    return level == 0 ? kRows : level == 1 ? kKT : level == 2 ? kKeys : level == 3 ? kQT : level == 4 ? kWaveRows : MMFS_E_DIMS;
}

int64_t mmfs_llama_attn_train_workspace_bytes(int64_t B, int64_t H, int64_t L)
{
    using namespace mmfs;
    if (attn::batch_heads_check(MMFS_F16, B, H, L, 0, 0) || L > kLlamaTrainMaxL) return MMFS_E_DIMS;       // (no dtype to ask about)
    return B * H * L * (int64_t)sizeof(float);                             // delta
}

int mmfs_llama_attn_train_rope(int dtype, const void *q, const void *k, const int64_t *position_ids, const float *cos_table,
                               const float *sin_table, int64_t max_pos, void *q_rot, void *k_rot, int64_t B, int64_t L,
                               int64_t H, int64_t D, void *stream)
{
    using namespace mmfs;
    bool empty;
    const int rc = train_check(dtype, B, H, D, L, max_pos, empty);
    if (rc || empty) return rc;
    const bool rope = max_pos != 0;
    if (const int rt = check_tensors({{q, 16}, {k, 16}, {position_ids, 8}, {q_rot, 16}, {k_rot, 16}, {cos_table, 16, rope},
                                      {sin_table, 16, rope}}))
        return rt;
    const int64_t total = B * L * H * 8;
    return by_half_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(llama_train_rope<T>, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                           (hipStream_t)stream, (const T *)q, (const T *)k, position_ids, cos_table, sin_table, max_pos,
                           (T *)q_rot, (T *)k_rot, total, (int)H);
        return (int)hipGetLastError();
    });
}

int mmfs_llama_attn_train_forward(int dtype, const void *q_rot, const void *k_rot, const void *v, void *context, float *lse,
                                  int64_t B, int64_t L, int64_t H, int64_t D, void *stream)
{
    using namespace mmfs;
    bool empty;
    const int rc = train_check(dtype, B, H, D, L, 0, empty);
    if (rc || empty) return rc;
    if (const int rt = check_tensors({{q_rot, 16}, {k_rot, 16}, {v, 16}, {context, 16}, {lse, 4}})) return rt;
    const int64_t tiles = (L + kRows - 1) / kRows;
    return by_half_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(llama_train_fwd<T>, dim3((unsigned)(tiles * B * H)), dim3(kThreads), 0, (hipStream_t)stream,
                           (const T *)q_rot, (const T *)k_rot, (const T *)v, (T *)context, lse, (int)L, (int)H, (int)(B * H));
        return (int)hipGetLastError();
    });
}

int mmfs_llama_attn_train_backward(int dtype, const void *q_rot, const void *k_rot, const void *v, const void *context,
                                   const void *grad_context, const float *lse, const int64_t *position_ids,
                                   const float *cos_table, const float *sin_table, int64_t max_pos, void *grad_q, void *grad_k,
                                   void *grad_v, float *workspace, int64_t B, int64_t L, int64_t H, int64_t D, void *stream)
{
    using namespace mmfs;
    bool empty;
    const int rc = train_check(dtype, B, H, D, L, max_pos, empty);
    if (rc || empty) return rc;
    const bool rope = max_pos != 0;
    if (const int rt = check_tensors({{q_rot, 16}, {k_rot, 16}, {v, 16}, {context, 16}, {grad_context, 16}, {lse, 4},
                                      {position_ids, 8}, {grad_q, 16}, {grad_k, 16}, {grad_v, 16}, {workspace, 16},
                                      {cos_table, 16, rope}, {sin_table, 16, rope}}))
        return rt;
    const int64_t qtiles = (L + kRows - 1) / kRows, ktiles = (L + kKeys - 1) / kKeys;
    return by_half_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(llama_train_dq<T>, dim3((unsigned)(qtiles * B * H)), dim3(kThreads), 0, (hipStream_t)stream,
                           (const T *)q_rot, (const T *)k_rot, (const T *)v, (const T *)context, (const T *)grad_context, lse,
                           position_ids, cos_table, sin_table, max_pos, (T *)grad_q, workspace, (int)L, (int)H, (int)(B * H));
        const int e = (int)hipGetLastError();
        if (e) return e;
        hipLaunchKernelGGL(llama_train_dkdv<T>, dim3((unsigned)(ktiles * B * H)), dim3(kThreads), 0, (hipStream_t)stream,
                           (const T *)q_rot, (const T *)k_rot, (const T *)v, (const T *)grad_context, lse,
                           (const float *)workspace, position_ids, cos_table, sin_table, max_pos, (T *)grad_k, (T *)grad_v,
                           (int)L, (int)H, (int)(B * H));
        return (int)hipGetLastError();
    });
}

}  // extern "C"
