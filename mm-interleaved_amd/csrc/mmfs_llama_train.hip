// mmfs_llama_train.hip -- the LLM's self-attention in TRAINING: what the reference's _forward_train
// (mm_interleaved/models/utils/monkey_patch/llama_flash_attn_train_monkey_patch.py:35-82) asks of flash_attn_func(q, k, v,
// 0.0, softmax_scale=None, causal=True) between the three Linear layers and o_proj, forward and backward, without a tensor
// of size L x L.  No cache, no src_row, no bias: q, k, v, dO and every output are token-major [B, L, H 128] of T (bf16 /
// fp16) as the Linear layers produce and consume them; arithmetic is fp32; D = 128.
//     q_rot, k_rot = rope(q), rope(k)                                        (llama_train_rope)
//     s(j, t)      = q_rot[b, j, h] . k_rot[b, t, h] / sqrt(128)             key t is live for query j iff t <= j
//     context      = softmax_t(s) v,   lse = ln sum_t exp s                  (attn_train_fwd)
//     dq, dk, dv   of the UNROTATED q, k and of v                            (attn_train_dq, attn_train_dkdv)
// A masked score is SELECTED (to -Inf forward, p = ds = 0 backward), never added to, and a product over a 16 x 16 block
// that the diagonal crosses is not a matrix product at all (below): a NaN in token t's k or v reaches no query j < t, a NaN
// in query j's dO reaches no dk, dv of a key t > j.  Rows at or behind L in a partial tile are staged as zeros and never stored.
//
//   llama_train_rope    llama_rope_append's rotation without the cache: 8 lanes a (token, head), fp32, one rounding;
//                       a position outside [0, max_pos) makes that token's q_rot and k_rot NaN.
//   The three walks     mmfs_attn_train.h's (its header describes them), instantiated with LlamaTrain below: D = 128, the causal
//                       mask, each tile staged where it is used, the inverse rotation in the backward epilogues, the heaviest
//                       tiles first.  The forward is llama_attn_prefill's organisation: key tiles up to the diagonal only,
//                       the heaviest (last) query tiles first.  dkdv sweeps the query tiles of 64 from its own to the end,
//                       the heaviest (first) key blocks first; dq and dkdv keep 64 and 128 accumulator registers a block.
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
//
// Resources (make asm, gfx950; no spills, no scratch):
//                                VGPRs  AGPRs  LDS bytes  waves / SIMD
//   llama_train_rope   bf16       62     0      0          8
//   llama_train_rope   fp16       78     0      0          6
//   attn_train_fwd     bf16       182    0      34816      2
//   attn_train_fwd     fp16       182    0      34816      2
//   attn_train_dq      bf16       174    84     52224      1
//   attn_train_dq      fp16       174    84     52224      1
//   attn_train_dkdv    bf16       244    136    70144      1
//   attn_train_dkdv    fp16       244    136    70144      1
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
#include "mmfs_attn_train.h"

namespace mmfs {

namespace {

using namespace attn;

constexpr int kD = kLlamaD;
constexpr int kLdR = kLdRows<kD>;

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

// what mmfs_attn_train.h's walks ask of a family
struct LlamaTrain {
    static constexpr int kD = mmfs::kD;
    static constexpr bool kCausal = true, kAhead = false, kHeavyFirst = true, kLseOptional = false;
    static constexpr int kWaves[3] = {2, 1, 1};

    struct TileRegs {};                     // each tile is staged where it is used: nothing is held
    template <typename T>
    static __device__ __forceinline__ void put(const T *base, const int64_t off, const int64_t ld, const int r0, const int L,
                                               const TileRegs &, uint16_t *rows, uint16_t *trans, const int tid)
    {
        stage_tile<T>(base + off, ld, r0, L, rows, trans, tid);
    }
};

// every entry's checks of (dtype, B, H, D, L) and of the rotary table's length (the forward has none: 0); ``empty``: OK
// without a launch
int train_check(int dtype, int64_t B, int64_t H, int64_t D, int64_t L, int64_t max_pos, bool &empty)
{
    return train_entry_check(llama_train_check(dtype, B, H, D, L), B, H, L, max_pos, empty);
}

}  // namespace
}  // namespace mmfs

// the backward kernels' rotary parameters (attn::RopeArgs's members) as the kernels' template arguments; __restrict__ as on
// the kernels' other pointers (without it dq compiled differently)
#define LLAMA_ROPE_ARGS const int64_t *__restrict__, const float *__restrict__, const float *__restrict__, int64_t

extern "C" {

int mmfs_llama_attn_train_supported(int dtype, int64_t D, int64_t L) { return mmfs::attn::llama_train_supported(dtype, D, L); }

int64_t mmfs_llama_attn_train_tiles(int level) { return mmfs::attn::train_tiles(level); }

int64_t mmfs_llama_attn_train_workspace_bytes(int64_t B, int64_t H, int64_t L)
{
    return mmfs::attn::train_workspace_bytes(B, H, L, mmfs::attn::kLlamaTrainMaxL);
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
        hipLaunchKernelGGL((attn_train_fwd<T, LlamaTrain>), dim3((unsigned)(tiles * B * H)), dim3(kThreads), 0, (hipStream_t)stream,
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
        hipLaunchKernelGGL((attn_train_dq<T, LlamaTrain, LLAMA_ROPE_ARGS>), dim3((unsigned)(qtiles * B * H)), dim3(kThreads), 0, (hipStream_t)stream,
                           (const T *)q_rot, (const T *)k_rot, (const T *)v, (const T *)context, (const T *)grad_context, lse,
                           position_ids, cos_table, sin_table, max_pos, (T *)grad_q, workspace, (int)L, (int)H, (int)(B * H));
        const int e = (int)hipGetLastError();
        if (e) return e;
        hipLaunchKernelGGL((attn_train_dkdv<T, LlamaTrain, LLAMA_ROPE_ARGS>), dim3((unsigned)(ktiles * B * H)), dim3(kThreads), 0, (hipStream_t)stream,
                           (const T *)q_rot, (const T *)k_rot, (const T *)v, (const T *)grad_context, lse,
                           (const float *)workspace, position_ids, cos_table, sin_table, max_pos, (T *)grad_k, (T *)grad_v,
                           (int)L, (int)H, (int)(B * H));
        return (int)hipGetLastError();
    });
}

}  // extern "C"
