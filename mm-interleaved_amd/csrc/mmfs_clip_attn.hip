// mmfs_clip_attn.hip -- the CLIP ViT's self-attention: what the reference's CLIPXAttention
// (mm_interleaved/models/encoders/vit_adapter/xattn.py:21-141) asks of xformers.ops.memory_efficient_attention(q, k, v)
// between the three Linear layers and out_proj, forward and backward, without a tensor of size L x L.  Full (non-causal)
// attention, no mask, no bias, no dropout: q, k, v, dO and every output are token-major [B, L, H 64] of T (bf16 / fp16) as
// the Linear layers produce and consume them; arithmetic is fp32; D = 64.
//     s(j, t)    = q[b, j, h] . k[b, t, h] / 8
//     context    = softmax_t(s) v,   lse = ln sum_t exp s  (fp32, [B, H, L])            (attn_train_fwd)
//     dq, dk, dv                                                                        (attn_train_dq, attn_train_dkdv)
// The three kernels are mmfs_attn_train.h's tile walks (its header describes them), instantiated with ClipAttn below: D = 64,
// every (query, key) pair in front of L live -- so every second product is a plain matrix product and there is nothing like
// diag_fma here --, tiles held in registers one ahead, scaled stores (dq = dQ / 8; the row constants are -8 lse and -delta),
// index order, the compiler's choice of waves.  The forward's lse may be NULL (no backward follows).  dkdv sweeps ALL query
// tiles.  Key 0 is live for every row, so the running maximum is finite from the first tile on (the online-softmax step
// says where it relies on that).
//   Tile sizes       128 query rows / 64 keys (fwd, dq), 128 keys / 64 queries (dkdv): mmfs_llama_train.hip's, taken over so
//                    that the two families share their walks.  NOBODY HAS MEASURED ANOTHER CHOICE.  What was weighed: at
//                    L = 257 the third query tile holds one live row; its three idle waves and its second block skip every
//                    product, so the tile costs its share of staging (5 key tiles) and one block's products -- a third of
//                    the workgroups, a 17th of the work.  A 64-row tile would leave a fifth of the workgroups so and stage K
//                    and V five times a head instead of three.  The last key tile at L = 257 holds one live key: one 16-key
//                    block of four is computed.  At L = 257 a head's whole K and V (2 x 33 KB) would fit in LDS and the walk
//                    would need no barrier but the first; not done here: the staged tile is what the L = 1025 shape needs
//                    anyway, and one organisation serves both.  profiles/clip_attn.md holds what was measured.
//   Staging          A tile goes global memory -> registers (load) -> LDS (put), and the NEXT tile's loads are issued
//                    right behind the barrier that publishes the current one, so they are in flight while it is multiplied:
//                    16 registers a lane (dkdv: 18, with -8 lse and -delta).  Measured against staging each tile where it is
//                    used: forward 37.7 -> 36.1 / 105.9 -> 95.9 us, backward 117.6 -> 103.6 / 331.5 -> 276.4 us at
//                    (B, L) = (32, 257) / (8, 1025), H = 16, bf16; the same bits (profiles/clip_attn.md).
//
// Resources (make asm, gfx950; no spills, no scratch; the compiler's own choice of waves per SIMD):
//                                         VGPRs  AGPRs  LDS bytes  waves / SIMD
//   attn_train_fwd<ClipAttn>    bf16       134    32     17920      3
//   attn_train_fwd<ClipAttn>    fp16       134    32     17920      3
//   attn_train_dq<ClipAttn>     bf16       132    36     27136      3
//   attn_train_dq<ClipAttn>     fp16       133    32     27136      3
//   attn_train_dkdv<ClipAttn>   bf16       188    64     36352      2
//   attn_train_dkdv<ClipAttn>   fp16       190    64     36352      2
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
#include "mmfs_attn_train.h"
#include "../../include/mmfs_clip_attn.h"

namespace mmfs {

namespace {

using namespace attn;

constexpr int kLdR = kLdRows<kClipD>;

// what mmfs_attn_train.h's walks ask of a family
struct ClipAttn {
    static constexpr int kD = kClipD;
    static constexpr bool kCausal = false, kAhead = true, kHeavyFirst = false, kLseOptional = true;
    static constexpr int kWaves[3] = {0, 0, 0};

    // A tile is staged in two halves, so that the next tile's loads are in flight while the current one is multiplied.
    typedef uint4 TileRegs[2];              // the next tile, on its way

    // rows r0 .. r0 + 63 of one head's token-major slice (``base + off`` at the head's channel 0 of row 0, rows ``ld``
    // elements apart) -> registers: a lane holds 8 channels of 2 neighbouring rows; a row at or behind L is zeros
    template <typename T>
    static __device__ __forceinline__ void load(const T *__restrict__ base, const int64_t off, const int64_t ld, const int r0,
                                                const int L, uint4 (&vr)[2], const int tid)
    {
        const T *src = base + off;
        const int cg = tid & 7, kq = tid >> 3;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int row = r0 + 2 * kq + e;
            vr[e] = make_uint4(0u, 0u, 0u, 0u);
            if (row < L) vr[e] = *reinterpret_cast<const uint4 *>(src + (int64_t)row * ld + 8 * cg);
        }
    }

    // those registers -> LDS, row-major (``rows``) and / or transposed (``trans``), either may be null (the transposed
    // image takes a lane's share as 8 x 4 bytes)
    template <typename T>
    static __device__ __forceinline__ void put(const T *, const int64_t, const int64_t, const int, const int, const uint4 (&vr)[2],
                                               uint16_t *rows, uint16_t *trans, const int tid)
    {
        const int cg = tid & 7, kq = tid >> 3;
        if (rows) {
#pragma unroll
            for (int e = 0; e < 2; ++e) *reinterpret_cast<uint4 *>(rows + (2 * kq + e) * kLdR + 8 * cg) = vr[e];
        }
        if (trans) {
            const uint32_t w[2][4] = {{vr[0].x, vr[0].y, vr[0].z, vr[0].w}, {vr[1].x, vr[1].y, vr[1].z, vr[1].w}};
#pragma unroll
            for (int pr = 0; pr < 4; ++pr) {                                // channels 2 pr (low halves), 2 pr + 1 (high halves)
                const uint32_t lo = (w[0][pr] & 0xffffu) | (w[1][pr] << 16);
                const uint32_t hi = (w[0][pr] >> 16) | (w[1][pr] & 0xffff0000u);
                *reinterpret_cast<uint32_t *>(trans + (8 * cg + 2 * pr) * kLdT + 2 * kq) = lo;
                *reinterpret_cast<uint32_t *>(trans + (8 * cg + 2 * pr + 1) * kLdT + 2 * kq) = hi;
            }
        }
    }
};

// every entry's checks of (dtype, B, H, D, L); ``empty``: OK without a launch
int entry_check(int dtype, int64_t B, int64_t H, int64_t D, int64_t L, bool &empty)
{
    return train_entry_check(clip_check(dtype, B, H, D, L), B, H, L, 0, empty);
}

}  // namespace
}  // namespace mmfs

extern "C" {

int mmfs_clip_attn_supported(int dtype, int64_t D, int64_t L) { return mmfs::attn::clip_supported(dtype, D, L); }

int64_t mmfs_clip_attn_tiles(int level) { return mmfs::attn::train_tiles(level); }

int64_t mmfs_clip_attn_workspace_bytes(int64_t B, int64_t H, int64_t L)
{
    return mmfs::attn::train_workspace_bytes(B, H, L, mmfs::attn::kClipMaxL);
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
        hipLaunchKernelGGL((attn_train_fwd<T, ClipAttn>), dim3((unsigned)(tiles * B * H)), dim3(kThreads), 0, (hipStream_t)stream,
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
        hipLaunchKernelGGL((attn_train_dq<T, ClipAttn>), dim3((unsigned)(tiles * B * H)), dim3(kThreads), 0, (hipStream_t)stream,
                           (const T *)q, (const T *)k, (const T *)v, (const T *)out, (const T *)dout, lse, (T *)dq, workspace,
                           (int)L, (int)H, (int)(B * H));
        const int e = (int)hipGetLastError();
        if (e) return e;
        hipLaunchKernelGGL((attn_train_dkdv<T, ClipAttn>), dim3((unsigned)(tiles * B * H)), dim3(kThreads), 0, (hipStream_t)stream,
                           (const T *)q, (const T *)k, (const T *)v, (const T *)dout, lse, (const float *)workspace, (T *)dk,
                           (T *)dv, (int)L, (int)H, (int)(B * H));
        return (int)hipGetLastError();
    });
}

}  // extern "C"
