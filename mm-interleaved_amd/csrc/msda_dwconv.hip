// msda_dwconv.hip -- the depthwise 3x3 convolution of the ViT-Adapter's ConvFFN in the token layout, with bias and an
// optional exact (erf) GELU, forward and backward.
//
// The reference (mm_interleaved/models/encoders/vit_adapter/adapter_modules.py:64-89) cuts the pyramid's tokens
// [B, N, C] into three maps, transposes each to [B, C, h, w], convolves, transposes back, concatenates and applies
// GELU as one more pass.  The tokens already lie channels-last, the layout of every kernel here: a lane owns 16 bytes
// of channels and consecutive lanes read one contiguous token row.
//     x [B, N, C]: L maps one after the other, level l = h_l x w_l tokens, row-major, N = sum h_l w_l
//     w [C, 1, 3, 3] (nn.Conv2d's, read where it lies), bias [C] or none
//     y[b, p, c] = bias[c] + sum_{ky,kx} w[c, ky, kx] x[b, p + (ky-1, kx-1), c]          (fp32, ONE rounding to T)
//     a = gelu(y_T), y_T = y as rounded to the storage type (act = none: the output is y_T)
// A tap outside its own map is skipped by predicate, never multiplied by 0: a non-finite input reaches exactly the
// outputs whose window covers it, and no tap crosses from one map into the next.
//
// Forward (dwconv_fwd): a lane owns one column of one strip of kFwdRows rows of a map and one 16-byte channel vector.
// It walks down the column; every input row it reads (its own pixel and the two horizontal neighbours -- the lanes
// next to it read the same rows, so they come from the vector cache) is scattered into the three output rows it
// touches, held as three rotating fp32 accumulators.  The 9 weights of the lane's channels are loaded once per lane.
// y_T is stored only when the caller hands a pointer for it (a backward will need it); the activation is computed
// from the rounded y_T in the same instantiation either way, so calls with and without gradients agree bit for bit.
//
// Backward (dwconv_bwd): the same walk with g_y = g_a gelu'(y_T), gelu'(y) = Phi(y) + y phi(y) (act = none: g_y = g_a).
// One row of g_y (three columns) serves the three grad_x rows it touches AND the 27 weight-gradient terms of the x rows
// under it, so grad_x, grad_w and grad_b come from ONE pass.  9 weights + 9 weight-gradient sums + windows per channel
// are > 200 VGPRs at 8 channels per lane: the backward gives a lane 4 channels (8-byte accesses for 16-bit storage).
// grad_w / grad_b without float atomics, in two stages: the lanes of a workgroup that share channels add their sums in
// an LDS tree, the workgroup stores its fp32 partial row [10, C] (9 taps + bias; every element written, nothing to
// clear) into caller-provided scratch, and dwconv_wgrad_reduce adds the rows in a fixed order: deterministic.
//   Longest chain of sequential fp32 additions into one weight-gradient element, for the tests' bound:
//     n = kBwdRows (a lane's strip) + log2(items per workgroup) (LDS tree) + ceil(workgroups / 16) (a reducer lane's
//         rows) + 4 (the reducer's tree) + 2
//   with 4-channel lanes per token CL = C / 4, lanes per workgroup row CLB = min(2^ceil(log2 CL), 256),
//   items per workgroup 256 / CLB, items = B * sum_l ceil(h_l / kBwdRows) * w_l.
//
// Level extents reach the kernels by value (ConvLevels, at most 8 levels): no device table, no allocation, no
// synchronisation -- the launches can be captured into a graph.
#include "msda_host.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>

namespace mmfs {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxLevels = 8;
constexpr int kFwdRows = 8;             // rows of a forward strip
constexpr int kBwdRows = 16;            // rows of a backward strip
constexpr int kBwdVec = 4;              // channels per lane of the backward
constexpr int kSums = 10;               // 9 taps + bias per channel
constexpr int kRedRows = 16, kRedCols = 16;     // dwconv_wgrad_reduce: row lanes x element lanes of a workgroup

struct ConvLevels {
    int n;
    int h[kMaxLevels], w[kMaxLevels];
    int start[kMaxLevels];              // first token of the level
    int item0[kMaxLevels];              // first (strip, column) item of the level within a sample
    int items;                          // items per sample
};

struct Item { int h, w, x, r0, r1; int64_t tok0; };      // a column x of rows [r0, r1) of an h x w map starting at token tok0

// item j of a sample -> its level and place, by selects over the (at most 8) levels: the struct stays in scalar registers
template <int ROWS> __device__ __forceinline__ Item locate_item(const ConvLevels &lv, int j)
{
    int h = lv.h[0], w = lv.w[0], st = lv.start[0], i0 = 0;
#pragma unroll
    for (int l = 1; l < kMaxLevels; ++l) {
        const bool in = l < lv.n && j >= lv.item0[l];
        h = in ? lv.h[l] : h; w = in ? lv.w[l] : w; st = in ? lv.start[l] : st; i0 = in ? lv.item0[l] : i0;
    }
    Item it;
    const int k = j - i0;
    it.h = h; it.w = w; it.x = k % w; it.r0 = (k / w) * ROWS; it.r1 = min(h, it.r0 + ROWS); it.tok0 = st;
    return it;
}

__device__ __forceinline__ float gelu_f(float y) { return 0.5f * y * (1.f + erff(y * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_grad_f(float y)
{
    return 0.5f * (1.f + erff(y * 0.70710678118654752f)) + y * 0.39894228040143268f * expf(-0.5f * y * y);
}

// ---------------------------------------------------------------- forward: lane <-> (sample, strip, column, 16-byte channel vector)
template <typename T, bool GELU>
__global__ void __launch_bounds__(kThreads)
dwconv_fwd(const T *__restrict__ x, const T *__restrict__ wgt, const T *__restrict__ bias, T *__restrict__ out,
           T *__restrict__ pre, const ConvLevels lv, const int CV, const int64_t N, const int64_t total)
{
    typedef Vec16<T> V;
    constexpr int VEC = V::N;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int cv = (int)(i % CV);
    const int64_t bi = i / CV;
    const Item it = locate_item<kFwdRows>(lv, (int)(bi % lv.items));
    const int64_t C = (int64_t)CV * VEC;
    const int64_t base = ((bi / lv.items) * N + it.tok0) * C + (int64_t)cv * VEC;
    const T *xb = x + base;

    // the lane's 9 * VEC weights lie contiguously (144 bytes): wk[tap][channel]
    float wk[9][VEC], bv[VEC];
    {
        float flat[9 * VEC];
        const uint4 *wp = reinterpret_cast<const uint4 *>(wgt + (int64_t)cv * VEC * 9);
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            float part[VEC];
            V::unpack(wp[q], part);
#pragma unroll
            for (int e = 0; e < VEC; ++e) flat[q * VEC + e] = part[e];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k)
#pragma unroll
            for (int e = 0; e < VEC; ++e) wk[k][e] = flat[e * 9 + k];
    }
    if (bias) {
        load_vec<T, VEC>(bias + (int64_t)cv * VEC, bv);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) bv[e] = 0.f;
    }
    const bool has_l = it.x > 0, has_r = it.x + 1 < it.w;
    float a0[VEC], a1[VEC], a2[VEC];            // output rows r - 1, r, r + 1
#pragma unroll
    for (int e = 0; e < VEC; ++e) a0[e] = a1[e] = a2[e] = bv[e];
    // the next row's three vectors are requested before this row's arithmetic (a row outside the map: a clamped read
    // nobody uses), so a lane's walk is not one memory latency per row
    auto fetch = [&](int r, uint4 (&raw)[3]) {
        const T *row = xb + ((int64_t)min(max(r, 0), it.h - 1) * it.w + it.x) * C;
        raw[0] = *reinterpret_cast<const uint4 *>(has_l ? row - C : row);
        raw[1] = *reinterpret_cast<const uint4 *>(row);
        raw[2] = *reinterpret_cast<const uint4 *>(has_r ? row + C : row);
    };
    uint4 nxt[3];
    fetch(it.r0 - 1, nxt);
    for (int r = it.r0 - 1; r <= it.r1; ++r) {
        const uint4 cur[3] = {nxt[0], nxt[1], nxt[2]};
        if (r < it.r1) fetch(r + 1, nxt);
        if (r >= 0 && r < it.h) {
            float c[VEC], lf[VEC], rt[VEC];
            V::unpack(cur[0], lf);
            V::unpack(cur[1], c);
            V::unpack(cur[2], rt);
            // input row r is tap row ky = 2 of output row r - 1, ky = 1 of row r, ky = 0 of row r + 1
            if (has_l) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    a0[e] = fmaf(wk[6][e], lf[e], a0[e]); a1[e] = fmaf(wk[3][e], lf[e], a1[e]); a2[e] = fmaf(wk[0][e], lf[e], a2[e]);
                }
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                a0[e] = fmaf(wk[7][e], c[e], a0[e]); a1[e] = fmaf(wk[4][e], c[e], a1[e]); a2[e] = fmaf(wk[1][e], c[e], a2[e]);
            }
            if (has_r) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    a0[e] = fmaf(wk[8][e], rt[e], a0[e]); a1[e] = fmaf(wk[5][e], rt[e], a1[e]); a2[e] = fmaf(wk[2][e], rt[e], a2[e]);
                }
            }
        }
        if (r - 1 >= it.r0) {                   // output row r - 1 is complete
            const int64_t o = base + ((int64_t)(r - 1) * it.w + it.x) * C;
            const uint4 yt = V::pack(a0);       // the one rounding
            if (GELU) {
                if (pre) *reinterpret_cast<uint4 *>(pre + o) = yt;
                float yv[VEC];
                V::unpack(yt, yv);
#pragma unroll
                for (int e = 0; e < VEC; ++e) yv[e] = gelu_f(yv[e]);
                *reinterpret_cast<uint4 *>(out + o) = V::pack(yv);
            } else {
                *reinterpret_cast<uint4 *>(out + o) = yt;
            }
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) { a0[e] = a1[e]; a1[e] = a2[e]; a2[e] = bv[e]; }
    }
}

// 4 channels of T <-> floats as one aligned access (8 bytes for 16-bit storage, 16 for fp32)
template <typename T> __device__ __forceinline__ void load4(const T *p, float (&o)[4])
{
    T tmp[4];
    __builtin_memcpy(tmp, __builtin_assume_aligned(p, 4 * sizeof(T)), 4 * sizeof(T));
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = to_f32(tmp[e]);
}
template <typename T> __device__ __forceinline__ void store4(T *p, const float (&v)[4])
{
    T tmp[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) tmp[e] = (T)v[e];
    __builtin_memcpy(__builtin_assume_aligned(p, 4 * sizeof(T)), tmp, 4 * sizeof(T));
}

// ---------------------------------------------------------------- backward: grad_x and the workgroup's partial of grad_w / grad_b
// Thread (item slot tid / CLB, channel lane tid % CLB); blockIdx.y cuts token rows of more than 256 channel lanes.
template <typename T, bool GELU>
__global__ void __launch_bounds__(kThreads)
dwconv_bwd(const T *__restrict__ g_out, const T *__restrict__ x, const T *__restrict__ pre, const T *__restrict__ wgt,
           T *__restrict__ grad_x, float *__restrict__ partial, const ConvLevels lv, const int CL, const int CLB,
           const int64_t N, const int64_t n_items)
{
    constexpr int VEC = kBwdVec;
    __shared__ float red[kSums * VEC * kThreads];
    const int tid = threadIdx.x;
    const int cl = blockIdx.y * CLB + tid % CLB;
    const int slot = tid / CLB, IPB = kThreads / CLB;
    const int64_t bi = (int64_t)blockIdx.x * IPB + slot;
    const bool active = cl < CL && bi < n_items;
    const int64_t C = (int64_t)CL * VEC;

    float gw[9][VEC], gb[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        gb[e] = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) gw[k][e] = 0.f;
    }
    if (active) {
        const Item it = locate_item<kBwdRows>(lv, (int)(bi % lv.items));
        const int64_t base = ((bi / lv.items) * N + it.tok0) * C + (int64_t)cl * VEC;
        float wk[9][VEC];
        {
            float flat[9 * VEC];
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                float part[VEC];
                load4<T>(wgt + ((int64_t)cl * 9 + q) * VEC, part);
#pragma unroll
                for (int e = 0; e < VEC; ++e) flat[q * VEC + e] = part[e];
            }
#pragma unroll
            for (int k = 0; k < 9; ++k)
#pragma unroll
                for (int e = 0; e < VEC; ++e) wk[k][e] = flat[e * 9 + k];
        }
        const bool has_l = it.x > 0, has_r = it.x + 1 < it.w;
        float d0[VEC], d1[VEC], d2[VEC];        // grad_x rows r - 1, r, r + 1
        float xm[VEC], xc[VEC], xp[VEC];        // x rows r - 1, r, r + 1 (used only for rows of the strip)
#pragma unroll
        for (int e = 0; e < VEC; ++e) d0[e] = d1[e] = d2[e] = xm[e] = xc[e] = 0.f;
        load4<T>(x + base + ((int64_t)it.r0 * it.w + it.x) * C, xp);
        for (int r = it.r0 - 1; r <= it.r1; ++r) {
            const bool m_ok = r - 1 >= it.r0, c_ok = r >= it.r0 && r < it.r1, p_ok = r + 1 < it.r1;
            if (r >= 0 && r < it.h) {
                // g_y of (r, x - 1), (r, x), (r, x + 1)
                const int64_t o = base + ((int64_t)r * it.w + it.x) * C;
                float gl[VEC], gc[VEC], gr[VEC];
                auto gy = [&](int64_t at, float (&g)[VEC]) {
                    load4<T>(g_out + at, g);
                    if (GELU) {
                        float yv[VEC];
                        load4<T>(pre + at, yv);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) g[e] *= gelu_grad_f(yv[e]);
                    }
                };
                gy(o, gc);
                gy(has_l ? o - C : o, gl);
                gy(has_r ? o + C : o, gr);
                // g_y[q] meets x[p] / grad_x[p] through tap (ky, kx) with p = q + (ky - 1, kx - 1):
                // row r - 1 <-> ky = 0, r <-> ky = 1, r + 1 <-> ky = 2;  column x + 1 <-> kx = 0, x <-> 1, x - 1 <-> 2
                auto taps = [&](const float (&g)[VEC], auto kx_tag) {
                    constexpr int kx = decltype(kx_tag)::value;
                    if (m_ok) {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) { d0[e] = fmaf(wk[kx][e], g[e], d0[e]); gw[kx][e] = fmaf(xm[e], g[e], gw[kx][e]); }
                    }
                    if (c_ok) {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) { d1[e] = fmaf(wk[3 + kx][e], g[e], d1[e]); gw[3 + kx][e] = fmaf(xc[e], g[e], gw[3 + kx][e]); }
                    }
                    if (p_ok) {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) { d2[e] = fmaf(wk[6 + kx][e], g[e], d2[e]); gw[6 + kx][e] = fmaf(xp[e], g[e], gw[6 + kx][e]); }
                    }
                };
                if (has_r) taps(gr, std::integral_constant<int, 0>());
                taps(gc, std::integral_constant<int, 1>());
                if (has_l) taps(gl, std::integral_constant<int, 2>());
                if (c_ok) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) gb[e] += gc[e];
                }
            }
            if (m_ok) store4<T>(grad_x + base + ((int64_t)(r - 1) * it.w + it.x) * C, d0);
#pragma unroll
            for (int e = 0; e < VEC; ++e) { d0[e] = d1[e]; d1[e] = d2[e]; d2[e] = 0.f; xm[e] = xc[e]; xc[e] = xp[e]; }
            if (r + 2 < it.r1) load4<T>(x + base + ((int64_t)(r + 2) * it.w + it.x) * C, xp);
        }
    }

    // the workgroup's sums: a tree over the item slots in LDS (idle lanes bring zeros), then one fp32 row [10, C]
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
#pragma unroll
        for (int k = 0; k < 9; ++k) red[(k * VEC + e) * kThreads + tid] = gw[k][e];
        red[(9 * VEC + e) * kThreads + tid] = gb[e];
    }
    for (int s = IPB / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (slot < s) {
#pragma unroll
            for (int v = 0; v < kSums * VEC; ++v) red[v * kThreads + tid] += red[v * kThreads + tid + s * CLB];
        }
    }
    if (slot == 0 && cl < CL) {                 // (its own values: no barrier after the last step)
        float *dst = partial + (int64_t)blockIdx.x * kSums * C + (int64_t)cl * VEC;
#pragma unroll
        for (int k = 0; k < kSums; ++k)
            *reinterpret_cast<float4 *>(dst + k * C) =
                make_float4(red[(k * VEC + 0) * kThreads + tid], red[(k * VEC + 1) * kThreads + tid],
                            red[(k * VEC + 2) * kThreads + tid], red[(k * VEC + 3) * kThreads + tid]);
    }
}

// ---------------------------------------------------------------- second stage: partial [rows, 10, C] fp32 -> grad_w [C, 9], grad_b [C]
template <typename T>
__global__ void __launch_bounds__(kRedRows * kRedCols)
dwconv_wgrad_reduce(const float *__restrict__ partial, const int rows, const int C, T *__restrict__ grad_w, T *__restrict__ grad_b)
{
    __shared__ float red[kRedRows][kRedCols + 1];
    const int col = threadIdx.x % kRedCols, rl = threadIdx.x / kRedCols;
    const int E = kSums * C;
    const int e = blockIdx.x * kRedCols + col;
    float s = 0.f;
    if (e < E)
        for (int r = rl; r < rows; r += kRedRows) s += partial[(int64_t)r * E + e];
    red[rl][col] = s;
    for (int o = kRedRows / 2; o >= 1; o >>= 1) {
        __syncthreads();
        if (rl < o) red[rl][col] += red[rl + o][col];
    }
    if (rl == 0 && e < E) {
        const int k = e / C, c = e % C;
        if (k < 9) grad_w[(int64_t)c * 9 + k] = (T)red[0][col];
        else if (grad_b) grad_b[c] = (T)red[0][col];
    }
}

struct ConvPlan {
    ConvLevels fwd, bwd;
    int CV;                     // 16-byte channel vectors per token (forward lanes)
    int CL, CLB, IPB;           // backward: 4-channel lanes per token, lanes per workgroup row, items per workgroup
    int64_t fwd_total;          // forward lanes
    int64_t bwd_items, bwd_blocks;
    bool empty;
};

int fill_levels(const int64_t *level_hw, int L, int64_t N, int rows, ConvLevels *lv)
{
    int64_t tok = 0, items = 0;
    lv->n = L;
    for (int l = 0; l < kMaxLevels; ++l) {
        if (l >= L) { lv->h[l] = lv->w[l] = 1; lv->start[l] = 0; lv->item0[l] = 0x7fffffff; continue; }
        const int64_t h = level_hw[2 * l], w = level_hw[2 * l + 1];
        if (h <= 0 || w <= 0 || h > 0x7fffffffLL || w > 0x7fffffffLL || h * w > 0x7fffffffLL - tok) return MMFS_E_DIMS;
        lv->h[l] = (int)h; lv->w[l] = (int)w; lv->start[l] = (int)tok; lv->item0[l] = (int)items;
        tok += h * w;
        items += ((h + rows - 1) / rows) * w;
    }
    if (tok != N) return MMFS_E_DIMS;
    lv->items = (int)items;
    return MMFS_OK;
}

// the checks every entry shares, in the header's order; MMFS_OK with plan->empty set for B * N * C == 0
int make_plan(int dtype, const int64_t *level_hw, int64_t B, int64_t N, int64_t C, int64_t L, int act, ConvPlan *p)
{
    const int es = elem_size(dtype);
    if (!es) return MMFS_E_DTYPE;
    if (B < 0 || N < 0 || C < 0) return MMFS_E_DIMS;
    if (L < 1 || L > kMaxLevels || (C * es) % 16 || (act != MMFS_DWCONV_ACT_NONE && act != MMFS_DWCONV_ACT_GELU))
        return MMFS_E_UNSUPPORTED;
    p->empty = B == 0 || N == 0 || C == 0;
    if (p->empty) return MMFS_OK;
    if (!level_hw) return MMFS_E_NULLPTR;
    if (N > 0x7fffffffLL || C > (1 << 24) || B > 0x7fffffffLL) return MMFS_E_DIMS;
    int rc;
    if ((rc = fill_levels(level_hw, (int)L, N, kFwdRows, &p->fwd)) || (rc = fill_levels(level_hw, (int)L, N, kBwdRows, &p->bwd)))
        return rc;
    p->CV = (int)(C * es / 16);
    p->CL = (int)(C / kBwdVec);
    p->CLB = 1;
    while (p->CLB < p->CL && p->CLB < kThreads) p->CLB *= 2;
    p->IPB = kThreads / p->CLB;
    p->fwd_total = B * p->fwd.items * p->CV;
    p->bwd_items = B * p->bwd.items;
    p->bwd_blocks = (p->bwd_items + p->IPB - 1) / p->IPB;
    if ((p->fwd_total + kThreads - 1) / kThreads > 0x7fffffffLL || p->bwd_blocks > 0x7fffffffLL ||
        p->bwd_blocks * kSums * C > (int64_t)1 << 40)
        return MMFS_E_DIMS;
    return MMFS_OK;
}

}  // namespace
}  // namespace mmfs

extern "C" {

int mmfs_dwconv_tokens_supported(int dtype, int64_t C, int64_t L, int act)
{
    using namespace mmfs;
    const int es = elem_size(dtype);
    return es && C >= 0 && (C * es) % 16 == 0 && L >= 1 && L <= kMaxLevels &&
           (act == MMFS_DWCONV_ACT_NONE || act == MMFS_DWCONV_ACT_GELU);
}

int mmfs_dwconv_tokens_forward(int dtype, const void *x, const void *weight, const void *bias, void *out, void *pre,
                               const int64_t *level_hw, int64_t B, int64_t N, int64_t C, int64_t L, int act, void *stream)
{
    using namespace mmfs;
    ConvPlan p;
    const int rc = make_plan(dtype, level_hw, B, N, C, L, act, &p);
    if (rc || p.empty) return rc;
    if (const int rt = check_tensors({{x, 16}, {weight, 16}, maybe(bias, 16), {out, 16}, maybe(pre, 16)})) return rt;
    const unsigned blocks = (unsigned)((p.fwd_total + kThreads - 1) / kThreads);
    return by_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        if (act == MMFS_DWCONV_ACT_GELU)
            hipLaunchKernelGGL((dwconv_fwd<T, true>), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, (const T *)x,
                               (const T *)weight, (const T *)bias, (T *)out, (T *)pre, p.fwd, p.CV, N, p.fwd_total);
        else
            hipLaunchKernelGGL((dwconv_fwd<T, false>), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, (const T *)x,
                               (const T *)weight, (const T *)bias, (T *)out, (T *)nullptr, p.fwd, p.CV, N, p.fwd_total);
        return (int)hipGetLastError();
    });
}

int64_t mmfs_dwconv_tokens_backward_workspace_bytes(int dtype, const int64_t *level_hw, int64_t B, int64_t N, int64_t C,
                                                    int64_t L, int act)
{
    using namespace mmfs;
    ConvPlan p;
    const int rc = make_plan(dtype, level_hw, B, N, C, L, act, &p);
    if (rc) return rc;
    return p.empty ? 0 : p.bwd_blocks * kSums * C * (int64_t)sizeof(float);
}

int mmfs_dwconv_tokens_backward(int dtype, const void *grad_out, const void *x, const void *pre, const void *weight,
                                void *grad_x, void *grad_weight, void *grad_bias, void *workspace,
                                const int64_t *level_hw, int64_t B, int64_t N, int64_t C, int64_t L, int act, void *stream)
{
    using namespace mmfs;
    ConvPlan p;
    const int rc = make_plan(dtype, level_hw, B, N, C, L, act, &p);
    if (rc || p.empty) return rc;
    const int es = elem_size(dtype);
    if (const int rt = check_tensors({{grad_out, 16}, {x, 16}, {pre, 16, act == MMFS_DWCONV_ACT_GELU}, {weight, 16}, {grad_x, 16},
                                      {workspace, 16}, {grad_weight, es}, maybe(grad_bias, es)}))
        return rt;
    const dim3 grid((unsigned)p.bwd_blocks, (unsigned)((p.CL + p.CLB - 1) / p.CLB));
    const int E = (int)(kSums * C);
    return by_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        if (act == MMFS_DWCONV_ACT_GELU)
            hipLaunchKernelGGL((dwconv_bwd<T, true>), grid, dim3(kThreads), 0, (hipStream_t)stream, (const T *)grad_out,
                               (const T *)x, (const T *)pre, (const T *)weight, (T *)grad_x, (float *)workspace, p.bwd,
                               p.CL, p.CLB, N, p.bwd_items);
        else
            hipLaunchKernelGGL((dwconv_bwd<T, false>), grid, dim3(kThreads), 0, (hipStream_t)stream, (const T *)grad_out,
                               (const T *)x, (const T *)nullptr, (const T *)weight, (T *)grad_x, (float *)workspace, p.bwd,
                               p.CL, p.CLB, N, p.bwd_items);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL((dwconv_wgrad_reduce<T>), dim3((unsigned)((E + kRedCols - 1) / kRedCols)), dim3(kRedRows * kRedCols),
                           0, (hipStream_t)stream, (const float *)workspace, (int)p.bwd_blocks, (int)C, (T *)grad_weight,
                           (T *)grad_bias);
        return (int)hipGetLastError();
    });
}

}  // extern "C"
