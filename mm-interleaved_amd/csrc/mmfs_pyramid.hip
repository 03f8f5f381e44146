// mmfs_pyramid.hip -- the ViT-Adapter's output pyramid in the token layout, packed for the feature bank, forward and
// backward.
//
// The reference (mm_interleaved/models/encoders/vit_adapter/vit_adapter_hf.py:137-153, encoders/visual_tokenizer.py:74-82)
// transposes the adapter's tokens and the four ViT maps into [B, C, h, w] copies, runs adapter_up, three bilinear
// resizes, five adds and one position add per level, and the bank builder transposes all of it back.  Here every
// input is read where it lies and the packed token-major pyramid [B, sum h_l w_l, C] is written once.  H x W is the ViT
// map (both even); the levels are 4H x 4W, 2H x 2W, H x W, H/2 x W/2, in this order in the packed row:
//     level 1 = up + c1 + bilinear x4 (x1) + pos_1        up [B, 4HW, 4C]: adapter_up as a GEMM on the c2 tokens, columns
//     level 2 = c2 + bilinear x2 (x2) + pos_2                (di, dj, o); pixel (2i + di, 2j + dj) reads row (i, j), block (di, dj)
//     level 3 = c3 + x3 + pos_3                           c [B, 21 HW / 4, C] = c2 | c3 | c4;  x_l [B, HW, C]
//     level 4 = c4 + mean 2x2 (x4) + pos_4                c1 [B, C, 4H, 4W] (NCHW) or [B, 4H, 4W, C] (channels_last)
// pos_l [h_l w_l, C] fp32 or none.  fp32 arithmetic, ONE rounding to the storage type at the store.  The resizes are
// F.interpolate's (align_corners = False): source coordinate max((o + 0.5) / s - 0.5, 0), second index clamped at the
// edge, i.e. the weights {0.75, 0.25} (x2) and {0.625, 0.875, 0.125, 0.375} (x4); x0.5 is the 2x2 mean.  A tap whose
// weight is 0 (only the second tap of the clamped first rows / columns) is NOT read: a non-finite input reaches
// exactly the outputs that hold it under a non-zero weight.  A levels mask (bit l - 1 = level l) selects the levels
// that are produced; the packed row holds the selected ones only.
//
// Forward: pyramid_fwd_rows -- a lane owns one output token and one 16-byte channel vector, consecutive lanes lie
// along C; it serves levels 2..4, and level 1 when c1 is token-major.  pyramid_fwd_c1_nchw -- level 1 for NCHW c1: a
// workgroup moves a 64-pixel x 64-channel tile of c1 through LDS (16-byte reads along the pixels) and its lanes then
// do the same sum as the row walk.
// Backward: no atomics, no clears, every element has one writer, bit-reproducible.  pyramid_bwd_rows: g_up (level 1's
// gradient rows permuted into the (di, dj, o) column blocks) and a token-major g_c1 are copies; g_x1 / g_x2 are gathered
// by their owner from at most 8 x 8 / 4 x 4 gradient pixels with the forward's weights; g_x3 is a copy; g_x4 = 0.25 g_4.
// pyramid_bwd_c1_nchw: level 1's gradient transposed through the LDS tile into NCHW.  g_c is levels 2..4 of the
// gradient itself (the caller's view).  Outputs of levels that are masked out are not touched, and an output whose
// pointer is NULL (a gradient nobody needs) is not computed.
//
// Error bound of an element against fp64 on the same storage-rounded inputs (tests/test_pyramid_head_gpu.py):
//     |got - want| <= u_T |want| + (n + 1) u_32 sum |terms| + t_T,   n = the element's term count:
//     forward  level 1: 6 (up, c1, 4 taps), level 2: 5, level 3: 2, level 4: 5, + 1 with a position table (at most 7);
//     backward g_x1: 64, g_x2: 16, g_x3: 1, g_x4: 1, g_up and g_c1: 1 (copies).
// (A term is weight x value with a weight that is exact in fp32; each joins the sum with one fp32 rounding.)
//
// The extents reach the kernels by value (Pyr): no device table, no allocation, no synchronisation -- the launches can
// be captured into a graph.  Offsets are 64-bit.
#include "msda_host.h"
#include <hip/hip_runtime.h>

namespace mmfs {

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;               // pixels x channels of a transposition tile
constexpr int kNone = 0x7fffffff;       // first item of a segment the row walk does not serve

struct Pyr {
    int H, W;                           // the ViT map
    int S;                              // tokens of a packed row
    int out0[4];                        // first token of level l + 1 in the packed row
    int rows;                           // items (tokens) per sample of the row walk
    int row0[5];                        // first item of a segment: forward the four levels; backward level 1's
                                        // gradient rows (g_up, token-major g_c1), g_x1, g_x2, g_x3, g_x4
};

// one axis of F.interpolate's bilinear resize by S (align_corners = False): output o reads i0 and i1 with w0 and w1
struct Lin { int i0, i1; float w0, w1; };
template <int S> __device__ __forceinline__ Lin lin(int o, int n)
{
    const float src = fmaxf(((float)o + 0.5f) * (1.f / S) - 0.5f, 0.f);
    Lin t;
    t.i0 = (int)src;
    t.w1 = src - (float)t.i0;
    t.w0 = 1.f - t.w1;
    t.i1 = min(t.i0 + 1, n - 1);
    return t;
}
// the weight of source i in output o of that axis
template <int S> __device__ __forceinline__ float lin_weight(int o, int i, int n)
{
    const Lin t = lin<S>(o, n);
    return (t.i0 == i ? t.w0 : 0.f) + (t.i1 == i ? t.w1 : 0.f);
}

template <typename T, int VEC>
__device__ __forceinline__ void fma_row(float (&acc)[VEC], float w, const T *p)
{
    float v[VEC];
    Vec16<T>::unpack(*reinterpret_cast<const uint4 *>(p), v);
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = fmaf(w, v[e], acc[e]);
}

// acc += bilinear x S of the n_y x n_x map at ``map`` (the lane's channels of its first token), output pixel (y, x)
template <typename T, int S, int VEC>
__device__ __forceinline__ void add_bilinear(float (&acc)[VEC], const T *map, int y, int x, int ny, int nx, int64_t C)
{
    const Lin ty = lin<S>(y, ny), tx = lin<S>(x, nx);
    const T *r0 = map + (int64_t)ty.i0 * nx * C, *r1 = map + (int64_t)ty.i1 * nx * C;
    fma_row<T, VEC>(acc, ty.w0 * tx.w0, r0 + tx.i0 * C);
    if (tx.w1 != 0.f) fma_row<T, VEC>(acc, ty.w0 * tx.w1, r0 + tx.i1 * C);
    if (ty.w1 != 0.f) {
        fma_row<T, VEC>(acc, ty.w1 * tx.w0, r1 + tx.i0 * C);
        if (tx.w1 != 0.f) fma_row<T, VEC>(acc, ty.w1 * tx.w1, r1 + tx.i1 * C);
    }
}

template <int VEC> __device__ __forceinline__ void add_pos(float (&acc)[VEC], const float *pos)
{
    if (!pos) return;
    float p[VEC];
    load_vec<float, VEC>(pos, p);
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] += p[e];
}

// level 1 at pixel t = (y, x) of sample b, the lane's channels ch: acc holds c1 on entry
template <typename T, int VEC>
__device__ __forceinline__ void level1_sum(float (&acc)[VEC], const T *up, const T *x1, const float *pos, const Pyr &g,
                                           int64_t b, int t, int64_t C, int ch)
{
    const int w = 4 * g.W, y = t / w, x = t - y * w;
    const int64_t HW = (int64_t)g.H * g.W;
    const int64_t urow = b * 4 * HW + (int64_t)(y >> 1) * (2 * g.W) + (x >> 1);
    fma_row<T, VEC>(acc, 1.f, up + (urow * 4 + (y & 1) * 2 + (x & 1)) * C + ch);
    add_bilinear<T, 4, VEC>(acc, x1 + b * HW * C + ch, y, x, g.H, g.W, C);
    add_pos<VEC>(acc, pos ? pos + (int64_t)t * C + ch : nullptr);
}

// item k of a sample -> its segment and the item within it, by selects: the struct stays in scalar registers
template <int N> __device__ __forceinline__ int locate_segment(const Pyr &g, int k, int &t)
{
    int seg = 0, k0 = 0;
#pragma unroll
    for (int s = 0; s < N; ++s) {
        const bool in = k >= g.row0[s];
        seg = in ? s : seg; k0 = in ? g.row0[s] : k0;
    }
    t = k - k0;
    return seg;
}

// ---------------------------------------------------------------- forward, row walk: lane <-> (sample, token, 16-byte channel vector)
template <typename T>
__global__ void __launch_bounds__(kThreads)
pyramid_fwd_rows(const T *__restrict__ c, const T *__restrict__ x1, const T *__restrict__ x2, const T *__restrict__ x3,
                 const T *__restrict__ x4, const T *__restrict__ up, const T *__restrict__ c1,
                 const float *__restrict__ p1, const float *__restrict__ p2, const float *__restrict__ p3,
                 const float *__restrict__ p4, T *__restrict__ out, const Pyr g, const int CV, const int64_t total)
{
    typedef Vec16<T> V;
    constexpr int VEC = V::N;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % CV) * VEC;
    const int64_t r = i / CV, b = r / g.rows;
    int t;
    const int lev = locate_segment<4>(g, (int)(r - b * g.rows), t);
    const int64_t C = (int64_t)CV * VEC, HW = (int64_t)g.H * g.W, Nc = HW * 21 / 4;
    float acc[VEC];
    if (lev == 0) {
        V::unpack(*reinterpret_cast<const uint4 *>(c1 + (b * 16 * HW + t) * C + ch), acc);
        level1_sum<T, VEC>(acc, up, x1, p1, g, b, t, C, ch);
    } else if (lev == 1) {
        const int w = 2 * g.W, y = t / w, x = t - y * w;
        V::unpack(*reinterpret_cast<const uint4 *>(c + (b * Nc + t) * C + ch), acc);
        add_bilinear<T, 2, VEC>(acc, x2 + b * HW * C + ch, y, x, g.H, g.W, C);
        add_pos<VEC>(acc, p2 ? p2 + (int64_t)t * C + ch : nullptr);
    } else if (lev == 2) {
        V::unpack(*reinterpret_cast<const uint4 *>(c + (b * Nc + 4 * HW + t) * C + ch), acc);
        fma_row<T, VEC>(acc, 1.f, x3 + (b * HW + t) * C + ch);
        add_pos<VEC>(acc, p3 ? p3 + (int64_t)t * C + ch : nullptr);
    } else {
        const int w = g.W / 2, y = t / w, x = t - y * w;
        V::unpack(*reinterpret_cast<const uint4 *>(c + (b * Nc + 5 * HW + t) * C + ch), acc);
        const T *q = x4 + (b * HW + (int64_t)(2 * y) * g.W + 2 * x) * C + ch;
        fma_row<T, VEC>(acc, 0.25f, q);
        fma_row<T, VEC>(acc, 0.25f, q + C);
        fma_row<T, VEC>(acc, 0.25f, q + g.W * C);
        fma_row<T, VEC>(acc, 0.25f, q + g.W * C + C);
        add_pos<VEC>(acc, p4 ? p4 + (int64_t)t * C + ch : nullptr);
    }
    *reinterpret_cast<uint4 *>(out + (b * g.S + g.out0[lev] + t) * C + ch) = V::pack(acc);     // the one rounding
}

// ---------------------------------------------------------------- forward, level 1 with NCHW c1: a 64 x 64 tile through LDS
// Workgroup <-> (sample, 64 pixels, 64 channels); 16 H W is a multiple of 64, C of the vector (a vector of channels
// is all inside or all outside the tile's live part).
template <typename T>
__global__ void __launch_bounds__(kThreads)
pyramid_fwd_c1_nchw(const T *__restrict__ x1, const T *__restrict__ up, const T *__restrict__ c1,
                    const float *__restrict__ p1, T *__restrict__ out, const Pyr g, const int C, const int c_tiles,
                    const int p_tiles)
{
    typedef Vec16<T> V;
    constexpr int VEC = V::N;
    constexpr int PITCH = kTile + 4 / (int)sizeof(T);          // + 1 dword: transposed reads hit distinct banks
    constexpr int VPR = kTile / VEC;                           // vectors per tile row, either way
    __shared__ __attribute__((aligned(16))) T tile[kTile * PITCH];
    const int tid = threadIdx.x;
    const int ctile = blockIdx.x % c_tiles;
    const int64_t rest = blockIdx.x / c_tiles, b = rest / p_tiles;
    const int t0 = (int)(rest - b * p_tiles) * kTile, c0 = ctile * kTile;
    const int nc = min(kTile, C - c0);
    const int64_t P = (int64_t)16 * g.H * g.W;
    const T *src = c1 + (b * C + c0) * P + t0;
    for (int i = tid; i < kTile * VPR; i += kThreads) {
        const int cc = i / VPR, v = i - cc * VPR;
        if (cc < nc) {
            const uint4 q = *reinterpret_cast<const uint4 *>(src + (int64_t)cc * P + v * VEC);
            uint32_t *dst = reinterpret_cast<uint32_t *>(tile + cc * PITCH + v * VEC);
            dst[0] = q.x; dst[1] = q.y; dst[2] = q.z; dst[3] = q.w;
        }
    }
    __syncthreads();
    for (int i = tid; i < kTile * VPR; i += kThreads) {
        const int t = i / VPR, v = i - t * VPR;
        if (v * VEC < nc) {
            float acc[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = to_f32(tile[(v * VEC + e) * PITCH + t]);
            const int ch = c0 + v * VEC;
            level1_sum<T, VEC>(acc, up, x1, p1, g, b, t0 + t, C, ch);
            *reinterpret_cast<uint4 *>(out + (b * g.S + g.out0[0] + t0 + t) * C + ch) = V::pack(acc);
        }
    }
}

// ---------------------------------------------------------------- backward, row walk
// acc = sum over the gradient pixels of the S-times larger map ``gmap`` that read source pixel (i, j), with the
// forward's weights; a pixel under weight 0 is not read
template <typename T, int S, int VEC>
__device__ __forceinline__ void gather_bilinear(float (&acc)[VEC], const T *gmap, int i, int j, int ny, int nx, int64_t C)
{
    const int y_lo = max(0, S * i - S / 2), y_hi = min(S * ny - 1, S * i + S + S / 2 - 1);
    const int x_lo = max(0, S * j - S / 2), x_hi = min(S * nx - 1, S * j + S + S / 2 - 1);
    for (int oy = y_lo; oy <= y_hi; ++oy) {
        const float wy = lin_weight<S>(oy, i, ny);
        if (wy == 0.f) continue;
        const T *row = gmap + (int64_t)oy * (S * nx) * C;
        for (int ox = x_lo; ox <= x_hi; ++ox) {
            const float wx = lin_weight<S>(ox, j, nx);
            if (wx != 0.f) fma_row<T, VEC>(acc, wy * wx, row + ox * C);
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
pyramid_bwd_rows(const T *__restrict__ gr, T *__restrict__ g_up, T *__restrict__ g_c1, T *__restrict__ g_x1,
                 T *__restrict__ g_x2, T *__restrict__ g_x3, T *__restrict__ g_x4, const Pyr g, const int CV,
                 const int64_t total)
{
    typedef Vec16<T> V;
    constexpr int VEC = V::N;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % CV) * VEC;
    const int64_t r = i / CV, b = r / g.rows;
    int t;
    const int seg = locate_segment<5>(g, (int)(r - b * g.rows), t);
    const int64_t C = (int64_t)CV * VEC, HW = (int64_t)g.H * g.W;
    const T *grow = gr + b * g.S * C + ch;                     // the sample's packed gradient row, the lane's channels
    if (seg == 0) {
        const int w = 4 * g.W, y = t / w, x = t - y * w;
        const uint4 q = *reinterpret_cast<const uint4 *>(grow + (int64_t)(g.out0[0] + t) * C);
        const int64_t urow = b * 4 * HW + (int64_t)(y >> 1) * (2 * g.W) + (x >> 1);
        if (g_up) *reinterpret_cast<uint4 *>(g_up + (urow * 4 + (y & 1) * 2 + (x & 1)) * C + ch) = q;
        if (g_c1) *reinterpret_cast<uint4 *>(g_c1 + (b * 16 * HW + t) * C + ch) = q;
        return;
    }
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    const int y = t / g.W, x = t - y * g.W;
    T *dst;
    if (seg == 1) {
        gather_bilinear<T, 4, VEC>(acc, grow + (int64_t)g.out0[0] * C, y, x, g.H, g.W, C);
        dst = g_x1;
    } else if (seg == 2) {
        gather_bilinear<T, 2, VEC>(acc, grow + (int64_t)g.out0[1] * C, y, x, g.H, g.W, C);
        dst = g_x2;
    } else if (seg == 3) {
        fma_row<T, VEC>(acc, 1.f, grow + (int64_t)(g.out0[2] + t) * C);
        dst = g_x3;
    } else {
        fma_row<T, VEC>(acc, 0.25f, grow + (int64_t)(g.out0[3] + (y >> 1) * (g.W / 2) + (x >> 1)) * C);
        dst = g_x4;
    }
    *reinterpret_cast<uint4 *>(dst + (b * HW + t) * C + ch) = V::pack(acc);
}

// ---------------------------------------------------------------- backward, g_c1 in NCHW: level 1's gradient rows transposed (bits only)
template <int BYTES>
__global__ void __launch_bounds__(kThreads)
pyramid_bwd_c1_nchw(const void *__restrict__ gr_, void *__restrict__ g_c1_, const Pyr g, const int C, const int c_tiles,
                    const int p_tiles)
{
    typedef typename Word<BYTES>::type E;
    constexpr int VEC = 16 / BYTES;
    constexpr int PITCH = kTile + 4 / BYTES;
    constexpr int VPR = kTile / VEC;
    __shared__ __attribute__((aligned(16))) E tile[kTile * PITCH];
    const int tid = threadIdx.x;
    const int ctile = blockIdx.x % c_tiles;
    const int64_t rest = blockIdx.x / c_tiles, b = rest / p_tiles;
    const int t0 = (int)(rest - b * p_tiles) * kTile, c0 = ctile * kTile;
    const int nc = min(kTile, C - c0);
    const int64_t P = (int64_t)16 * g.H * g.W;
    const E *src = (const E *)gr_ + (b * g.S + g.out0[0] + t0) * C + c0;
    for (int i = tid; i < kTile * VPR; i += kThreads) {
        const int t = i / VPR, v = i - t * VPR;
        if (v * VEC < nc) {
            const uint4 q = *reinterpret_cast<const uint4 *>(src + (int64_t)t * C + v * VEC);
            E x[VEC];
            __builtin_memcpy(x, &q, 16);
#pragma unroll
            for (int e = 0; e < VEC; ++e) tile[(v * VEC + e) * PITCH + t] = x[e];
        }
    }
    __syncthreads();
    E *dst = (E *)g_c1_ + (b * C + c0) * P + t0;
    for (int i = tid; i < kTile * VPR; i += kThreads) {
        const int cc = i / VPR, v = i - cc * VPR;
        if (cc < nc) {
            const uint32_t *s = reinterpret_cast<const uint32_t *>(tile + cc * PITCH + v * VEC);
            *reinterpret_cast<uint4 *>(dst + (int64_t)cc * P + v * VEC) = make_uint4(s[0], s[1], s[2], s[3]);
        }
    }
}

bool supported(int es, int64_t C, int64_t H, int64_t W, int levels)
{
    return es && C >= 0 && (C * es) % 16 == 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && levels >= 1 && levels <= 15;
}

struct Plan {
    Pyr fwd, bwd;
    int CV, c_tiles, p_tiles;
    int64_t fwd_total, bwd_total, tile_blocks;      // lanes of the two row walks, workgroups of a tile kernel
    bool empty;
};

// the backward's row walk over the segments that are wanted: level 1's gradient rows (g_up, token-major g_c1), g_x1 .. g_x4
void lay_out_backward(Plan *p, int64_t B, const bool (&seg_on)[5])
{
    const int64_t HW = (int64_t)p->bwd.H * p->bwd.W, seg[5] = {16 * HW, HW, HW, HW, HW};
    int64_t br = 0;
    for (int s = 0; s < 5; ++s) {
        p->bwd.row0[s] = seg_on[s] ? (int)br : kNone;
        if (seg_on[s]) br += seg[s];
    }
    p->bwd.rows = (int)br;
    p->bwd_total = B * br * p->CV;
}

// the checks every entry shares, in the header's order; MMFS_OK with plan->empty set for B * C == 0
int make_plan(int dtype, int64_t B, int64_t H, int64_t W, int64_t C, int levels, int c1_layout, Plan *p)
{
    const int es = elem_size(dtype);
    if (!es) return MMFS_E_DTYPE;
    if (B < 0 || H < 0 || W < 0 || C < 0) return MMFS_E_DIMS;
    if (!supported(es, C, H, W, levels) || (c1_layout != MMFS_PYRAMID_C1_NCHW && c1_layout != MMFS_PYRAMID_C1_NHWC))
        return MMFS_E_UNSUPPORTED;
    p->empty = B == 0 || C == 0;
    if (p->empty) return MMFS_OK;
    if (H > (1 << 12) || W > (1 << 12) || C > (1 << 24) || B > 0x7fffffffLL) return MMFS_E_DIMS;     // 16 H W <= 2^28
    const int64_t HW = H * W, px[4] = {16 * HW, 4 * HW, HW, HW / 4};
    const bool rows1 = c1_layout == MMFS_PYRAMID_C1_NHWC;
    Pyr &f = p->fwd, &b = p->bwd;
    f.H = b.H = (int)H; f.W = b.W = (int)W;
    int64_t tok = 0, fr = 0;
    for (int l = 0; l < 4; ++l) {
        const bool on = (levels >> l) & 1;
        f.out0[l] = b.out0[l] = on ? (int)tok : 0;
        const bool walk = on && (l > 0 || rows1);
        f.row0[l] = walk ? (int)fr : kNone;
        if (on) tok += px[l];
        if (walk) fr += px[l];
    }
    f.row0[4] = kNone;
    f.S = b.S = (int)tok; f.rows = (int)fr;
    // (the backward's segments depend on which outputs are wanted: lay_out_backward; bounded here by all of them)
    const int64_t br = 20 * HW;
    p->CV = (int)(C * es / 16);
    p->c_tiles = (int)((C + kTile - 1) / kTile);
    p->p_tiles = (int)(px[0] / kTile);
    p->fwd_total = B * fr * p->CV;
    p->bwd_total = B * br * p->CV;
    b.rows = 0;
    p->tile_blocks = (levels & 1) && !rows1 ? B * p->p_tiles * p->c_tiles : 0;      // (the forward's; the backward's is this or 0)
    if ((p->fwd_total + kThreads - 1) / kThreads > 0x7fffffffLL || (p->bwd_total + kThreads - 1) / kThreads > 0x7fffffffLL ||
        p->tile_blocks > 0x7fffffffLL)
        return MMFS_E_DIMS;
    return MMFS_OK;
}

}  // namespace
}  // namespace mmfs

extern "C" {

int mmfs_pyramid_head_supported(int dtype, int64_t C, int64_t H, int64_t W, int levels)
{
    return mmfs::supported(mmfs::elem_size(dtype), C, H, W, levels);
}

int mmfs_pyramid_head_forward(int dtype, const void *c, const void *x1, const void *x2, const void *x3, const void *x4,
                              const void *up, const void *c1, const float *pos1, const float *pos2, const float *pos3,
                              const float *pos4, void *out, int64_t B, int64_t H, int64_t W, int64_t C, int levels,
                              int c1_layout, void *stream)
{
    using namespace mmfs;
    Plan p;
    const int rc = make_plan(dtype, B, H, W, C, levels, c1_layout, &p);
    if (rc || p.empty) return rc;
    // a level's pointers are looked at only if the mask has the level; its position table may be NULL
    auto of = [&](int mask, const void *p, bool needed) { return Tensor{(levels & mask) ? p : nullptr, 16, (levels & mask) && needed}; };
    if (const int rt = check_tensors({{out, 16}, of(14, c, true), of(1, up, true), of(1, c1, true), of(1, x1, true), of(2, x2, true),
                                      of(4, x3, true), of(8, x4, true), of(1, pos1, false), of(2, pos2, false), of(4, pos3, false),
                                      of(8, pos4, false)}))
        return rt;
    return by_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        if (p.fwd_total) {
            hipLaunchKernelGGL((pyramid_fwd_rows<T>), dim3((unsigned)((p.fwd_total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                               (hipStream_t)stream, (const T *)c, (const T *)x1, (const T *)x2, (const T *)x3, (const T *)x4,
                               (const T *)up, (const T *)c1, pos1, pos2, pos3, pos4, (T *)out, p.fwd, p.CV, p.fwd_total);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return (int)e;
        }
        if (p.tile_blocks)
            hipLaunchKernelGGL((pyramid_fwd_c1_nchw<T>), dim3((unsigned)p.tile_blocks), dim3(kThreads), 0, (hipStream_t)stream,
                               (const T *)x1, (const T *)up, (const T *)c1, pos1, (T *)out, p.fwd, (int)C, p.c_tiles, p.p_tiles);
        return (int)hipGetLastError();
    });
}

int mmfs_pyramid_head_backward(int dtype, const void *grad_out, void *grad_up, void *grad_c1, void *grad_x1, void *grad_x2,
                               void *grad_x3, void *grad_x4, int64_t B, int64_t H, int64_t W, int64_t C, int levels,
                               int c1_layout, void *stream)
{
    using namespace mmfs;
    Plan p;
    const int rc = make_plan(dtype, B, H, W, C, levels, c1_layout, &p);
    if (rc || p.empty) return rc;
    const bool rows1 = c1_layout == MMFS_PYRAMID_C1_NHWC;
    // a NULL output is a gradient nobody asked for: its segment leaves the row walk (pointers of levels outside the mask
    // are not looked at)
    void *gx[4] = {grad_x1, grad_x2, grad_x3, grad_x4};
    for (int l = 0; l < 4; ++l)
        if (!((levels >> l) & 1)) gx[l] = nullptr;
    if (!(levels & 1)) grad_up = grad_c1 = nullptr;
    if (const int rt = check_tensors({{grad_out, 16}, maybe(gx[0], 16), maybe(gx[1], 16), maybe(gx[2], 16), maybe(gx[3], 16),
                                      maybe(grad_up, 16), maybe(grad_c1, 16)}))
        return rt;
    void *rows_c1 = rows1 ? grad_c1 : nullptr;
    const bool seg_on[5] = {grad_up || rows_c1, gx[0] != nullptr, gx[1] != nullptr, gx[2] != nullptr, gx[3] != nullptr};
    lay_out_backward(&p, B, seg_on);
    const bool tile = grad_c1 && !rows1;
    const int es = elem_size(dtype);
    return by_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        if (p.bwd_total) {
            hipLaunchKernelGGL((pyramid_bwd_rows<T>), dim3((unsigned)((p.bwd_total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                               (hipStream_t)stream, (const T *)grad_out, (T *)grad_up, (T *)rows_c1, (T *)gx[0], (T *)gx[1],
                               (T *)gx[2], (T *)gx[3], p.bwd, p.CV, p.bwd_total);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return (int)e;
        }
        if (!tile) return (int)hipSuccess;
        const unsigned blocks = (unsigned)(B * p.p_tiles * p.c_tiles);
        if (es == 4)
            hipLaunchKernelGGL((pyramid_bwd_c1_nchw<4>), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream,
                               grad_out, grad_c1, p.bwd, (int)C, p.c_tiles, p.p_tiles);
        else
            hipLaunchKernelGGL((pyramid_bwd_c1_nchw<2>), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream,
                               grad_out, grad_c1, p.bwd, (int)C, p.c_tiles, p.p_tiles);
        return (int)hipGetLastError();
    });
}

}  // extern "C"
