// mmfs_sequence.hip -- the interleaved sequence built on the device: the token embeddings with the
// visual embeddings and the <soi> token in place, and the per-image context of the image decoder, forward and backward.
//
// The reference (mm_interleaved/models/mm_interleaved.py:144-171, :254-304) finds the special tokens with nonzero() on
// the host's clock, scatters in four passes over [B L, C], and builds the image decoder's context in a Python loop over
// the images with a device scalar per slice.  Here ONE launch turns text_ids [B, L] into int32 tables (seq_index) and
// every other kernel reads them: nothing returns to the host, sizes travel by value, nothing is allocated -- the
// launches can be captured into a graph.
//
//   seq_index        img_rank [B L]: the row-major rank of an image token, -1 for any other token and for a rank >= n_vis
//                    img_pos [n_vis]: its inverse, -1 where no such token exists
//                    soi_row / soi_col [n_images]: row and column of the k-th <soi>, row-major, -1 past the last one
//                    row_first [B + 1]: images of row b are row_first[b] .. row_first[b + 1] (both at most n_images)
//                    counts [2]: image tokens and <soi> tokens found (not clamped)
//                    One workgroup of 1024 lanes scans chunks of 1024 tokens: a wave scan by shuffles, the 16 wave totals
//                    through LDS (double-buffered: one barrier per chunk), the running totals in registers.
//   seq_embed_fwd    out[r] = img_rank[r] >= 0 ? vis[img_rank[r]] : T(text[r]);  text is stored as T or as fp32.  A row
//                    whose id is <soi>: out[r] = round_T(float(out[r]) + float(soi_token)) -- one add, one rounding, on
//                    the value ALREADY rounded to T, as scatter_add in T does.  Every other row is a copy (bits).
//   seq_embed_bwd    grad_text[r] = img_rank[r] >= 0 ? 0 : grad[r] (text's type);  grad_vis[k] = img_pos[k] >= 0 ?
//                    grad[img_pos[k]] : 0;  grad_soi = sum over the <soi> rows k = 0 .. min(counts[1], n_images) - 1 in
//                    ascending k, fp32, one rounding (a lane per channel vector walks the rows).  One launch, every
//                    element of the three written; an output whose pointer is NULL is not computed.
//   seq_context_fwd  image i has the window (row_i, col_i, len_i): row_i = soi_row[i]; col_i = start_idx[i] when the caller
//                    gives one, else soi_col[i]; bos_i = max(bos_idx[i], 0) or 0; len_i = col_i - bos_i + 1, and 0 when
//                    row_i < 0 or col_i is outside [0, L); clamped to [0, max_len].
//                        out[i, j] = round_T(float(src[row_i, col_i - j]) + float(pos[j]))     j < len_i
//                                  = round_T(float(pad_row)               + float(pos[j]))     len_i <= j < max_len
//                        mask[i, j] = j < len_i  (int64)
//                    A NULL pad_row counts as 0; with a NULL pos the value is copied (bits), not added.  pos is stored
//                    in T: the reference rounds its table to the storage type before it adds.
//   seq_context_bwd  grad_src[b, t] = sum of grad_out[i, col_i - t] over the images i of row b (row_first) with
//                    0 <= col_i - t < len_i, in ascending i, fp32, one rounding; zero where no window covers the token.
//   seq_context_bwd_pad   grad_pad = sum_i sum_{len_i <= j < max_len} grad_out[i, j]: stage 1, a lane per (image, channel
//                    vector) adds its rows in ascending j into fp32 scratch [n_images, C] (the caller's; every element
//                    written); stage 2, a lane per channel vector adds the images in ascending i and rounds once.
// No atomics, no clears, one writer per element, a fixed order: every result is bit-reproducible.  A value that does
// not take part is not touched: a padded row is pad_row + pos, whatever src holds.
//
// Longest chain of sequential fp32 additions into one element (the n of the tests' bound (n - 1) 2^-24 sum |terms|;
// the first term joins an accumulator of 0 exactly):
//     grad_soi:  n = min(counts[1], n_images), the <soi> rows
//     grad_src:  n = the images of the row whose window covers the token (at most row_first[b + 1] - row_first[b])
//     grad_pad:  n = max_i (max_len - len_i) + n_images - 1   (stage 1's rows of one image, then the other images' sums)
// Forward: one addition, one rounding.
//
// A lane owns one 16-byte channel vector of one row and consecutive lanes lie along C.  Offsets are 64-bit.  Results that
// the same call does not read again leave with the non-temporal hint.
#include "msda_host.h"
#include <hip/hip_runtime.h>

namespace mmfs {

namespace {

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;
constexpr int64_t kMaxTokens = 1 << 22;         // seq_index: B * L (and n_vis, n_images) at most
constexpr int kPadUnroll = 4;                   // stage 1 of grad_pad: independent loads in flight, added in order

// ---------------------------------------------------------------- the tables
__global__ void __launch_bounds__(kScanThreads)
seq_index(const int64_t *__restrict__ ids, const int N, const int B, const int L, const int64_t image_id, const int64_t soi_id,
          const int n_vis, const int n_images, int32_t *__restrict__ img_rank, int32_t *__restrict__ img_pos,
          int32_t *__restrict__ soi_row, int32_t *__restrict__ soi_col, int32_t *__restrict__ row_first,
          int32_t *__restrict__ counts)
{
    __shared__ uint32_t wave_total[2][kScanThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base_img = 0, base_soi = 0;             // found before the chunk (the same in every lane)
    for (int c0 = 0, it = 0; c0 < N; c0 += kScanThreads, ++it) {
        const int t = c0 + tid;
        const int64_t id = t < N ? ids[t] : 0;
        const bool im = t < N && id == image_id, so = t < N && id == soi_id;
        // both counts of a chunk are at most 1024: one word carries them, image tokens low, <soi> high
        const uint32_t v = (im ? 1u : 0u) | (so ? 0x10000u : 0u);
        uint32_t inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wave_total[it & 1][wave] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kScanThreads / 64; ++w) {
            const uint32_t x = wave_total[it & 1][w];
            total += x;
            before += w < wave ? x : 0u;
        }
        const uint32_t exc = before + inc - v;
        const int ri = base_img + (int)(exc & 0xffffu), rs = base_soi + (int)(exc >> 16);
        if (t < N) {
            const bool placed = im && ri < n_vis;
            img_rank[t] = placed ? ri : -1;
            if (placed) img_pos[ri] = t;
            const int row = t / L, col = t - row * L;
            if (so && rs < n_images) { soi_row[rs] = row; soi_col[rs] = col; }
            if (col == 0) row_first[row] = min(rs, n_images);
        }
        base_img += (int)(total & 0xffffu);
        base_soi += (int)(total >> 16);
    }
    for (int k = min(base_img, n_vis) + tid; k < n_vis; k += kScanThreads) img_pos[k] = -1;
    for (int k = min(base_soi, n_images) + tid; k < n_images; k += kScanThreads) { soi_row[k] = -1; soi_col[k] = -1; }
    if (N == 0)
        for (int b = tid; b < B; b += kScanThreads) row_first[b] = 0;
    if (tid == 0) {
        row_first[B] = min(base_soi, n_images);
        counts[0] = base_img;
        counts[1] = base_soi;
    }
}

template <int VEC> __device__ __forceinline__ void zero(float (&v)[VEC])
{
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = 0.f;
}

template <typename T, int VEC> __device__ __forceinline__ void add_row(float (&acc)[VEC], const T *p)
{
    float v[VEC];
    load_vec<T, VEC>(p, v);
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] += v[e];
}

// ---------------------------------------------------------------- embeddings: lane <-> (token row, 16-byte channel vector of T)
template <typename T, typename TX>
__global__ void __launch_bounds__(kThreads)
seq_embed_fwd(const TX *__restrict__ text, const T *__restrict__ vis, const T *__restrict__ soi,
              const int64_t *__restrict__ ids, const int64_t soi_id, const int32_t *__restrict__ img_rank,
              T *__restrict__ out, const int CV, const int64_t total)
{
    typedef Vec16<T> V;
    constexpr int VEC = V::N;
    constexpr bool kSame = sizeof(TX) == sizeof(T);             // text is stored as T
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % CV) * VEC;
    const int64_t r = i / CV, C = (int64_t)CV * VEC;
    const int rank = img_rank[r];
    const bool is_soi = ids[r] == soi_id;
    T *dst = out + r * C + ch;
    if (!is_soi && (kSame || rank >= 0)) {                      // a copy
        const void *src = rank >= 0 ? (const void *)(vis + (int64_t)rank * C + ch) : (const void *)(text + r * C + ch);
        store16_stream(dst, *reinterpret_cast<const uint4 *>(src));
        return;
    }
    float v[VEC];
    if (rank >= 0) load_vec<T, VEC>(vis + (int64_t)rank * C + ch, v);
    else load_vec<TX, VEC>(text + r * C + ch, v);
    if (is_soi) {
        if (!kSame && rank < 0) {                               // the reference's cast comes before its scatter_add
            const uint4 q = V::pack(v);
            V::unpack(q, v);
        }
        add_row<T, VEC>(v, soi + ch);
    }
    store_vec<T, VEC, true>(dst, v);
}

// items: the token rows (grad_text), the visual rows (grad_vis), one more for grad_soi
template <typename T, typename TX>
__global__ void __launch_bounds__(kThreads)
seq_embed_bwd(const T *__restrict__ grad, const int32_t *__restrict__ img_rank, const int32_t *__restrict__ img_pos,
              const int32_t *__restrict__ soi_row, const int32_t *__restrict__ soi_col, const int32_t *__restrict__ counts,
              TX *__restrict__ g_text, T *__restrict__ g_vis, T *__restrict__ g_soi, const int CV, const int64_t rows,
              const int64_t n_vis, const int n_images, const int L, const int64_t total)
{
    typedef Vec16<T> V;
    constexpr int VEC = V::N;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % CV) * VEC;
    int64_t k = i / CV;
    const int64_t C = (int64_t)CV * VEC;
    if (k < rows) {
        if (!g_text) return;
        float v[VEC];
        zero<VEC>(v);
        if (img_rank[k] < 0) load_vec<T, VEC>(grad + k * C + ch, v);
        store_vec<TX, VEC, true>(g_text + k * C + ch, v);       // (exact: TX is T or wider)
        return;
    }
    k -= rows;
    if (k < n_vis) {
        if (!g_vis) return;
        const int p = img_pos[k];
        const uint4 q = p >= 0 ? *reinterpret_cast<const uint4 *>(grad + (int64_t)p * C + ch) : make_uint4(0, 0, 0, 0);
        store16_stream(g_vis + k * C + ch, q);
        return;
    }
    if (!g_soi) return;
    const int n = min(counts[1], n_images);
    float acc[VEC];
    zero<VEC>(acc);
    for (int s = 0; s < n; ++s) add_row<T, VEC>(acc, grad + ((int64_t)soi_row[s] * L + soi_col[s]) * C + ch);
    store_vec<T, VEC, false>(g_soi + ch, acc);
}

// ---------------------------------------------------------------- the image decoder's context
struct Ctx {
    const int32_t *soi_row, *soi_col, *row_first;
    const int64_t *start_idx, *bos_idx;         // the caller's image_start_token_idx / nearest_bos_idxs, or null
    int L, n_images, max_len;
};

struct Window { int row, col, len; };           // rows col, col - 1, .. col - len + 1 of text row ``row``; len in [0, max_len]

__device__ __forceinline__ Window window_of(const Ctx &g, int i)
{
    Window w;
    w.row = g.soi_row[i];
    const int64_t col = g.start_idx ? g.start_idx[i] : (int64_t)g.soi_col[i];
    const int64_t bos_i = g.bos_idx ? g.bos_idx[i] : 0, bos = bos_i > 0 ? bos_i : 0;
    const bool live = w.row >= 0 && col >= 0 && col < g.L;
    const int64_t len = live ? col - bos + 1 : 0;
    w.col = live ? (int)col : 0;
    w.len = len < 0 ? 0 : len > g.max_len ? g.max_len : (int)len;
    return w;
}

// lane <-> (image, position j, channel vector)
template <typename T>
__global__ void __launch_bounds__(kThreads)
seq_context_fwd(const T *__restrict__ src, const T *__restrict__ pad_row, const T *__restrict__ pos, T *__restrict__ out,
                int64_t *__restrict__ mask, const Ctx g, const int CV, const int64_t total)
{
    typedef Vec16<T> V;
    constexpr int VEC = V::N;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int cv = (int)(i % CV), ch = cv * VEC;
    const int64_t r = i / CV, C = (int64_t)CV * VEC;
    const int img = (int)(r / g.max_len), j = (int)(r - (int64_t)img * g.max_len);
    const Window w = window_of(g, img);
    const bool in = j < w.len;
    if (cv == 0) __builtin_nontemporal_store((int64_t)(in ? 1 : 0), mask + r);
    const T *s = in ? src + ((int64_t)w.row * g.L + (w.col - j)) * C + ch : (pad_row ? pad_row + ch : nullptr);
    T *dst = out + r * C + ch;
    if (!pos) {
        store16_stream(dst, s ? *reinterpret_cast<const uint4 *>(s) : make_uint4(0, 0, 0, 0));
        return;
    }
    float v[VEC];
    zero<VEC>(v);
    if (s) load_vec<T, VEC>(s, v);
    add_row<T, VEC>(v, pos + (int64_t)j * C + ch);
    store_vec<T, VEC, true>(dst, v);
}

// lane <-> (token (b, t), channel vector)
template <typename T>
__global__ void __launch_bounds__(kThreads)
seq_context_bwd(const T *__restrict__ grad_out, T *__restrict__ grad_src, const Ctx g, const int CV, const int64_t total)
{
    typedef Vec16<T> V;
    constexpr int VEC = V::N;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % CV) * VEC;
    const int64_t r = i / CV, C = (int64_t)CV * VEC;
    const int b = (int)(r / g.L), t = (int)(r - (int64_t)b * g.L);
    float acc[VEC];
    zero<VEC>(acc);
    const int hi = min(g.row_first[b + 1], g.n_images);
    for (int k = max(g.row_first[b], 0); k < hi; ++k) {
        const Window w = window_of(g, k);
        const int j = w.col - t;
        if (w.row == b && j >= 0 && j < w.len) add_row<T, VEC>(acc, grad_out + ((int64_t)k * g.max_len + j) * C + ch);
    }
    store_vec<T, VEC, true>(grad_src + r * C + ch, acc);
}

// grad_pad, stage 1: lane <-> (image, channel vector), the image's padded rows in ascending j -> scratch [n_images, C]
template <typename T>
__global__ void __launch_bounds__(kThreads)
seq_context_bwd_pad(const T *__restrict__ grad_out, float *__restrict__ scratch, const Ctx g, const int CV, const int64_t total)
{
    typedef Vec16<T> V;
    constexpr int VEC = V::N;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % CV) * VEC;
    const int img = (int)(i / CV);
    const int64_t C = (int64_t)CV * VEC;
    const Window w = window_of(g, img);
    const T *row = grad_out + (int64_t)img * g.max_len * C + ch;
    float acc[VEC];
    zero<VEC>(acc);
    int j = w.len;
    for (; j + kPadUnroll <= g.max_len; j += kPadUnroll) {
        uint4 q[kPadUnroll];
#pragma unroll
        for (int u = 0; u < kPadUnroll; ++u) q[u] = *reinterpret_cast<const uint4 *>(row + (int64_t)(j + u) * C);
#pragma unroll
        for (int u = 0; u < kPadUnroll; ++u) {
            float v[VEC];
            V::unpack(q[u], v);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] += v[e];
        }
    }
    for (; j < g.max_len; ++j) add_row<T, VEC>(acc, row + (int64_t)j * C);
    store_vec<float, VEC, false>(scratch + (int64_t)img * C + ch, acc);
}

// stage 2: lane <-> channel vector, the images in ascending i, one rounding
template <typename T>
__global__ void __launch_bounds__(kThreads)
seq_context_bwd_pad_sum(const float *__restrict__ scratch, T *__restrict__ grad_pad, const int n_images, const int CV)
{
    typedef Vec16<T> V;
    constexpr int VEC = V::N;
    const int cv = blockIdx.x * kThreads + threadIdx.x;
    if (cv >= CV) return;
    const int64_t C = (int64_t)CV * VEC;
    float acc[VEC];
    zero<VEC>(acc);
    for (int k = 0; k < n_images; ++k) add_row<float, VEC>(acc, scratch + k * C + cv * VEC);
    store_vec<T, VEC, false>(grad_pad + cv * VEC, acc);
}

bool supported(int es, int64_t C) { return es && C > 0 && (C * es) % 16 == 0; }

unsigned blocks_of(int64_t lanes) { return (unsigned)((lanes + kThreads - 1) / kThreads); }
bool grid_fits(int64_t lanes) { return (lanes + kThreads - 1) / kThreads <= 0x7fffffffLL; }

// dtype, sizes and width of the two embed entries
int check_embed(int dtype, int text_dtype, int64_t rows, int64_t C, int64_t n_vis)
{
    const int es = elem_size(dtype);
    if (!es || !elem_size(text_dtype)) return MMFS_E_DTYPE;
    if (rows < 0 || C < 0 || n_vis < 0) return MMFS_E_DIMS;
    if (!supported(es, C) || (text_dtype != dtype && text_dtype != MMFS_F32)) return MMFS_E_UNSUPPORTED;
    if (rows > kMaxTokens || n_vis > kMaxTokens || C > (1 << 24)) return MMFS_E_DIMS;
    return MMFS_OK;
}

int check_context(int dtype, int64_t B, int64_t L, int64_t C, int64_t n_images, int64_t max_len, int64_t seq_len)
{
    const int es = elem_size(dtype);
    if (!es) return MMFS_E_DTYPE;
    if (B < 0 || L < 0 || C < 0 || n_images < 0 || seq_len < 0 || max_len < 1 || max_len > seq_len) return MMFS_E_DIMS;
    if (!supported(es, C)) return MMFS_E_UNSUPPORTED;
    if (B * L > kMaxTokens || B > kMaxTokens || L > kMaxTokens || n_images > kMaxTokens || max_len > kMaxTokens || C > (1 << 24))
        return MMFS_E_DIMS;
    return MMFS_OK;
}

}  // namespace
}  // namespace mmfs

extern "C" {

int mmfs_sequence_supported(int dtype, int64_t C) { return mmfs::supported(mmfs::elem_size(dtype), C); }

int mmfs_sequence_index(const int64_t *text_ids, int64_t B, int64_t L, int64_t image_token_id, int64_t soi_token_id,
                        int64_t n_vis, int64_t n_images, int32_t *img_rank, int32_t *img_pos, int32_t *soi_row,
                        int32_t *soi_col, int32_t *row_first, int32_t *counts, void *stream)
{
    using namespace mmfs;
    if (B < 0 || L < 0 || n_vis < 0 || n_images < 0) return MMFS_E_DIMS;
    if (B > kMaxTokens || L > kMaxTokens || B * L > kMaxTokens || n_vis > kMaxTokens || n_images > kMaxTokens) return MMFS_E_DIMS;
    const int64_t N = B * L;
    if (const int rc = check_tensors({{row_first, 4}, {counts, 4}, {text_ids, 8, N != 0}, {img_rank, 4, N != 0},
                                      {img_pos, 4, n_vis != 0}, {soi_row, 4, n_images != 0}, {soi_col, 4, n_images != 0}}))
        return rc;
    hipLaunchKernelGGL(seq_index, dim3(1), dim3(kScanThreads), 0, (hipStream_t)stream, text_ids, (int)N, (int)B, (int)L,
                       image_token_id, soi_token_id, (int)n_vis, (int)n_images, img_rank, img_pos, soi_row, soi_col, row_first,
                       counts);
    return (int)hipGetLastError();
}

int mmfs_sequence_embed_forward(int dtype, int text_dtype, const void *text, const void *vis, const void *soi_token,
                                const int64_t *text_ids, int64_t soi_token_id, const int32_t *img_rank, void *out,
                                int64_t rows, int64_t C, int64_t n_vis, void *stream)
{
    using namespace mmfs;
    const int rc = check_embed(dtype, text_dtype, rows, C, n_vis);
    if (rc || rows == 0) return rc;
    if (const int rt = check_tensors({{text, 16}, {vis, 16, n_vis != 0}, {soi_token, 16}, {out, 16}, {text_ids, 8}, {img_rank, 4}}))
        return rt;
    const int es = elem_size(dtype), CV = (int)(C * es / 16);
    const int64_t total = rows * CV;
    if (!grid_fits(total)) return MMFS_E_DIMS;
    return by_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        if (text_dtype == dtype)
            hipLaunchKernelGGL((seq_embed_fwd<T, T>), dim3(blocks_of(total)), dim3(kThreads), 0, (hipStream_t)stream,
                               (const T *)text, (const T *)vis, (const T *)soi_token, text_ids, soi_token_id, img_rank, (T *)out,
                               CV, total);
        else
            hipLaunchKernelGGL((seq_embed_fwd<T, float>), dim3(blocks_of(total)), dim3(kThreads), 0, (hipStream_t)stream,
                               (const float *)text, (const T *)vis, (const T *)soi_token, text_ids, soi_token_id, img_rank,
                               (T *)out, CV, total);
        return (int)hipGetLastError();
    });
}

int mmfs_sequence_embed_backward(int dtype, int text_dtype, const void *grad, const int32_t *img_rank, const int32_t *img_pos,
                                 const int32_t *soi_row, const int32_t *soi_col, const int32_t *counts, void *grad_text,
                                 void *grad_vis, void *grad_soi, int64_t rows, int64_t L, int64_t C, int64_t n_vis,
                                 int64_t n_images, void *stream)
{
    using namespace mmfs;
    const int rc = check_embed(dtype, text_dtype, rows, C, n_vis);
    if (rc) return rc;
    if (L < 0 || n_images < 0 || n_images > kMaxTokens || (L ? rows % L != 0 : rows != 0)) return MMFS_E_DIMS;
    if (!n_vis) grad_vis = nullptr;
    if (!rows) grad_text = nullptr;
    if (!grad_text && !grad_vis && !grad_soi) return MMFS_OK;
    const bool soi = grad_soi != nullptr;
    if (const int rt = check_tensors({{grad, 16, rows != 0}, {img_rank, 4, rows != 0}, {img_pos, 4, grad_vis != nullptr}, {counts, 4, soi},
                                      {soi_row, 4, soi && n_images}, {soi_col, 4, soi && n_images}, maybe(grad_text, 16),
                                      maybe(grad_vis, 16), maybe(grad_soi, 16)}))
        return rt;
    const int es = elem_size(dtype), CV = (int)(C * es / 16);
    const int64_t total = (rows + n_vis + 1) * CV;
    if (!grid_fits(total)) return MMFS_E_DIMS;
    return by_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        if (text_dtype == dtype)
            hipLaunchKernelGGL((seq_embed_bwd<T, T>), dim3(blocks_of(total)), dim3(kThreads), 0, (hipStream_t)stream,
                               (const T *)grad, img_rank, img_pos, soi_row, soi_col, counts, (T *)grad_text, (T *)grad_vis,
                               (T *)grad_soi, CV, rows, n_vis, (int)n_images, (int)L, total);
        else
            hipLaunchKernelGGL((seq_embed_bwd<T, float>), dim3(blocks_of(total)), dim3(kThreads), 0, (hipStream_t)stream,
                               (const T *)grad, img_rank, img_pos, soi_row, soi_col, counts, (float *)grad_text, (T *)grad_vis,
                               (T *)grad_soi, CV, rows, n_vis, (int)n_images, (int)L, total);
        return (int)hipGetLastError();
    });
}

int mmfs_sequence_context_forward(int dtype, const void *src, const void *pad_row, const void *pos, const int32_t *soi_row,
                                  const int32_t *soi_col, const int64_t *start_idx, const int64_t *bos_idx, void *out,
                                  int64_t *mask, int64_t B, int64_t L, int64_t C, int64_t n_images, int64_t max_len,
                                  int64_t seq_len, void *stream)
{
    using namespace mmfs;
    const int rc = check_context(dtype, B, L, C, n_images, max_len, seq_len);
    if (rc || n_images == 0) return rc;
    // (the rows' first columns: soi_col, or start_idx in its place)
    if (const int rt = check_tensors({{soi_row, 4}, {soi_col, 4, !start_idx}, maybe(start_idx, 8), maybe(bos_idx, 8), {mask, 8},
                                      {out, 16}, {src, 16, B * L != 0}, maybe(pad_row, 16), maybe(pos, 16)}))
        return rt;
    const int es = elem_size(dtype), CV = (int)(C * es / 16);
    const int64_t total = n_images * max_len * CV;
    if (!grid_fits(total)) return MMFS_E_DIMS;
    const Ctx g = {soi_row, soi_col, nullptr, start_idx, bos_idx, (int)L, (int)n_images, (int)max_len};
    return by_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL((seq_context_fwd<T>), dim3(blocks_of(total)), dim3(kThreads), 0, (hipStream_t)stream, (const T *)src,
                           (const T *)pad_row, (const T *)pos, (T *)out, mask, g, CV, total);
        return (int)hipGetLastError();
    });
}

int64_t mmfs_sequence_context_backward_workspace_bytes(int dtype, int64_t C, int64_t n_images)
{
    using namespace mmfs;
    const int es = elem_size(dtype);
    if (!es) return MMFS_E_DTYPE;
    if (C < 0 || n_images < 0 || n_images > kMaxTokens || C > (1 << 24)) return MMFS_E_DIMS;
    if (!supported(es, C)) return MMFS_E_UNSUPPORTED;
    return n_images * C * (int64_t)sizeof(float);
}

int mmfs_sequence_context_backward(int dtype, const void *grad_out, const int32_t *soi_row, const int32_t *soi_col,
                                   const int32_t *row_first, const int64_t *start_idx, const int64_t *bos_idx, void *grad_src,
                                   void *grad_pad, void *workspace, int64_t B, int64_t L, int64_t C, int64_t n_images,
                                   int64_t max_len, int64_t seq_len, void *stream)
{
    using namespace mmfs;
    const int rc = check_context(dtype, B, L, C, n_images, max_len, seq_len);
    if (rc) return rc;
    if (B * L == 0) grad_src = nullptr;
    if (!grad_src && !grad_pad) return MMFS_OK;
    const bool im = n_images != 0;
    if (const int rt = check_tensors({{grad_out, 16, im}, {soi_row, 4, im}, {soi_col, 4, im && !start_idx}, maybe(start_idx, 8),
                                      maybe(bos_idx, 8), {row_first, 4, grad_src != nullptr}, {workspace, 16, grad_pad && im},
                                      maybe(grad_src, 16), maybe(grad_pad, 16)}))
        return rt;
    const int es = elem_size(dtype), CV = (int)(C * es / 16);
    const int64_t src_total = B * L * CV, pad_total = n_images * CV;
    if (!grid_fits(src_total) || !grid_fits(pad_total)) return MMFS_E_DIMS;
    const Ctx g = {soi_row, soi_col, row_first, start_idx, bos_idx, (int)L, (int)n_images, (int)max_len};
    return by_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        if (grad_src) {
            hipLaunchKernelGGL((seq_context_bwd<T>), dim3(blocks_of(src_total)), dim3(kThreads), 0, (hipStream_t)stream,
                               (const T *)grad_out, (T *)grad_src, g, CV, src_total);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return (int)e;
        }
        if (!grad_pad) return (int)hipSuccess;
        if (pad_total) {
            hipLaunchKernelGGL((seq_context_bwd_pad<T>), dim3(blocks_of(pad_total)), dim3(kThreads), 0, (hipStream_t)stream,
                               (const T *)grad_out, (float *)workspace, g, CV, pad_total);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return (int)e;
        }
        hipLaunchKernelGGL((seq_context_bwd_pad_sum<T>), dim3(blocks_of(CV)), dim3(kThreads), 0, (hipStream_t)stream,
                           (const float *)workspace, (T *)grad_pad, (int)n_images, CV);
        return (int)hipGetLastError();
    });
}

}  // extern "C"
