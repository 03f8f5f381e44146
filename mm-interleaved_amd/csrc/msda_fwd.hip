// msda_fwd.hip -- forward kernels of multi-scale deformable attention for gfx950.
//
// Replaces the reference forward
//   mm_interleaved/models/utils/ops/src/cuda/ms_deform_im2col_cuda.cuh:240-302
//   (one thread per output scalar, every thread re-deriving every tap)
// with a design built around the 64-wide wavefront and the LDS:
//
//   * a workgroup owns QPB consecutive queries of ONE (batch, head) pair; the head is
//     chosen from the block index so a head's value slice stays in one XCD's L2;
//   * the workgroup first turns the tile's sampling locations / attention weights
//     (read once, coalesced) into tap records in LDS: 4 pixel-row indices and 4
//     weights already multiplied by the attention weight;
//   * then LPI = D*sizeof(T)/16 lanes cooperate on one query: every lane owns one
//     16-byte channel vector, so each corner of a tap is a single fully coalesced
//     D*sizeof(T)-byte row read, and the record is an LDS broadcast read;
//   * accumulation is fp32 in registers (the reference's opmath), no cross-lane
//     traffic at all in the forward; the result is stored as one 16-byte vector.
//
// A scalar kernel (one thread per output element) covers head widths that are not
// 16-byte * power-of-two, and fp64.
#include "msda_gather.h"
#include "msda_launch.h"

namespace mmfs {

constexpr int kThreads = 256;
constexpr int kRecsPerBlock = 512;      // tap records staged per chunk (16 KiB)
#ifndef MMFS_FWD_UNROLL
#define MMFS_FWD_UNROLL 2      // measured on MI355X: 2 -> 183 us, 1 -> 198, 4 -> 235, 8 -> 231 (cfg2, bf16)
#endif
constexpr int kUnroll = MMFS_FWD_UNROLL;   // taps in flight per lane (4x row reads each)

// The flat-address kernels' tap record (tap_record's, msda_gather.h, with pixel-row indices for byte offsets): -1 for a
// corner that reads nothing.  Flat addresses have no descriptor to stop a row that a malformed level table puts past S.
__device__ __forceinline__ void flat_record(float lx, float ly, float a, int Hl, int Wl, int lstart, int S,
                                            uint4 &rows, uint4 &ww)
{
    const Tap<float> t = locate<float>(lx, ly, Hl, Wl, lstart);
    const float gy = 1.f - t.fy, gx = 1.f - t.fx;
    int row[4] = {-1, -1, -1, -1};
    if (a != 0.f) {
        row[0] = t.row[0]; row[1] = t.row[1]; row[2] = t.row[2]; row[3] = t.row[3];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) row[c] = row[c] < S ? row[c] : -1;
    rows = make_uint4(row[0], row[1], row[2], row[3]);
    ww = make_uint4(__float_as_uint(gy * gx * a), __float_as_uint(gy * t.fx * a),
                    __float_as_uint(t.fy * gx * a), __float_as_uint(t.fy * t.fx * a));
}
// BUF = true : row reads through a buffer descriptor (32-bit offsets, hardware zero for
//              corners outside the map)               -- slabs < 2 GiB, the normal case
// BUF = false: 64-bit flat addresses, clamped read + select
//
// BT is the bank's type: T, or fp8e4m3_t for the inference-only fp8 bank (16 channels per lane, its fp32 scale per
// (bank row, channel) applied once at the store -- include/mmfs_msda.h "fp8 bank"); loc / attn / out stay T.
template <typename T, int LPI, bool BUF, typename BT>
__global__ void __launch_bounds__(kThreads)
msda_fwd_vec(const BT *__restrict__ value, const int64_t *__restrict__ shapes,
             const int64_t *__restrict__ start, const T *__restrict__ loc,
             const T *__restrict__ attn, T *__restrict__ out, const Dims d, const float *__restrict__ vscale)
{
    typedef Vec16<BT> V;
    constexpr int VEC = V::N;
    constexpr int QPB = kThreads / LPI;           // queries per block
    constexpr int KC = (kRecsPerBlock / QPB) > kUnroll ? (kRecsPerBlock / QPB) : kUnroll;  // samples per query per chunk (pow2)
    constexpr int STRIDE = 2 * KC + 1;            // uint4 units; +1 breaks the bank alignment
    __shared__ uint4 lds[QPB * STRIDE];
    __shared__ LevelLds levels;
    constexpr bool kPipe = BUF && KC <= 64;                // live words + the pipelined walk (msda_gather.h)
    constexpr int QPW = 64 / LPI > 0 ? 64 / LPI : 1;       // queries per wave
    __shared__ unsigned long long live[kThreads / 64];

    const BlockCoord bc = block_coord(d, QPB);
    const int tid = threadIdx.x;
    if (kPipe && tid < kThreads / 64) live[tid] = 0ull;
    levels.load(shapes, start, d.L, tid, kThreads);
    const bool pair_ok = ((uintptr_t)loc & (2 * sizeof(T) - 1)) == 0;
    __syncthreads();
    const int qi = tid / LPI, lig = tid % LPI;
    const int q = bc.q0 + qi;
    const bool q_ok = q < d.Nq;
    const int Ksel = d.K;

    const int64_t HD = (int64_t)d.H * d.D;
    const BT *slab = value + ((int64_t)value_row(d, bc.b) * d.S) * HD + (int64_t)bc.h * d.D;   // this (b, h)
    const BT *vbase = slab + lig * VEC;
    const uint32_t row_bytes = (uint32_t)(HD * sizeof(BT));
    const uint32_t lane_off = (uint32_t)(lig * 16);
    __amdgpu_buffer_rsrc_t rsrc;
    if (BUF) rsrc = make_slab_rsrc(slab, ((int64_t)d.S * HD - (int64_t)bc.h * d.D) * (int64_t)sizeof(BT));

    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.f;

    for (int k0 = 0; k0 < Ksel; k0 += KC) {
        const int kc = min(KC, Ksel - k0);
        const int kc_pad = (kc + kUnroll - 1) / kUnroll * kUnroll;
        if (k0 > 0) __syncthreads();              // previous chunk fully consumed
        // ---- stage: locations + weights -> tap records (coalesced over samples)
        for (int r = tid; r < QPB * kc_pad; r += kThreads) {
            const int rq = r / kc_pad, kk = r - rq * kc_pad;
            float lx = -8.f, ly = -8.f, a = 0.f;                  // padding: outside every map, weight 0
            int Hl = 1, Wl = 1, lstart = 0;
            const int sq = bc.q0 + rq;
            if (kk < kc && sq < d.Nq) {
                const int k = k0 + kk;
                const int l = k / d.P;
                const int64_t s = (((int64_t)bc.b * d.Nq + sq) * d.H + bc.h) * d.K + k;
                load_xy(loc, s, pair_ok, lx, ly);
                a = to_f32(attn[s]);
                levels.get(shapes, start, l, Hl, Wl, lstart);
            }
            uint4 rows, ww;
            if (BUF) tap_record(lx, ly, a, Hl, Wl, lstart, row_bytes, rows, ww);
            else flat_record(lx, ly, a, Hl, Wl, lstart, d.S, rows, ww);
            uint4 *dst = &lds[rq * STRIDE + 2 * kk];
            dst[0] = rows;
            dst[1] = ww;
            if (kPipe) mark_live<QPW>(live, rq, kk, ww);
        }
        __syncthreads();
        if (kPipe) {
            gather_live<V>(take_live(live, tid), &lds[qi * STRIDE], rsrc, lane_off, acc);
        } else if (q_ok) {
            const uint4 *recs = &lds[qi * STRIDE];
            if (BUF) {
                gather_all<V, kUnroll>(recs, kc_pad, rsrc, lane_off, acc);
            } else {
                // ---- 64-bit flat addresses: clamped read + select, kUnroll taps in flight per lane
                for (int kk = 0; kk < kc_pad; kk += kUnroll) {
                    uint4 raw[kUnroll][4];
                    float w[kUnroll][4];
                    bool ok[kUnroll][4];
                    uint4 rrs[kUnroll];
                    uint32_t any_w = 0u;
#pragma unroll
                    for (int u = 0; u < kUnroll; ++u) {
                        rrs[u] = recs[2 * (kk + u)];
                        const uint4 ww = recs[2 * (kk + u) + 1];
                        any_w |= (ww.x | ww.y | ww.z | ww.w) << 1;
                        w[u][0] = __uint_as_float(ww.x); w[u][1] = __uint_as_float(ww.y);
                        w[u][2] = __uint_as_float(ww.z); w[u][3] = __uint_as_float(ww.w);
                    }
                    if (__builtin_amdgcn_ballot_w64(any_w != 0u) == 0ull) continue;      // (as gather_all)
#pragma unroll
                    for (int u = 0; u < kUnroll; ++u) {
                        const uint4 rr = rrs[u];
                        const int rows[4] = {(int)rr.x, (int)rr.y, (int)rr.z, (int)rr.w};
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            ok[u][c] = rows[c] >= 0;
                            const int64_t off = (int64_t)max(rows[c], 0) * HD;
                            raw[u][c] = *reinterpret_cast<const uint4 *>(vbase + off);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            float v[VEC];
                            V::unpack(raw[u][c], v);
                            const float wc = w[u][c];
#pragma unroll
                            for (int i = 0; i < VEC; ++i) acc[i] = fmaf(wc, ok[u][c] ? v[i] : 0.f, acc[i]);
                        }
                    }
                }
            }
        }
    }
    if (q_ok) {
        T *o = out + (((int64_t)bc.b * d.Nq + q) * d.H + bc.h) * d.D + lig * VEC;
        apply_scale<BT, VEC>(acc, vscale, (int64_t)value_row(d, bc.b) * HD + (int64_t)bc.h * d.D + lig * VEC);
        store_vec<T, VEC, true>(o, acc);                 // (the output is not read again in the step: profiles/r03_experiments.md r03j)
    }
}

// Scalar fallback: any D, any storage type (incl. fp64).  One thread per output
// element, same arithmetic.  Not a tuned path: the real head widths (32, 64, 128)
// all take msda_fwd_vec.
template <typename T>
__global__ void __launch_bounds__(kThreads)
msda_fwd_scalar(const T *__restrict__ value, const int64_t *__restrict__ shapes,
                const int64_t *__restrict__ start, const T *__restrict__ loc,
                const T *__restrict__ attn, T *__restrict__ out, const Dims d, const int64_t total)
{
    typedef typename Acc<T>::type A;
    const int64_t HD = (int64_t)d.H * d.D;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * kThreads) {
        const int c = (int)(idx % d.D);
        const int64_t item = idx / d.D;                 // (b*Nq + q)*H + h
        const int h = (int)(item % d.H);
        const int64_t b = item / d.H / d.Nq;
        const T *vb = value + (int64_t)value_row(d, (int)b) * d.S * HD + (int64_t)h * d.D + c;
        A acc = 0;
        for (int k = 0; k < d.K; ++k) {
            const int l = k / d.P;
            const int64_t s = item * d.K + k;
            const Tap<A> t = locate<A>((A)loc[2 * s], (A)loc[2 * s + 1], (int)shapes[2 * l],
                                       (int)shapes[2 * l + 1], (int)start[l]);
            const A gy = 1 - t.fy, gx = 1 - t.fx;
            const A v1 = t.row[0] >= 0 ? (A)vb[(int64_t)t.row[0] * HD] : (A)0;
            const A v2 = t.row[1] >= 0 ? (A)vb[(int64_t)t.row[1] * HD] : (A)0;
            const A v3 = t.row[2] >= 0 ? (A)vb[(int64_t)t.row[2] * HD] : (A)0;
            const A v4 = t.row[3] >= 0 ? (A)vb[(int64_t)t.row[3] * HD] : (A)0;
            acc += (gy * gx * v1 + gy * t.fx * v2 + t.fy * gx * v3 + t.fy * t.fx * v4) * (A)attn[s];
        }
        out[idx] = (T)acc;
    }
}

// ---------------------------------------------------------------- launchers
template <typename T, int LPI, typename BT = T>
static hipError_t launch_vec(const void *value, const int64_t *shapes, const int64_t *start,
                             const void *loc, const void *attn, void *out, Dims d, hipStream_t st,
                             const float *vscale = nullptr)
{
    constexpr int QPB = kThreads / LPI;
    d.q_tiles = (d.Nq + QPB - 1) / QPB;
    const int64_t blocks = (int64_t)d.B * d.q_tiles * d.H;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    // one (batch) slab of value must be addressable with 31-bit byte offsets for the buffer path
    const bool buf = (int64_t)d.S * d.H * d.D * (int64_t)sizeof(BT) <= kMaxSlabBytes;
    if (buf)
        hipLaunchKernelGGL((msda_fwd_vec<T, LPI, true, BT>), dim3((unsigned)blocks), dim3(kThreads), 0, st,
                           (const BT *)value, shapes, start, (const T *)loc, (const T *)attn, (T *)out, d, vscale);
    else
        hipLaunchKernelGGL((msda_fwd_vec<T, LPI, false, BT>), dim3((unsigned)blocks), dim3(kThreads), 0, st,
                           (const BT *)value, shapes, start, (const T *)loc, (const T *)attn, (T *)out, d, vscale);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_scalar(const void *value, const int64_t *shapes, const int64_t *start,
                                const void *loc, const void *attn, void *out, Dims d, hipStream_t st)
{
    const int64_t total = (int64_t)d.B * d.Nq * d.H * d.D;
    const int64_t blocks = std::min<int64_t>((total + kThreads - 1) / kThreads, 256 * 32);
    hipLaunchKernelGGL((msda_fwd_scalar<T>), dim3((unsigned)blocks), dim3(kThreads), 0, st,
                       (const T *)value, shapes, start, (const T *)loc, (const T *)attn, (T *)out, d, total);
    return hipGetLastError();
}

template <typename T>
static hipError_t dispatch_fwd(const void *value, const int64_t *shapes, const int64_t *start,
                               const void *loc, const void *attn, void *out, const Dims &d, hipStream_t st)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    if (d.D % VEC == 0) {
        switch (d.D / VEC) {
#define MMFS_CASE(n) case n: return launch_vec<T, n>(value, shapes, start, loc, attn, out, d, st);
            MMFS_CASE(1) MMFS_CASE(2) MMFS_CASE(4) MMFS_CASE(8) MMFS_CASE(16) MMFS_CASE(32) MMFS_CASE(64)
#undef MMFS_CASE
            default: break;
        }
    }
    return launch_scalar<T>(value, shapes, start, loc, attn, out, d, st);
}

hipError_t forward(int dtype, const void *value, const int64_t *shapes, const int64_t *start,
                   const void *loc, const void *attn, void *out, const Dims &d, hipStream_t st, int algo)
{
    if (algo == 4 || (algo == 0 && fwd_wq_applies(dtype, d)))
        return forward_wq(dtype, value, shapes, start, loc, attn, out, d, st);
    if (algo == 3 || (algo == 0 && fwd_q8_applies(dtype, d)))
        return forward_q8(dtype, value, shapes, start, loc, attn, out, d, st);
    if (algo == 2 || (algo == 0 && fwd_mma_applies(dtype, d)))
        return forward_mma(dtype, value, shapes, start, loc, attn, out, d, st);
    switch (dtype) {
        case MMFS_F32: return dispatch_fwd<float>(value, shapes, start, loc, attn, out, d, st);
        case MMFS_F16: return dispatch_fwd<half_t>(value, shapes, start, loc, attn, out, d, st);
        case MMFS_BF16: return dispatch_fwd<bf16_t>(value, shapes, start, loc, attn, out, d, st);
        case MMFS_F64: return launch_scalar<double>(value, shapes, start, loc, attn, out, d, st);
        default: return hipErrorInvalidValue;
    }
}

bool fwd_fp8_supported(const Dims &d)
{
    const int lpi = d.D / 16;
    return d.D % 16 == 0 && lpi >= 1 && lpi <= 16 && (lpi & (lpi - 1)) == 0;
}

template <typename T>
static hipError_t dispatch_fwd_fp8(const void *q, const float *scale, const int64_t *shapes, const int64_t *start,
                                   const void *loc, const void *attn, void *out, const Dims &d, hipStream_t st)
{
    switch (d.D / 16) {
#define MMFS_CASE(n) case n: return launch_vec<T, n, fp8e4m3_t>(q, shapes, start, loc, attn, out, d, st, scale);
        MMFS_CASE(1) MMFS_CASE(2) MMFS_CASE(4) MMFS_CASE(8) MMFS_CASE(16)
#undef MMFS_CASE
        default: return hipErrorInvalidValue;
    }
}

// fp8 bank: the row gather only (the matrix-core forwards stay 16-bit)
hipError_t forward_fp8(int dtype, const void *q, const float *scale, const int64_t *shapes, const int64_t *start,
                       const void *loc, const void *attn, void *out, const Dims &d, hipStream_t st)
{
    if (!fwd_fp8_supported(d) || !elem_size(dtype)) return hipErrorInvalidValue;
    return by_type(dtype, [&](auto t) { return dispatch_fwd_fp8<decltype(t)>(q, scale, shapes, start, loc, attn, out, d, st); });
}

}  // namespace mmfs
