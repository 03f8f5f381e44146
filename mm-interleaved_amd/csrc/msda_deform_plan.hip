// msda_deform_plan.hip -- the sampling plan of the image encoder's MSDeformAttn (ViT-Adapter) in one kernel each way,
// and the plan feeding the row-gather sampler in one kernel for calls without gradients.
//
// Between its two Linear heads and the op the module
// (mm_interleaved/models/encoders/vit_adapter/ops/modules/ms_deform_attn.py:108-127) runs a softmax over the L*P
// logits of a (sample, query, head), a division of the offsets by the level extent (or a product with the box), the
// add of the reference point, a cast and two copies.  All of it is a function of one row of each head and one
// reference point:
//     off   [N, Lq, H, L, P, 2]    logit [N, Lq, H, L, P]        (storage type T; token rows ld_off / ld_att elements
//                                                                 apart: two column ranges of ONE GEMM result)
//     ref   [Nr, Lq, Lref, R] fp32   Nr in {1, N}, Lref in {1, L}, R in {2, 4}
//     R = 2:  loc = ref + off / (W_l, H_l)        R = 4:  loc = ref[:2] + off / P * ref[2:] * 0.5
//     attn = softmax over (l, p)
// evaluated in fp32 and rounded to T once, at the store.  mmfs_plan.hip's lane scheme: one lane owns one level row of
// P logits / P locations, the G = 2^k >= L lanes of an item reduce with wave shuffles (L = 1: none).  The backward
// is the same map (softmax backward a_i (g_i - sum_j a_j g_j); offsets' gradient times the forward's scale) and
// needs neither atomics nor clears: every element of both gradients has exactly one writer.  No gradient for ref.
//
// deform_sample_fwd is msda_fwd_vec (csrc/msda_fwd.hip) with its staging replaced, as mmfs_sample_fwd is for MMFS:
// the workgroup evaluates the plan of its 256 / LPI queries with the SAME device functions, lane groups and
// reduction order as deform_plan_fwd, rounds locations and weights to T, and turns them into tap records in LDS, which
// it walks with msda_fwd_vec's own functions (msda_gather.h).
#include "msda_gather.h"
#include "msda_host.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>

namespace mmfs {

namespace {

constexpr int kThreads = 256;
constexpr int kSampleRecs = 512;        // tap records staged per chunk (as msda_fwd_vec)
constexpr int kMaxLevels = 8;

struct DeformDims {
    int N, Lq, H, L, P, Nr, Lref, R;
    int G;                  // lane-group width: the power of two >= L
    int ld_off, ld_att;     // elements between two tokens' rows of off / logit (H*L*P*2, H*L*P when packed)
};

// reference point and offset scale of (sample nb, query q, level l):  loc = ref + off * scale
__device__ __forceinline__ void row_geometry(const float *__restrict__ ref, const DeformDims &d, int nb, int q, int l,
                                             int Hl, int Wl, float &rx, float &ry, float &sx, float &sy)
{
    const float *r = ref + (((int64_t)(d.Nr == 1 ? 0 : nb) * d.Lq + q) * d.Lref + (d.Lref == 1 ? 0 : l)) * d.R;
    rx = r[0]; ry = r[1];
    if (d.R == 2) {
        sx = 1.f / (float)Wl; sy = 1.f / (float)Hl;
    } else {
        const float c = 0.5f / (float)d.P;                  // (P is a power of two: exact)
        sx = r[2] * c; sy = r[3] * c;
    }
}

// softmax statistics of an item: every lane of the group brings its row's logits (-inf for a lane without a row)
template <int P>
__device__ __forceinline__ void softmax_stats(const float (&lg)[P], int G, float &m, float &inv)
{
    m = -INFINITY;
#pragma unroll
    for (int p = 0; p < P; ++p) m = fmaxf(m, lg[p]);
    m = group_max(m, G);
    float z = 0.f;
#pragma unroll
    for (int p = 0; p < P; ++p) z += __expf(lg[p] - m);
    z = group_add(z, G);
    inv = 1.f / z;
}

// A row's weights and locations as the numbers of the storage type (held in floats).  fp32 results behind an opaque
// register, THEN rounded: the compiler would otherwise fold ``(half)fma(a, b, c)`` into one mixed-precision
// instruction that rounds the exact sum once, and the two kernels that evaluate the plan would part on ties
// (csrc/mmfs_plan.hip has the measured case).
template <typename T, int P>
__device__ __forceinline__ void row_values(const float (&lg)[P], float m, float inv, const float (&of)[2 * P],
                                           float rx, float ry, float sx, float sy, float (&w)[P], float (&xy)[2 * P])
{
#pragma unroll
    for (int p = 0; p < P; ++p) {
        float wgt = __expf(lg[p] - m);
        wgt *= inv;
        float lx = fmaf(of[2 * p], sx, rx), ly = fmaf(of[2 * p + 1], sy, ry);
        asm volatile("" : "+v"(lx), "+v"(ly), "+v"(wgt));
        w[p] = to_f32((T)wgt); xy[2 * p] = to_f32((T)lx); xy[2 * p + 1] = to_f32((T)ly);
    }
}

// ---------------------------------------------------------------- plan forward: lane <-> (item, level)
template <typename T, int P>
__global__ void __launch_bounds__(kThreads)
deform_plan_fwd(const T *__restrict__ off, const T *__restrict__ logit, const float *__restrict__ ref,
                const int64_t *__restrict__ shapes, T *__restrict__ loc, T *__restrict__ attn, const DeformDims d)
{
    const int G = d.G;
    const int gl = threadIdx.x % G;
    const int64_t item = (int64_t)blockIdx.x * (kThreads / G) + threadIdx.x / G;      // (nb*Lq + q)*H + h
    const bool act = item < (int64_t)d.N * d.Lq * d.H && gl < d.L;
    const int64_t it = act ? item : 0;
    const int h = (int)(it % d.H);
    const int64_t nq = it / d.H;
    const int q = (int)(nq % d.Lq), nb = (int)(nq / d.Lq);
    float lg[P];
    if (act) {
        load_row<T, P>(logit + nq * d.ld_att + (h * d.L + gl) * P, lg);
    } else {
#pragma unroll
        for (int p = 0; p < P; ++p) lg[p] = -INFINITY;
    }
    float m, inv;
    softmax_stats<P>(lg, G, m, inv);
    if (!act) return;
    float of[2 * P], w[P], xy[2 * P], rx, ry, sx, sy;
    load_row<T, 2 * P>(off + nq * d.ld_off + (h * d.L + gl) * 2 * P, of);
    row_geometry(ref, d, nb, q, gl, (int)shapes[2 * gl], (int)shapes[2 * gl + 1], rx, ry, sx, sy);
    row_values<T, P>(lg, m, inv, of, rx, ry, sx, sy, w, xy);
    const int64_t row = item * d.L + gl;
    store_row<T, P>(attn + row * P, w);
    store_row<T, 2 * P>(loc + row * 2 * P, xy);
}

// ---------------------------------------------------------------- plan backward: the same map, one writer per element
template <typename T, int P>
__global__ void __launch_bounds__(kThreads)
deform_plan_bwd(const T *__restrict__ grad_loc, const T *__restrict__ grad_attn, const T *__restrict__ attn,
                const float *__restrict__ ref, const int64_t *__restrict__ shapes,
                T *__restrict__ grad_off, T *__restrict__ grad_logit, const DeformDims d)
{
    const int G = d.G;
    const int gl = threadIdx.x % G;
    const int64_t item = (int64_t)blockIdx.x * (kThreads / G) + threadIdx.x / G;
    const bool act = item < (int64_t)d.N * d.Lq * d.H && gl < d.L;
    const int64_t it = act ? item : 0;
    const int h = (int)(it % d.H);
    const int64_t nq = it / d.H;
    const int q = (int)(nq % d.Lq), nb = (int)(nq / d.Lq);
    const int64_t row = it * d.L + gl;
    float w[P], g[P];
    float part = 0.f;
    if (act) {
        load_row<T, P>(attn + row * P, w);
        load_row<T, P>(grad_attn + row * P, g);
#pragma unroll
        for (int p = 0; p < P; ++p) part += w[p] * g[p];
    }
    const float dot = group_add(part, G);
    if (!act) return;
    float dl[P], gxy[2 * P], rx, ry, sx, sy;
    load_row<T, 2 * P>(grad_loc + row * 2 * P, gxy);
    row_geometry(ref, d, nb, q, gl, (int)shapes[2 * gl], (int)shapes[2 * gl + 1], rx, ry, sx, sy);
#pragma unroll
    for (int p = 0; p < P; ++p) {
        dl[p] = w[p] * (g[p] - dot);
        gxy[2 * p] *= sx;
        gxy[2 * p + 1] *= sy;
    }
    store_row<T, P>(grad_logit + nq * d.ld_att + (h * d.L + gl) * P, dl);
    store_row<T, 2 * P>(grad_off + nq * d.ld_off + (h * d.L + gl) * 2 * P, gxy);
}

// ---------------------------------------------------------------- plan -> sampler, one kernel (no gradients)
template <typename T, int LPI, int P>
__global__ void __launch_bounds__(kThreads)
deform_sample_fwd(const T *__restrict__ value, const int64_t *__restrict__ shapes, const int64_t *__restrict__ start,
                  const T *__restrict__ off, const T *__restrict__ logit, const float *__restrict__ ref,
                  T *__restrict__ out, const Dims d, const DeformDims pd)
{
    typedef Vec16<T> V;
    constexpr int VEC = V::N;
    constexpr int QPB = kThreads / LPI;
    constexpr int KC = (kSampleRecs / QPB) > P ? (kSampleRecs / QPB) : P;      // samples per query per chunk: whole rows of P
    static_assert(KC % P == 0 && KC <= 64, "chunks hold whole rows of P points; one bit per sample in the live mask");
    constexpr int STRIDE = 2 * KC + 1;                      // uint4 units; +1 breaks the bank alignment
    constexpr int QPW = 64 / LPI;                           // queries per wave
    __shared__ uint4 lds[QPB * STRIDE];
    __shared__ int lvl[kMaxLevels * 3];                     // Hl, Wl, start
    __shared__ float2 stat[QPB];                            // softmax max and 1 / sum per query of the tile
    __shared__ unsigned long long live[kThreads / 64];      // samples of the chunk that weigh something for a query of the wave

    const BlockCoord bc = block_coord(d, QPB);
    const int tid = threadIdx.x;
    const int qi = tid / LPI, lig = tid % LPI;
    const int q = bc.q0 + qi;
    const bool q_ok = q < d.Nq;
    const int G = pd.G;
    const int64_t HD = (int64_t)d.H * d.D;
    const T *slab = value + ((int64_t)bc.b * d.S) * HD + (int64_t)bc.h * d.D;
    const uint32_t row_bytes = (uint32_t)(HD * sizeof(T));
    const uint32_t lane_off = (uint32_t)(lig * 16);
    const __amdgpu_buffer_rsrc_t rsrc = make_slab_rsrc(slab, ((int64_t)d.S * HD - (int64_t)bc.h * d.D) * (int64_t)sizeof(T));
    if (tid < pd.L) { lvl[3 * tid] = (int)shapes[2 * tid]; lvl[3 * tid + 1] = (int)shapes[2 * tid + 1]; lvl[3 * tid + 2] = (int)start[tid]; }
    if (tid < kThreads / 64) live[tid] = 0ull;

    // ---- softmax statistics of the tile's queries: lane groups of G per query, as deform_plan_fwd
    for (int base = 0; base < QPB * G; base += kThreads) {
        if (base + (tid & ~63) >= QPB * G) continue;        // (whole waves only: the groups shuffle)
        const int s = base + tid, rq = s / G, gl = s % G;
        const int sq = bc.q0 + rq;
        const bool act = rq < QPB && sq < d.Nq && gl < pd.L;
        float lg[P];
        if (act) {
            load_row<T, P>(logit + ((int64_t)bc.b * pd.Lq + sq) * pd.ld_att + (bc.h * pd.L + gl) * P, lg);
        } else {
#pragma unroll
            for (int p = 0; p < P; ++p) lg[p] = -INFINITY;
        }
        float m, inv;
        softmax_stats<P>(lg, G, m, inv);
        if (act && gl == 0) stat[rq] = make_float2(m, inv);
    }
    __syncthreads();

    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.f;

    for (int k0 = 0; k0 < d.K; k0 += KC) {
        const int kc = min(KC, d.K - k0);                   // a multiple of P
        const int rows = kc / P;
        if (k0 > 0) __syncthreads();
        // ---- stage: one lane per (query, level row): the row's P weights and locations, rounded to the storage type
        // like the tensors of the two-call path, then location -> tap record as msda_fwd_vec does from its tensors
        for (int s = tid; s < QPB * rows; s += kThreads) {
            const int rq = s / rows, rr = s - rq * rows, gl = k0 / P + rr;
            const int sq = bc.q0 + rq;
            uint4 *dst = &lds[rq * STRIDE + 2 * rr * P];
            if (sq >= d.Nq) {
                uint4 rows, ww;
                tap_record_none(rows, ww);
#pragma unroll
                for (int p = 0; p < P; ++p) { dst[2 * p] = rows; dst[2 * p + 1] = ww; }
                continue;
            }
            const int64_t tk = (int64_t)bc.b * pd.Lq + sq;
            float lg[P], of[2 * P], w[P], xy[2 * P], rx, ry, sx, sy;
            load_row<T, P>(logit + tk * pd.ld_att + (bc.h * pd.L + gl) * P, lg);
            load_row<T, 2 * P>(off + tk * pd.ld_off + (bc.h * pd.L + gl) * 2 * P, of);
            const int Hl = lvl[3 * gl], Wl = lvl[3 * gl + 1], lstart = lvl[3 * gl + 2];
            row_geometry(ref, pd, bc.b, sq, gl, Hl, Wl, rx, ry, sx, sy);
            const float2 st2 = stat[rq];
            row_values<T, P>(lg, st2.x, st2.y, of, rx, ry, sx, sy, w, xy);
#pragma unroll
            for (int p = 0; p < P; ++p) {
                uint4 rows, ww;
                tap_record(xy[2 * p], xy[2 * p + 1], w[p], Hl, Wl, lstart, row_bytes, rows, ww);
                dst[2 * p] = rows;
                dst[2 * p + 1] = ww;
                mark_live<QPW>(live, rq, rr * P + p, ww);
            }
        }
        __syncthreads();
        gather_live<V>(take_live(live, tid), &lds[qi * STRIDE], rsrc, lane_off, acc);
    }
    if (q_ok) {
        T *o = out + (((int64_t)bc.b * d.Nq + q) * d.H + bc.h) * d.D + lig * VEC;
        store_vec<T, VEC, true>(o, acc);
    }
}

// dtype / dimension checks shared by the three entries (MMFS_OK: ``d`` is filled, leading dimensions packed)
int check_dims(int dtype, int64_t N, int64_t Lq, int64_t H, int64_t L, int64_t P, int64_t Nr, int64_t Lref, int64_t R,
               DeformDims *d)
{
    const int64_t lim = 0x7fffffffLL;
    if (!elem_size(dtype)) return MMFS_E_DTYPE;
    if (N < 0 || Lq < 0 || H <= 0 || L <= 0 || P <= 0) return MMFS_E_DIMS;
    if (N > lim || Lq > lim || H > lim || N * Lq > lim || N * Lq * H > lim) return MMFS_E_DIMS;
    if ((Nr != 1 && Nr != N) || (Lref != 1 && Lref != L) || (R != 2 && R != 4)) return MMFS_E_DIMS;
    if ((P != 2 && P != 4 && P != 8) || L > kMaxLevels) return MMFS_E_UNSUPPORTED;
    if (H * L * P * 2 > lim) return MMFS_E_DIMS;
    d->N = (int)N; d->Lq = (int)Lq; d->H = (int)H; d->L = (int)L; d->P = (int)P;
    d->Nr = (int)Nr; d->Lref = (int)Lref; d->R = (int)R;
    d->G = 1;
    while (d->G < d->L) d->G *= 2;
    d->ld_off = (int)(H * L * P * 2); d->ld_att = (int)(H * L * P);
    return MMFS_OK;
}

template <typename F> int by_type_and_points(int dtype, int64_t P, F &&f)
{
    return by_type(dtype, [&](auto tag_t) { return by_int<2, 4, 8>(P, [&](auto tag_p) { return f(tag_t, tag_p); }); });
}

// lanes per query of the fused sampler for head rows of D elements, 0 when it does not serve them
int sampler_lpi(int es, int64_t D)
{
    const int vec = 16 / es;
    if (D <= 0 || D % vec) return 0;
    const int64_t lpi = D / vec;
    return (lpi == 2 || lpi == 4 || lpi == 8 || lpi == 16 || lpi == 32) ? (int)lpi : 0;
}

}  // namespace
}  // namespace mmfs

extern "C" {

int mmfs_deform_plan_supported(int dtype, int64_t L, int64_t P, int64_t R, int64_t D)
{
    using namespace mmfs;
    const int es = elem_size(dtype);
    if (!es || L <= 0 || L > kMaxLevels || (P != 2 && P != 4 && P != 8) || (R != 2 && R != 4)) return 0;
    return 1 | (sampler_lpi(es, D) ? 2 : 0);
}

int mmfs_deform_plan_forward(int dtype, const void *off, const void *logit, int64_t ld_off, int64_t ld_att,
                             const float *ref, const int64_t *shapes, void *loc, void *attn,
                             int64_t N, int64_t Lq, int64_t H, int64_t L, int64_t P, int64_t Nr, int64_t Lref, int64_t R,
                             void *stream)
{
    using namespace mmfs;
    DeformDims d;
    const int rc = check_dims(dtype, N, Lq, H, L, P, Nr, Lref, R, &d);
    if (rc) return rc;
    const int64_t items = N * Lq * H;
    if (items == 0) return MMFS_OK;
    // (two phases: the outputs' alignment is looked at after the rows of the inputs)
    int rr = check_tensors({{off, 1}, {logit, 1}, {ref, 1}, {shapes, 1}, {loc, 1}, {attn, 1}});
    if (rr) return rr;
    const int es = elem_size(dtype);
    if ((rr = heads_rows(ld_off, H * L * P * 2, off, 2 * P, es)) || (rr = heads_rows(ld_att, H * L * P, logit, P, es)) ||
        (rr = check_tensors({{loc, 16}, {attn, 16}})))
        return rr;
    d.ld_off = (int)ld_off; d.ld_att = (int)ld_att;
    const int ipb = kThreads / d.G;
    const unsigned blocks = (unsigned)((items + ipb - 1) / ipb);
    return by_type_and_points(dtype, P, [&](auto tag_t, auto tag_p) {
        typedef decltype(tag_t) T;
        constexpr int PP = decltype(tag_p)::value;
        hipLaunchKernelGGL((deform_plan_fwd<T, PP>), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream,
                           (const T *)off, (const T *)logit, ref, shapes, (T *)loc, (T *)attn, d);
        return (int)hipGetLastError();
    });
}

int mmfs_deform_plan_backward(int dtype, const void *grad_loc, const void *grad_attn, const void *attn,
                              const float *ref, const int64_t *shapes, void *grad_off, void *grad_logit,
                              int64_t ld_off, int64_t ld_att,
                              int64_t N, int64_t Lq, int64_t H, int64_t L, int64_t P, int64_t Nr, int64_t Lref, int64_t R,
                              void *stream)
{
    using namespace mmfs;
    DeformDims d;
    const int rc = check_dims(dtype, N, Lq, H, L, P, Nr, Lref, R, &d);
    if (rc) return rc;
    const int64_t items = N * Lq * H;
    if (items == 0) return MMFS_OK;
    int rr = check_tensors({{grad_loc, 1}, {grad_attn, 1}, {attn, 1}, {ref, 1}, {shapes, 1}, {grad_off, 1}, {grad_logit, 1}});
    if (rr) return rr;
    const int es = elem_size(dtype);
    if ((rr = heads_rows(ld_off, H * L * P * 2, grad_off, 2 * P, es)) || (rr = heads_rows(ld_att, H * L * P, grad_logit, P, es)) ||
        (rr = check_tensors({{grad_loc, 16}, {grad_attn, 16}, {attn, 16}})))
        return rr;
    d.ld_off = (int)ld_off; d.ld_att = (int)ld_att;
    const int ipb = kThreads / d.G;
    const unsigned blocks = (unsigned)((items + ipb - 1) / ipb);
    return by_type_and_points(dtype, P, [&](auto tag_t, auto tag_p) {
        typedef decltype(tag_t) T;
        constexpr int PP = decltype(tag_p)::value;
        hipLaunchKernelGGL((deform_plan_bwd<T, PP>), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream,
                           (const T *)grad_loc, (const T *)grad_attn, (const T *)attn, ref, shapes,
                           (T *)grad_off, (T *)grad_logit, d);
        return (int)hipGetLastError();
    });
}

int mmfs_deform_sample_forward(int dtype, const void *value, const int64_t *shapes, const int64_t *start,
                               const void *off, const void *logit, int64_t ld_off, int64_t ld_att,
                               const float *ref, void *out,
                               int64_t N, int64_t S, int64_t Lq, int64_t H, int64_t D, int64_t L, int64_t P,
                               int64_t Nr, int64_t Lref, int64_t R, void *stream)
{
    using namespace mmfs;
    DeformDims pd;
    const int rc = check_dims(dtype, N, Lq, H, L, P, Nr, Lref, R, &pd);
    if (rc) return rc;
    if (S < 0 || D <= 0 || S > 0x7ffffffdLL || H * D > 0x7fffffffLL) return MMFS_E_DIMS;
    if (N * Lq * H == 0) return MMFS_OK;
    const int es = elem_size(dtype);
    const int lpi = sampler_lpi(es, D);
    if (!lpi || S == 0 || S * H * D * (int64_t)es > kMaxSlabBytes) return MMFS_E_UNSUPPORTED;
    int rr = check_tensors({{value, 16}, {out, 16}, {shapes, 1}, {start, 1}, {off, 1}, {logit, 1}, {ref, 1}});
    if (rr) return rr;
    if ((rr = heads_rows(ld_off, H * L * P * 2, off, 2 * P, es)) || (rr = heads_rows(ld_att, H * L * P, logit, P, es)))
        return rr;
    pd.ld_off = (int)ld_off; pd.ld_att = (int)ld_att;
    Dims d = {};
    d.B = (int)N; d.S = (int)S; d.H = (int)H; d.D = (int)D; d.L = (int)L; d.Nq = (int)Lq; d.P = (int)P;
    d.K = d.L * d.P;
    d.Bv = d.B; d.vdiv = 1;
    return by_type_and_points(dtype, P, [&](auto tag_t, auto tag_p) {
        typedef decltype(tag_t) T;
        constexpr int PP = decltype(tag_p)::value;
        auto go = [&](auto tag_lpi) {
            constexpr int LPI = decltype(tag_lpi)::value;
            constexpr int QPB = kThreads / LPI;
            Dims dd = d;
            dd.q_tiles = (d.Nq + QPB - 1) / QPB;
            const int64_t blocks = (int64_t)d.B * dd.q_tiles * d.H;
            if (blocks > 0x7fffffffLL) return (int)MMFS_E_DIMS;
            hipLaunchKernelGGL((deform_sample_fwd<T, LPI, PP>), dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream,
                               (const T *)value, shapes, start, (const T *)off, (const T *)logit, ref, (T *)out, dd, pd);
            return (int)hipGetLastError();
        };
        return by_int<2, 4, 8, 16, 32>(lpi, go);
    });
}

}  // extern "C"
