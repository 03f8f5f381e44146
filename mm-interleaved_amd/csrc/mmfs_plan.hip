// mmfs_plan.hip -- the MMFS "sampling plan" fused into one kernel each way.
//
// Between its Linear layers and the deformable-attention op the reference runs ~20 elementwise /
// reduction kernels over [N, Lq, H, n*L, P(+1)] tensors
// (mm_interleaved/models/utils/ops/modules/mmfs.py:181-265): add the per-image relative-position
// term, scale offsets per level, add the visibility penalty, overwrite the sink logit, softmax
// over all n*L*(P+1) logits, split points / sinks, divide offsets by the level extent, add the
// reference point, cast.  With the two linear heads rewritten as  head(Wq) + table[relpos]
// (mmfs_amd/modules/mmfs.py) everything after the GEMMs is a per-(sample, query, head) function
// of two small vectors and two table rows; this file evaluates it in one pass, in fp32, from
//     off_q  [N, Lq, H, P, 2]      = sampling_offsets(q')          (bias included)
//     att_q  [N, Lq, H, L, P]      = attention_weights(q'), point columns only (the sink column
//                                    is a constant, mmfs.py:225, and is never computed)
//     off_tab[M, H, P, 2], att_tab[M, H, L, P]     = head.weight @ query_relpos rows
//     relpos [N, Lr, n] int64      (0 = image not visible; Lr = 1 or Lq)
// to
//     loc  [N, Lq, H, n*L, P, 2],  attn [N, Lq, H, n*L, P],  sink [N, Lq, H] (sum of sink weights).
//
// One lane owns one (image, level) row of P logits / P locations (a 16-byte vector for bf16 P=8);
// the 2^k >= n*L lanes of an item reduce with wave shuffles.  The backward walks runs of consecutive
// queries and keeps the gradient of the lane's table row in registers (the relative position of
// an image changes at most once per image along the sequence), flushing it with a few float atomics.
#include "msda_env.h"
#include "msda_gather.h"
#include "msda_host.h"
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>

namespace mmfs {

namespace {

constexpr int kThreads = 256;
constexpr int kQueryRun = 8;            // backward: consecutive queries a lane group walks (table grads in registers)

struct PlanDims {
    int N, Lq, H, L, P, n, M, Lr, Nr;
    int ld_off, ld_att;     // elements between the rows of two tokens in off_q / att_q (H*2P / H*L*P when packed)
    int ld_toff, ld_tatt;   // the same for the two tables' rows (plan kernels; the sampler's tables are packed)
};

// ---------------------------------------------------------------- the plan row
// One (image, level) row of an item's plan, evaluated by plan_forward_kernel, mmfs_sample_fwd and mmfs_sample_decode
// through THESE functions: the fused samplers' locations and weights are the plan kernel's bits by construction.

// lane group: G = 2^k lanes, one per (image, level) row of P points; reductions stay inside it.  G known at compile
// time (the plan kernels) or not (the samplers): the same butterfly, the same order of sums (msda_device.h)
template <int G> struct LaneGroup {
    __device__ __forceinline__ float max(float v) const { return group_max<G>(v); }
    __device__ __forceinline__ float add(float v) const { return group_add<G>(v); }
};
struct LaneGroupRt {
    int G;
    __device__ __forceinline__ float max(float v) const { return group_max(v, G); }
    __device__ __forceinline__ float add(float v) const { return group_add(v, G); }
};

// logits of row gl (= image k, level l) of the item (nb, q, h): att_q + table row + visibility penalty.  Returns the
// image's relative position (its table row; 0 = not visible, mmfs.py:203-218)
//   att_q [N, Lq, H, L, P]  att_tab [M, H, L, P]   (the dead sink column is not computed at all)
template <typename T, int P>
__device__ __forceinline__ int64_t row_logits(const T *__restrict__ att_q, const T *__restrict__ att_tab,
                                              const int64_t *__restrict__ relpos, const PlanDims &d, int nb, int q, int h,
                                              int gl, float (&lg)[P])
{
    const int k = gl / d.L, l = gl % d.L;
    const int64_t r = relpos[((int64_t)nb * d.Lr + (d.Lr == 1 ? 0 : q)) * d.n + k];
    float a[P], t[P];
    load_row<T, P>(att_q + ((int64_t)nb * d.Lq + q) * d.ld_att + (h * d.L + l) * P, a);
    load_row<T, P>(att_tab + r * d.ld_tatt + (h * d.L + l) * P, t);
    const float pen = r == 0 ? -10000.f : 0.f;
#pragma unroll
    for (int p = 0; p < P; ++p) lg[p] = a[p] + t[p] + pen;
    return r;
}

// Softmax statistics of an item over its rows' logits and one sink slot per row (mmfs.py:225): every lane of the group
// brings its row's logits (act false: a lane without a row).  Leaves exp(logit - m) in lg (0 without a row).
template <int P, typename Grp>
__device__ __forceinline__ void sink_softmax(float (&lg)[P], bool act, float sink_logit, const Grp grp,
                                             float &m, float &inv, float &sink_sum)
{
    m = sink_logit;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        if (!act) lg[p] = -INFINITY;
        m = fmaxf(m, lg[p]);
    }
    m = grp.max(m);
    float z = act ? __expf(sink_logit - m) : 0.f;           // this row's sink slot
    const float my_sink = z;
#pragma unroll
    for (int p = 0; p < P; ++p) { lg[p] = __expf(lg[p] - m); z += lg[p]; }
    z = grp.add(z);
    inv = 1.f / z;
    sink_sum = grp.add(my_sink) * inv;
}

// the row's offsets (query side + the table row of relative position r), reference point and offset scale:
// loc = ref + (offset_q + offset_table) * ratio_l / (W, H)        (mmfs.py:193-198, 243-250)
template <typename T, int P>
__device__ __forceinline__ void row_geometry(const T *__restrict__ off_q, const T *__restrict__ off_tab,
                                             const float *__restrict__ ref, const float *__restrict__ ratios,
                                             const PlanDims &d, int nb, int q, int h, int gl, int64_t r, float Hl, float Wl,
                                             float (&oq)[2 * P], float (&ot)[2 * P], float &rx, float &ry, float &sx, float &sy)
{
    load_row<T, 2 * P>(off_q + ((int64_t)nb * d.Lq + q) * d.ld_off + h * 2 * P, oq);
    load_row<T, 2 * P>(off_tab + r * d.ld_toff + h * 2 * P, ot);
    rx = ref[((int64_t)(d.Nr == 1 ? 0 : nb) * d.Lq + q) * 2];
    ry = ref[((int64_t)(d.Nr == 1 ? 0 : nb) * d.Lq + q) * 2 + 1];
    const int l = gl % d.L;
    sx = ratios[l] / Wl; sy = ratios[l] / Hl;
}

// A point's weight and location as the numbers of the storage type (held in floats); e: sink_softmax's exp(logit - m).
// An fp32 result, THEN rounded to the storage type.  For fp16 storage the compiler folds ``(half)fma(a, b, c)`` into
// v_fma_mixlo_f16, which rounds the exact sum ONCE; with offsets that are halves and scales that are powers of two the
// fp32 result often sits exactly on a half-precision tie, where the two roundings part (a golden: one location in 4608
// -> two outputs one unit apart between a kernel that rounds twice and one that rounds once).
// The opaque register keeps the fp32 rounding.
template <typename T> __device__ __forceinline__ float point_weight(float e, float inv)
{
    float wgt = e * inv;
    asm volatile("" : "+v"(wgt));
    return to_f32((T)wgt);
}
// (o: the row's offsets as (x, y) pairs, query side and table side; p: the point)
template <typename T, int P>
__device__ __forceinline__ void point_location(const float (&oq)[2 * P], const float (&ot)[2 * P], int p, float rx, float ry,
                                               float sx, float sy, float &x, float &y)
{
    float lx = fmaf(oq[2 * p] + ot[2 * p], sx, rx), ly = fmaf(oq[2 * p + 1] + ot[2 * p + 1], sy, ry);
    asm volatile("" : "+v"(lx), "+v"(ly));
    x = to_f32((T)lx); y = to_f32((T)ly);
}

// Forward: lane <-> one (item, image, level) row of P logits; G lanes (>= n*L) form an item.
template <typename T, int P, int G>
__global__ void __launch_bounds__(kThreads)
plan_forward_kernel(const T *__restrict__ off_q, const T *__restrict__ att_q,
                    const T *__restrict__ off_tab, const T *__restrict__ att_tab,
                    const int64_t *__restrict__ relpos, const float *__restrict__ ref,
                    const int64_t *__restrict__ shapes, const float *__restrict__ ratios,
                    T *__restrict__ loc, T *__restrict__ attn, float *__restrict__ sink, const PlanDims d)
{
    constexpr int IPB = kThreads / G;                       // items per workgroup
    const int gl = threadIdx.x % G;                         // row of the item: kl = k*L + l
    const int64_t item = (int64_t)blockIdx.x * IPB + threadIdx.x / G;     // (nb*Lq + q)*H + h
    const int nL = d.n * d.L;
    const bool item_ok = item < (int64_t)d.N * d.Lq * d.H;
    const bool act = item_ok && gl < nL;
    const int64_t it = item_ok ? item : 0;
    const int h = (int)(it % d.H);
    const int64_t nq = it / d.H;
    const int q = (int)(nq % d.Lq);
    const int nb = (int)(nq / d.Lq);

    float lg[P], m, inv, sink_sum;
    int64_t r = 0;
    if (act) r = row_logits<T, P>(att_q, att_tab, relpos, d, nb, q, h, gl, lg);
    sink_softmax<P>(lg, act, -logf((float)nL), LaneGroup<G>(), m, inv, sink_sum);
    if (item_ok && gl == 0) sink[item] = sink_sum;
    if (!act) return;
    float w[P];
#pragma unroll
    for (int p = 0; p < P; ++p) w[p] = point_weight<T>(lg[p], inv);
    const int64_t row = item * nL + gl;
    store_row<T, P>(attn + row * P, w);
    float oq[2 * P], ot[2 * P], xy[2 * P], rx, ry, sx, sy;
    row_geometry<T, P>(off_q, off_tab, ref, ratios, d, nb, q, h, gl, r, (float)shapes[2 * gl], (float)shapes[2 * gl + 1],
                       oq, ot, rx, ry, sx, sy);
#pragma unroll
    for (int p = 0; p < P; ++p) point_location<T, P>(oq, ot, p, rx, ry, sx, sy, xy[2 * p], xy[2 * p + 1]);
    store_row<T, 2 * P>(loc + row * 2 * P, xy);
}

// Backward: same lane <-> row map; a lane group walks kQueryRun consecutive queries of one
// (sample, head) and keeps the gradients of ITS table row (image k's relative position) in
// registers, flushing them with P + 2P float atomics when the relative position changes or the
// run ends.  d_att_q / d_off_q need the sum over the images of a level / over the levels of an
// image: done through a per-group LDS slab.
// (OT: the type the query-side gradients are stored in -- fp32, or the storage type for a caller that casts them anyway)
template <typename T, typename OT, int P, int G>
__global__ void __launch_bounds__(kThreads)
plan_backward_kernel(const T *__restrict__ grad_loc, const T *__restrict__ grad_attn,
                     const float *__restrict__ grad_sink, const T *__restrict__ attn,
                     const float *__restrict__ sink, const int64_t *__restrict__ relpos,
                     const int64_t *__restrict__ shapes, const float *__restrict__ ratios,
                     OT *__restrict__ d_off_q, OT *__restrict__ d_att_q,
                     float *__restrict__ d_off_tab, float *__restrict__ d_att_tab, const PlanDims d)
{
    constexpr int GPB = kThreads / G;                       // lane groups per workgroup
    __shared__ float slab[GPB][G][3 * P];                   // per row: dlogit[P] | doff[2P]
    __shared__ long long seg_key[GPB][G];                   // (sample*H + head, relpos) of the row's table grads
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    const int q_runs = (d.Lq + kQueryRun - 1) / kQueryRun;
    const int64_t unit = (int64_t)blockIdx.x * GPB + grp;   // (nb*H + h)*q_runs + run
    const int nL = d.n * d.L;
    const bool unit_ok = unit < (int64_t)d.N * d.H * q_runs;
    const int64_t u = unit_ok ? unit : 0;
    const int run = (int)(u % q_runs);
    const int h = (int)((u / q_runs) % d.H);
    const int nb = (int)(u / q_runs / d.H);
    const bool act = unit_ok && gl < nL;
    const int k = act ? gl / d.L : 0, l = act ? gl % d.L : 0;
    const float sx = act ? ratios[l] / (float)shapes[2 * gl + 1] : 0.f;
    const float sy = act ? ratios[l] / (float)shapes[2 * gl] : 0.f;

    float t_att[P], t_off[2 * P];
    int64_t t_rp = -1;
#pragma unroll
    for (int p = 0; p < P; ++p) { t_att[p] = 0.f; t_off[2 * p] = 0.f; t_off[2 * p + 1] = 0.f; }
    auto flush = [&]() {
        if (t_rp < 0) return;
        float *ta = d_att_tab + t_rp * d.ld_tatt + (h * d.L + l) * P;
        float *to = d_off_tab + t_rp * d.ld_toff + h * 2 * P;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            __hip_atomic_fetch_add(ta + p, t_att[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(to + 2 * p, t_off[2 * p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(to + 2 * p + 1, t_off[2 * p + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            t_att[p] = 0.f; t_off[2 * p] = 0.f; t_off[2 * p + 1] = 0.f;
        }
    };

    const int q_lo = run * kQueryRun, q_hi = min(d.Lq, q_lo + kQueryRun);
    for (int q = q_lo; q < q_hi; ++q) {
        const int64_t item = ((int64_t)nb * d.Lq + q) * d.H + h;
        float w[P], g[P], dl[P], dof[2 * P];
        float part = 0.f;
        int64_t r = 0;
        if (act) {
            r = relpos[((int64_t)nb * d.Lr + (d.Lr == 1 ? 0 : q)) * d.n + k];
            if (r != t_rp) { flush(); t_rp = r; }
            const int64_t row = item * nL + gl;
            load_row<T, P>(attn + row * P, w);
            load_row<T, P>(grad_attn + row * P, g);
#pragma unroll
            for (int p = 0; p < P; ++p) part += w[p] * g[p];
        }
        // softmax backward: dlogit_i = w_i (g_i - sum_j w_j g_j), the sinks' share included
        float dot = group_add<G>(part);
        if (unit_ok && grad_sink) dot += grad_sink[item] * sink[item];
        if (act) {
            float gxy[2 * P];
            load_row<T, 2 * P>(grad_loc + (item * nL + gl) * 2 * P, gxy);
#pragma unroll
            for (int p = 0; p < P; ++p) {
                dl[p] = w[p] * (g[p] - dot);
                dof[2 * p] = gxy[2 * p] * sx;
                dof[2 * p + 1] = gxy[2 * p + 1] * sy;
                t_att[p] += dl[p];
                t_off[2 * p] += dof[2 * p];
                t_off[2 * p + 1] += dof[2 * p + 1];
                slab[grp][gl][p] = dl[p];
                slab[grp][gl][P + 2 * p] = dof[2 * p];
                slab[grp][gl][P + 2 * p + 1] = dof[2 * p + 1];
            }
        }
        __builtin_amdgcn_wave_barrier();            // a group never spans waves (G <= 64)
        // d_att_q[item, l, :] = sum over images k of dlogit[k*L + l, :]  (rows l < L do it)
        if (unit_ok && gl < d.L) {
            float acc[P];
#pragma unroll
            for (int p = 0; p < P; ++p) acc[p] = 0.f;
            for (int kk = 0; kk < d.n; ++kk)
#pragma unroll
                for (int p = 0; p < P; ++p) acc[p] += slab[grp][kk * d.L + gl][p];
            store_row<OT, P>(d_att_q + (item / d.H) * d.ld_att + (h * d.L + gl) * P, acc);
        }
        // d_off_q[item, :, :] = sum over all rows (images and levels) of doff  (row 0 does it)
        if (unit_ok && gl == 0) {
            float acc[2 * P];
#pragma unroll
            for (int p = 0; p < 2 * P; ++p) acc[p] = 0.f;
            for (int rr = 0; rr < nL; ++rr)
#pragma unroll
                for (int p = 0; p < 2 * P; ++p) acc[p] += slab[grp][rr][P + p];
            store_row<OT, 2 * P>(d_off_q + (item / d.H) * d.ld_off + h * 2 * P, acc);
        }
        __builtin_amdgcn_wave_barrier();
    }
    // ---- the table rows are shared by every query of a (sample, head): same-address atomics
    //      serialise in L2 (measured: 6.6 ms when every lane group flushed its own), so the groups
    //      of the workgroup -- consecutive query runs, normally the same table row -- are summed
    //      through LDS first and only the first group of each equal-key segment issues atomics.
    __syncthreads();
#pragma unroll
    for (int p = 0; p < P; ++p) {
        slab[grp][gl][p] = t_att[p];
        slab[grp][gl][P + 2 * p] = t_off[2 * p];
        slab[grp][gl][P + 2 * p + 1] = t_off[2 * p + 1];
    }
    // (nb * H + h < 2^31 and t_rp < M <= 2^31 - 1 by check_dims: 32 bits each, no two rows share a key)
    seg_key[grp][gl] = (act && t_rp >= 0) ? (((long long)nb * d.H + h) << 32 | (long long)t_rp) : -1LL - grp;
    __syncthreads();
    if (act && t_rp >= 0 && (grp == 0 || seg_key[grp - 1][gl] != seg_key[grp][gl])) {
        const long long key = seg_key[grp][gl];
        for (int g2 = grp + 1; g2 < GPB && seg_key[g2][gl] == key; ++g2) {
#pragma unroll
            for (int p = 0; p < P; ++p) {
                t_att[p] += slab[g2][gl][p];
                t_off[2 * p] += slab[g2][gl][P + 2 * p];
                t_off[2 * p + 1] += slab[g2][gl][P + 2 * p + 1];
            }
        }
        flush();
    }
}


// ---------------------------------------------------------------- plan -> sampler, one kernel (forward / inference)
// SURVEY.md 8f N1, second half: the sampling plan feeds the sampler directly -- the locations and weights
// [N, Lq, H, n*L, P(, 2)] never exist in HBM.  This is msda_fwd_vec (csrc/msda_fwd.hip) with its staging
// replaced: instead of reading loc / attn it evaluates the plan for its 256 / LPI queries of one (sample,
// head) from the heads' outputs and table rows with the plan row's functions above (plan_forward_kernel's lane
// groups and reduction order, results rounded to the storage type before use) and walks the records with
// msda_fwd_vec's functions (msda_gather.h), so the output is bit-identical to plan_forward +
// ms_deform_attn_forward.  Forward only: the backward needs loc / attn as
// tensors (the sort scans them, the plan backward reads the weights), so training keeps the two kernels.
constexpr int kSampleRecs = 512;        // tap records staged per chunk (as msda_fwd_vec)
constexpr int kSampleUnroll = 2;

// BT: the bank's type, T or fp8e4m3_t (scales [Bv, H*D] applied at the store, as msda_fwd_vec; the ignore-token term
// stays in T)
template <typename T, int LPI, int P, typename BT>
__global__ void __launch_bounds__(kThreads)
mmfs_sample_fwd(const BT *__restrict__ value, const int64_t *__restrict__ shapes, const int64_t *__restrict__ start,
                const T *__restrict__ off_q, const T *__restrict__ att_q,
                const T *__restrict__ off_tab, const T *__restrict__ att_tab,
                const int64_t *__restrict__ relpos, const float *__restrict__ ref, const float *__restrict__ ratios,
                T *__restrict__ out, float *__restrict__ sink, const Dims d, const PlanDims pd, const int G,
                const T *__restrict__ token, const float *__restrict__ vscale)
{
    typedef Vec16<BT> V;
    constexpr int VEC = V::N;
    constexpr int QPB = kThreads / LPI;
    constexpr int KC = (kSampleRecs / QPB) > P ? (kSampleRecs / QPB) : P;      // samples per query per chunk: whole rows of P
    __shared__ float ssum[QPB];                           // the queries' summed sink weights (for the ignore-token term)
    static_assert(KC % P == 0 && KC % kSampleUnroll == 0, "chunks hold whole rows of P points");
    constexpr int STRIDE = 2 * KC + 1;
    __shared__ uint4 lds[QPB * STRIDE];
    __shared__ LevelLds levels;
    __shared__ float2 stat[QPB];                          // softmax max and 1 / sum per query of the tile
    __shared__ float4 plan[QPB * KC];                     // {x, y, weight} of the chunk's samples
    constexpr bool kPipe = KC <= 64;                      // live words + the pipelined walk, as in msda_fwd_vec
    constexpr int QPW = 64 / LPI > 0 ? 64 / LPI : 1;
    __shared__ unsigned long long live[kThreads / 64];

    const BlockCoord bc = block_coord(d, QPB);
    const int tid = threadIdx.x;
    const int qi = tid / LPI, lig = tid % LPI;
    const int q = bc.q0 + qi;
    const bool q_ok = q < d.Nq;
    const int nL = d.L;                                   // = n * levels per image
    const int64_t HD = (int64_t)d.H * d.D;
    const BT *slab = value + ((int64_t)value_row(d, bc.b) * d.S) * HD + (int64_t)bc.h * d.D;
    const uint32_t row_bytes = (uint32_t)(HD * sizeof(BT));
    const uint32_t lane_off = (uint32_t)(lig * 16);
    const __amdgpu_buffer_rsrc_t rsrc = make_slab_rsrc(slab, ((int64_t)d.S * HD - (int64_t)bc.h * d.D) * (int64_t)sizeof(BT));
    levels.load(shapes, start, nL, tid, kThreads);
    if (kPipe && tid < kThreads / 64) live[tid] = 0ull;
    const float sink_logit = -logf((float)nL);

    // ---- softmax statistics of the tile's queries (lane group of G per query, like the plan kernel)
    for (int base = 0; base < QPB * G; base += kThreads) {
        if (base + (tid & ~63) >= QPB * G) continue;      // (whole waves only: the groups shuffle)
        const int s = base + tid, rq = s / G, gl = s % G;
        const int sq = bc.q0 + rq;
        const bool item_ok = rq < QPB && sq < d.Nq;
        const bool act = item_ok && gl < nL;
        float lg[P], m, inv, sink_sum;
        if (act) row_logits<T, P>(att_q, att_tab, relpos, pd, bc.b, sq, bc.h, gl, lg);
        sink_softmax<P>(lg, act, sink_logit, LaneGroupRt{G}, m, inv, sink_sum);
        if (item_ok && gl == 0) {
            stat[rq] = make_float2(m, inv);
            ssum[rq] = sink_sum;
            if (sink != nullptr) sink[((int64_t)bc.b * pd.Lq + sq) * pd.H + bc.h] = sink_sum;
        }
    }
    __syncthreads();

    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.f;

    for (int k0 = 0; k0 < d.K; k0 += KC) {
        const int kc = min(KC, d.K - k0);                 // a multiple of P (and of the unroll)
        const int rows = kc / P;
        if (k0 > 0) __syncthreads();
        // ---- stage, step 1: one lane per (query, row): the row's P weights and locations, rounded to the
        // storage type like the tensors of the two-kernel path, parked in LDS
        for (int s = tid; s < QPB * rows; s += kThreads) {
            const int rq = s / rows, rr = s - rq * rows, gl = k0 / P + rr;
            const int sq = bc.q0 + rq;
            float4 *dst = &plan[rq * KC + rr * P];
            if (sq >= d.Nq) {
#pragma unroll
                for (int p = 0; p < P; ++p) dst[p] = make_float4(-8.f, -8.f, 0.f, 0.f);      // outside every map, weight 0
                continue;
            }
            float lg[P], oq[2 * P], ot[2 * P], rx, ry, sx, sy;
            const int64_t r = row_logits<T, P>(att_q, att_tab, relpos, pd, bc.b, sq, bc.h, gl, lg);
            const float2 st2 = stat[rq];
#pragma unroll
            for (int p = 0; p < P; ++p) lg[p] = __expf(lg[p] - st2.x);
            int Hl, Wl, lstart;
            levels.get(shapes, start, gl, Hl, Wl, lstart);
            row_geometry<T, P>(off_q, off_tab, ref, ratios, pd, bc.b, sq, bc.h, gl, r, (float)Hl, (float)Wl, oq, ot, rx, ry, sx, sy);
#pragma unroll
            for (int p = 0; p < P; ++p) {
                float x, y;
                point_location<T, P>(oq, ot, p, rx, ry, sx, sy, x, y);
                dst[p] = make_float4(x, y, point_weight<T>(lg[p], st2.y), 0.f);
            }
        }
        __syncthreads();
        // ---- stage, step 2: one lane per sample: location -> tap record (as msda_fwd_vec does from its tensors)
        for (int r = tid; r < QPB * kc; r += kThreads) {
            const int rq = r / kc, kk = r - rq * kc, gl = (k0 + kk) / P;
            const float4 pl = plan[rq * KC + kk];
            int Hl, Wl, lstart;
            levels.get(shapes, start, gl, Hl, Wl, lstart);
            uint4 rows4, ww;
            tap_record(pl.x, pl.y, pl.z, Hl, Wl, lstart, row_bytes, rows4, ww);
            uint4 *dst = &lds[rq * STRIDE + 2 * kk];
            dst[0] = rows4;
            dst[1] = ww;
            if (kPipe) mark_live<QPW>(live, rq, kk, ww);
        }
        __syncthreads();
        // ---- gather (msda_gather.h, as msda_fwd_vec)
        if (kPipe) gather_live<V>(take_live(live, tid), &lds[qi * STRIDE], rsrc, lane_off, acc);
        else if (q_ok) gather_all<V, kSampleUnroll>(&lds[qi * STRIDE], kc, rsrc, lane_off, acc);
    }
    if (q_ok) {
        T *o = out + (((int64_t)bc.b * d.Nq + q) * d.H + bc.h) * d.D + lig * VEC;
        apply_scale<BT, VEC>(acc, vscale, (int64_t)value_row(d, bc.b) * HD + (int64_t)bc.h * d.D + lig * VEC);
        if (token != nullptr) add_ignore_token<T, VEC>(acc, token + (int64_t)bc.h * d.D + lig * VEC, ssum[qi]);
        store_vec<T, VEC, false>(o, acc);
    }
}

// ---------------------------------------------------------------- the same for a handful of queries (a decode step)
// One new token per sequence is ONE query per (sample, head), and mmfs_sample_fwd serves it with 8 of a workgroup's
// 256 lanes: softmax statistics (index -> table row: two dependent round trips), barrier, the same rows again for the
// plan, barrier, tap records, barrier, and then the query's 24 samples two at a time -- a dozen dependent round trips,
// 13.9 us per call for 4 tokens (profiles/r03by_decode_kernel_stats.csv; 64-lane workgroups of the
// same kernel: 13.6, r04w).  Here a 64-lane workgroup (one wave: its barriers are free) owns ONE query:
//   A  lane gl < n*L evaluates row gl of the plan ONCE (logits, softmax over the lane group, locations) -- with the
//      plan row's functions above, so locations and weights are the same bits;
//   B  lane s evaluates sample s's tap record from A's row (LDS);
//   C  the 64 / LPI lane groups take the samples round-robin, EVERY row load of the query in flight at once, and add
//      their partial sums up in a fixed tree.
// Three dependent global round trips (index, table rows, value rows).  Against the two-kernel path (and mmfs_sample_fwd)
// the same products in fp32, summed in another order: equal within one rounding of the storage type, not bit for bit
// (mmfs_sample_forward_groups tells a caller which kernel a shape takes).
constexpr int kDecodeMaxQ = 8;          // queries per (sample, head) up to which a workgroup per query pays
constexpr int kDecodeMaxK = 256;        // samples per query held as tap records
constexpr int kDecodeBatch = 4;         // samples in flight per lane group (16 row loads per lane)

template <typename T, int LPI, int P, typename BT>
__global__ void __launch_bounds__(64)
mmfs_sample_decode(const BT *__restrict__ value, const int64_t *__restrict__ shapes, const int64_t *__restrict__ start,
                   const T *__restrict__ off_q, const T *__restrict__ att_q,
                   const T *__restrict__ off_tab, const T *__restrict__ att_tab,
                   const int64_t *__restrict__ relpos, const float *__restrict__ ref, const float *__restrict__ ratios,
                   T *__restrict__ out, float *__restrict__ sink, const Dims d, const PlanDims pd, const int G,
                   const T *__restrict__ token, const float *__restrict__ vscale)
{
    typedef Vec16<BT> V;
    constexpr int VEC = V::N;
    constexpr int NSUB = 64 / LPI;
    __shared__ float4 plan[kDecodeMaxK];                  // {x, y, weight} per sample, rounded to the storage type
    __shared__ int rowinfo[64 * 3];                       // Hl, Wl, start of the rows' levels
    __shared__ uint4 recs[2 * kDecodeMaxK];               // per sample: four row offsets, four corner weights
    const int tid = threadIdx.x;
    const int h = blockIdx.x % d.H;
    const int q = (blockIdx.x / d.H) % d.Nq, b = blockIdx.x / d.H / d.Nq;
    const int nL = d.L;
    const int64_t HD = (int64_t)d.H * d.D;
    const BT *slab = value + ((int64_t)value_row(d, b) * d.S) * HD + (int64_t)h * d.D;
    const uint32_t row_bytes = (uint32_t)(HD * sizeof(BT));
    const __amdgpu_buffer_rsrc_t rsrc = make_slab_rsrc(slab, ((int64_t)d.S * HD - (int64_t)h * d.D) * (int64_t)sizeof(BT));

    // ---- A: row gl of the plan (lanes of the first lane group; the others idle through the shuffles)
    float sink_sum;
    {
        const int gl = tid;
        const bool act = gl < nL;
        float lg[P], oq[2 * P], ot[2 * P], m, inv, rx, ry, sx, sy;
        if (act) {
            const int64_t r = row_logits<T, P>(att_q, att_tab, relpos, pd, b, q, h, gl, lg);
            const int Hl = (int)shapes[2 * gl], Wl = (int)shapes[2 * gl + 1];
            rowinfo[3 * gl] = Hl; rowinfo[3 * gl + 1] = Wl; rowinfo[3 * gl + 2] = (int)start[gl];
            row_geometry<T, P>(off_q, off_tab, ref, ratios, pd, b, q, h, gl, r, (float)Hl, (float)Wl, oq, ot, rx, ry, sx, sy);
        }
        sink_softmax<P>(lg, act, -logf((float)nL), LaneGroupRt{G}, m, inv, sink_sum);
        if (tid == 0 && sink != nullptr) sink[((int64_t)b * pd.Lq + q) * pd.H + h] = sink_sum;
        if (act) {
#pragma unroll
            for (int p = 0; p < P; ++p) {
                float x, y;
                point_location<T, P>(oq, ot, p, rx, ry, sx, sy, x, y);
                plan[gl * P + p] = make_float4(x, y, point_weight<T>(lg[p], inv), 0.f);
            }
        }
    }
    sink_sum = __shfl(sink_sum, 0, 64);
    __syncthreads();
    // ---- B: one lane per sample: location -> tap record (as msda_fwd_vec does from its tensors)
    for (int s = tid; s < d.K; s += 64) {
        const int gl = s / P;
        const float4 pl = plan[s];
        uint4 rows, ww;
        tap_record(pl.x, pl.y, pl.z, rowinfo[3 * gl], rowinfo[3 * gl + 1], rowinfo[3 * gl + 2], row_bytes, rows, ww);
        recs[2 * s] = rows;
        recs[2 * s + 1] = ww;
    }
    __syncthreads();
    // ---- C: lane group `sub` takes samples sub, sub + NSUB, ...; a batch's row loads all leave before the first is used
    const int sub = tid / LPI, lig = tid % LPI;
    const uint32_t lane_off = (uint32_t)(lig * 16);
    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < d.K; k0 += NSUB * kDecodeBatch) {
        uint4 raw[kDecodeBatch][4], wq[kDecodeBatch];
#pragma unroll
        for (int u = 0; u < kDecodeBatch; ++u) {
            const int kk = k0 + u * NSUB + sub;
            uint4 rr;
            tap_record_none(rr, wq[u]);
            if (kk < d.K) { rr = recs[2 * kk]; wq[u] = recs[2 * kk + 1]; }
            load_rows(rsrc, rr, lane_off, raw[u]);
        }
#pragma unroll
        for (int u = 0; u < kDecodeBatch; ++u) fma_rows<V>(raw[u], wq[u], acc);
    }
#pragma unroll
    for (int o = 32; o >= LPI; o >>= 1)
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += __shfl_xor(acc[i], o, 64);
    if (sub == 0) {
        T *o = out + (((int64_t)b * d.Nq + q) * d.H + h) * d.D + lig * VEC;
        apply_scale<BT, VEC>(acc, vscale, (int64_t)value_row(d, b) * HD + (int64_t)h * d.D + lig * VEC);
        if (token != nullptr) add_ignore_token<T, VEC>(acc, token + (int64_t)h * d.D + lig * VEC, sink_sum);
        store_vec<T, VEC, false>(o, acc);
    }
}

// lane groups that share a query's samples: 1 = mmfs_sample_fwd (sums in sample order, bit-identical to plan + op)
int sample_groups(int64_t Lq, int64_t K, int64_t nL, int lpi)
{
    const char *e = mmfs::knob_str(mmfs::K_SAMPLE_DECODE);   // (the tests hold both kernels to the same goldens)
    if ((e && e[0] == '0') || Lq > kDecodeMaxQ || K > kDecodeMaxK || nL > 64 || lpi > 32) return 1;
    return 64 / lpi;
}

int check_dims(int64_t N, int64_t Lq, int64_t H, int64_t L, int64_t P, int64_t n, int64_t M, int64_t Lr,
               int64_t Nr, PlanDims *d)
{
    const int64_t lim = 0x7fffffffLL;
    if (N < 0 || Lq < 0 || H <= 0 || L <= 0 || P <= 0 || n <= 0 || M <= 0) return MMFS_E_DIMS;
    if (N > lim || Lq > lim || H > lim || n > lim || M > lim) return MMFS_E_DIMS;
    if ((Lr != 1 && Lr != Lq) || (Nr != 1 && Nr != N)) return MMFS_E_DIMS;
    if ((P != 4 && P != 8 && P != 16) || n * L > 64) return MMFS_E_UNSUPPORTED;
    if (N * Lq * H > lim) return MMFS_E_DIMS;
    d->N = (int)N; d->Lq = (int)Lq; d->H = (int)H; d->L = (int)L; d->P = (int)P; d->n = (int)n;
    d->M = (int)M; d->Lr = (int)Lr; d->Nr = (int)Nr;
    d->ld_off = d->ld_toff = (int)(H * 2 * P);
    d->ld_att = d->ld_tatt = (int)(H * L * P);
    return MMFS_OK;
}

}  // namespace
}  // namespace mmfs

// dispatch over the lane-group width G (the power of two >= n*L, 4 .. 64); the points per row P: by_int<4, 8, 16>
template <typename F> static int for_group(int nL, F &&f)
{
    int G = 4;
    while (G < nL) G *= 2;
    return mmfs::by_int<4, 8, 16, 32, 64>(G, f);
}

extern "C" {

int mmfs_plan_forward(int dtype, const void *off_q, const void *att_q, const void *off_tab,
                      const void *att_tab, const int64_t *relpos, const float *ref,
                      const int64_t *shapes, const float *ratios, void *loc, void *attn, float *sink,
                      int64_t N, int64_t Lq, int64_t H, int64_t L, int64_t P, int64_t n, int64_t M,
                      int64_t Lr, int64_t Nr, void *stream)
{
    return mmfs_plan_forward_heads(dtype, off_q, att_q, 0, 0, off_tab, att_tab, 0, 0, relpos, ref, shapes, ratios, loc, attn,
                                   sink, N, Lq, H, L, P, n, M, Lr, Nr, stream);
}

int mmfs_plan_forward_heads(int dtype, const void *off_q, const void *att_q, int64_t ld_off, int64_t ld_att,
                            const void *off_tab, const void *att_tab, int64_t ld_toff, int64_t ld_tatt,
                            const int64_t *relpos, const float *ref,
                            const int64_t *shapes, const float *ratios, void *loc, void *attn, float *sink,
                            int64_t N, int64_t Lq, int64_t H, int64_t L, int64_t P, int64_t n, int64_t M,
                            int64_t Lr, int64_t Nr, void *stream)
{
    using namespace mmfs;
    const int es = elem_size(dtype);
    if (!es) return MMFS_E_DTYPE;
    PlanDims d;
    const int rc = check_dims(N, Lq, H, L, P, n, M, Lr, Nr, &d);
    if (rc) return rc;
    const int64_t items = N * Lq * H;
    if (items == 0) return MMFS_OK;
    // (the rows of the four matrices: heads_rows; nothing else is refused for its alignment)
    int rr = check_tensors({{off_q, 1}, {att_q, 1}, {off_tab, 1}, {att_tab, 1}, {relpos, 1}, {ref, 1}, {shapes, 1}, {ratios, 1},
                            {loc, 1}, {attn, 1}, {sink, 1}});
    if (rr) return rr;
    if ((rr = heads_rows(ld_off, H * 2 * P, off_q, 2 * P, es)) || (rr = heads_rows(ld_att, H * L * P, att_q, P, es)) ||
        (rr = heads_rows(ld_toff, H * 2 * P, off_tab, 2 * P, es)) || (rr = heads_rows(ld_tatt, H * L * P, att_tab, P, es)))
        return rr;
    d.ld_off = (int)ld_off; d.ld_att = (int)ld_att; d.ld_toff = (int)ld_toff; d.ld_tatt = (int)ld_tatt;
    hipStream_t st = (hipStream_t)stream;
    auto go = [&](auto tag_t, auto tag_p) {
        typedef decltype(tag_t) T;
        constexpr int PP = decltype(tag_p)::value;
        return for_group(d.n * d.L, [&](auto tag_g) {
            constexpr int G = decltype(tag_g)::value;
            const unsigned blocks = (unsigned)((items + kThreads / G - 1) / (kThreads / G));
            hipLaunchKernelGGL((plan_forward_kernel<T, PP, G>), dim3(blocks), dim3(kThreads), 0, st,
                               (const T *)off_q, (const T *)att_q, (const T *)off_tab, (const T *)att_tab,
                               relpos, ref, shapes, ratios, (T *)loc, (T *)attn, sink, d);
            return (int)hipGetLastError();
        });
    };
    return by_type(dtype, [&](auto tag_t) { return by_int<4, 8, 16>(P, [&](auto tag_p) { return go(tag_t, tag_p); }); });
}

int mmfs_plan_backward(int dtype, const void *grad_loc, const void *grad_attn, const float *grad_sink,
                       const void *attn, const float *sink, const int64_t *relpos,
                       const int64_t *shapes, const float *ratios,
                       float *d_off_q, float *d_att_q, float *d_off_tab, float *d_att_tab,
                       int64_t N, int64_t Lq, int64_t H, int64_t L, int64_t P, int64_t n, int64_t M,
                       int64_t Lr, int64_t Nr, void *stream)
{
    return mmfs_plan_backward_heads(dtype, grad_loc, grad_attn, grad_sink, attn, sink, relpos, shapes, ratios, d_off_q, d_att_q,
                                    0, 0, 0, d_off_tab, d_att_tab, 0, 0, N, Lq, H, L, P, n, M, Lr, Nr, stream);
}

int mmfs_plan_backward_heads(int dtype, const void *grad_loc, const void *grad_attn, const float *grad_sink,
                             const void *attn, const float *sink, const int64_t *relpos,
                             const int64_t *shapes, const float *ratios,
                             void *d_off_q, void *d_att_q, int64_t ld_off, int64_t ld_att, int q_grads_in_storage_type,
                             float *d_off_tab, float *d_att_tab, int64_t ld_toff, int64_t ld_tatt,
                             int64_t N, int64_t Lq, int64_t H, int64_t L, int64_t P, int64_t n, int64_t M,
                             int64_t Lr, int64_t Nr, void *stream)
{
    using namespace mmfs;
    const int es = elem_size(dtype);
    if (!es) return MMFS_E_DTYPE;
    PlanDims d;
    const int rc = check_dims(N, Lq, H, L, P, n, M, Lr, Nr, &d);
    if (rc) return rc;
    if (N * Lq * H == 0) return MMFS_OK;
    // (grad_sink may be NULL; the rows of the four gradients: heads_rows)
    int rr = check_tensors({{grad_loc, 1}, {grad_attn, 1}, {attn, 1}, {sink, 1}, {relpos, 1}, {shapes, 1}, {ratios, 1},
                            {d_off_q, 1}, {d_att_q, 1}, {d_off_tab, 1}, {d_att_tab, 1}});
    if (rr) return rr;
    const int qes = q_grads_in_storage_type ? es : 4;
    if ((rr = heads_rows(ld_off, H * 2 * P, d_off_q, 2 * P, qes)) || (rr = heads_rows(ld_att, H * L * P, d_att_q, P, qes)) ||
        (rr = heads_rows(ld_toff, H * 2 * P, d_off_tab, 1, 4)) || (rr = heads_rows(ld_tatt, H * L * P, d_att_tab, 1, 4)))
        return rr;
    d.ld_off = (int)ld_off; d.ld_att = (int)ld_att; d.ld_toff = (int)ld_toff; d.ld_tatt = (int)ld_tatt;
    const int64_t units = N * H * ((Lq + kQueryRun - 1) / kQueryRun);
    hipStream_t st = (hipStream_t)stream;
    auto go = [&](auto tag_t, auto tag_p) {
        typedef decltype(tag_t) T;
        constexpr int PP = decltype(tag_p)::value;
        return for_group(d.n * d.L, [&](auto tag_g) {
            constexpr int G = decltype(tag_g)::value;
            const unsigned blocks = (unsigned)((units + kThreads / G - 1) / (kThreads / G));
            if (q_grads_in_storage_type && !std::is_same<T, float>::value)
                hipLaunchKernelGGL((plan_backward_kernel<T, T, PP, G>), dim3(blocks), dim3(kThreads), 0, st,
                                   (const T *)grad_loc, (const T *)grad_attn, grad_sink, (const T *)attn, sink,
                                   relpos, shapes, ratios, (T *)d_off_q, (T *)d_att_q, d_off_tab, d_att_tab, d);
            else
                hipLaunchKernelGGL((plan_backward_kernel<T, float, PP, G>), dim3(blocks), dim3(kThreads), 0, st,
                                   (const T *)grad_loc, (const T *)grad_attn, grad_sink, (const T *)attn, sink,
                                   relpos, shapes, ratios, (float *)d_off_q, (float *)d_att_q, d_off_tab, d_att_tab, d);
            return (int)hipGetLastError();
        });
    };
    return by_type(dtype, [&](auto tag_t) { return by_int<4, 8, 16>(P, [&](auto tag_p) { return go(tag_t, tag_p); }); });
}

int mmfs_sample_forward(int dtype, const void *value, const int64_t *shapes, const int64_t *start,
                        const void *off_q, const void *att_q, const void *off_tab, const void *att_tab,
                        const int64_t *relpos, const float *ref, const float *ratios, void *out, float *sink,
                        int64_t N, int64_t S, int64_t Lq, int64_t H, int64_t D, int64_t L, int64_t P, int64_t n,
                        int64_t M, int64_t Lr, int64_t Nr, void *stream)
{
    return mmfs_sample_forward_token(dtype, value, shapes, start, off_q, att_q, off_tab, att_tab, relpos, ref, ratios,
                                     nullptr, out, sink, N, S, Lq, H, D, L, P, n, M, Lr, Nr, stream);
}

int mmfs_sample_forward_token(int dtype, const void *value, const int64_t *shapes, const int64_t *start,
                              const void *off_q, const void *att_q, const void *off_tab, const void *att_tab,
                              const int64_t *relpos, const float *ref, const float *ratios, const void *token,
                              void *out, float *sink,
                              int64_t N, int64_t S, int64_t Lq, int64_t H, int64_t D, int64_t L, int64_t P, int64_t n,
                              int64_t M, int64_t Lr, int64_t Nr, void *stream)
{
    return mmfs_sample_forward_heads(dtype, value, shapes, start, off_q, att_q, 0, 0, off_tab, att_tab, relpos, ref, ratios,
                                     token, out, sink, N, S, Lq, H, D, L, P, n, M, Lr, Nr, stream);
}

int mmfs_sample_forward_heads(int dtype, const void *value, const int64_t *shapes, const int64_t *start,
                              const void *off_q, const void *att_q, int64_t ld_off, int64_t ld_att,
                              const void *off_tab, const void *att_tab,
                              const int64_t *relpos, const float *ref, const float *ratios, const void *token,
                              void *out, float *sink,
                              int64_t N, int64_t S, int64_t Lq, int64_t H, int64_t D, int64_t L, int64_t P, int64_t n,
                              int64_t M, int64_t Lr, int64_t Nr, void *stream)
{
    // (an empty batch is a bank of one row's worth: nothing is read)
    return mmfs_sample_forward_heads_shared(dtype, value, shapes, start, off_q, att_q, ld_off, ld_att, off_tab, att_tab, relpos,
                                            ref, ratios, token, out, sink, N, N > 0 ? N : 1, MMFS_BANK_TILE, S, Lq, H, D, L, P,
                                            n, M, Lr, Nr, stream);
}

static int sample_forward_any(int dtype, bool fp8, const void *value, const float *scale, const int64_t *shapes,
                              const int64_t *start, const void *off_q, const void *att_q, int64_t ld_off, int64_t ld_att,
                              const void *off_tab, const void *att_tab,
                              const int64_t *relpos, const float *ref, const float *ratios, const void *token,
                              void *out, float *sink,
                              int64_t N, int64_t Nv, int layout, int64_t S, int64_t Lq, int64_t H, int64_t D, int64_t L,
                              int64_t P, int64_t n, int64_t M, int64_t Lr, int64_t Nr, void *stream);

int mmfs_sample_forward_heads_shared(int dtype, const void *value, const int64_t *shapes, const int64_t *start,
                                     const void *off_q, const void *att_q, int64_t ld_off, int64_t ld_att,
                                     const void *off_tab, const void *att_tab,
                                     const int64_t *relpos, const float *ref, const float *ratios, const void *token,
                                     void *out, float *sink,
                                     int64_t N, int64_t Nv, int layout, int64_t S, int64_t Lq, int64_t H, int64_t D, int64_t L,
                                     int64_t P, int64_t n, int64_t M, int64_t Lr, int64_t Nr, void *stream)
{
    return sample_forward_any(dtype, false, value, nullptr, shapes, start, off_q, att_q, ld_off, ld_att, off_tab, att_tab, relpos,
                              ref, ratios, token, out, sink, N, Nv, layout, S, Lq, H, D, L, P, n, M, Lr, Nr, stream);
}

int mmfs_sample_forward_heads_fp8(int dtype, const void *q, const float *scale, const int64_t *shapes, const int64_t *start,
                                  const void *off_q, const void *att_q, int64_t ld_off, int64_t ld_att,
                                  const void *off_tab, const void *att_tab,
                                  const int64_t *relpos, const float *ref, const float *ratios, const void *token,
                                  void *out, float *sink,
                                  int64_t N, int64_t Nv, int layout, int64_t S, int64_t Lq, int64_t H, int64_t D, int64_t L,
                                  int64_t P, int64_t n, int64_t M, int64_t Lr, int64_t Nr, void *stream)
{
    return sample_forward_any(dtype, true, q, scale, shapes, start, off_q, att_q, ld_off, ld_att, off_tab, att_tab, relpos,
                              ref, ratios, token, out, sink, N, Nv, layout, S, Lq, H, D, L, P, n, M, Lr, Nr, stream);
}

// the shared-bank sampler on a 16-bit / fp32 bank of the output's type, or (fp8) on an e4m3 bank with its scales
static int sample_forward_any(int dtype, bool fp8, const void *value, const float *scale, const int64_t *shapes,
                              const int64_t *start, const void *off_q, const void *att_q, int64_t ld_off, int64_t ld_att,
                              const void *off_tab, const void *att_tab,
                              const int64_t *relpos, const float *ref, const float *ratios, const void *token,
                              void *out, float *sink,
                              int64_t N, int64_t Nv, int layout, int64_t S, int64_t Lq, int64_t H, int64_t D, int64_t L,
                              int64_t P, int64_t n, int64_t M, int64_t Lr, int64_t Nr, void *stream)
{
    using namespace mmfs;
    const int es = elem_size(dtype);
    if (!es) return MMFS_E_DTYPE;
    const int bes = fp8 ? 1 : es;                                           // the bank's element size
    PlanDims pd;
    const int rc = check_dims(N, Lq, H, L, P, n, M, Lr, Nr, &pd);
    if (rc) return rc;
    Dims d;
    if (const int rb = set_bank(&d, N, Nv, layout)) return rb;              // (Nv = N: the unshared call)
    if (S < 0 || D <= 0 || S > 0x7ffffffdLL || H * D > 0x7fffffffLL) return MMFS_E_DIMS;
    if (N * Lq * H == 0) return MMFS_OK;
    if (P == 16 || S == 0) return MMFS_E_UNSUPPORTED;                       // (P = 16: the two-kernel path)
    const int vec = 16 / bes;
    if (D % vec) return MMFS_E_UNSUPPORTED;
    const int lpi = (int)(D / vec);
    if (lpi < 1 || lpi > (fp8 ? 16 : 64) || (lpi & (lpi - 1))) return MMFS_E_UNSUPPORTED;
    if (S * H * D * (int64_t)bes > kMaxSlabBytes) return MMFS_E_UNSUPPORTED;       // buffer-descriptor rows only
    int rr = check_tensors({{value, 16}, {out, 16}, maybe(token, 16), {scale, 16, fp8}, {shapes, 1}, {start, 1}, {off_q, 1},
                            {att_q, 1}, {off_tab, 1}, {att_tab, 1}, {relpos, 1}, {ref, 1}, {ratios, 1}});
    if (rr) return rr;
    // token rows of off_q / att_q: packed, or ld elements apart (columns of one wider matrix); vector loads of P
    // (2 P) elements need the rows aligned like the packed ones -- to the whole row of a point, not heads_rows' 16 bytes
    if ((rr = rows_range(ld_off, H * 2 * P)) || (rr = rows_range(ld_att, H * L * P)) ||
        (rr = rows_aligned(ld_off, es, off_q, 2 * P * es)) || (rr = rows_aligned(ld_att, es, att_q, P * es)))
        return rr;
    pd.ld_off = (int)ld_off; pd.ld_att = (int)ld_att;
    d.B = (int)N; d.S = (int)S; d.H = (int)H; d.D = (int)D; d.L = (int)(n * L); d.Nq = (int)Lq; d.P = (int)P;
    d.K = d.L * d.P; d.lazy_attn = 0; d.blocks4 = 0;
    int G = 4;
    while (G < d.L) G *= 2;                                                 // the plan kernel's lane-group width
    hipStream_t st = (hipStream_t)stream;
    auto go = [&](auto tag_t, auto tag_b, auto tag_lpi, auto tag_p) {
        typedef decltype(tag_t) T;
        typedef decltype(tag_b) BT;
        constexpr int LPI = decltype(tag_lpi)::value, PP = decltype(tag_p)::value;
        constexpr int QPB = kThreads / LPI;
        Dims dd = d;
        dd.q_tiles = (d.Nq + QPB - 1) / QPB;
        const int64_t blocks = (int64_t)d.B * dd.q_tiles * d.H;
        if (blocks > 0x7fffffffLL) return (int)MMFS_E_DIMS;
        hipLaunchKernelGGL((mmfs_sample_fwd<T, LPI, PP, BT>), dim3((unsigned)blocks), dim3(kThreads), 0, st,
                           (const BT *)value, shapes, start, (const T *)off_q, (const T *)att_q,
                           (const T *)off_tab, (const T *)att_tab, relpos, ref, ratios, (T *)out, sink, dd, pd, G,
                           (const T *)token, scale);
        return (int)hipGetLastError();
    };
    auto go_decode = [&](auto tag_t, auto tag_b, auto tag_lpi, auto tag_p) {
        typedef decltype(tag_t) T;
        typedef decltype(tag_b) BT;
        constexpr int LPI = decltype(tag_lpi)::value, PP = decltype(tag_p)::value;
        if constexpr (LPI <= 32) {
            hipLaunchKernelGGL((mmfs_sample_decode<T, LPI, PP, BT>), dim3((unsigned)(d.B * d.Nq * d.H)), dim3(64), 0, st,
                               (const BT *)value, shapes, start, (const T *)off_q, (const T *)att_q,
                               (const T *)off_tab, (const T *)att_tab, relpos, ref, ratios, (T *)out, sink, d, pd, G,
                               (const T *)token, scale);
            return (int)hipGetLastError();
        } else {
            return (int)MMFS_E_UNSUPPORTED;
        }
    };
    const bool decode = sample_groups(Lq, d.K, d.L, lpi) > 1;
    auto by_p = [&](auto tag_t, auto tag_b, auto tag_lpi) {
        return by_int<4, 8>(P, [&](auto tag_p) {
            return decode ? go_decode(tag_t, tag_b, tag_lpi, tag_p) : go(tag_t, tag_b, tag_lpi, tag_p);
        });
    };
    auto by_lpi = [&](auto tag_t) {
        typedef decltype(tag_t) T;
        if (fp8)                                                           // (16 channels per lane: D = 16 .. 256)
            return by_int<1, 2, 4, 8, 16>(lpi, [&](auto tag_lpi) { return by_p(tag_t, fp8e4m3_t{}, tag_lpi); });
        return by_int<1, 2, 4, 8, 16, 32, 64>(lpi, [&](auto tag_lpi) { return by_p(tag_t, T{}, tag_lpi); });
    };
    return by_type(dtype, by_lpi);
}

int mmfs_sample_forward_groups(int dtype, int64_t Lq, int64_t D, int64_t nL, int64_t P)
{
    const int es = mmfs::elem_size(dtype);
    if (!es || D <= 0 || D % (16 / es) || (P != 4 && P != 8) || nL <= 0 || Lq <= 0) return 0;
    const int64_t lpi = D / (16 / es);
    if (lpi > 64 || (lpi & (lpi - 1))) return 0;
    return mmfs::sample_groups(Lq, nL * P, nL, (int)lpi);
}

}  // extern "C"
