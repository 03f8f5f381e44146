// msda_gather.h -- the row-gather sampler core: what msda_fwd_vec (csrc/msda_fwd.hip), mmfs_sample_fwd /
// mmfs_sample_decode (csrc/mmfs_plan.hip) and deform_sample_fwd (csrc/msda_deform_plan.hip) do once a sample's
// location and weight are known.  The hosts differ in where those come from (tensors, or a plan evaluated in the
// kernel), in their LDS declarations and in their epilogue; the tap record, the walks over the records and the sums
// are these functions, so the fused samplers equal plan + op bit for bit by construction.
//
// A tap record is two uint4 in LDS: the byte offsets of the sample's four pixel rows in the workgroup's (batch, head)
// slab (kOobOffset for a corner that reads nothing: the buffer descriptor answers 0 without touching memory), and the
// four corner weights already multiplied by the attention weight.
#pragma once
#include "msda_device.h"

namespace mmfs {

// location + weight -> tap record.  A zero attention weight (an image the token cannot see: the masked softmax gives
// exactly 0, mmfs.py:203-231) reads no rows at all -- every corner is marked "outside".
__device__ __forceinline__ void tap_record(float lx, float ly, float a, int Hl, int Wl, int lstart, uint32_t row_bytes,
                                           uint4 &rows, uint4 &ww)
{
    const Tap<float> t = locate<float>(lx, ly, Hl, Wl, lstart);
    const float gy = 1.f - t.fy, gx = 1.f - t.fx;
    int row[4] = {-1, -1, -1, -1};
    if (a != 0.f) {
        row[0] = t.row[0]; row[1] = t.row[1]; row[2] = t.row[2]; row[3] = t.row[3];
    }
    uint32_t off[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)      // pixel row -> byte offset in the slab, or "outside"
        off[c] = row[c] >= 0 ? (uint32_t)row[c] * row_bytes : kOobOffset;
    rows = make_uint4(off[0], off[1], off[2], off[3]);
    ww = make_uint4(__float_as_uint(gy * gx * a), __float_as_uint(gy * t.fx * a),
                    __float_as_uint(t.fy * gx * a), __float_as_uint(t.fy * t.fx * a));
}

// the record of a sample that does not exist (padding, a query past the end)
__device__ __forceinline__ void tap_record_none(uint4 &rows, uint4 &ww)
{
    rows = make_uint4(kOobOffset, kOobOffset, kOobOffset, kOobOffset);
    ww = make_uint4(0u, 0u, 0u, 0u);
}

// does the record weigh anything?  (sign bit aside: -0 is zero too)
__device__ __forceinline__ bool tap_weighs(const uint4 &ww) { return ((ww.x | ww.y | ww.z | ww.w) << 1) != 0u; }

// Live words: bit kk of a wave's word says that sample kk of the chunk weighs something for at least one query of
// the wave.  Set with mark_live while staging; the gather walks the set bits, so a tap nobody needs is never issued
// and the walk has a counted trip -- the shape the compiler's wait-count pass pipelines cleanly.
// QPW: queries per wave.
template <int QPW>
__device__ __forceinline__ void mark_live(unsigned long long *live, int rq, int kk, const uint4 &ww)
{
    if (tap_weighs(ww)) atomicOr(&live[rq / QPW], 1ull << kk);
}

// a wave's word as a wave-uniform value, and the word cleared (mine; the next chunk's staging sets it after the barrier)
__device__ __forceinline__ unsigned long long take_live(unsigned long long *live, int tid)
{
    const int wv = tid >> 6;
    const unsigned long long mraw = live[wv];
    const unsigned long long m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(mraw >> 32)) << 32) |
                                 (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)mraw);
    if ((tid & 63) == 0) live[wv] = 0ull;
    return m;
}

// a record's four row reads: this lane's 16 bytes of each
__device__ __forceinline__ void load_rows(__amdgpu_buffer_rsrc_t rsrc, const uint4 &rows, uint32_t lane_off, uint4 (&raw)[4])
{
    raw[0] = buffer_load16(rsrc, rows.x + lane_off);
    raw[1] = buffer_load16(rsrc, rows.y + lane_off);
    raw[2] = buffer_load16(rsrc, rows.z + lane_off);
    raw[3] = buffer_load16(rsrc, rows.w + lane_off);
}

// four rows x four weights into acc, corner by corner (V = Vec16 of the bank's type)
template <typename V>
__device__ __forceinline__ void fma_rows(const uint4 (&raw)[4], const uint4 &ww, float (&acc)[V::N])
{
    const float w4[4] = {__uint_as_float(ww.x), __uint_as_float(ww.y), __uint_as_float(ww.z), __uint_as_float(ww.w)};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float v[V::N];
        V::unpack(raw[c], v);
#pragma unroll
        for (int i = 0; i < V::N; ++i) acc[i] = fmaf(w4[c], v[i], acc[i]);
    }
}

// The walk over a wave's live records (m: take_live's word; recs: the lane's query's records), software-pipelined:
// the 4 row reads of the next live tap are in flight while the current one is multiplied (4..8 reads in flight per
// lane).  Sums in sample order.
template <typename V>
__device__ __forceinline__ void gather_live(unsigned long long m, const uint4 *recs, __amdgpu_buffer_rsrc_t rsrc,
                                            uint32_t lane_off, float (&acc)[V::N])
{
    uint4 rawA[4], rawB[4], wA, wB;
    auto issue = [&](uint4 (&raw)[4], uint4 &ww) {
        const int kk = __builtin_ctzll(m);
        m &= m - 1ull;
        const uint4 rr = recs[2 * kk];
        ww = recs[2 * kk + 1];
        load_rows(rsrc, rr, lane_off, raw);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto consume = [&](const uint4 (&raw)[4], const uint4 &ww) {
        fma_rows<V>(raw, ww, acc);
#pragma unroll
        for (int i = 0; i < V::N; ++i) asm volatile("" : "+v"(acc[i]));     // the sums are due HERE, not after the next reads
        __builtin_amdgcn_sched_barrier(0);
    };
    const int n_live = __builtin_popcountll(m);
    if (n_live & 1) { issue(rawA, wA); consume(rawA, wA); }
    if (n_live >= 2) {
        issue(rawA, wA);
        for (int i = 2; i < n_live - 1; i += 2) {
            issue(rawB, wB);
            consume(rawA, wA);
            issue(rawA, wA);
            consume(rawB, wB);
        }
        issue(rawB, wB);
        consume(rawA, wA);
        consume(rawB, wB);
    }
}

// The walk without the live word (chunks of more than 64 samples per query): records [0, n) of the lane's query,
// UNROLL taps (4 * UNROLL row reads) in flight per lane; n is a multiple of UNROLL.  When every tap of every query of
// the wave weighs zero (consecutive tokens share what they can see, so whole waves are blind to an image) there is
// nothing to read and nothing to add: an "outside" row costs no data but its load still costs the address path its
// cycles.  Call with the lanes whose query exists.
template <typename V, int UNROLL>
__device__ __forceinline__ void gather_all(const uint4 *recs, int n, __amdgpu_buffer_rsrc_t rsrc, uint32_t lane_off,
                                           float (&acc)[V::N])
{
    for (int kk = 0; kk < n; kk += UNROLL) {
        uint4 raw[UNROLL][4];
        float w[UNROLL][4];
        uint4 rrs[UNROLL];
        uint32_t any_w = 0u;
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            rrs[u] = recs[2 * (kk + u)];
            const uint4 ww = recs[2 * (kk + u) + 1];
            any_w |= (ww.x | ww.y | ww.z | ww.w) << 1;          // (sign bit aside: -0 is zero too)
            w[u][0] = __uint_as_float(ww.x); w[u][1] = __uint_as_float(ww.y);
            w[u][2] = __uint_as_float(ww.z); w[u][3] = __uint_as_float(ww.w);
        }
        if (__builtin_amdgcn_ballot_w64(any_w != 0u) == 0ull) continue;
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) load_rows(rsrc, rrs[u], lane_off, raw[u]);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float v[V::N];
                V::unpack(raw[u][c], v);
#pragma unroll
                for (int i = 0; i < V::N; ++i) acc[i] = fmaf(w[u][c], v[i], acc[i]);
            }
    }
}

// The sinks' share goes to the ignore token (mmfs.py:236-241, 274): out + token * sink, with the framework statement's
// roundings -- sampled output, sink weight and product each rounded to the storage type first.  Two roundings, as the
// framework's two kernels: the product must not be contracted into the sum -- __fmul_rn / __fadd_rn do not stop this
// compiler, an opaque register does.  token: the lane's VEC channels of the head's token row.
template <typename T, int VEC>
__device__ __forceinline__ void add_ignore_token(float (&acc)[VEC], const T *token, float sink_sum)
{
    const float sw = to_f32((T)sink_sum);
    float tk[VEC];
    load_vec<T, VEC>(token, tk);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        float prod = tk[i] * sw;
        asm volatile("" : "+v"(prod));
        acc[i] = to_f32((T)acc[i]) + to_f32((T)prod);
    }
}

}  // namespace mmfs
