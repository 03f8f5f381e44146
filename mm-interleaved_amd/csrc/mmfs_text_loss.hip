// mmfs_text_loss.hip -- the text loss of the training step on the device: the cross-entropy of the text
// decoder's logits [B, L, V], read once in their storage type, and its gradient, written once.
//
// The reference (mm_interleaved/models/mm_interleaved.py:449-476) casts the logits to fp32, permutes them to [B, V, L],
// slices and copies, and hands the copy to F.cross_entropy: an fp32 copy, a permuted copy, an fp32 log_softmax and, going
// back, an fp32 gradient, a permuted copy and a cast -- about ten row-sized passes.  The mathematics needs three: one
// read forward, one read and one write backward.  Nothing returns to the host, sizes travel by value, nothing is
// allocated: the launches can be captured into a graph.
//
// Row (b, first + j) of the logits, j < n, is scored against labels[b, j]; first + n <= L.  A label is VALID when it is
// not ignore_index and lies in [0, V); a label that is neither ignore_index nor inside [0, V) is OUT OF RANGE: its row is
// treated as ignored (no element of the row is read through it) and counted.
//
//   text_loss_fwd     one workgroup of 256 lanes per scored row.  An ignored or out-of-range row is not read:
//                     lse = loss = 0.  Otherwise one pass with a running (m, s) per lane, s = sum exp(x - m):
//                         m' = max(m, max of the vector);  base = m' == -Inf ? 0 : m'
//                         s  = s exp(m - base) + sum_e exp(x_e - base);  m = m'
//                     exp(m - base) is exp(0) = 1 exactly while the maximum stands.  ``base`` keeps -Inf out of the
//                     subtractions: a lane that has seen only -Inf holds (m, s) = (-Inf, 0) and stays there, and
//                     (-Inf, 0) joins a finite pair with weight exp(-Inf) = 0.  +Inf and NaN entries give NaN, as
//                     x - max(x) does in the fp32 statement; a row of -Inf alone gives lse = -Inf and loss = NaN there
//                     too.  A lane loads 16 bytes; with V odd and 2-byte elements a row starts on any 2-byte boundary, so
//                     each row peels the elements before its first 16-byte boundary (head) and behind its last (tail),
//                     one element per lane, and its body loads are aligned.  Lanes are combined by wave shuffles
//                     (offsets 32 .. 1 downwards, lane 0 holds the wave's pair), the four waves through LDS in
//                     ascending order.  lse = m + logf(s);  loss = lse - x[label].
//   text_loss_reduce  one workgroup of 1024 lanes: lane t adds rows t, t + 1024, .. in ascending order, the 64 lanes of a
//                     wave by shuffles, the 16 waves in ascending order; valid and out-of-range rows are counted as
//                     integers.  out[0] = sum / n_valid (mean; 0 / 0 = NaN when every row is ignored) or the sum;
//                     counts = {n_valid, n_out_of_range}.  No atomics, nothing to clear: bit-reproducible.
//   text_loss_bwd     one workgroup per row of the whole [B, L] grid; every element of grad is written.  A scored, valid
//                     row:  grad[i] = round_T((exp(x[i] - lse) - [i == label]) g),  g = up[0] / n_valid (mean),
//                     up[0] (sum) or up[row] (none), read from device memory.  Every other row: zeros.
//                     Store policy: the NON-TEMPORAL hint.  The head's GEMM reads the gradient next; measured against
//                     plain stores, forward + backward + that product at [2, 2048, 32003] took 1.056 against 1.059 ms in
//                     bf16 (level: the spread is 0.015) and 7.27 against 7.44 ms in f32, forward + backward alone 0.170
//                     against 0.206 ms in bf16 and 0.328 against 0.339 ms in f32 (profiles/text_loss.md).  The plain
//                     variant lost or tied everywhere and is gone.
//
// exp(d) is v_exp_f32(d * log2(e)) -- the hardware's base-2 exponential, 1 unit in the last place (2^-23 relative) with
// denormal results flushed to 0 (AMD "Graphics Core Next Architecture, Generation 3" ISA reference, VOP1 V_EXP_F32: "1ULP
// accuracy, denormals are flushed"; the CDNA guides list the same opcode).  log is the device library's logf (once per
// row), which the HIP documentation's table of math functions lists at 1 unit; the bounds allow 2.
//
// Error bounds (what tests/test_text_loss_gpu.py holds the results to, against fp64 on the stored logits; units of
// 2^-24 =: e, first order; the maximum m is exact):
//   one term exp(x - base):  the subtraction e |d|, log2(e) rounded (e / 2) |d|, the product e |d|, the instruction 2 e:
//       relative (2.5 |d| + 2) e.  A later change of the maximum multiplies by exp(m - m'): the exponents of a term's
//       factors add up to x - M (M the row's maximum) exactly, so ALL its exponent errors together are 2.5 e (M - x);
//       weighted by the term's share p of s:  2.5 e D,  D = sum_i p_i (M - x_i).
//   roundings a term passes besides: its own instruction (2), the vector's sum (at most 8 additions: 8), then per later step
//       of its lane the factor's instruction (2), the product (1), the addition (1): 4 per step, and 5 per combine step
//       (two factors of which one is exact, two products, one addition).
//       steps of a lane   n = 1 (the peeled element) + ceil(floor(V / VEC) / 256)      VEC = 16 bytes / sizeof(T)
//       combine steps     c = 6 (shuffles) + 3 (waves)
//       a term below 2^-126 is flushed to 0: V 2^-126 against s >= 1 (the maximum's own term is exp(0) = 1)
//       => s is relative  (2.5 D + 10 + 4 n + 5 c) e + V 2^-126
//   lse = m + logf(s):  d(log s) = ds / s;  logf 2 units of |log s|: 4 e |log s|;  the sum e |lse|
//       |lse - ref| <= (2.5 D + 10 + 4 n + 5 c) e + V 2^-126 + 4 e |log s| + e |lse|                   =: E_lse
//   loss = lse - x[label]:  E_loss = E_lse + e |loss|
//   mean / sum:  a lane's chain ceil(rows / 1024), 6 shuffle steps, 15 wave steps, the quotient (2.5 units):
//       |out - ref| <= sum_r E_loss(r) / N + (ceil(rows / 1024) + 21 + 3) e sum_r |loss_r| / N       (N = 1 for the sum)
//   grad:  p = exp(x - lse): (2.5 |x - lse| + 2) e p + E_lse p;  p - [i == label]: e |p - [..]|;  g = up / n_valid: 3 e
//       (the quotient of an exact integer, 2.5 units, rounded up);  the product e;  one rounding to T (u_T, t_T):
//       a p below 2^-126 is flushed to 0:
//       |grad - ref| <= u_T |ref| + t_T + |g| (p ((2.5 |x - lse| + 2) e + E_lse) + 5 e |p - [i == label]| + 2^-126)
//
// Offsets are 64-bit: B L V passes 2^31 elements at ordinary batch sizes.
#include "mmfs_attn_core.h"
#include <hip/hip_runtime.h>

namespace mmfs {

namespace {

using attn::exp_hw;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kReduceThreads = 1024;
constexpr int64_t kMaxRows = 1 << 22;           // B * L at most
constexpr int64_t kMaxVocab = 1 << 24;

enum { kNone = 0, kSum = 1, kMean = 2 };        // ``reduction`` of the two entries

// 0: ignored, 1: valid, 2: out of range
__device__ __forceinline__ int label_class(int64_t label, int64_t ignore_index, int V)
{
    if (label == ignore_index) return 0;
    return label >= 0 && label < V ? 1 : 2;
}

// the running pair of a lane / a wave
struct Lse { float m, s; };

__device__ __forceinline__ float base_of(float m) { return m == -INFINITY ? 0.f : m; }

__device__ __forceinline__ void join(Lse &a, float m, float s)
{
    const float mm = fmaxf(a.m, m), base = base_of(mm);
    a.s = a.s * exp_hw(a.m - base) + s * exp_hw(m - base);
    a.m = mm;
}

template <int VEC> __device__ __forceinline__ void take(Lse &a, const float (&v)[VEC])
{
    float vm = v[0];
#pragma unroll
    for (int e = 1; e < VEC; ++e) vm = fmaxf(vm, v[e]);
    const float mm = fmaxf(a.m, vm), base = base_of(mm);
    float acc = 0.f;
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc += exp_hw(v[e] - base);
    a.s = a.s * exp_hw(a.m - base) + acc;
    a.m = mm;
}

// a row of V elements of T at ``row``: head elements before the first 16-byte boundary, nvec aligned vectors, tail elements
struct Peel { int head, nvec, tail; };

template <typename T> __device__ __forceinline__ Peel peel_of(const T *row, int V)
{
    constexpr int VEC = Vec16<T>::N;
    Peel p;
    const int to_boundary = (int)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) / sizeof(T));
    p.head = to_boundary < V ? to_boundary : V;
    p.nvec = (V - p.head) / VEC;
    p.tail = V - p.head - p.nvec * VEC;
    return p;
}

// the element a lane peels (tid < head + tail), as its index in the row
__device__ __forceinline__ int peeled_index(const Peel &p, int tid, int vec)
{
    return tid < p.head ? tid : p.head + p.nvec * vec + (tid - p.head);
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
text_loss_fwd(const T *__restrict__ x, const int64_t *__restrict__ labels, float *__restrict__ loss, float *__restrict__ lse,
              const int L, const int V, const int first, const int n, const int64_t ignore_index)
{
    constexpr int VEC = Vec16<T>::N;
    __shared__ float wave_m[kWaves], wave_s[kWaves];
    const int r = blockIdx.x, b = r / n, j = r - b * n;          // scored row r = (b, j)
    const int tid = threadIdx.x;
    const int64_t label = labels[r];
    if (label_class(label, ignore_index, V) != 1) {
        if (tid == 0) { loss[r] = 0.f; lse[r] = 0.f; }
        return;
    }
    const T *row = x + ((int64_t)b * L + first + j) * V;
    const Peel p = peel_of(row, V);
    Lse a = {-INFINITY, 0.f};
    if (tid < p.head + p.tail) {
        const float v[1] = {to_f32(row[peeled_index(p, tid, VEC)])};
        take<1>(a, v);
    }
    const T *body = row + p.head;
#pragma unroll 2
    for (int k = tid; k < p.nvec; k += kThreads) {
        float v[VEC];
        load_vec<T, VEC>(body + (int64_t)k * VEC, v);
        take<VEC>(a, v);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float m = __shfl_down(a.m, o, 64), s = __shfl_down(a.s, o, 64);
        join(a, m, s);
    }
    if ((tid & 63) == 0) { wave_m[tid >> 6] = a.m; wave_s[tid >> 6] = a.s; }
    __syncthreads();
    if (tid == 0) {
        Lse t = {wave_m[0], wave_s[0]};
#pragma unroll
        for (int w = 1; w < kWaves; ++w) join(t, wave_m[w], wave_s[w]);
        const float l = t.m + logf(t.s);
        lse[r] = l;
        loss[r] = l - to_f32(row[label]);
    }
}

__global__ void __launch_bounds__(kReduceThreads)
text_loss_reduce(const float *__restrict__ loss, const int64_t *__restrict__ labels, float *__restrict__ out,
                 int32_t *__restrict__ counts, const int rows, const int V, const int64_t ignore_index, const int reduction)
{
    __shared__ float wave_sum_[kReduceThreads / 64];
    __shared__ int wave_valid[kReduceThreads / 64], wave_bad[kReduceThreads / 64];
    const int tid = threadIdx.x;
    float sum = 0.f;
    int valid = 0, bad = 0;
    for (int r = tid; r < rows; r += kReduceThreads) {
        const int c = label_class(labels[r], ignore_index, V);
        valid += c == 1;
        bad += c == 2;
        if (out) sum += loss[r];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        sum += __shfl_down(sum, o, 64);
        valid += __shfl_down(valid, o, 64);
        bad += __shfl_down(bad, o, 64);
    }
    if ((tid & 63) == 0) { wave_sum_[tid >> 6] = sum; wave_valid[tid >> 6] = valid; wave_bad[tid >> 6] = bad; }
    __syncthreads();
    if (tid == 0) {
        float total = wave_sum_[0];
        int nv = wave_valid[0], nb = wave_bad[0];
        for (int w = 1; w < kReduceThreads / 64; ++w) { total += wave_sum_[w]; nv += wave_valid[w]; nb += wave_bad[w]; }
        if (out) out[0] = reduction == kMean ? total / (float)nv : total;
        counts[0] = nv;
        counts[1] = nb;
    }
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
text_loss_bwd(const T *__restrict__ x, const int64_t *__restrict__ labels, const float *__restrict__ lse,
              const float *__restrict__ up, const int32_t *__restrict__ counts, T *__restrict__ grad, const int L, const int V,
              const int first, const int n, const int64_t ignore_index, const int reduction)
{
    constexpr int VEC = Vec16<T>::N;
    const int row_id = blockIdx.x, b = row_id / L, j = row_id - b * L - first;
    const int tid = threadIdx.x;
    const bool scored = j >= 0 && j < n;
    const int r = scored ? b * n + j : 0;
    const int64_t label = scored ? labels[r] : ignore_index;
    const bool valid = scored && label_class(label, ignore_index, V) == 1;
    const int64_t off = (int64_t)row_id * V;
    T *grow = grad + off;
    const Peel p = peel_of(grow, V);             // (x and grad are both 16-byte aligned: one peel serves the two rows)
    T *gbody = grow + p.head;
    if (!valid) {
        if (tid < p.head + p.tail) store_stream<T>(grow + peeled_index(p, tid, VEC), (T)0.f);
        float z[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) z[e] = 0.f;
        for (int k = tid; k < p.nvec; k += kThreads) store_vec<T, VEC, true>(gbody + (int64_t)k * VEC, z);
        return;
    }
    const float l = lse[r];
    const float g = reduction == kNone ? up[r] : reduction == kMean ? up[0] / (float)counts[0] : up[0];
    const int lab = (int)label;
    const T *row = x + off;
    if (tid < p.head + p.tail) {
        const int i = peeled_index(p, tid, VEC);
        store_stream<T>(grow + i, (T)((exp_hw(to_f32(row[i]) - l) - (i == lab ? 1.f : 0.f)) * g));
    }
    const T *body = row + p.head;
#pragma unroll 2
    for (int k = tid; k < p.nvec; k += kThreads) {
        float v[VEC];
        load_vec<T, VEC>(body + (int64_t)k * VEC, v);
        const int i0 = p.head + k * VEC;
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = (exp_hw(v[e] - l) - (i0 + e == lab ? 1.f : 0.f)) * g;
        store_vec<T, VEC, true>(gbody + (int64_t)k * VEC, v);
    }
}

bool supported(int es, int64_t V) { return es && V >= 1 && V <= kMaxVocab; }

int check(int dtype, int64_t B, int64_t L, int64_t V, int64_t first, int64_t n, int reduction)
{
    const int es = elem_size(dtype);
    if (!es) return MMFS_E_DTYPE;
    if (B < 0 || L < 0 || V < 0 || first < 0 || n < 0 || first > L || n > L - first) return MMFS_E_DIMS;
    if (B > kMaxRows || L > kMaxRows || B * L > kMaxRows || V > kMaxVocab) return MMFS_E_DIMS;
    if (reduction != kNone && reduction != kSum && reduction != kMean) return MMFS_E_UNSUPPORTED;
    if (B * L && !supported(es, V)) return MMFS_E_UNSUPPORTED;
    return MMFS_OK;
}

}  // namespace
}  // namespace mmfs

extern "C" {

int mmfs_text_loss_supported(int dtype, int64_t V) { return mmfs::supported(mmfs::elem_size(dtype), V); }

int mmfs_text_loss_forward(int dtype, const void *logits, const int64_t *labels, float *loss, float *lse, float *out,
                           int32_t *counts, int64_t B, int64_t L, int64_t V, int64_t first, int64_t n, int64_t ignore_index,
                           int reduction, void *stream)
{
    using namespace mmfs;
    const int rc = check(dtype, B, L, V, first, n, reduction);
    if (rc) return rc;
    const int64_t rows = B * n;
    const bool any = rows != 0;
    if (const int rt = check_tensors({{counts, 4}, {out, 4, reduction != kNone}, {logits, 16, any}, {labels, 8, any}, {loss, 4, any},
                                      {lse, 4, any}}))
        return rt;
    if (rows) {
        const int e = by_type(dtype, [&](auto tag) {
            typedef decltype(tag) T;
            hipLaunchKernelGGL((text_loss_fwd<T>), dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream,
                               (const T *)logits, labels, loss, lse, (int)L, (int)V, (int)first, (int)n, ignore_index);
            return (int)hipGetLastError();
        });
        if (e) return e;
    }
    hipLaunchKernelGGL(text_loss_reduce, dim3(1), dim3(kReduceThreads), 0, (hipStream_t)stream, loss, labels,
                       reduction == kNone ? nullptr : out, counts, (int)rows, (int)V, ignore_index, reduction);
    return (int)hipGetLastError();
}

int mmfs_text_loss_backward(int dtype, const void *logits, const int64_t *labels, const float *lse, const float *upstream,
                            const int32_t *counts, void *grad, int64_t B, int64_t L, int64_t V, int64_t first, int64_t n,
                            int64_t ignore_index, int reduction, void *stream)
{
    using namespace mmfs;
    const int rc = check(dtype, B, L, V, first, n, reduction);
    if (rc) return rc;
    if (B * L == 0) return MMFS_OK;
    const bool any = B * n != 0;
    if (const int rt = check_tensors({{grad, 16}, {logits, 16, any}, {labels, 8, any}, {lse, 4, any}, {upstream, 4, any},
                                      {counts, 4, any && reduction == kMean}}))
        return rt;
    return by_type(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL((text_loss_bwd<T>), dim3((unsigned)(B * L)), dim3(kThreads), 0, (hipStream_t)stream,
                           (const T *)logits, labels, lse, upstream, counts, (T *)grad, (int)L, (int)V, (int)first, (int)n,
                           ignore_index, reduction);
        return (int)hipGetLastError();
    });
}

}  // extern "C"
