// mmfs_bank_fp8.hip -- the fp8 (OCP e4m3) value bank's quantiser (include/mmfs_msda.h "fp8 bank").
//
// x [nbanks * Bv, R, C] (f32 / f16 / bf16) -> q [nbanks * Bv, R, C] e4m3 and scale [nbanks * Bv, C] fp32, with one scale
// per (bank row, column):
//     amax = max |x| over the finite elements of the column;  scale = amax / 448;
//     q = e4m3(RNE(clamp(x / scale, -448, 448)));  scale == 0 -> +0;  x not finite -> 0x7f (NaN)
// Four launches on the stream, for any number of banks:
//   1  mmfs::zero_fill of scale (a kernel: a memset node inside a graph is not ordered like one)
//   2  column maxima: a lane reads 16 columns of kRowsPerItem rows and atomicMax'es the bit patterns of its nonnegative
//      maxima into scale (the order of the maxima does not matter: deterministic)
//   3  scale = amax / 448 in place
//   4  quantise: a lane turns 16 elements into 16 bytes (one 16-byte store), 8 v_cvt_pk_fp8_f32
#include "../../include/mmfs_msda.h"
#include "msda_device.h"
#include "msda_launch.h"
#include <cfloat>

namespace mmfs {
namespace {

constexpr int kQThreads = 256;
constexpr int kRowsPerItem = 64;        // rows a lane folds into its 16 column maxima before the atomics
constexpr float kE4m3Max = 448.f;
constexpr uint32_t kE4m3NaN = 0x7fu;

// 16 consecutive elements of x as fp32
template <typename X>
__device__ __forceinline__ void load16(const X *p, float (&v)[16])
{
    load_vec<X, 16>(p, v);
}

template <typename X>
__global__ void __launch_bounds__(kQThreads)
bank_amax_kernel(const X *__restrict__ x, uint32_t *__restrict__ amax, int64_t rows, int64_t R, int64_t C)
{
    const int64_t CG = C / 16, RC = (R + kRowsPerItem - 1) / kRowsPerItem;
    const int64_t items = rows * RC * CG;
    for (int64_t it = (int64_t)blockIdx.x * kQThreads + threadIdx.x; it < items; it += (int64_t)gridDim.x * kQThreads) {
        const int64_t cg = it % CG, rc = (it / CG) % RC, row = it / CG / RC;
        const int64_t r0 = rc * kRowsPerItem, r1 = min(R, r0 + kRowsPerItem);
        float m[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) m[i] = 0.f;
        const X *p = x + (row * R + r0) * C + cg * 16;
        for (int64_t r = r0; r < r1; ++r, p += C) {
            float v[16];
            load16<X>(p, v);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float a = fabsf(v[i]);
                m[i] = a <= FLT_MAX && a > m[i] ? a : m[i];          // (NaN and inf fail the first test)
            }
        }
        uint32_t *dst = amax + row * C + cg * 16;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (m[i] > 0.f) atomicMax(dst + i, __float_as_uint(m[i]));
    }
}

__global__ void __launch_bounds__(kQThreads) bank_scale_kernel(float *__restrict__ scale, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * kQThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kQThreads)
        scale[i] = scale[i] / kE4m3Max;               // (the amax bit pattern is the float itself)
}

__device__ __forceinline__ float clamp448(float y) { return fminf(fmaxf(y, -kE4m3Max), kE4m3Max); }

// two elements -> two e4m3 codes in byte pair HI of w
template <bool HI>
__device__ __forceinline__ int q2(float xa, float xb, float sa, float sb, int w)
{
    const float ya = sa != 0.f ? clamp448(xa / sa) : 0.f, yb = sb != 0.f ? clamp448(xb / sb) : 0.f;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(ya, yb, w, HI);
    constexpr int sh = HI ? 16 : 0;
    // a non-finite element is NaN, not clamped (fminf / fmaxf would make it 448)
    if (!(fabsf(xa) <= FLT_MAX)) w = (w & ~(0xff << sh)) | (int)(kE4m3NaN << sh);
    if (!(fabsf(xb) <= FLT_MAX)) w = (w & ~(0xff << (sh + 8))) | (int)(kE4m3NaN << (sh + 8));
    return w;
}

template <typename X>
__global__ void __launch_bounds__(kQThreads)
bank_quantize_kernel(const X *__restrict__ x, const float *__restrict__ scale, uint8_t *__restrict__ q,
                     int64_t rows, int64_t R, int64_t C)
{
    const int64_t CG = C / 16;
    const int64_t items = rows * R * CG;
    for (int64_t it = (int64_t)blockIdx.x * kQThreads + threadIdx.x; it < items; it += (int64_t)gridDim.x * kQThreads) {
        const int64_t cg = it % CG, rr = it / CG, row = rr / R;        // rr = row * R + r
        float v[16], s[16];
        load16<X>(x + rr * C + cg * 16, v);
        load_vec<float, 16>(scale + row * C + cg * 16, s);
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int t = q2<false>(v[4 * j], v[4 * j + 1], s[4 * j], s[4 * j + 1], 0);
            t = q2<true>(v[4 * j + 2], v[4 * j + 3], s[4 * j + 2], s[4 * j + 3], t);
            w[j] = (uint32_t)t;
        }
        *reinterpret_cast<uint4 *>(q + rr * C + cg * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

unsigned grid_for(int64_t items)
{
    return (unsigned)std::min<int64_t>(std::max<int64_t>(1, (items + kQThreads - 1) / kQThreads), 256 * 64);
}

template <typename X>
hipError_t quantize(const void *x, int64_t rows, int64_t R, int64_t C, void *q, float *scale, hipStream_t st)
{
    hipError_t e = zero_fill(scale, (size_t)(rows * C) * sizeof(float), st);
    if (e != hipSuccess) return e;
    const int64_t amax_items = rows * ((R + kRowsPerItem - 1) / kRowsPerItem) * (C / 16);
    hipLaunchKernelGGL((bank_amax_kernel<X>), dim3(grid_for(amax_items)), dim3(kQThreads), 0, st,
                       (const X *)x, (uint32_t *)scale, rows, R, C);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(bank_scale_kernel, dim3(grid_for(rows * C)), dim3(kQThreads), 0, st, scale, rows * C);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL((bank_quantize_kernel<X>), dim3(grid_for(rows * R * (C / 16))), dim3(kQThreads), 0, st,
                       (const X *)x, (const float *)scale, (uint8_t *)q, rows, R, C);
    return hipGetLastError();
}

}  // namespace
}  // namespace mmfs

extern "C" int mmfs_bank_quantize_fp8(int dtype, const void *x, int64_t nbanks, int64_t Bv, int64_t R, int64_t C,
                                      void *q, float *scale, void *stream)
{
    using namespace mmfs;
    if (!elem_size(dtype)) return MMFS_E_DTYPE;
    const int64_t lim = 0x7fffffffLL;
    if (nbanks < 0 || Bv < 0 || R < 0 || C < 0 || nbanks > lim || Bv > lim || R > lim || C > lim) return MMFS_E_DIMS;
    if (C % 16) return MMFS_E_UNSUPPORTED;                                   // (C = H*D, D a multiple of 16)
    const int64_t rows = nbanks * Bv;
    if (rows == 0 || C == 0) return MMFS_OK;
    if (const int rc = check_tensors({{x, 16}, {q, 16}, {scale, 16}})) return rc;
    hipStream_t st = (hipStream_t)stream;
    return (int)by_type(dtype, [&](auto t) { return quantize<decltype(t)>(x, rows, R, C, q, scale, st); });
}
