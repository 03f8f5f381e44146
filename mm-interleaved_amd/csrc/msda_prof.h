// msda_prof.h -- the phase clock of the kernels' development builds (tools/exp_build.sh NAME "-DMMFS_PROFILE_..."):
// shader clocks per phase, kept in registers and flushed once at the end (an atomic per phase would sit in the very
// vmcnt queue the phases wait on), one row of counters per workgroup modulo the slots -- no contended atomics --
// summed by the host readout behind the file's extern "C" mmfs_debug_*_profile.
//
// A translation unit says what is its own BEFORE it includes this header:
//     #ifdef MMFS_PROFILE_<ITS SWITCH>
//     #define MMFS_PROF_COUNTERS g_..._prof        // the counter symbol; left undefined, every macro below is a no-op
//     #endif
//     #define MMFS_PROF_SLOTS 4096                 // rows of counters
//     #define MMFS_PROF_N 8                        // counters per row
//     #define MMFS_PROF_LANE ((threadIdx.x & 63) == 0)     // which lanes flush (lane 0 of every wave / of the workgroup)
// and puts MMFS_PROF_STORAGE; at the namespace scope the symbol lives in.  In a kernel: PROF_DECL; once, PROF(i) at the
// end of phase i, PROF_COUNT(i, v) for a plain count, PROF_FLUSH() at the end (PROF_FLUSH_ROW(r): into row r).
#pragma once
#include <hip/hip_runtime.h>

#ifdef MMFS_PROF_COUNTERS
#define MMFS_PROF_STORAGE __device__ unsigned long long MMFS_PROF_COUNTERS[MMFS_PROF_SLOTS * MMFS_PROF_N]
#define PROF_DECL unsigned long long prof_c = __builtin_readcyclecounter(), prof_t[MMFS_PROF_N] = {}
#define PROF(i) do { const unsigned long long tn = __builtin_readcyclecounter(); prof_t[i] += tn - prof_c; prof_c = tn; } while (0)
#define PROF_COUNT(i, v) do { prof_t[i] += (unsigned long long)(v); } while (0)
#define PROF_FLUSH_ROW(r) do { if (MMFS_PROF_LANE) for (int i_ = 0; i_ < MMFS_PROF_N; ++i_) atomicAdd(&MMFS_PROF_COUNTERS[(r) * MMFS_PROF_N + i_], prof_t[i_]); } while (0)
#else
#define MMFS_PROF_STORAGE static_assert(true, "")
#define PROF_DECL do {} while (0)
#define PROF(i) do {} while (0)
#define PROF_COUNT(i, v) do {} while (0)
#define PROF_FLUSH_ROW(r) do {} while (0)
#endif
#define PROF_FLUSH() PROF_FLUSH_ROW(blockIdx.x % MMFS_PROF_SLOTS)

namespace mmfs {

// The readout of SLOTS rows of N counters: out[0 .. OUT_N) = the rows' sums (OUT_N >= N: what the caller's buffer holds
// beyond the counters reads zero); reset: the counters are cleared behind it.
template <int SLOTS, int N, int OUT_N = N>
int prof_readout(const void *symbol, unsigned long long *out, int reset)
{
    static unsigned long long host[SLOTS * N];
    hipError_t e = hipMemcpyFromSymbol(host, symbol, sizeof(host));
    for (int i = 0; i < OUT_N; ++i) out[i] = 0;
    for (int s = 0; s < SLOTS; ++s)
        for (int i = 0; i < N; ++i) out[i] += host[s * N + i];
    if (e == hipSuccess && reset) {
        for (auto &v : host) v = 0;
        e = hipMemcpyToSymbol(symbol, host, sizeof(host));
    }
    return (int)e;
}

// ... and of N counters the tool wants row by row (msda_dense.hip; the sort's per-level clocks, msda_bwd_block.hip)
template <int N>
int prof_copyout(const void *symbol, unsigned long long *out, int reset)
{
    hipError_t e = hipMemcpyFromSymbol(out, symbol, N * sizeof(unsigned long long));
    if (e == hipSuccess && reset) {
        unsigned long long z[N] = {0};
        e = hipMemcpyToSymbol(symbol, z, sizeof(z));
    }
    return (int)e;
}

}  // namespace mmfs
