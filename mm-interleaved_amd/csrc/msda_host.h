// msda_host.h -- the small host-side checks and dispatchers that every extern "C" entry and every launcher shares.
#pragma once
#include "../../include/mmfs_msda.h"
#include "msda_device.h"
#include <stdint.h>

namespace mmfs {

// bytes of an element of ``dtype`` (enum mmfs_dtype), 0 for a type the caller does not serve (fp64: only the op does)
inline int elem_size(int dtype, bool f64 = false)
{
    switch (dtype) {
        case MMFS_F32: return 4;
        case MMFS_F16: case MMFS_BF16: return 2;
        case MMFS_F64: return f64 ? 8 : 0;
        default: return 0;
    }
}

// rows ``ld`` elements apart (0 = packed, ``cols``), vector accesses of ``vec`` elements of ``es`` bytes: dimensions and
// alignment (load_row / store_row: accesses of at most 16 bytes)
inline int heads_rows(int64_t &ld, int64_t cols, const void *p, int64_t vec, int64_t es)
{
    if (ld == 0) ld = cols;
    if (ld < cols || ld > 0x7fffffffLL) return MMFS_E_DIMS;
    const int64_t a = vec * es < 16 ? vec * es : 16;
    if ((ld * es) % a || (uintptr_t)p % (uintptr_t)a) return MMFS_E_ALIGN;
    return MMFS_OK;
}

// f(T()) for the storage type of a dtype that elem_size serves without fp64; whatever f returns (a status, a hipError_t)
template <typename F> auto by_type(int dtype, F &&f) -> decltype(f(float()))
{
    if (dtype == MMFS_F32) return f(float());
    if (dtype == MMFS_F16) return f(half_t());
    return f(bf16_t());
}

// the same for an entry that serves the two 16-bit types alone (it has refused the others)
template <typename F> auto by_half_type(int dtype, F &&f) -> decltype(f(half_t()))
{
    return dtype == MMFS_F16 ? f(half_t()) : f(bf16_t());
}

// Bytes per copy (16 / 8 / 4, else 2) of a re-pack that moves chunks of ``chunk_bytes`` between these two pointers: the
// widest access both ends are aligned for that divides the chunk.  An odd chunk has none: the caller refuses it.
inline int repack_copy_bytes(const void *a, const void *b, int chunk_bytes)
{
    const bool al = (((uintptr_t)a | (uintptr_t)b) % 16) == 0;
    if (al && chunk_bytes % 16 == 0) return 16;
    if (al && chunk_bytes % 8 == 0) return 8;
    if (al && chunk_bytes % 4 == 0) return 4;
    return 2;
}

}  // namespace mmfs
