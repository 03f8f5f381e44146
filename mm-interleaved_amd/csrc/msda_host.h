// msda_host.h -- the small host-side checks and dispatchers that every extern "C" entry and every launcher shares.
#pragma once
#include "../../include/mmfs_msda.h"
#include "msda_device.h"
#include <stdint.h>
#include <initializer_list>
#include <type_traits>

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

inline bool misaligned(const void *p, int esize) { return ((uintptr_t)p % (uintptr_t)esize) != 0; }

// An entry point's pointer contract, as a list: MMFS_E_NULLPTR if a pointer that has to be there is NULL, else
// MMFS_E_ALIGN if any is not a multiple of its alignment (1: a level table, which no entry refuses for its alignment).
// ``needed`` = false, or maybe(): the pointer may be NULL, and NULL counts as aligned.
struct Tensor { const void *p; int align; bool needed = true; };
inline Tensor maybe(const void *p, int align) { return {p, align, false}; }
inline int check_tensors(std::initializer_list<Tensor> ts)
{
    for (const Tensor &t : ts) if (t.needed && !t.p) return MMFS_E_NULLPTR;
    for (const Tensor &t : ts) if (misaligned(t.p, t.align)) return MMFS_E_ALIGN;
    return MMFS_OK;
}

inline int check_workspace(const void *workspace, int64_t have, int64_t need)
{
    if (!workspace || have < need) return MMFS_E_NULLPTR;
    return misaligned(workspace, 16) ? MMFS_E_ALIGN : MMFS_OK;
}

inline int64_t round256(int64_t x) { return (x + 255) / 256 * 256; }

// A bank of Bv rows behind B query rows (MMFS_BANK_*): MMFS_E_DIMS / MMFS_E_UNSUPPORTED, or d->Bv and d->vdiv set.
inline int set_bank(Dims *d, int64_t B, int64_t Bv, int layout)
{
    if (Bv <= 0 || B % Bv != 0) return MMFS_E_DIMS;
    if (layout != MMFS_BANK_TILE && layout != MMFS_BANK_INTERLEAVE) return MMFS_E_UNSUPPORTED;
    if (B > 0) {
        d->Bv = (int)Bv;
        d->vdiv = layout == MMFS_BANK_INTERLEAVE ? (int)(B / Bv) : 1;
    }
    return MMFS_OK;
}

// rows ``ld`` elements apart (0 = packed, ``cols``): the range half of heads_rows ...
inline int rows_range(int64_t &ld, int64_t cols)
{
    if (ld == 0) ld = cols;
    return ld < cols || ld > 0x7fffffffLL ? MMFS_E_DIMS : MMFS_OK;
}

// ... and its alignment half: rows of ``es``-byte elements and their base pointer, read ``bytes`` at a time
inline int rows_aligned(int64_t ld, int64_t es, const void *p, int64_t bytes)
{
    return (ld * es) % bytes || (uintptr_t)p % (uintptr_t)bytes ? MMFS_E_ALIGN : MMFS_OK;
}

// rows ``ld`` elements apart (0 = packed, ``cols``), vector accesses of ``vec`` elements of ``es`` bytes: dimensions and
// alignment (load_row / store_row: accesses of at most 16 bytes)
inline int heads_rows(int64_t &ld, int64_t cols, const void *p, int64_t vec, int64_t es)
{
    if (const int rc = rows_range(ld, cols)) return rc;
    return rows_aligned(ld, es, p, vec * es < 16 ? vec * es : 16);
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

// f(std::integral_constant<int, V>()) for the V of the list that equals ``v``, for the last V otherwise (the ``default:``
// arm of the switch this stands for); whatever f returns
template <int V, int... Rest, typename F> auto by_int(int64_t v, F &&f) -> decltype(f(std::integral_constant<int, V>()))
{
    if constexpr (sizeof...(Rest) == 0) return f(std::integral_constant<int, V>());
    else return v == V ? f(std::integral_constant<int, V>()) : by_int<Rest...>(v, f);
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
