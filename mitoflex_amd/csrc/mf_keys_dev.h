// Device helpers that the filter kernels (mf_kernels.hip) and the record-assignment kernels (mf_assign.hip) share: a k-mer's
// canonical key straight from the packed stream, the look-up of a key in the open-address bait table, the invalid-base index.
#pragma once
#include "mf_common.h"
#include <hip/hip_runtime.h>

namespace mf {

__device__ __forceinline__ uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh)
{   // (hi:lo >> sh) & 0xffffffff, sh in [0,31]  -> v_alignbit_b32
    return __funnelshift_r(lo, hi, sh);
}

// first index i with npos[i] >= v, through the block index
__device__ __forceinline__ uint64_t npos_lower_bound(const ReadsView &R, uint64_t v)
{
    const uint64_t b = v >> NPOS_BLK_SHIFT;
    uint64_t lo = R.npos_blk[b], hi = R.npos_blk[b + 1];          // the answer lies in [lo, hi]
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (R.npos[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
}

template <int KW> struct Key;
template <> struct Key<1> { uint64_t lo; };
template <> struct Key<2> { uint64_t lo, hi; };

// canonical k-mer whose first base is global base g
template <int KW>
__device__ __forceinline__ Key<KW> canonical_at(const uint32_t *__restrict__ words, uint64_t g, int k);

template <>
__device__ __forceinline__ Key<1> canonical_at<1>(const uint32_t *__restrict__ words, uint64_t g, int k)
{
    const uint64_t bit = 2 * g;
    const uint64_t wi = bit >> 5; const uint32_t sh = (uint32_t)bit & 31;
    const uint32_t w0 = words[wi], w1 = words[wi + 1], w2 = words[wi + 2];
    uint64_t fwd = ((uint64_t)alignbit(w2, w1, sh) << 32) | alignbit(w1, w0, sh);
    if (k < 32) fwd &= (1ULL << (2 * k)) - 1;
    const uint64_t rc = revcomp1(fwd, k);
    return Key<1>{fwd < rc ? fwd : rc};
}

template <>
__device__ __forceinline__ Key<2> canonical_at<2>(const uint32_t *__restrict__ words, uint64_t g, int k)
{
    const uint64_t bit = 2 * g;
    const uint64_t wi = bit >> 5; const uint32_t sh = (uint32_t)bit & 31;
    const uint32_t w0 = words[wi], w1 = words[wi + 1], w2 = words[wi + 2], w3 = words[wi + 3], w4 = words[wi + 4];
    uint64_t lo = ((uint64_t)alignbit(w2, w1, sh) << 32) | alignbit(w1, w0, sh);
    uint64_t hi = ((uint64_t)alignbit(w4, w3, sh) << 32) | alignbit(w3, w2, sh);
    hi &= (1ULL << (2 * k - 64)) - 1;                 // 33 <= k <= 63
    uint64_t rlo, rhi; revcomp2(lo, hi, k, rlo, rhi);
    const bool f = (hi < rhi) || (hi == rhi && lo < rlo);
    return f ? Key<2>{lo, hi} : Key<2>{rlo, rhi};
}

// canonical_at, and which text is the canonical form: rev = 0 the forward text of the window, 1 its reverse complement, 2 both (the
// window is its own reverse complement: even k only)
template <int KW>
__device__ __forceinline__ Key<KW> oriented_at(const uint32_t *__restrict__ words, uint64_t g, int k, uint32_t &rev);

template <>
__device__ __forceinline__ Key<1> oriented_at<1>(const uint32_t *__restrict__ words, uint64_t g, int k, uint32_t &rev)
{
    const uint64_t bit = 2 * g;
    const uint64_t wi = bit >> 5; const uint32_t sh = (uint32_t)bit & 31;
    const uint32_t w0 = words[wi], w1 = words[wi + 1], w2 = words[wi + 2];
    uint64_t fwd = ((uint64_t)alignbit(w2, w1, sh) << 32) | alignbit(w1, w0, sh);
    if (k < 32) fwd &= (1ULL << (2 * k)) - 1;
    const uint64_t rc = revcomp1(fwd, k);
    rev = fwd < rc ? 0u : fwd == rc ? 2u : 1u;
    return Key<1>{fwd < rc ? fwd : rc};
}

template <>
__device__ __forceinline__ Key<2> oriented_at<2>(const uint32_t *__restrict__ words, uint64_t g, int k, uint32_t &rev)
{
    const uint64_t bit = 2 * g;
    const uint64_t wi = bit >> 5; const uint32_t sh = (uint32_t)bit & 31;
    const uint32_t w0 = words[wi], w1 = words[wi + 1], w2 = words[wi + 2], w3 = words[wi + 3], w4 = words[wi + 4];
    uint64_t lo = ((uint64_t)alignbit(w2, w1, sh) << 32) | alignbit(w1, w0, sh);
    uint64_t hi = ((uint64_t)alignbit(w4, w3, sh) << 32) | alignbit(w3, w2, sh);
    hi &= (1ULL << (2 * k - 64)) - 1;                 // 33 <= k <= 63
    uint64_t rlo, rhi; revcomp2(lo, hi, k, rlo, rhi);
    const bool f = (hi < rhi) || (hi == rhi && lo < rlo);
    rev = f ? 0u : (hi == rhi && lo == rlo) ? 2u : 1u;
    return f ? Key<2>{lo, hi} : Key<2>{rlo, rhi};
}

__device__ __forceinline__ bool table_contains(const KmerSetView &S, Key<1> v)
{
    uint64_t slot = hash_key1(v.lo) & S.slot_mask;
    uint64_t e = S.keys[slot];
    while (e < v.lo) { slot = (slot + 1) & S.slot_mask; e = S.keys[slot]; }   // ordered table
    return e == v.lo;
}
__device__ __forceinline__ bool table_contains(const KmerSetView &S, Key<2> v)
{
    uint64_t slot = hash_key2(v.lo, v.hi) & S.slot_mask;
    for (;;) {
        const ulonglong2 e = reinterpret_cast<const ulonglong2 *>(S.keys)[slot];
        const bool less = (e.y < v.hi) || (e.y == v.hi && e.x < v.lo);
        if (!less) return e.x == v.lo && e.y == v.hi;
        slot = (slot + 1) & S.slot_mask;
    }
}

// the slot that holds key v, or ~0 when the set does not hold it (the same walk as table_contains)
__device__ __forceinline__ uint64_t table_find(const KmerSetView &S, Key<1> v)
{
    uint64_t slot = hash_key1(v.lo) & S.slot_mask;
    uint64_t e = S.keys[slot];
    while (e < v.lo) { slot = (slot + 1) & S.slot_mask; e = S.keys[slot]; }
    return e == v.lo ? slot : ~0ULL;
}
__device__ __forceinline__ uint64_t table_find(const KmerSetView &S, Key<2> v)
{
    uint64_t slot = hash_key2(v.lo, v.hi) & S.slot_mask;
    for (;;) {
        const ulonglong2 e = reinterpret_cast<const ulonglong2 *>(S.keys)[slot];
        const bool less = (e.y < v.hi) || (e.y == v.hi && e.x < v.lo);
        if (!less) return (e.x == v.lo && e.y == v.hi) ? slot : ~0ULL;
        slot = (slot + 1) & S.slot_mask;
    }
}

} // namespace mf
