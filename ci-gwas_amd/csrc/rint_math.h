// rint_math.h -- the integer arithmetic of the rank-based inverse normal transform (cusk_phen_rint of include/cusk_hip.h,
// where the rule is stated), written once for the device kernels of phen_rint.hip and for the host self test
// (tools/rint_selftest.cpp), which compiles the same text with a C++ compiler.
//
//   rint_key        the order-preserving uint32 image of a float: -0.0 on the image of +0.0, a missing value (NaN, +-Inf)
//                   on 0xFFFFFFFF, which no finite float has (FLT_MAX maps to 0xFF7FFFFF)
//   rint_pair_low   the lower index of the t-th compare-exchange pair of bitonic step j; its partner is rint_partner
//   rint_ascending  the direction of the pair inside merge size k
//   rint_lower / rint_upper   the counts of sorted keys below a key / not above it
//   rint_rank2      twice the average rank, from those two counts
//   rint_npad, rint_trait_bytes   the padded row of keys and the workspace of one trait
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RINT_HD __host__ __device__ __forceinline__
#else
#define RINT_HD inline
#endif

namespace cusk {
namespace rintm {

constexpr uint32_t kMissingKey = 0xFFFFFFFFu;

// bits: the float's own 32 bits
RINT_HD uint32_t rint_key(uint32_t bits)
{
    if ((bits & 0x7F800000u) == 0x7F800000u) return kMissingKey;  // NaN, +-Inf
    if (bits == 0x80000000u) bits = 0u;                           // -0.0 == +0.0
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// Step j (a power of two) pairs i with i ^ j for every i whose bit j is clear; the t-th such i, t = 0 .. n/2 - 1
// (I: the index type, uint32_t inside a tile and size_t across a row)
template <typename I>
RINT_HD I rint_pair_low(I t, I j)
{
    return t + (t & ~(j - 1));
}
template <typename I>
RINT_HD I rint_partner(I i, I j)
{
    return i ^ j;
}
// inside merge size k (a power of two >= 2 j) the pair (i, i ^ j), i < i ^ j, ends with the smaller key at i when this holds
RINT_HD bool rint_ascending(size_t i, size_t k) { return (i & k) == 0; }
// the pair is exchanged
RINT_HD bool rint_exchange(uint32_t at_low, uint32_t at_high, bool ascending) { return (at_low > at_high) == ascending && at_low != at_high; }

// #{ j < n : keys[j] < key } and #{ j < n : keys[j] <= key } of ascending keys
RINT_HD uint32_t rint_lower(const uint32_t *keys, uint32_t n, uint32_t key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
RINT_HD uint32_t rint_upper(const uint32_t *keys, uint32_t n, uint32_t key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] <= key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// rank2 = 2 lo + eq + 1 with lo = lower and eq = upper - lower: at most 2 n, n < 2^31
RINT_HD uint32_t rint_rank2(uint32_t lower, uint32_t upper) { return lower + upper + 1u; }

// the next power of two >= max(N, tile); tile is a power of two, N < 2^31
RINT_HD size_t rint_npad(size_t N, size_t tile)
{
    size_t v = tile;
    while (v < N) v <<= 1;
    return v;
}

// workspace of one trait: the padded keys and one rank2 per individual
RINT_HD size_t rint_trait_bytes(size_t N, size_t tile) { return 4 * (rint_npad(N, tile) + N); }

}  // namespace rintm
}  // namespace cusk
