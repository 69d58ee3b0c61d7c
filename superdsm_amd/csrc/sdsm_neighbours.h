// The two integer decisions of the neighbourhood tables, shared by the kernel (sdsm_neighbours.hip) and the host helpers
// sdsm_neighbour_halfwidth and sdsm_neighbour_slot (sdsm_host.cpp): one function each, compiled for both sides, so the device cannot
// disagree with what the CPU tests check.  Integers only.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define SDSM_NB_HD __host__ __device__
#else
#define SDSM_NB_HD
#endif

#define SDSM_NEIGHBOUR_MAX_D2_INLINE 4096        // == SDSM_NEIGHBOUR_MAX_D2 of include/sdsm.h (a reach of 64 pixels)
#define SDSM_NEIGHBOUR_MAX_REACH_INLINE 64

// floor(sqrt(n)) for 0 <= n <= 4096 + 127 (so the root is at most 64, and t * t below stays far from overflow): one bit of the root per
// step, from bit 6 down.
SDSM_NB_HD inline int sdsm_neighbour_isqrt_inline(int n)
{
    int r = 0;
    for (int b = SDSM_NEIGHBOUR_MAX_REACH_INLINE; b; b >>= 1) {
        const int t = r + b;
        if (t * t <= n) r = t;
    }
    return r;
}

// The largest |d_col| with d_row^2 + d_col^2 <= max_d2: the half-width of row d_row of the disk of squared radius max_d2.  -1 when the
// row lies outside the disk (d_row^2 > max_d2) or an argument is bad (max_d2 outside 1 .. 4096).
SDSM_NB_HD inline int sdsm_neighbour_halfwidth_inline(int max_d2, int d_row)
{
    if (max_d2 < 1 || max_d2 > SDSM_NEIGHBOUR_MAX_D2_INLINE) return -1;
    if (d_row < -SDSM_NEIGHBOUR_MAX_REACH_INLINE || d_row > SDSM_NEIGHBOUR_MAX_REACH_INLINE) return -1;      // (also keeps d_row * d_row small)
    const int rest = max_d2 - d_row * d_row;
    return rest < 0 ? -1 : sdsm_neighbour_isqrt_inline(rest);
}

// The first slot the pair `key` = (uint64)a << 32 | b is tried at in a table of `capacity` slots, a power of two >= 1: the hash of
// sdsm_overlap_pairs (multiplicative; the high bits, which depend on every bit of the key, are folded onto the low ones).  Probing is
// linear from there.
SDSM_NB_HD inline uint64_t sdsm_neighbour_slot_inline(uint64_t key, uint64_t capacity)
{
    const uint64_t h = key * 0x9E3779B97F4A7C15ull;
    return (h ^ (h >> 31)) & (capacity - 1);
}
