// The class of a bit quad, shared by the tile kernel of the connected parts (sdsm_parts.hip) and the host helper sdsm_parts_quad
// (sdsm_host.cpp): one function, compiled for both sides, so the device cannot disagree with what the CPU tests check.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define SDSM_PARTS_HD __host__ __device__
#else
#define SDSM_PARTS_HD
#endif

#define SDSM_PARTS_QUAD_NONE 0
#define SDSM_PARTS_QUAD_Q1 1
#define SDSM_PARTS_QUAD_Q3 2
#define SDSM_PARTS_QUAD_QD 3

// The window of 2 x 2 places  a b / c d  (a upper left, d lower right) against the mask of `label`: Q1 with exactly one place of the
// label, Q3 with exactly three, QD with exactly the two on a diagonal, NONE otherwise (no place, two side by side, all four).
SDSM_PARTS_HD inline int sdsm_parts_quad_inline(int32_t a, int32_t b, int32_t c, int32_t d, int32_t label)
{
    const int ia = a == label, ib = b == label, ic = c == label, id = d == label;
    const int m = ia + ib + ic + id;
    if (m == 1) return SDSM_PARTS_QUAD_Q1;
    if (m == 3) return SDSM_PARTS_QUAD_Q3;
    if (m == 2 && ia == id) return SDSM_PARTS_QUAD_QD;       // (two places and a == d in the mask: both diagonal places, or both of the other diagonal)
    return SDSM_PARTS_QUAD_NONE;
}
