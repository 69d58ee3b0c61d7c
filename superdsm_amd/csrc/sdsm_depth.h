// The shell of a depth, shared by the depth kernel (sdsm_depth.hip) and the host helper sdsm_depth_shell (sdsm_host.cpp): one function,
// compiled for both sides, so the device cannot disagree with what the CPU tests check.  The float root is an estimate only: the two
// integer loops make the result the integer root by construction.
#pragma once
#include <cstdint>
#include <cmath>

#if defined(__HIP__) || defined(__HIPCC__)
#define SDSM_DEPTH_HD __host__ __device__
#else
#define SDSM_DEPTH_HD
#endif

#define SDSM_DEPTH_MAX_SHELLS_INLINE 32

// floor(sqrt(x)) for 0 <= x < 2^31 (the deepest pixel of the largest image has d2 = 32 768^2 = 2^30): a float estimate (within 1 of the
// root: a float carries 24 bits, the root has 16), then the correction that makes it the integer root.
SDSM_DEPTH_HD inline int32_t sdsm_depth_isqrt_inline(int32_t x)
{
    int32_t r = (int32_t)sqrtf((float)x);
    while ((int64_t)r * r > x) r--;
    while ((int64_t)(r + 1) * (r + 1) <= x) r++;
    return r;
}

// The shell of a pixel of squared depth d2 >= 1 among n_shells >= 1: k = min(n_shells - 1, isqrt(d2 - 1)), that is ceil(sqrt(d2)) - 1
// capped.  Shell 0 holds d2 == 1, shell 1 d2 in 2 .. 4, shell 2 d2 in 5 .. 9; the last shell collects every deeper pixel.
SDSM_DEPTH_HD inline int sdsm_depth_shell_inline(int32_t d2, int n_shells)
{
    const int32_t k = sdsm_depth_isqrt_inline(d2 - 1);
    return k < n_shells - 1 ? k : n_shells - 1;
}
