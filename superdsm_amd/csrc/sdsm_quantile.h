// The ranks of a quantile, shared by the intensity kernels (sdsm_intensity.hip) and the host helper sdsm_quantile_ranks
// (sdsm_host.cpp): one function, compiled for both sides, so the device cannot disagree with what the CPU tests check.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define SDSM_HD __host__ __device__
#else
#define SDSM_HD
#endif

// The two order statistics between which the quantile num / den of n >= 1 sorted values lies (0 <= num <= den, 1 <= den <= 10^6,
// n < 2^31: h < 2^51).  h = (n - 1) num, lo = h div den, rem = h mod den, hi = lo + (rem != 0); the quantile is
// v[lo] + (v[hi] - v[lo]) * rem / den.
SDSM_HD inline void sdsm_quantile_ranks_inline(int64_t n, int32_t num, int32_t den, int64_t *lo, int64_t *hi, int64_t *rem)
{
    const int64_t h = (n - 1) * (int64_t)num;
    *lo = h / den;
    *rem = h % den;
    *hi = *lo + (*rem != 0 ? 1 : 0);
}
