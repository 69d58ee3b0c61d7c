// The two integer decisions of the texture tables, shared by the kernels (sdsm_texture.hip) and the host helpers sdsm_texture_level and
// sdsm_texture_cell (sdsm_host.cpp): one function each, compiled for both sides, so the device cannot disagree with what the CPU tests
// check.  The only floating-point operations are comparisons.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define SDSM_TEX_HD __host__ __device__
#else
#define SDSM_TEX_HD
#endif

// The grey level of a finite value g among n_edges strictly increasing finite edges: the number of edges <= g (np.searchsorted(edges, g,
// side='right')), by binary search.  -0.0 compares as 0.0 (IEEE comparison).  0 <= level <= n_edges.
SDSM_TEX_HD inline int sdsm_texture_level_inline(const double *edges, int n_edges, double g)
{
    int lo = 0, hi = n_edges;                    // edges[0 .. lo - 1] <= g < edges[hi ..]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] <= g) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The place of the cell (i, j), 0 <= i <= j < levels, in the packed upper triangle, row by row: ascending places are ascending (i, j).
// levels <= 256: below 32 896.
SDSM_TEX_HD inline int sdsm_texture_cell_inline(int levels, int i, int j)
{
    return (i * (2 * levels - i + 1)) / 2 + (j - i);
}
