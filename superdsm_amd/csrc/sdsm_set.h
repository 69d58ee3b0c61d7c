// What the image-set kernels of sdsm_c2f.hip, sdsm_render.hip and sdsm_post.hip share.  A launch serves a whole set through one
// flattened grid; its kernels take a prefix table of the images' items (workgroups, columns, rows, objects) by value.  A single image
// is the set of one.
#pragma once
#include <cstdint>

// the image of item x of a flattened grid: the last i with start[i] <= x (images without items are passed over)
__device__ __forceinline__ int set_find(const int32_t *start, int n, int x)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
