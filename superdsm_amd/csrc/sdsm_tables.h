// What the table kernels share (sdsm_measure.hip, sdsm_shape.hip, sdsm_intensity.hip, sdsm_texture.hip, sdsm_neighbours.hip,
// sdsm_depth.hip): the images of a launch, the order key of a double, the scale exponent of an image and the quantised root of a squared
// distance, the guard and the walk of an object's bit-packed fragment, and the slot claims of the LDS label tables and the global pair
// tables.  Everything is inlined into its kernel.
#pragma once
#include "sdsm_common.h"
#include "sdsm_set.h"
#include <cmath>

typedef unsigned long long u64;
typedef long long i64;

struct SetImages {                               // the images of a launch
    int32_t n;
    int32_t H[SDSM_MAX_SET_IMAGES], W[SDSM_MAX_SET_IMAGES];
    int64_t off[SDSM_MAX_SET_IMAGES];            // first pixel of the image in the packed buffers
};

struct SetLabels : SetImages {                   // and their label tables
    int64_t rec_off[SDSM_MAX_SET_IMAGES];        // first record (measure), entry of d_label_obj (shape) or table slot (overlap) of the image
    int32_t n_labels[SDSM_MAX_SET_IMAGES];
    int32_t start[SDSM_MAX_SET_IMAGES + 1];      // flattened grid: first workgroup of the image
};

inline SetLabels make_set(const sdsm_set_image *images, int n_images)
{
    SetLabels S{};
    S.n = n_images;
    for (int i = 0; i < n_images; i++) { S.H[i] = images[i].H; S.W[i] = images[i].W; S.off[i] = images[i].offset; }
    return S;
}

// the monotone 64-bit key of a double: a < b iff key(a) < key(b); -0.0 is made +0.0 first
__device__ __forceinline__ u64 dkey(double v)
{
    if (v == 0.0) v = 0.0;
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}

__device__ __forceinline__ double dkey_inv(u64 k)
{
    return __longlong_as_double((i64)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

__device__ __forceinline__ bool finite_bits(double g)
{
    return (((u64)__double_as_longlong(g) >> 52) & 0x7ff) != 0x7ff;
}

// e of an image from the bits of its max finite |g| (k_absmax of sdsm_measure.hip leaves them in device memory): the smallest e with
// max < 2^e, clamped to -960 .. 1024; 0 without a non-zero pixel
__device__ __forceinline__ int scale_exp(u64 maxbits)
{
    if (maxbits == 0) return 0;
    const int E = (int)(maxbits >> 52);
    const int e = E == 0 ? -960 : E - 1022;
    return e < -960 ? -960 : e;
}

// q(d2) = floor(sqrt(d2 * 2^32)): a float estimate (relative error below 2^-22), one Newton step from the exact 64-bit residual, which
// leaves it within a few units, then the correction that makes it the integer root by construction.  d2 < 2^31: x < 2^63, r < 2^32.
__host__ __device__ inline u64 quantised_distance(int32_t d2)
{
    if (d2 <= 0) return 0;
    const u64 x = (u64)(uint32_t)d2 << 32;
    u64 r = (u64)(sqrtf((float)d2) * 65536.0f);              // >= 65536
    const i64 e = (i64)(x - r * r);                          // (the difference of the unsigned products, read as signed)
    r = (u64)((i64)r + (i64)floorf((float)e / (2.0f * (float)r)));
    while (r * r > x) r--;
    while ((r + 1) * (r + 1) <= x) r++;
    return r;
}

// A round of an exact radix select, once its 256-bin histogram stands in LDS: one wavefront (the caller tests tid < 64) scans it, lane l
// owning the bins 4 l .. 4 l + 3, and the one lane whose bins hold rank r publishes the bin, the rank that remains inside it and its count.
__device__ __forceinline__ void select_bin(const uint32_t *hist, int tid, uint32_t r, uint32_t &sel_bin, uint32_t &sel_r, uint32_t &sel_cnt)
{
    const uint32_t h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
    const uint32_t sum = h0 + h1 + h2 + h3;
    uint32_t incl = sum;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o);
        if (tid >= o) incl += t;
    }
    const uint32_t excl = incl - sum;
    if (r >= excl && r < incl) {                 // exactly one lane
        uint32_t rr = r - excl, c = h0;
        int b = 0;
        if (rr >= h0) {
            rr -= h0; b = 1; c = h1;
            if (rr >= h1) {
                rr -= h1; b = 2; c = h2;
                if (rr >= h2) { rr -= h2; b = 3; c = h3; }
            }
        }
        sel_bin = 4 * tid + b; sel_r = rr; sel_cnt = c;
    }
}

// ---- an object's fragment: h * w bits, contiguous from bits[0] on, for the box (r0, c0, h, w) of an H x W image ------------------------
struct Fragment { int H, W, r0, c0, h, w; };

// The box of object i and the shape of its image `im` (0 x 0 when `im` is no image of the set).  False when the box does not lie in that
// image: the caller writes its empty result and reads neither a bit nor a pixel.
__device__ __forceinline__ bool fragment_box(const SetImages &S, int im, const int32_t *boxes, int i, Fragment &f)
{
    const bool im_ok = im >= 0 && im < S.n;
    f.H = im_ok ? S.H[im] : 0; f.W = im_ok ? S.W[im] : 0;
    f.r0 = boxes[4 * i]; f.c0 = boxes[4 * i + 1]; f.h = boxes[4 * i + 2]; f.w = boxes[4 * i + 3];
    return im_ok && f.r0 >= 0 && f.c0 >= 0 && f.h >= 1 && f.w >= 1 && f.h <= f.H && f.w <= f.W && f.r0 <= f.H - f.h && f.c0 <= f.W - f.w;
}

// f(bit index in the fragment, row, column in the image) for every set bit of the fragment, its words dealt to STRIDE threads
template <int STRIDE, class F>
__device__ __forceinline__ void each_set_bit(const uint32_t *bits, const Fragment &b, int tid, F f)
{
    const uint32_t n_bits = (uint32_t)b.h * (uint32_t)b.w, n_words = (n_bits + 31) >> 5;
    for (uint32_t k = tid; k < n_words; k += STRIDE) {
        uint32_t word = bits[k];
        if (k == n_words - 1 && (n_bits & 31)) word &= (1u << (n_bits & 31)) - 1;       // the bits past h * w are not the object's
        while (word) {
            const uint32_t p = (k << 5) + (uint32_t)__builtin_ctz(word);
            word &= word - 1;
            f(p, b.r0 + (int)(p / (uint32_t)b.w), b.c0 + (int)(p % (uint32_t)b.w));
        }
    }
}

// ---- slot claims ----------------------------------------------------------------------------------------------------------------------
// found(slot) for the slot of `label` in an LDS table of 1 << BITS keys (-1: free), claimed if need be: linear probing from the
// multiplicative hash.  False when PROBES slots belong to other labels: the caller then goes to the global atomics, correct and slow.
template <int BITS, int PROBES, class F>
__device__ __forceinline__ bool lds_label_slot(int32_t *keys, int32_t label, F found)
{
    uint32_t s = ((uint32_t)label * 2654435761u) >> (32 - BITS);
    for (int k = 0; k < PROBES; k++, s = (s + 1) & ((1u << BITS) - 1)) {
        const int32_t old = atomicCAS(&keys[s], -1, label);
        if (old != -1 && old != label) continue;
        found(s);
        return true;
    }
    return false;
}

// the same as a value: the slot, or -1 (where the caller does one thing with it, as sdsm_neighbours.hip)
template <int BITS, int PROBES>
__device__ __forceinline__ int lds_label_slot(int32_t *keys, int32_t label)
{
    int slot = -1;
    lds_label_slot<BITS, PROBES>(keys, label, [&](uint32_t s) { slot = (int)s; });
    return slot;
}

constexpr u64 PAIR_FREE = ~0ull;                 // a free slot of a pair table (no pair has this key: labels are >= 0, or <= 65535)

// found(slot) for the slot of the pair `key` in a global table of cap slots (a power of two): linear probing from first_slot, at most cap
// tries.  A key is written once (free -> key, by compare-and-swap) and never changes, so a slot read as another pair's stays that pair's.
// False when the table is full: the caller counts the pair in status[1] and drops it, and the host launches again with a larger table.
template <class F>
__device__ __forceinline__ bool pair_table_slot(u64 *keys, int64_t cap, u64 first_slot, u64 key, F found)
{
    const u64 mask = (u64)cap - 1;
    u64 s = first_slot;
    for (int64_t k = 0; k < cap; k++, s = (s + 1) & mask) {
        u64 old = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == PAIR_FREE) old = atomicCAS(keys + s, PAIR_FREE, key);
        if (old != PAIR_FREE && old != key) continue;
        found(s);
        return true;
    }
    return false;
}
