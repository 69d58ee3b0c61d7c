// The word functions of the skeleton tables, shared by the thinning kernel (sdsm_skeleton.hip) and the host helpers sdsm_skeleton_deletable
// and sdsm_skeleton_thin (sdsm_host.cpp): one set of functions, compiled for both sides, so the device cannot disagree with what the CPU
// tests check.  A binary image is held as ROW-ALIGNED 64-bit words: bit b of word j of row r is the pixel (r, 64 j + b); the bits of a
// row's last word at and past the width are 0 and stay 0 (nothing here ever sets a bit).
//
// Ring of a pixel, clockwise from north: 0 N(-1,0), 1 NE(-1,1), 2 E(0,1), 3 SE(1,1), 4 S(1,0), 5 SW(1,-1), 6 W(0,-1), 7 NW(-1,-1).
//
// LDS budget of the kernel: two planes (the image before and after a subiteration) of SDSM_SKELETON_LDS_WORDS 64-bit words, 2 * 3072 * 8
// = 48 KB, plus 2 KB of row staging for the wavefront path and the reduction cells: three workgroups per compute unit of 160 KB.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define SDSM_SKELETON_HD __host__ __device__
#else
#define SDSM_SKELETON_HD
#endif

#define SDSM_SKELETON_LDS_WORDS_INLINE 3072      /* SDSM_SKELETON_LDS_WORDS of include/sdsm.h */

typedef unsigned long long sdsm_skel_word;

// deletable(code, d) of the definition: code bit k = ring pixel k, d one of the ring bits 0 (N), 4 (S), 2 (E), 6 (W).  -1: d is none of them
// or the code has a bit above 255.
SDSM_SKELETON_HD inline int sdsm_skeleton_deletable_inline(int code, int d)
{
    if (code < 0 || code > 255 || (d != 0 && d != 2 && d != 4 && d != 6)) return -1;
    int x[10];
    for (int k = 0; k < 10; k++) x[k] = (code >> (k & 7)) & 1;
    int connectivity = 0, set = 0;
    for (int k = 0; k < 8; k += 2) connectivity += (1 - x[k]) * (x[k + 1] | x[k + 2]);
    for (int k = 0; k < 8; k++) set += x[k];
    return x[d] == 0 && connectivity == 1 && set >= 2;
}

// The eight neighbour planes of the word `mid` of a row: up, row and down are the words (left, mid, right) of the row above, the row
// itself and the row below; a word outside the image is 0.
SDSM_SKELETON_HD inline void sdsm_skeleton_planes(const sdsm_skel_word up[3], const sdsm_skel_word row[3], const sdsm_skel_word down[3], sdsm_skel_word n[8])
{
    n[0] = up[1];
    n[1] = (up[1] >> 1) | (up[2] << 63);
    n[2] = (row[1] >> 1) | (row[2] << 63);
    n[3] = (down[1] >> 1) | (down[2] << 63);
    n[4] = down[1];
    n[5] = (down[1] << 1) | (down[0] >> 63);
    n[6] = (row[1] << 1) | (row[0] >> 63);
    n[7] = (up[1] << 1) | (up[0] >> 63);
}

// The pixels of the centre word c that the subiteration of direction d (0, 2, 4, 6) removes: the bit-sliced form of deletable().
SDSM_SKELETON_HD inline sdsm_skel_word sdsm_skeleton_remove(sdsm_skel_word c, const sdsm_skel_word n[8], int d)
{
    sdsm_skel_word one = 0, two = 0;             // at least one / at least two of the four t_k
    for (int k = 0; k < 8; k += 2) {
        const sdsm_skel_word t = ~n[k] & (n[k + 1] | n[(k + 2) & 7]);
        two |= one & t;
        one |= t;
    }
    const sdsm_skel_word simple = one & ~two;
    sdsm_skel_word some = 0, many = 0;           // at least one / at least two of the eight neighbours
    for (int k = 0; k < 8; k++) {
        many |= some & n[k];
        some |= n[k];
    }
    return c & simple & many & ~n[d];
}

// What a word of the skeleton adds to the record's counts
struct sdsm_skeleton_counts { int n_skeleton, n_end, n_isolated, n_branch, n_orth, n_diag; };

SDSM_SKELETON_HD inline int sdsm_skeleton_popcount(sdsm_skel_word x)
{
    return __builtin_popcountll(x);
}

// The classes of the pixels of the centre word c of a skeleton with the neighbour planes n: ends (exactly one ring neighbour), isolated
// pixels (none), branch pixels (at least three transitions 0 -> 1 around the ring), and the pairs this word owns: with its eastern and
// southern neighbour (4-adjacent), and with its south-eastern and south-western one where both common 4-neighbours are clear.
SDSM_SKELETON_HD inline void sdsm_skeleton_classify(sdsm_skel_word c, const sdsm_skel_word n[8], sdsm_skeleton_counts &k)
{
    sdsm_skel_word some = 0, many = 0;
    for (int i = 0; i < 8; i++) {
        many |= some & n[i];
        some |= n[i];
    }
    sdsm_skel_word t1 = 0, t2 = 0, t3 = 0;       // at least one / two / three transitions
    for (int i = 0; i < 8; i++) {
        const sdsm_skel_word t = ~n[i] & n[(i + 1) & 7];
        t3 |= t2 & t;
        t2 |= t1 & t;
        t1 |= t;
    }
    k.n_skeleton += sdsm_skeleton_popcount(c);
    k.n_end += sdsm_skeleton_popcount(c & some & ~many);
    k.n_isolated += sdsm_skeleton_popcount(c & ~some);
    k.n_branch += sdsm_skeleton_popcount(c & t3);
    k.n_orth += sdsm_skeleton_popcount(c & n[2]) + sdsm_skeleton_popcount(c & n[4]);
    k.n_diag += sdsm_skeleton_popcount(c & n[3] & ~n[2] & ~n[4]) + sdsm_skeleton_popcount(c & n[5] & ~n[6] & ~n[4]);
}

// The cnt <= 64 bits from flat bit p0 on of a window of n_words32 uint32 words (bit p of the window is bit p & 31 of word p >> 5), as the
// low bits of a word; no word at or past n_words32 is read.
SDSM_SKELETON_HD inline sdsm_skel_word sdsm_skeleton_flat_bits(const uint32_t *bits, uint32_t n_words32, uint32_t p0, int cnt)
{
    const uint32_t k = p0 >> 5;
    const int s = (int)(p0 & 31);
    const sdsm_skel_word a = k < n_words32 ? bits[k] : 0, b = k + 1 < n_words32 ? bits[k + 1] : 0, c = k + 2 < n_words32 ? bits[k + 2] : 0;
    sdsm_skel_word v = (a | (b << 32)) >> s;
    if (s) v |= c << (64 - s);
    return cnt >= 64 ? v : v & ((1ull << cnt) - 1);
}

// Word k of the flat window (bits 32 k .. 32 k + 31 of the h x w image, the bits past h w clear) from its row-aligned plane of nw words
// a row.
SDSM_SKELETON_HD inline uint32_t sdsm_skeleton_flat_word(const sdsm_skel_word *plane, uint32_t w, uint32_t nw, uint32_t n_bits, uint32_t k)
{
    uint32_t p = k << 5, out = 0;
    const uint32_t end = p + 32 < n_bits ? p + 32 : n_bits;
    uint32_t r = p / w, c = p % w;
    while (p < end) {
        uint32_t take = end - p;
        if (w - c < take) take = w - c;
        if (64 - (c & 63) < take) take = 64 - (c & 63);                        // take <= 32
        const uint32_t piece = (uint32_t)(plane[(size_t)r * nw + (c >> 6)] >> (c & 63)) & (take >= 32 ? 0xffffffffu : (1u << take) - 1);
        out |= piece << (p & 31);
        p += take; c += take;
        if (c == w) { c = 0; r++; }
    }
    return out;
}
