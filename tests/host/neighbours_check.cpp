// Stand-alone check of the two inline helpers of superdsm_amd/csrc/sdsm_neighbours.h (the functions the neighbourhood kernel uses and
// sdsm_neighbour_halfwidth / sdsm_neighbour_slot export), meant to be built as host code with AddressSanitizer and
// UndefinedBehaviorSanitizer linked in.  Walks every max_d2 in 1 .. 4096 and every row d_row in -66 .. 66: the half-width must be the
// largest d_col with d_row^2 + d_col^2 <= max_d2, found here by counting up, or -1 for a row outside the disk; it fills a table of
// exactly 2 * reach + 1 entries per disk the way the kernel does, so a row too many is the sanitizer's to find.  Then bad arguments, the
// integer root at every argument it takes, and the first probe position in tables of 1 .. 2^40 slots.  Writes the number of pixels of
// the disks of max_d2 = 1, 2, 25, 400 and 4096 (centre included) to stdout, one per line.  Exit status 0 when everything held.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../superdsm_amd/csrc/sdsm_neighbours.h"

int main()
{
    for (int n = 0; n <= SDSM_NEIGHBOUR_MAX_D2_INLINE + 127; n++) {
        const int r = sdsm_neighbour_isqrt_inline(n);
        if (r < 0 || r * r > n || (r + 1) * (r + 1) <= n) return 1;
    }
    for (int max_d2 = 1; max_d2 <= SDSM_NEIGHBOUR_MAX_D2_INLINE; max_d2++) {
        const int reach = sdsm_neighbour_isqrt_inline(max_d2);
        std::vector<int16_t> table(2 * reach + 1);
        long pixels = 0;
        for (int d_row = -66; d_row <= 66; d_row++) {
            const int w = sdsm_neighbour_halfwidth_inline(max_d2, d_row);
            if (d_row * d_row > max_d2) {
                if (w != -1) return 2;
                continue;
            }
            int want = 0;
            while (d_row * d_row + (want + 1) * (want + 1) <= max_d2) want++;
            if (w != want || w > reach) return 3;
            table[d_row + reach] = (int16_t)w;               // (|d_row| <= reach here, as in the kernel)
            pixels += 2 * w + 1;
        }
        if (table[reach] != reach) return 4;
        if (max_d2 == 1 || max_d2 == 2 || max_d2 == 25 || max_d2 == 400 || max_d2 == 4096) std::printf("%ld\n", pixels);
    }
    const int refused[] = {
        sdsm_neighbour_halfwidth_inline(0, 0),
        sdsm_neighbour_halfwidth_inline(-1, 0),
        sdsm_neighbour_halfwidth_inline(SDSM_NEIGHBOUR_MAX_D2_INLINE + 1, 0),
        sdsm_neighbour_halfwidth_inline(INT_MAX, 0),
        sdsm_neighbour_halfwidth_inline(INT_MIN, 0),
        sdsm_neighbour_halfwidth_inline(4096, 65),
        sdsm_neighbour_halfwidth_inline(4096, -65),
        sdsm_neighbour_halfwidth_inline(4096, INT_MAX),      // (no d_row * d_row: the range is tested first)
        sdsm_neighbour_halfwidth_inline(4096, INT_MIN),
        sdsm_neighbour_halfwidth_inline(3, 2),
    };
    for (int r : refused)
        if (r != -1) return 5;
    const uint64_t keys[] = {0, 1, ((uint64_t)1 << 32) | 2, ((uint64_t)65534 << 32) | 65535, ~(uint64_t)0 - 1};
    for (int bits = 0; bits <= 40; bits++) {
        const uint64_t capacity = (uint64_t)1 << bits;
        for (uint64_t key : keys)
            if (sdsm_neighbour_slot_inline(key, capacity) >= capacity) return 6;
    }
    if (sdsm_neighbour_slot_inline(((uint64_t)1 << 32) | 2, 1) != 0) return 7;
    return 0;
}
