// Stand-alone check of the host helper sdsm_parts_quad (superdsm_amd/csrc/sdsm_host.cpp, which takes the class from the inline function
// of csrc/sdsm_parts.h that the tile kernel of the connected parts uses), meant to be built as host code with AddressSanitizer and
// UndefinedBehaviorSanitizer linked in: reads lines "a b c d label" from the file argv[1] and writes the class per line to stdout.  Then
// it counts the bit quads of a small mask with a hole, window by window over the zero-padded mask, and checks Euler's number under both
// adjacencies.  Exit status 0 when everything held.
#include <cstdint>
#include <cstdio>

#include "../../include/sdsm.h"

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *fp = std::fopen(argv[1], "r");
    if (!fp) return 2;
    int a, b, c, d, label;
    while (std::fscanf(fp, "%d %d %d %d %d", &a, &b, &c, &d, &label) == 5) std::printf("%d\n", sdsm_parts_quad(a, b, c, d, label));
    std::fclose(fp);
    // the ends of the label range and labels that differ in the high bits only
    if (sdsm_parts_quad(65535, 0, 0, 65535, 65535) != 3 || sdsm_parts_quad(INT32_MIN, INT32_MAX, 0, 0, INT32_MAX) != 1) return 3;
    if (sdsm_parts_quad(65536 + 7, 7, 7, 7, 7) != 2 || sdsm_parts_quad(7, 7, 7, 7, 7) != 0 || sdsm_parts_quad(7, 7, 0, 0, 7) != 0) return 3;
    // a ring of label 5 with one more pixel touching it by a corner: one part and one hole under 8, two parts and one hole under 4
    enum { H = 5, W = 4 };
    static const int32_t map[H][W] = {{5, 5, 5, 0}, {5, 9, 5, 0}, {5, 5, 5, 0}, {0, 0, 0, 5}, {0, 0, 0, 0}};
    auto at = [&](int r, int col) -> int32_t { return r >= 0 && r < H && col >= 0 && col < W ? map[r][col] : 0; };
    long q[4] = {0, 0, 0, 0};
    for (int i = 0; i <= H; i++)
        for (int j = 0; j <= W; j++) q[sdsm_parts_quad(at(i - 1, j - 1), at(i - 1, j), at(i, j - 1), at(i, j), 5)]++;
    if (q[0] + q[1] + q[2] + q[3] != (H + 1) * (W + 1)) return 4;
    const long four = q[1] - q[2] + 2 * q[3], eight = q[1] - q[2] - 2 * q[3];
    if (four % 4 || eight % 4 || four / 4 != 2 - 1 || eight / 4 != 1 - 1) return 5;
    return 0;
}
