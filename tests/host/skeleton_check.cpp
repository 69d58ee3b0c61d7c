// Stand-alone check of the host helpers sdsm_skeleton_deletable, sdsm_skeleton_workspace_words and sdsm_skeleton_thin
// (superdsm_amd/csrc/sdsm_host.cpp, which takes the word functions from csrc/sdsm_skeleton.h that the skeleton kernel uses), meant to be
// built as host code with AddressSanitizer and UndefinedBehaviorSanitizer linked in: reads lines "h w <h w characters 0 / 1>" from the file
// argv[1], thins each mask from exactly sized buffers -- once into a second buffer, once in place -- and writes "cycles <bits>" per line to
// stdout; then makes the rejected calls.  Exit status 0 when both thinnings agreed, every rejected call was refused and the workspace rule
// held on both sides of the limits.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/sdsm.h"

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *fp = std::fopen(argv[1], "r");
    if (!fp) return 2;
    int h, w;
    while (std::fscanf(fp, "%d %d", &h, &w) == 2) {
        if (h < 1 || w < 1 || (long long)h * w > 1000000) return 2;
        const size_t n = (size_t)h * w, words = (n + 31) / 32;
        std::string text(n + 1, '\0');
        if (std::fscanf(fp, (" %" + std::to_string(n) + "s").c_str(), &text[0]) != 1) return 2;
        std::vector<uint32_t> bits(words, 0), out(words, 0xffffffffu);       // exactly the words of the window: a read or write past them is caught
        for (size_t p = 0; p < n; p++)
            if (text[p] == '1') bits[p >> 5] |= 1u << (p & 31);
        if (n & 31) bits[words - 1] |= ~0u << (n & 31);                       // garbage past h w: ignored
        const int cycles = sdsm_skeleton_thin(h, w, bits.data(), out.data());
        const int again = sdsm_skeleton_thin(h, w, bits.data(), bits.data());
        if (cycles < 0 || again != cycles || bits != out) return 7;
        std::string line(n, '0');
        for (size_t p = 0; p < n; p++)
            if ((out[p >> 5] >> (p & 31)) & 1u) line[p] = '1';
        std::printf("%d %s\n", cycles, line.c_str());
    }
    std::fclose(fp);
    uint32_t one = 1;
    const int refused[] = {
        sdsm_skeleton_thin(0, 1, &one, &one),
        sdsm_skeleton_thin(1, 0, &one, &one),
        sdsm_skeleton_thin(-3, 4, &one, &one),
        sdsm_skeleton_thin(65536, 32768, &one, &one),                         // h w = 2^31
        sdsm_skeleton_thin(1, 1, nullptr, &one),
        sdsm_skeleton_thin(1, 1, &one, nullptr),
        sdsm_skeleton_deletable(256, 0),
        sdsm_skeleton_deletable(-1, 0),
        sdsm_skeleton_deletable(28, 1),
        sdsm_skeleton_deletable(28, 8),
    };
    for (int r : refused)
        if (r != -1) return 3;
    if (sdsm_skeleton_thin(1, 1, &one, &one) != 0 || one != 1) return 4;
    int count[4] = {0, 0, 0, 0};
    for (int code = 0; code < 256; code++)
        for (int k = 0; k < 4; k++) count[k] += sdsm_skeleton_deletable(code, 2 * k);
    for (int c : count)
        if (c != 41) return 5;
    if (sdsm_skeleton_workspace_words(64, 64) != 0 || sdsm_skeleton_workspace_words(SDSM_SKELETON_LDS_WORDS, 64) != 0 ||
        sdsm_skeleton_workspace_words(SDSM_SKELETON_LDS_WORDS + 1, 64) != 2 * (SDSM_SKELETON_LDS_WORDS + 1) || sdsm_skeleton_workspace_words(0, 5) != 0 ||
        sdsm_skeleton_workspace_words(5, -1) != 0 || sdsm_skeleton_workspace_words(65535, 32768) != 2ll * 65535 * 512)
        return 6;
    return 0;
}
