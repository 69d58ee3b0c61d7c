// Stand-alone check of the host helpers sdsm_texture_level and sdsm_texture_cell (superdsm_amd/csrc/sdsm_host.cpp, the inline functions of
// csrc/sdsm_texture.h that the texture kernels use), meant to be built as host code with AddressSanitizer and UndefinedBehaviorSanitizer
// linked in.  Reads from the file argv[1] a line "n_edges" and n_edges edges (hexadecimal floats), then lines "value"; writes the level of
// every value to stdout, one per line.  Then walks every cell of the packed triangle at 1, 2 and 256 levels: the places must count up from
// 0 in (i, j) order to levels * (levels + 1) / 2 - 1.  Exit status 0 when every accepted call succeeded and every rejected one was refused.
#include <cstdio>
#include <limits>
#include <vector>

#include "../../include/sdsm.h"

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *fp = std::fopen(argv[1], "r");
    if (!fp) return 2;
    int n_edges = -1;
    if (std::fscanf(fp, "%d", &n_edges) != 1 || n_edges < 0 || n_edges > SDSM_TEXTURE_MAX_LEVELS - 1) { std::fclose(fp); return 2; }
    std::vector<double> edges(n_edges);                                   // exactly n_edges doubles: a read past them is the sanitizer's to find
    for (int k = 0; k < n_edges; k++)
        if (std::fscanf(fp, "%la", &edges[k]) != 1) { std::fclose(fp); return 2; }
    double v;
    while (std::fscanf(fp, "%la", &v) == 1) {
        const int level = sdsm_texture_level(n_edges ? edges.data() : nullptr, n_edges, v);
        if (level < 0 || level > n_edges) { std::fclose(fp); return 1; }
        std::printf("%d\n", level);
    }
    std::fclose(fp);
    for (int levels : {1, 2, SDSM_TEXTURE_MAX_LEVELS}) {
        int place = 0;
        for (int i = 0; i < levels; i++)
            for (int j = i; j < levels; j++)
                if (sdsm_texture_cell(levels, i, j) != place++) return 4;
        if (place != levels * (levels + 1) / 2) return 4;
    }
    const double one = 1.0, inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int refused[] = {
        sdsm_texture_level(&one, -1, 0.0),
        sdsm_texture_level(&one, SDSM_TEXTURE_MAX_LEVELS, 0.0),           // 256 edges would be 257 levels
        sdsm_texture_level(nullptr, 1, 0.0),
        sdsm_texture_level(&one, 1, inf),
        sdsm_texture_level(&one, 1, -inf),
        sdsm_texture_level(&one, 1, nan),
        sdsm_texture_cell(0, 0, 0),
        sdsm_texture_cell(SDSM_TEXTURE_MAX_LEVELS + 1, 0, 0),
        sdsm_texture_cell(4, 2, 1),                                       // below the diagonal
        sdsm_texture_cell(4, -1, 1),
        sdsm_texture_cell(4, 1, 4),
    };
    for (int r : refused)
        if (r != -1) return 3;
    return 0;
}
