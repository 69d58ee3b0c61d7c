// Stand-alone check of the host helpers sdsm_depth_shell and sdsm_depth_workspace_pixels (superdsm_amd/csrc/sdsm_host.cpp, which takes the
// shell from the inline function of csrc/sdsm_depth.h that the depth kernel uses), meant to be built as host code with AddressSanitizer
// and UndefinedBehaviorSanitizer linked in: reads lines "d2 n_shells" from the file argv[1], writes the shell per line to stdout, and makes
// the rejected calls.  Exit status 0 when every rejected call was refused and the workspace rule held on both sides of the cap.
#include <cstdint>
#include <cstdio>

#include "../../include/sdsm.h"

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *fp = std::fopen(argv[1], "r");
    if (!fp) return 2;
    long long d2;
    int n_shells;
    while (std::fscanf(fp, "%lld %d", &d2, &n_shells) == 2) std::printf("%d\n", sdsm_depth_shell(d2, n_shells));
    std::fclose(fp);
    const int refused[] = {
        sdsm_depth_shell(0, 8),                                           // no depth
        sdsm_depth_shell(-1, 8),
        sdsm_depth_shell(INT64_MIN, 8),
        sdsm_depth_shell(1ll << 31, 8),                                   // beyond every image
        sdsm_depth_shell(INT64_MAX, 8),
        sdsm_depth_shell(5, 0),
        sdsm_depth_shell(5, -3),
        sdsm_depth_shell(5, SDSM_DEPTH_MAX_SHELLS + 1),
    };
    for (int r : refused)
        if (r != -1) return 3;
    if (sdsm_depth_shell((1ll << 31) - 1, 32) != 31 || sdsm_depth_shell(1, 1) != 0) return 4;
    if (sdsm_depth_workspace_pixels(1, SDSM_DEPTH_LDS_PIXELS) != 0 || sdsm_depth_workspace_pixels(1, SDSM_DEPTH_LDS_PIXELS + 1) != SDSM_DEPTH_LDS_PIXELS + 1) return 5;
    if (sdsm_depth_workspace_pixels(0, 5) != 0 || sdsm_depth_workspace_pixels(5, -1) != 0 || sdsm_depth_workspace_pixels(65535, 32768) != 65535ll * 32768) return 6;
    return 0;
}
