// Stand-alone check of the host helper sdsm_quantile_ranks (superdsm_amd/csrc/sdsm_host.cpp), meant to be built as host code with
// AddressSanitizer and UndefinedBehaviorSanitizer linked in: reads lines "n num den" from the file argv[1], writes "lo hi rem" per line
// to stdout, and makes the rejected calls.  Exit status 0 when every accepted call succeeded and every rejected one was refused.
#include <cinttypes>
#include <cstdint>
#include <cstdio>

#include "../../include/sdsm.h"

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *fp = std::fopen(argv[1], "r");
    if (!fp) return 2;
    long long n;
    int num, den;
    while (std::fscanf(fp, "%lld %d %d", &n, &num, &den) == 3) {
        int64_t lo = -1, hi = -1, rem = -1;
        if (sdsm_quantile_ranks(n, num, den, &lo, &hi, &rem) != SDSM_OK) { std::fclose(fp); return 1; }
        std::printf("%" PRId64 " %" PRId64 " %" PRId64 "\n", lo, hi, rem);
    }
    std::fclose(fp);
    int64_t lo, hi, rem;
    const int refused[] = {
        sdsm_quantile_ranks(0, 1, 2, &lo, &hi, &rem),                     // no value
        sdsm_quantile_ranks(1ll << 31, 1, 2, &lo, &hi, &rem),             // more than 2^31 - 1 values
        sdsm_quantile_ranks(5, 3, 2, &lo, &hi, &rem),                     // above 1
        sdsm_quantile_ranks(5, -1, 2, &lo, &hi, &rem),                    // below 0
        sdsm_quantile_ranks(5, 1, 0, &lo, &hi, &rem),
        sdsm_quantile_ranks(5, 1, SDSM_INTENSITY_MAX_DEN + 1, &lo, &hi, &rem),
        sdsm_quantile_ranks(5, 1, 2, nullptr, &hi, &rem),
    };
    for (int r : refused)
        if (r != SDSM_ERR_ARGUMENT) return 3;
    return 0;
}
