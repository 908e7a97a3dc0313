// snv_driver.cpp -- a stand-alone program over yaha_amd/csrc/snv_core.h (tests/test_snv_cpu.py builds it with the sanitizers): the verdict of ysnv::judge for
// every reference channel (N included) and every (r, x, y, other) in 0 .. 12, where x and y are the counts of the first two other channels in channel order, the
// third other channel holds x * y % 5, N holds `other`, DEL other / 2 and INS 3 (which nothing looks at).  Arguments: cM cE cH minAlt minDepth minQual; without
// them the header's defaults.  The first line has the header's default costs.
#include "../../yaha_amd/csrc/snv_core.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    ygpu_snv_params P = {};
    P.cost_match = ysnv::DEFAULT_CM; P.cost_error = ysnv::DEFAULT_CE; P.cost_het = ysnv::DEFAULT_CH; P.min_alt = 2; P.min_depth = 4; P.min_qual = 20;
    if (argc == 7) {
        P.cost_match = (uint32_t)atoi(argv[1]); P.cost_error = (uint32_t)atoi(argv[2]); P.cost_het = (uint32_t)atoi(argv[3]);
        P.min_alt = (uint32_t)atoi(argv[4]); P.min_depth = (uint32_t)atoi(argv[5]); P.min_qual = (uint32_t)atoi(argv[6]);
    }
    printf("defaults %d %d %d %d\n", (int)ysnv::DEFAULT_ERR, (int)ysnv::DEFAULT_CM, (int)ysnv::DEFAULT_CE, (int)ysnv::DEFAULT_CH);
    for (uint32_t rc = 0; rc <= 4; rc++) for (uint32_t r = 0; r <= 12; r++) for (uint32_t x = 0; x <= 12; x++) for (uint32_t y = 0; y <= 12; y++)
        for (uint32_t other = 0; other <= 12; other++) {
            uint32_t row[7] = {0, 0, 0, 0, other, other / 2, 3}; const uint32_t fill[3] = {x, y, x * y % 5}; uint32_t k = 0;
            if (rc < 4) { row[rc] = r; for (uint32_t ch = 0; ch < 4; ch++) if (ch != rc) row[ch] = fill[k++]; }
            else { row[0] = r; row[1] = x; row[2] = y; }
            ygpu_snv_call c = {}; const bool call = ysnv::judge(row, rc, P, &c);
            if (rc == 4) { printf("%u %u %u %u %u none %d\n", rc, r, x, y, other, call ? 1 : 0); continue; }
            printf("%u %u %u %u %u %d %u %u %u %u %u %u %u %u %u %u %u %u\n", rc, r, x, y, other, call ? 1 : 0, ysnv::infoRc(c.info), ysnv::infoAlt(c.info), ysnv::infoGt(c.info),
                c.ref_count, c.alt_count, c.depth, c.other, c.qual, c.gq, c.pl[0], c.pl[1], c.pl[2]);
        }
    return 0;
}
