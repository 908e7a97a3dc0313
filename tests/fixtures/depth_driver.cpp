// depth_driver.cpp -- TEST DRIVER, CPU tier only (tests/test_depth_cpu.py builds it into a scratch directory): yaha_amd/csrc/depth_core.h -- the walk of one record
// that host and device share -- on hand-made clumps.  Input (standard input, whitespace separated): bin minMapq nSeqs, then start length per sequence, then per
// clump: sro refLen mapQuality nOps and nOps pairs "code length".  Output: one line "result bases" per clump (0 counted, 1 MAPQ, 2 dropped), then "bins" and
// every bin's count.
#include "../../yaha_amd/csrc/depth_core.h"
#include <cstdio>
#include <vector>
int main()
{
    unsigned bin, q, ns;
    if (scanf("%u %u %u", &bin, &q, &ns) != 3) return 2;
    std::vector<uint32_t> st(ns), ln(ns), base(ns + 1);
    for (unsigned i = 0; i < ns; i++) if (scanf("%u %u", &st[i], &ln[i]) != 2) return 2;
    uint64_t nb = 0;
    if (!ydepth::layoutBins(ln.data(), ns, bin, base.data(), &nb)) return 3;
    std::vector<uint32_t> cov(nb, 0);
    const ydepth::Layout L{st.data(), ln.data(), base.data(), ns, bin, q};
    unsigned sro, rl, mq, no;
    while (scanf("%u %u %u %u", &sro, &rl, &mq, &no) == 4) {
        std::vector<uint32_t> ops(no);
        for (unsigned k = 0; k < no; k++) { char c; unsigned l; if (scanf(" %c %u", &c, &l) != 2) return 2; ops[k] = YGPU_OP_MAKE(c, l); }
        ygpu_clump c{}; c.sro = sro; c.refLen = (uint16_t)rl; c.n_ops = no;
        uint64_t bases = 0; bool oob = false;
        const int g = ydepth::walkClump(L, c, ops.data(), mq, [&](uint32_t b, uint32_t n) { if (b < nb) cov[b] += n; else oob = true; }, &bases);
        if (oob) return 4;
        printf("%d %llu\n", g, (unsigned long long)bases);
    }
    printf("bins");
    for (uint64_t b = 0; b < nb; b++) printf(" %u", cov[b]);
    printf("\n");
    return 0;
}
