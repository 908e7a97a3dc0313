// events_driver.cpp -- TEST DRIVER, CPU tier only (tests/test_events_cpu.py builds it into a scratch directory): yaha_amd/csrc/events_core.h -- what one record
// adds to the evidence track, the routine host and device share -- on hand-made clumps.  Input (standard input, whitespace separated): bin minMapq minClip nSeqs,
// then start length per sequence, then per clump: sro refLen sqo eqo qlen mapQuality nOps and nOps pairs "code length".  Output: one line "result" per clump
// (0 counted, 1 MAPQ, 2 dropped), then "bins" and every bin's five counts, bin-major.
#include "../../yaha_amd/csrc/events_core.h"
#include <cstdio>
#include <vector>
int main()
{
    unsigned bin, q, clip, ns;
    if (scanf("%u %u %u %u", &bin, &q, &clip, &ns) != 4) return 2;
    std::vector<uint32_t> st(ns), ln(ns), base(ns + 1);
    for (unsigned i = 0; i < ns; i++) if (scanf("%u %u", &st[i], &ln[i]) != 2) return 2;
    uint64_t nb = 0;
    if (!ydepth::layoutBins(ln.data(), ns, bin, base.data(), &nb)) return 3;
    std::vector<uint32_t> ev(nb * yevents::NCH, 0);
    const ydepth::Layout L{st.data(), ln.data(), base.data(), ns, bin, q};
    unsigned sro, rl, sqo, eqo, qlen, mq, no;
    while (scanf("%u %u %u %u %u %u %u", &sro, &rl, &sqo, &eqo, &qlen, &mq, &no) == 7) {
        std::vector<uint32_t> ops(no);
        for (unsigned k = 0; k < no; k++) { char c; unsigned l; if (scanf(" %c %u", &c, &l) != 2) return 2; ops[k] = YGPU_OP_MAKE(c, l); }
        ygpu_clump c{}; c.sro = sro; c.refLen = (uint16_t)rl; c.sqo = (uint16_t)sqo; c.eqo = (uint16_t)eqo; c.n_ops = no;
        bool oob = false;
        const int g = yevents::walkClump(L, clip, c, ops.data(), qlen, mq, [&](uint32_t b, uint32_t ch, uint32_t n) {
            if (b < nb && ch < (uint32_t)yevents::NCH) ev[(size_t)b * yevents::NCH + ch] += n; else oob = true; });
        if (oob) return 4;
        printf("%d\n", g);
    }
    printf("bins");
    for (size_t w = 0; w < ev.size(); w++) printf(" %u", ev[w]);
    printf("\n");
    return 0;
}
