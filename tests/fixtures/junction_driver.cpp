// junction_driver.cpp -- TEST DRIVER, CPU tier only (tests/test_junctions_cpu.py builds it into a scratch directory): yaha_amd/csrc/junction_core.h -- the
// junctions of one read, the routines host and device share -- on hand-made records.  Input (standard input, whitespace separated): minMapq nSeqs, then start
// length per sequence, then per read: qlen nRecords and per record sro refLen sqo eqo status mapQuality.  Output per read: "read <skipped by MAPQ> <junctions>",
// then one line per junction: ordinal seqA posA strandA seqB posB strandB type qgap.
#include "../../yaha_amd/csrc/junction_core.h"
#include <cstdio>
#include <vector>
int main()
{
    unsigned q, ns;
    if (scanf("%u %u", &q, &ns) != 2) return 2;
    std::vector<uint32_t> st(ns), ln(ns);
    for (unsigned i = 0; i < ns; i++) if (scanf("%u %u", &st[i], &ln[i]) != 2) return 2;
    const ydepth::Layout L = yjunc::layout(st.data(), ln.data(), ns, q);
    unsigned qlen, n, read = 0;
    while (scanf("%u %u", &qlen, &n) == 2) {
        std::vector<ygpu_clump> c(n); std::vector<uint32_t> status(n), mq(n);
        for (unsigned k = 0; k < n; k++) { unsigned sro, rl, sqo, eqo; if (scanf("%u %u %u %u %u %u", &sro, &rl, &sqo, &eqo, &status[k], &mq[k]) != 6) return 2;
            c[k] = ygpu_clump{}; c[k].sro = sro; c[k].refLen = (uint16_t)rl; c[k].sqo = (uint16_t)sqo; c[k].eqo = (uint16_t)eqo; }
        std::vector<ygpu_junction> out; uint32_t skipped = 0;
        const uint32_t nj = yjunc::readJunctions(L, n, qlen, read,
            [&](uint32_t k, const ygpu_clump **cp, uint32_t *s, uint32_t *m) { *cp = &c[k]; *s = status[k]; *m = mq[k]; }, [&](const ygpu_junction &j) { out.push_back(j); }, &skipped);
        if (nj != out.size()) return 3;
        printf("read %u %u\n", skipped, nj);
        for (const ygpu_junction &j : out) { if (j.read != read) return 4;
            printf("%u %u %u %c %u %u %c %u %d\n", j.ordinal, j.seqA, j.posA, j.strandA, j.seqB, j.posB, j.strandB, j.type, j.qgap); }
        read++;
    }
    return 0;
}
