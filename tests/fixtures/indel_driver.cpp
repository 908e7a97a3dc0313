// indel_driver.cpp -- TEST DRIVER, CPU tier only (tests/test_indels_cpu.py builds it into a scratch directory): yaha_amd/csrc/indel_core.h -- the indel events
// of one record and their keys, the routines host and device share -- on hand-made clumps, on one thread.  Input (standard input, whitespace separated):
// minMapq minLen nSeqs, then start length per sequence, then per clump: sro refLen sqo eqo mapQuality reversed nOps, nOps pairs "code length", and the read's
// FORWARD 4-bit codes as hex digits.  Output: one line per clump -- the result (0 counted, 1 MAPQ, 2 dropped), then every event as slot:type:length:bases in
// walk order (bases: the kept channels as digits, A0 C1 G2 T3 N4, '*' for a deletion) followed by the three key words in hex -- and a last line "order" with
// the indices of all events sorted by keyLess.
#include "../../yaha_amd/csrc/indel_core.h"
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>
static int hexv(char c) { return c >= '0' && c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }
int main()
{
    unsigned q, minLen, ns;
    if (scanf("%u %u %u", &q, &minLen, &ns) != 3) return 2;
    std::vector<uint32_t> st(ns), ln(ns), base(ns + 1);
    for (unsigned i = 0; i < ns; i++) if (scanf("%u %u", &st[i], &ln[i]) != 2) return 2;
    uint64_t nb = 0;
    if (!ydepth::layoutBins(ln.data(), ns, 1, base.data(), &nb)) return 3;
    const ydepth::Layout L{st.data(), ln.data(), base.data(), ns, 1, q};
    static char buf[1 << 20];
    std::vector<yindel::Key> all;
    unsigned sro, rl, sqo, eqo, mq, rev, no;
    while (scanf("%u %u %u %u %u %u %u", &sro, &rl, &sqo, &eqo, &mq, &rev, &no) == 7) {
        std::vector<uint32_t> ops(no);
        for (unsigned k = 0; k < no; k++) { char c; unsigned l; if (scanf(" %c %u", &c, &l) != 2) return 2; ops[k] = YGPU_OP_MAKE(c, l); }
        if (scanf("%1048575s", buf) != 1) return 2;
        const std::string rd(buf);
        // (the codes in a buffer of exactly the read's length: a walk that leaves the read is an AddressSanitizer report)
        std::vector<uint8_t> fwd(rd.size()); for (size_t i = 0; i < rd.size(); i++) fwd[i] = (uint8_t)hexv(rd[i]);
        ygpu_clump c{}; c.sro = sro; c.refLen = (uint16_t)rl; c.sqo = (uint16_t)sqo; c.eqo = (uint16_t)eqo; c.n_ops = no;
        std::vector<yindel::Key> mine;
        const int g = yindel::walkClump(L, c, ops.data(), fwd.data(), (uint32_t)fwd.size(), rev != 0, mq, minLen, [&](const yindel::Key &k) { mine.push_back(k); });
        printf("%d", g);
        for (const yindel::Key &k : mine) {
            if (!k.w0 || !k.w1 || !k.w2 || yindel::slotOfKey(k) >= nb) return 4;
            printf(" %u:%u:%u:", yindel::slotOfKey(k), yindel::typeOfKey(k), yindel::lenOfKey(k));
            if (yindel::typeOfKey(k) == (uint32_t)yindel::DEL) printf("*");
            for (uint32_t i = 0; i < yindel::keptOfKey(k); i++) printf("%u", yindel::baseOfKey(k, i));
            printf(":%llx:%llx:%llx", (unsigned long long)k.w0, (unsigned long long)k.w1, (unsigned long long)k.w2);
            all.push_back(k);
        }
        printf("\n");
    }
    std::vector<size_t> idx(all.size()); for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return yindel::keyLess(all[a], all[b]); });
    printf("order");
    for (size_t i : idx) printf(" %zu", i);
    printf("\n");
    return 0;
}
