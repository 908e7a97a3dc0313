// pileup_driver.cpp -- TEST DRIVER, CPU tier only (tests/test_pileup_cpu.py builds it into a scratch directory): yaha_amd/csrc/pileup_core.h -- what one record
// adds to the allele pileup and what a site is, the routines host and device share -- on hand-made clumps, on one thread.  Input (standard input, whitespace
// separated): minMapq minAlt nSeqs, then start length per sequence, then the reference's 4-bit codes as one string of hex digits (one digit per base of the
// image, offset 0 first), then per clump: sro refLen sqo eqo mapQuality reversed nOps, nOps pairs "code length", and the read's FORWARD 4-bit codes as hex
// digits.  Output: one line "result" per clump (0 counted, 1 MAPQ, 2 dropped), then "slots" and every slot's seven counts, slot-major, then "codes" and the
// channel chOfRead gives each of the 16 codes on a reversed read, then "candidates" (nonref >= 1) and "sites" (nonref >= minAlt) as slot numbers.
#include "../../yaha_amd/csrc/pileup_core.h"
#include <cstdio>
#include <string>
#include <vector>
static int hexv(char c) { return c >= '0' && c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }
int main()
{
    unsigned q, minAlt, ns;
    if (scanf("%u %u %u", &q, &minAlt, &ns) != 3) return 2;
    std::vector<uint32_t> st(ns), ln(ns), base(ns + 1);
    for (unsigned i = 0; i < ns; i++) if (scanf("%u %u", &st[i], &ln[i]) != 2) return 2;
    static char buf[1 << 20];
    if (scanf("%1048575s", buf) != 1) return 2;
    const std::string refHex(buf); std::vector<uint8_t> packed((refHex.size() + 1) / 2, 0);
    for (size_t i = 0; i < refHex.size(); i++) packed[i >> 1] |= (uint8_t)(hexv(refHex[i]) << ((i & 1) ? 0 : 4));
    uint64_t nb = 0;
    if (!ydepth::layoutBins(ln.data(), ns, 1, base.data(), &nb)) return 3;
    std::vector<uint32_t> pu(nb * ypileup::NCH, 0);
    const ydepth::Layout L{st.data(), ln.data(), base.data(), ns, 1, q};
    unsigned sro, rl, sqo, eqo, mq, rev, no;
    while (scanf("%u %u %u %u %u %u %u", &sro, &rl, &sqo, &eqo, &mq, &rev, &no) == 7) {
        std::vector<uint32_t> ops(no);
        for (unsigned k = 0; k < no; k++) { char c; unsigned l; if (scanf(" %c %u", &c, &l) != 2) return 2; ops[k] = YGPU_OP_MAKE(c, l); }
        if (scanf("%1048575s", buf) != 1) return 2;
        const std::string rd(buf);
        // (the codes in a buffer of exactly the read's length: a walk that leaves the read is an AddressSanitizer report)
        std::vector<uint8_t> fwd(rd.size()); for (size_t i = 0; i < rd.size(); i++) fwd[i] = (uint8_t)hexv(rd[i]);
        ygpu_clump c{}; c.sro = sro; c.refLen = (uint16_t)rl; c.sqo = (uint16_t)sqo; c.eqo = (uint16_t)eqo; c.n_ops = no;
        bool oob = false;
        const int g = ypileup::walkClump(L, c, ops.data(), fwd.data(), (uint32_t)fwd.size(), rev != 0, mq, [&](uint32_t s, uint32_t ch) {
            if (s < nb && ch < (uint32_t)ypileup::NCH) pu[(size_t)s * ypileup::NCH + ch] += 1; else oob = true; });
        if (oob) return 4;
        printf("%d\n", g);
    }
    printf("slots");
    for (size_t w = 0; w < pu.size(); w++) printf(" %u", pu[w]);
    printf("\ncodes");
    for (unsigned code = 0; code < 16; code++) { const uint8_t one = (uint8_t)code; printf(" %u", ypileup::chOfRead(&one, 1, 0, true)); }
    printf("\ncandidates");
    for (uint32_t s = 0; s < nb; s++) if (ypileup::isSiteAt(L, packed.data(), packed.size(), s, &pu[(size_t)s * ypileup::NCH], 1u)) printf(" %u", s);
    printf("\nsites");
    for (uint32_t s = 0; s < nb; s++) if (ypileup::isSite(&pu[(size_t)s * ypileup::NCH], ypileup::refCh(L, packed.data(), packed.size(), s), minAlt)) printf(" %u", s);
    printf("\n");
    return 0;
}
