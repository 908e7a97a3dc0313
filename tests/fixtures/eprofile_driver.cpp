// eprofile_driver.cpp -- TEST DRIVER (tests/test_eprofile_cpu.py and tests/test_gpu_eprofile.py build it into a scratch directory): yaha_amd/csrc/eprofile_core.h
// -- what one record adds to the error profile, the routines host and device share -- on hand-made clumps, on one thread.  Input (standard input, whitespace
// separated): minMapq nSeqs, then start length per sequence, then the packed reference image -- "@path" of a file with its bytes, or the 4-bit codes as one
// string of hex digits (one digit per base, offset 0 first) --, then nReads and every read's FORWARD 4-bit codes as hex digits ("-": an empty read), then per
// clump: read sro refLen sqo eqo mapQuality reversed nOps and nOps pairs "code length".  Output: one line per clump (0 counted, 1 MAPQ, 2 dropped), then
// "table" and the 1556 words.
#include "../../yaha_amd/csrc/eprofile_core.h"
#include <cstdio>
#include <string>
#include <vector>
static int hexv(char c) { return c >= '0' && c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }
int main()
{
    unsigned q, ns, nr;
    if (scanf("%u %u", &q, &ns) != 2) return 2;
    std::vector<uint32_t> st(ns), ln(ns);
    for (unsigned i = 0; i < ns; i++) if (scanf("%u %u", &st[i], &ln[i]) != 2) return 2;
    static char buf[1 << 22];
    if (scanf("%4194303s", buf) != 1) return 2;
    std::vector<uint8_t> packed;
    if (buf[0] == '@') {
        FILE *f = fopen(buf + 1, "rb"); if (!f) return 3;
        int ch; while ((ch = fgetc(f)) != EOF) packed.push_back((uint8_t)ch);
        fclose(f);
    } else {
        const std::string refHex(buf); packed.assign((refHex.size() + 1) / 2, 0);
        for (size_t i = 0; i < refHex.size(); i++) packed[i >> 1] |= (uint8_t)(hexv(refHex[i]) << ((i & 1) ? 0 : 4));
    }
    if (scanf("%u", &nr) != 1) return 2;
    // (every read's codes in a buffer of exactly its length: a walk that leaves the read is an AddressSanitizer report)
    std::vector<std::vector<uint8_t>> reads(nr);
    for (unsigned r = 0; r < nr; r++) {
        if (scanf("%4194303s", buf) != 1) return 2;
        const std::string rd(buf); if (rd == "-") continue;
        reads[r].resize(rd.size()); for (size_t i = 0; i < rd.size(); i++) reads[r][i] = (uint8_t)hexv(rd[i]);
    }
    std::vector<uint64_t> table((size_t)yeprofile::WORDS, 0);
    const ydepth::Layout L{st.data(), ln.data(), nullptr, ns, 1, q};
    unsigned rd, sro, rl, sqo, eqo, mq, rev, no; bool oob = false;
    while (scanf("%u %u %u %u %u %u %u %u", &rd, &sro, &rl, &sqo, &eqo, &mq, &rev, &no) == 8) {
        if (rd >= nr) return 2;
        std::vector<uint32_t> ops(no);
        for (unsigned k = 0; k < no; k++) { char c; unsigned l; if (scanf(" %c %u", &c, &l) != 2) return 2; ops[k] = YGPU_OP_MAKE(c, l); }
        ygpu_clump c{}; c.sro = sro; c.refLen = (uint16_t)rl; c.sqo = (uint16_t)sqo; c.eqo = (uint16_t)eqo; c.n_ops = no;
        const int g = yeprofile::walkClump(L, c, ops.data(), reads[rd].data(), (uint32_t)reads[rd].size(), rev != 0, mq, packed.data(), packed.size(),
            [&](uint32_t w, uint32_t n) { if (w < (uint32_t)yeprofile::WORDS) table[w] += n; else oob = true; });
        printf("%d\n", g);
    }
    if (oob) return 4;
    printf("table");
    for (size_t w = 0; w < table.size(); w++) printf(" %llu", (unsigned long long)table[w]);
    printf("\n");
    return 0;
}
