// oqc_driver.cpp -- TEST DRIVER, CPU tier only (tests/test_oqc_model.py builds it into a scratch directory under AddressSanitizer and UBSan): the post-filter of one
// read as yaha_amd/csrc/oqc_core.h states it -- yoqc::run, the one-thread routine the host compiles and the device stage takes its steps from -- on clump lists
// given on standard input, against the plain model of tests/oqc_model.py.
// Input (whitespace separated): GOCost GECost RCost MScore minNonOverlap BPCost maxBPLog FBS, FBS_PSLength and FBS_PSScore as the 32 bits of the floats; nSeqs, then
// start length per sequence; nReads; per read: qlen nClumps, the read's FORWARD 4-bit codes as hex digits ("-" for a read of no bases), then per clump: sro sqo eqo
// refLen totScore totLength status nOps and nOps pairs "code length".
// Output, per read: "read primaryCount m", then m lines "clump status mapQuality numSecondaries matchedPrimary" in print order.
// Every scratch array is an allocation of its own of exactly the size the header's comment promises -- keys n, stack 4 n + 8 ints, nodes / tbl / path n, one pool of
// sum(2 n_ops + 3) ints, prim / pa / push n, out n -- so that a step beyond any of them is a sanitizer report.
// The break point thresholds are RESTATED here (the bisection of host/oqc.cpp BPPTable::build, with the header's exactBPP): the host's table type is private to its
// translation unit.
#include "../../yaha_amd/csrc/oqc_core.h"
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
static int hexv(char c) { return c >= '0' && c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }
int main()
{
    yoqc::Params P; unsigned fbs, psl, pss, ns, nReads;
    if (scanf("%d %d %d %d %d %d %d %u %u %u", &P.GOCost, &P.GECost, &P.RCost, &P.MScore, &P.minNonOverlap, &P.BPCost, &P.maxBPLog, &fbs, &psl, &pss) != 10) return 2;
    P.FBS = (int)fbs; memcpy(&P.FBS_PSLength, &psl, 4); memcpy(&P.FBS_PSScore, &pss, 4);
    std::vector<uint32_t> thr;
    P.bppVmin = yoqc::exactBPP(11, P.BPCost, P.maxBPLog);
    { const int vmax = yoqc::exactBPP(0xFFFFFFFFu, P.BPCost, P.maxBPLog);
      for (int v = P.bppVmin + 1; v <= vmax; v++) {                          // smallest distance whose penalty is >= v
          uint64_t lo = 11, hi = 0xFFFFFFFFull;
          while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (yoqc::exactBPP((uint32_t)mid, P.BPCost, P.maxBPLog) >= v) hi = mid; else lo = mid + 1; }
          thr.push_back((uint32_t)lo);
      } }
    P.bppN = (int)thr.size(); P.bppThr = thr.data();
    if (scanf("%u", &ns) != 1) return 2;
    std::vector<uint32_t> st(ns), ln(ns);
    for (unsigned i = 0; i < ns; i++) if (scanf("%u %u", &st[i], &ln[i]) != 2) return 2;
    const yoqc::Seqs G{st.data(), ln.data(), ns};
    if (scanf("%u", &nReads) != 1) return 2;
    static char buf[1 << 17];
    for (unsigned r = 0; r < nReads; r++) {
        unsigned qlen, n;
        if (scanf("%u %u %131071s", &qlen, &n, buf) != 3) return 2;
        if (qlen && strlen(buf) != qlen) return 3;
        std::unique_ptr<uint8_t[]> codes(new uint8_t[qlen ? qlen : 1]);
        for (unsigned i = 0; i < qlen; i++) codes[i] = (uint8_t)hexv(buf[i]);
        std::unique_ptr<ygpu_clump[]> cl(new ygpu_clump[n ? n : 1]); std::vector<uint32_t> opsv; size_t poolInts = 0;
        for (unsigned k = 0; k < n; k++) {
            unsigned sro, sqo, eqo, rl, sc, tl, stt, no;
            if (scanf("%u %u %u %u %u %u %u %u", &sro, &sqo, &eqo, &rl, &sc, &tl, &stt, &no) != 8) return 2;
            ygpu_clump c; memset(&c, 0, sizeof c);
            c.sro = sro; c.sqo = (uint16_t)sqo; c.eqo = (uint16_t)eqo; c.refLen = (uint16_t)rl; c.totScore = (uint16_t)sc; c.totLength = (uint16_t)tl; c.status = (uint8_t)stt;
            c.op_start = (uint32_t)opsv.size(); c.n_ops = no;
            for (unsigned j = 0; j < no; j++) { char code; unsigned l; if (scanf(" %c %u", &code, &l) != 2) return 2; opsv.push_back(YGPU_OP_MAKE(code, l)); }
            cl[k] = c; poolInts += 2 * (size_t)no + 3;
        }
        if (n == 0) { printf("read 0 0\n"); continue; }                       // (postFilterBySimilarity returns at once, :903-904; the host never calls run() for such a read)
        std::unique_ptr<uint32_t[]> ops(new uint32_t[opsv.size() ? opsv.size() : 1]); memcpy(ops.get(), opsv.data(), 4 * opsv.size());
        std::unique_ptr<yoqc::SortKey[]> keys(new yoqc::SortKey[n]); std::unique_ptr<int[]> stack(new int[4 * (size_t)n + 8]), tbl(new int[n]), path(new int[n]), pool(new int[poolInts]);
        std::unique_ptr<yoqc::CNode[]> nodes(new yoqc::CNode[n]), prim(new yoqc::CNode[n]); std::unique_ptr<yoqc::PAttr[]> pa(new yoqc::PAttr[n]);
        std::unique_ptr<yoqc::OutRec[]> push(new yoqc::OutRec[n]), out(new yoqc::OutRec[n]);
        yoqc::Scratch S{keys.get(), stack.get(), (int)(4 * (size_t)n + 8), nullptr, nodes.get(), tbl.get(), path.get(), pool.get(), (int)poolInts, nullptr, prim.get(), pa.get(), push.get()};
        int pc = 0;
        const int m = yoqc::run(P, G, cl.get(), (int)n, ops.get(), (int)qlen, codes.get(), S, out.get(), &pc);
        printf("read %d %d\n", pc, m);
        for (int k = 0; k < m; k++) printf("%d %u %u %u %u\n", out[k].clump, out[k].status, out[k].mapQuality, out[k].numSecondaries, out[k].matchedPrimary);
    }
    return 0;
}
