// indelcall_driver.cpp -- a stand-alone program over yaha_amd/csrc/indelcall_core.h (tests/test_indelcall_cpu.py builds it with the sanitizers): it reads a
// crafted reference, raw alleles, pileup rows and parameters from the file named by its argument, normalises and merges the alleles with the core's one-thread
// routines and judges every merged allele.  Input, one item a line:
//   S n                      then n lines "start length": the sequences' offsets in the base image and their lengths
//   B letters                the base image, one letter an offset (A C G T, anything else N), packed here two a byte as the .nib2 has them
//   M max_shift
//   P cM cE cH minAlt minDepth minQual
//   A n                      then n lines "w0 w1 w2 count" (decimal)
//   R n                      then n lines "slot r0 .. r6"
// Output: "stats raw shifted merged skipped", then per merged allele in keyLess order "w0 w1 w2 count call a r d qual gq pl0 pl1 pl2 info".
#include "../../yaha_amd/csrc/indelcall_core.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

struct Less { bool operator()(const yindel::Key &a, const yindel::Key &b) const { return yindel::keyLess(a, b); } };

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r"); if (!f) return 2;
    std::vector<uint32_t> start, length; std::vector<uint8_t> packed; uint32_t maxShift = 256; ygpu_indelcall_params P = {};
    std::vector<ygpu_indel_entry> raw; std::map<uint32_t, std::vector<uint32_t>> rows;
    char tag; unsigned long long n;
    while (fscanf(f, " %c", &tag) == 1) {
        if (tag == 'S') { if (fscanf(f, "%llu", &n) != 1) return 2; for (unsigned long long i = 0; i < n; i++) { unsigned a, b; if (fscanf(f, "%u %u", &a, &b) != 2) return 2;
            start.push_back(a); length.push_back(b); } }
        else if (tag == 'B') {
            std::string s; int c; while ((c = fgetc(f)) == ' ') {} for (; c != EOF && c != '\n'; c = fgetc(f)) s.push_back((char)c);
            packed.assign((s.size() + 1) / 2, 0x44);
            for (size_t i = 0; i < s.size(); i++) {
                const uint8_t code = s[i] == 'T' ? 0 : s[i] == 'C' ? 1 : s[i] == 'A' ? 2 : s[i] == 'G' ? 3 : 4;
                packed[i >> 1] = (i & 1) ? (uint8_t)((packed[i >> 1] & 0xF0) | code) : (uint8_t)((packed[i >> 1] & 0x0F) | code << 4);
            }
        }
        else if (tag == 'M') { if (fscanf(f, "%u", &maxShift) != 1) return 2; }
        else if (tag == 'P') { if (fscanf(f, "%u %u %u %u %u %u", &P.cost_match, &P.cost_error, &P.cost_het, &P.min_alt, &P.min_depth, &P.min_qual) != 6) return 2; }
        else if (tag == 'A') { if (fscanf(f, "%llu", &n) != 1) return 2; for (unsigned long long i = 0; i < n; i++) { unsigned long long a, b, c; unsigned cnt;
            if (fscanf(f, "%llu %llu %llu %u", &a, &b, &c, &cnt) != 4) return 2; raw.push_back(ygpu_indel_entry{a, b, c, cnt, 0u}); } }
        else if (tag == 'R') { if (fscanf(f, "%llu", &n) != 1) return 2; for (unsigned long long i = 0; i < n; i++) { unsigned s; std::vector<uint32_t> r(7);
            if (fscanf(f, "%u %u %u %u %u %u %u %u", &s, &r[0], &r[1], &r[2], &r[3], &r[4], &r[5], &r[6]) != 8) return 2; rows[s] = r; } }
        else return 2;
    }
    fclose(f);
    std::vector<uint32_t> binBase(start.size() + 1, 0); uint64_t nSlots = 0;
    if (!ydepth::layoutBins(length.data(), (uint32_t)length.size(), 1, binBase.data(), &nSlots)) return 2;
    const ydepth::Layout L{start.data(), length.data(), binBase.data(), (uint32_t)start.size(), 1u, 0u};
    std::map<yindel::Key, uint64_t, Less> merged; unsigned long long shifted = 0, skipped = 0;
    for (const ygpu_indel_entry &e : raw) {
        const yindel::Key k{e.w0, e.w1, e.w2}; uint32_t seq = 0, cap = 0;
        if (!yindelcall::callable(L, nSlots, k, maxShift, &seq, &cap)) { skipped++; continue; }
        const uint32_t s = yindelcall::shiftOf(L, packed.data(), packed.size(), seq, k, cap);
        shifted += s != 0;
        merged[yindelcall::shifted(k, s)] += e.count;
    }
    printf("stats %zu %llu %llu %llu\n", raw.size(), shifted, (unsigned long long)(raw.size() - skipped - merged.size()), skipped);
    const std::vector<uint32_t> zero(7, 0);
    for (const auto &m : merged) {
        const uint32_t anchor = yindel::slotOfKey(m.first) - 1u; const auto at = rows.find(anchor);
        ygpu_indel_call c = {}; const uint32_t count = ysnv::sat32(m.second);
        const bool call = yindelcall::judgeAt(L, packed.data(), packed.size(), m.first, count, (at == rows.end() ? zero : at->second).data(), P, &c);
        printf("%llu %llu %llu %u %d %u %u %u %u %u %u %u %u %u\n", (unsigned long long)c.w0, (unsigned long long)c.w1, (unsigned long long)c.w2, count, call ? 1 : 0,
            c.alt_count, c.ref_count, c.depth, c.qual, c.gq, c.pl[0], c.pl[1], c.pl[2], c.info);
    }
    return 0;
}
