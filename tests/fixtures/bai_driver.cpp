// bai_driver.cpp -- the index of a sorted BAM (yaha_amd/csrc/bai_core.h through host/bai.cpp) and the host's ordering as a program of its own, for
// tests/test_bamsort_cpu.py: built plainly and under AddressSanitizer + UBSan, started as a process.  `bai_driver IN N_REF OUT`: IN holds one record per line --
// "ref pos span" in arrival order --; the driver makes a minimal BAM record of each (its name is its arrival number), orders them with bamSortOrder, writes
// OUT (header blocks, the sorted records' blocks, the end-of-file block: the host's encoder) and OUT.bai (baiBuild over the blocks' offsets read from BSIZE).
#include "../../yaha_amd/csrc/host/bai.cpp"
#include "../../yaha_amd/csrc/bgzf_core.h"
#include <cstdio>

static void add32(std::string &s, uint32_t v) { for (int k = 0; k < 4; k++) s += (char)(v >> (8 * k)); }
static void add16(std::string &s, uint32_t v) { for (int k = 0; k < 2; k++) s += (char)(v >> (8 * k)); }

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: bai_driver IN N_REF OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "r"); if (!f) { perror(argv[1]); return 2; }
    const size_t nRef = (size_t)atoi(argv[2]);
    std::vector<yaha::BamEntry> entries; std::vector<std::string> recs; unsigned ref, pos, span;
    while (fscanf(f, "%u %u %u", &ref, &pos, &span) == 3) {
        char name[16]; const int ln = snprintf(name, sizeof name, "%zu", recs.size()) + 1;
        const uint32_t end = pos + (span ? span : 1u), bin = ybai::reg2bin(pos, end);
        std::string r; add32(r, 0); add32(r, ref); add32(r, pos); r += (char)ln; r += (char)30; add16(r, bin); add16(r, span ? 1 : 0); add16(r, 0); add32(r, 0);
        add32(r, 0xFFFFFFFFu); add32(r, 0xFFFFFFFFu); add32(r, 0); r.append(name, (size_t)ln); if (span) add32(r, span << 4);
        const uint32_t body = (uint32_t)r.size() - 4u; for (int k = 0; k < 4; k++) r[(size_t)k] = (char)(body >> (8 * k));
        entries.push_back(yaha::BamEntry{ref, pos, (uint32_t)r.size(), end, bin}); recs.push_back(r);
    }
    fclose(f);
    const size_t n = entries.size();
    std::vector<uint32_t> perm(n); yaha::bamSortOrder(entries.data(), n, perm.data());
    std::vector<yaha::BamEntry> sorted(n); std::string stream;
    for (size_t j = 0; j < n; j++) { sorted[j] = entries[perm[j]]; stream += recs[perm[j]]; }
    std::string head = "BAM\1"; const std::string text = "@HD\tVN:1.0\tSO:coordinate\n"; add32(head, (uint32_t)text.size()); head += text; add32(head, (uint32_t)nRef);
    for (size_t k = 0; k < nRef; k++) { char nm[16]; const int ln = snprintf(nm, sizeof nm, "s%zu", k) + 1; add32(head, (uint32_t)ln); head.append(nm, (size_t)ln); add32(head, 1u << 29); }
    std::unique_ptr<ybgzf::HostWork> W(new ybgzf::HostWork);
    std::vector<uint8_t> a(ybgzf::bound(head.size())), b(ybgzf::bound(stream.size()) + 1);
    const uint64_t na = ybgzf::encodeStream((const uint8_t *)head.data(), head.size(), a.data(), *W, nullptr, nullptr);
    const uint64_t nb = ybgzf::encodeStream((const uint8_t *)stream.data(), stream.size(), b.data(), *W, nullptr, nullptr);
    std::vector<uint64_t> coffs(ybgzf::blocksOf(stream.size()) + 1); size_t nBlocks = 0;
    const uint64_t end = nb ? ybai::blockOffsets(b.data(), nb, na, coffs.data(), &nBlocks, coffs.size() - 1) : na;
    if (end != na + nb || nBlocks != ybgzf::blocksOf(stream.size())) { fprintf(stderr, "the blocks do not add up\n"); return 3; }
    coffs[nBlocks] = end;
    const std::string bai = yaha::baiBuild(sorted.data(), n, nRef, coffs.data(), nBlocks);
    uint8_t eof[ybgzf::EOF_BYTES]; ybgzf::putEof(eof);
    FILE *o = fopen(argv[3], "wb"); if (!o) { perror(argv[3]); return 2; }
    if (fwrite(a.data(), 1, na, o) != na || (nb && fwrite(b.data(), 1, nb, o) != nb) || fwrite(eof, 1, sizeof eof, o) != sizeof eof || fclose(o) != 0) { perror(argv[3]); return 2; }
    o = fopen((std::string(argv[3]) + ".bai").c_str(), "wb"); if (!o) { perror("bai"); return 2; }
    if (fwrite(bai.data(), 1, bai.size(), o) != bai.size() || fclose(o) != 0) { perror("bai"); return 2; }
    printf("{\"records\": %zu, \"blocks\": %zu, \"bai_bytes\": %zu}\n", n, nBlocks, bai.size());
    return 0;
}
