// bai.cpp -- FILE.bai of a coordinate-sorted BAM (-obsort): the layout and every rule are ../bai_core.h; this file owns the memory -- the stream offsets, the
// chunk list of a sequence ordered by bin, the bytes of the file.
#include "yaha_host.h"
#include "../bai_core.h"

namespace yaha {
static_assert(sizeof(BamEntry) == sizeof(ybai::Entry) && sizeof(BamEntry) == 20, "BamEntry is ybai::Entry");

// the host's ordering: perm[j] = the record at sorted place j, by (sequence, position), equal keys in the order they came in
void bamSortOrder(const BamEntry *e, size_t n, uint32_t *perm)
{
    for (size_t i = 0; i < n; i++) perm[i] = (uint32_t)i;
    std::stable_sort(perm, perm + n, [&](uint32_t a, uint32_t b) { return ybai::sortKey(e[a].ref, e[a].pos) < ybai::sortKey(e[b].ref, e[b].pos); });
}

std::string baiBuild(const BamEntry *sorted, size_t n, size_t nRefs, const uint64_t *coffs, size_t nBlocks)
{
    const ybai::Entry *e = (const ybai::Entry *)sorted;
    std::vector<uint64_t> offs(n + 1, 0);
    for (size_t i = 0; i < n; i++) offs[i + 1] = offs[i] + e[i].len;
    const uint64_t total = offs[n];
    auto vo = [&](uint64_t s) { return ybai::voffset(coffs, nBlocks, total, s); };
    std::string out = "BAI\1"; uint8_t w[8];
    auto add32 = [&](uint32_t v) { for (int k = 0; k < 4; k++) w[k] = (uint8_t)(v >> (8 * k)); out.append((const char *)w, 4); };
    auto add64 = [&](uint64_t v) { for (int k = 0; k < 8; k++) w[k] = (uint8_t)(v >> (8 * k)); out.append((const char *)w, 8); };
    add32((uint32_t)nRefs);
    struct Chunk { uint32_t bin; size_t i0, i1; };
    std::vector<Chunk> chunks; std::vector<uint64_t> ioffset;
    size_t i = 0;
    for (size_t ref = 0; ref < nRefs; ref++) {
        if (i >= n || e[i].ref != ref) { add32(0); add32(0); continue; }
        const size_t i1 = ybai::refEnd(e, n, i);
        chunks.clear();
        for (size_t c = i; c < i1;) { const size_t c1 = ybai::chunkEnd(e, i1, c); chunks.push_back(Chunk{e[c].bin, c, c1}); c = c1; }
        std::stable_sort(chunks.begin(), chunks.end(), [](const Chunk &a, const Chunk &b) { return a.bin < b.bin; });     // (stable: a bin's chunks stay in file order)
        uint32_t nBin = 1;
        for (size_t c = 0; c < chunks.size(); c++) if (c == 0 || chunks[c].bin != chunks[c - 1].bin) nBin++;
        add32(nBin);
        for (size_t c = 0; c < chunks.size();) {
            size_t c1 = c; while (c1 < chunks.size() && chunks[c1].bin == chunks[c].bin) c1++;
            add32(chunks[c].bin); add32((uint32_t)(c1 - c));
            for (; c < c1; c++) { add64(vo(offs[chunks[c].i0])); add64(vo(offs[chunks[c].i1])); }
        }
        add32(ybai::PSEUDO_BIN); add32(2); add64(vo(offs[i])); add64(vo(offs[i1])); add64((uint64_t)(i1 - i)); add64(0);
        const uint32_t nIntv = ybai::linearCount(e, i, i1);
        ioffset.assign(nIntv, 0);
        ybai::linearFill(e, offs.data(), i, i1, coffs, nBlocks, total, ioffset.data(), nIntv);
        add32(nIntv); for (uint32_t k = 0; k < nIntv; k++) add64(ioffset[k]);
        i = i1;
    }
    add64(0);
    return out;
}
}  // namespace yaha
