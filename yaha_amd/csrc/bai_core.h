// bai_core.h -- the BAI index of a coordinate-sorted BAM (-obsort), from the SAM specification's section 5: the pieces that need no memory of their own.
// host/bai.cpp puts them together; tests/fixtures/bai_driver.cpp runs them as a program of its own.  Nothing here allocates.
//
// The file (little-endian): "BAI\1", n_ref; per sequence n_bin, the bins in ascending bin number -- bin, n_chunk, (beg, end) pairs --, n_intv, ioffset[n_intv];
// at the end n_no_coor as a uint64 (0: no unmapped record is ever printed).
//   virtual offset of stream offset s (the sorted records one behind the other, the header not counted): coffs[s / 65280] << 16 | s % 65280, where coffs[k] is
//     the file offset of record block k (every block but the last holds exactly 65 280 bytes); the stream's end is coffs[nBlocks] << 16, the end-of-file block.
//   bin       a record's is reg2bin(pos, end), the value in its bin field; a CHUNK is a maximal run of records that follow each other in the file and share
//             sequence and bin: beg = the first one's first byte, end = the byte behind the last one.
//   37450     every sequence with records has this pseudo-bin as well, two chunks: (first record's start, last record's end), (number of records, 0).
//   linear    n_intv = ((largest end - 1) >> 14) + 1; ioffset[w] = the smallest start offset of the records that overlap the 16 384 bases of window w; a
//             window nothing overlaps repeats the one before it (0 when there is none).
//   A sequence without records has n_bin = 0 and n_intv = 0.
#pragma once
#include <cstdint>
#include <cstddef>

namespace ybai {
enum : uint32_t { PAYLOAD = 65280, PSEUDO_BIN = 37450, LINEAR_SHIFT = 14, MAX_REF_LENGTH = 1u << 29 };
// what the index needs of a record: sequence, 0-based position, bytes in the stream (block_size's four included), end (exclusive), bin
struct Entry { uint32_t ref, pos, len, end, bin; };

inline uint32_t reg2bin(uint32_t beg, uint32_t end)                       // end exclusive, end > beg
{
    --end;
    if (beg >> 14 == end >> 14) return 4681u + (beg >> 14);
    if (beg >> 17 == end >> 17) return 585u + (beg >> 17);
    if (beg >> 20 == end >> 20) return 73u + (beg >> 20);
    if (beg >> 23 == end >> 23) return 9u + (beg >> 23);
    if (beg >> 26 == end >> 26) return 1u + (beg >> 26);
    return 0;
}
inline uint64_t sortKey(uint32_t ref, uint32_t pos) { return (uint64_t)ref << 32 | pos; }
inline uint64_t sortKey(const Entry &e) { return sortKey(e.ref, e.pos); }

// coffs[0 .. nBlocks]: see above; total: the bytes of the stream
inline uint64_t voffset(const uint64_t *coffs, size_t nBlocks, uint64_t total, uint64_t s)
{
    if (s >= total || s / PAYLOAD >= nBlocks) return coffs[nBlocks] << 16;
    return coffs[s / PAYLOAD] << 16 | s % PAYLOAD;
}

// the file offsets of the blocks in data[0 .. n) (whole BGZF blocks, the first at file offset `at`), read from BSIZE: appended to coffs[*nBlocks ..), at most
// cap entries in all; returns the file offset behind the last block, or 0 when a header does not fit or cap is passed
inline uint64_t blockOffsets(const uint8_t *data, uint64_t n, uint64_t at, uint64_t *coffs, size_t *nBlocks, size_t cap)
{
    for (uint64_t p = 0; p < n;) {
        if (p + 18 > n || *nBlocks >= cap) return 0;
        coffs[(*nBlocks)++] = at + p;
        p += (uint64_t)(data[p + 16] | data[p + 17] << 8) + 1u;
        if (p > n) return 0;
    }
    return at + n;
}

// the chunk that starts with record i of e[0 .. n) (file order): returns the index behind its last record
inline size_t chunkEnd(const Entry *e, size_t n, size_t i)
{
    size_t j = i + 1;
    while (j < n && e[j].ref == e[i].ref && e[j].bin == e[i].bin) j++;
    return j;
}
// the records of the sequence that e[i] belongs to: the index behind its last one
inline size_t refEnd(const Entry *e, size_t n, size_t i)
{
    size_t j = i + 1;
    while (j < n && e[j].ref == e[i].ref) j++;
    return j;
}
// the linear index of one sequence's records e[i0 .. i1), whose stream offsets are offs[i0 .. i1): ioffset must hold linearCount() entries
inline uint32_t linearCount(const Entry *e, size_t i0, size_t i1)
{
    uint32_t maxEnd = 0;
    for (size_t i = i0; i < i1; i++) if (e[i].end > maxEnd) maxEnd = e[i].end;
    return i1 > i0 ? (((maxEnd ? maxEnd : 1u) - 1u) >> LINEAR_SHIFT) + 1u : 0u;
}
inline void linearFill(const Entry *e, const uint64_t *offs, size_t i0, size_t i1, const uint64_t *coffs, size_t nBlocks, uint64_t total, uint64_t *ioffset, uint32_t nIntv)
{
    const uint64_t unset = ~0ull;
    for (uint32_t w = 0; w < nIntv; w++) ioffset[w] = unset;
    for (size_t i = i0; i < i1; i++) {                                    // (file order: the first record that reaches a window has the smallest offset)
        const uint32_t w0 = e[i].pos >> LINEAR_SHIFT, w1 = ((e[i].end > e[i].pos ? e[i].end : e[i].pos + 1u) - 1u) >> LINEAR_SHIFT;
        const uint64_t v = voffset(coffs, nBlocks, total, offs[i]);
        for (uint32_t w = w0; w <= w1 && w < nIntv; w++) if (ioffset[w] == unset) ioffset[w] = v;
    }
    uint64_t before = 0;
    for (uint32_t w = 0; w < nIntv; w++) { if (ioffset[w] == unset) ioffset[w] = before; before = ioffset[w]; }
}
}  // namespace ybai
