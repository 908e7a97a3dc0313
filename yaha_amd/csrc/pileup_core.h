// pileup_core.h -- the allele pileup (-opu): which base the printed alignments carry at every reference base, and from it the sites where the reads disagree
// with the reference -- as ONE set of routines compiled for the host (host/pileup.cpp: the records the device did not count, the site table) and for the device
// (device/pileup_stage.h: a wave per clump behind the post-filter, the candidate selection), so that the two sides cannot drift apart.  No allocation, no
// library calls.
//
// The contract (every layer and every test shares it):
//   The layout is -ocov's with a bin of one base (depth_core.h, ydepth::layoutBins): one SLOT per reference base, sequence by sequence in index order.
//   pu[slot][ch] is uint32, slot-major, NCH = 7 channels in the order A, C, G, T, N, DEL, INS; a count that passes 2^32 - 1 wraps (not handled, as in -ocov).
//   Counts cover the records that get printed: a clump printClump drops (it spans two sequences, host/sam.cpp) adds nothing, a record with
//   mapQuality < minMapq adds nothing -- ydepth::gate, the two-sequence test first.
//   The walk keeps two cursors: `cur`, the reference offset, starts at c.sro and advances over M, R and D ops; `q`, the query offset, starts at c.sqo and
//   advances over M, R and I ops.  q is strand-local as sqo / eqo are: for a reversed clump (status & 1) it indexes the reverse-complement codes -- the base
//   printClump writes into SEQ -- so the pileup is in reference orientation.  One record adds
//     A C G T N   1 for every reference base under an M or R op, in the channel of the read's 4-bit code at q (T0 C1 A2 G3; every other code: N); whether
//                 the op is M or R is not consulted;
//     DEL         1 for every reference base under a D op;
//     INS         1 per I op, whatever its length, at the slot of min(cur, c.sro + c.refLen - 1) -- yevents::opEvents' rule, taken from there.
//   A base whose q lies past c.eqo (or past the read's last base) adds nothing: the walk never reads outside [sqo, eqo] of its read, whatever the ops add
//   up to (ygpu_inject_results can hand the stage ops that do not fit their clump).  Base qualities are not used.
//   The reverse-complement code of a read is kFourBitCompCodes[forward code] (Math.c:156: {2, 3, 0, 1, 4, 12, 7, 6, 9, 8, 15, 11, 5, 13, 14, 10}): codes
//   0 .. 3 map to code ^ 2, codes of 4 and above to codes of 4 and above -- all of them channel N.  So the channel of a reversed clump's base comes from the
//   FORWARD code at qlen - 1 - q, and only the forward codes have to be kept for the walk (chOfRead below; the device's snapshot copies them alone).
//   Sites: refCh(slot) is the channel of the reference's own 4-bit code at that base (4 and above: N);
//   nonref = A + C + G + T + N + DEL - pu[slot][refCh] + INS; a slot is a SITE when nonref >= minAlt, minAlt >= 1 (isSite below: the host's writer with
//   -pumin, the device's candidate selection with 1).
#pragma once
#include "events_core.h"

namespace ypileup {

enum { A = 0, C = 1, G = 2, T = 3, N = 4, DEL = 5, INS = 6, NCH = 7 };
using ydepth::COUNTED; using ydepth::SKIPPED_MAPQ; using ydepth::DROPPED;

// the channel of a 4-bit code, a read's or the reference's (T0 C1 A2 G3; 4 and above: N)
YDP_FN uint32_t chOfCode(uint32_t code) { return code == 0 ? (uint32_t)T : code == 1 ? (uint32_t)C : code == 2 ? (uint32_t)A : code == 3 ? (uint32_t)G : (uint32_t)N; }
// the channel of a read's base at strand-local query offset q < qlen, from its FORWARD codes (one a byte)
YDP_FN uint32_t chOfRead(const uint8_t *fwd, uint32_t qlen, uint32_t q, bool reversed)
{
    const uint32_t code = fwd[reversed ? qlen - 1 - q : q] & 0xFu;
    return chOfCode(reversed && code < 4 ? code ^ 2u : code);
}
// one past the last query offset the walk may read: inside [sqo, eqo] and inside the read
YDP_FN uint32_t qEnd(const ygpu_clump &c, uint32_t qlen) { const uint32_t e = (uint32_t)c.eqo + 1u; return e < qlen ? e : qlen; }
// query bases an op consumes (M, R, I)
YDP_FN uint32_t opQuery(uint32_t op) { const char code = YGPU_OP_CODE(op); return code == 'M' || code == 'R' || code == 'I' ? YGPU_OP_LEN(op) : 0u; }
// the slot of absolute reference offset `off` of sequence seq (a bin of one base: no division)
YDP_FN uint32_t slotOf(const ydepth::Layout &L, int seq, uint32_t off) { const uint32_t s = L.seqStart[seq]; return L.binBase[seq] + (off >= s ? off - s : 0u); }
// the sequence a slot belongs to: the last s with binBase[s] <= slot (empty sequences repeat their neighbour's word and are skipped)
YDP_FN uint32_t seqOfSlot(const ydepth::Layout &L, uint32_t slot)
{
    uint32_t lo = 0, hi = L.nSeqs - 1;
    while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (L.binBase[mid] <= slot) lo = mid; else hi = mid - 1; }
    return lo;
}
// the reference's own code at a slot, from the packed 4-bit image of nBaseBytes bytes (two bases a byte, the even offset in the high nibble).  A slot number is
// not a reference offset -- sequences are padded in the image -- so it goes through the sequence table; an offset past the image (a table that does not
// belong to it) reads nothing and is N.
YDP_FN uint32_t refCode(const ydepth::Layout &L, const uint8_t *bases, uint64_t nBaseBytes, uint32_t slot)
{
    const uint32_t s = seqOfSlot(L, slot), off = L.seqStart[s] + (slot - L.binBase[s]);
    if ((uint64_t)(off >> 1) >= nBaseBytes) return 4u;
    const uint8_t b = bases[off >> 1];
    return (off & 1u) ? (uint32_t)(b & 0xFu) : (uint32_t)(b >> 4);
}
YDP_FN uint32_t refCh(const ydepth::Layout &L, const uint8_t *bases, uint64_t nBaseBytes, uint32_t slot) { return chOfCode(refCode(L, bases, nBaseBytes, slot)); }
// reads that disagree with the reference at a slot (64 bits: seven wrapped words still add up without a second wrap)
YDP_FN uint64_t nonref(const uint32_t *row, uint32_t refChannel)
{
    return (uint64_t)row[A] + row[C] + row[G] + row[T] + row[N] + row[DEL] - row[refChannel] + row[INS];
}
YDP_FN bool isSite(const uint32_t *row, uint32_t refChannel, uint32_t minAlt) { return nonref(row, refChannel) >= (uint64_t)minAlt; }
// the same for a slot nobody looked the reference up for yet: untouched slots -- nearly all of a sparse array -- leave before the sequence table is searched
YDP_FN bool isSiteAt(const ydepth::Layout &L, const uint8_t *bases, uint64_t nBaseBytes, uint32_t slot, const uint32_t *row, uint32_t minAlt)
{
    if (!(row[A] | row[C] | row[G] | row[T] | row[N] | row[DEL] | row[INS])) return false;
    return isSite(row, refCh(L, bases, nBaseBytes, slot), minAlt);
}

// The whole walk of one record on one thread: gate, then its ops -> add(slot, channel), one call per count.  fwd: the read's forward codes, qlen of them;
// reversed: status & 1 of the record as it is printed.  Returns COUNTED / SKIPPED_MAPQ / DROPPED.
template <class Add> YDP_FN int walkClump(const ydepth::Layout &L, const ygpu_clump &c, const uint32_t *ops, const uint8_t *fwd, uint32_t qlen, bool reversed,
                                          uint32_t mapQuality, Add add)
{
    int seq = -1; const int g = ydepth::gate(L, c, mapQuality, &seq);
    if (g != COUNTED) return g;
    const uint32_t qe = qEnd(c, qlen); uint32_t cur = c.sro, q = c.sqo < qe ? c.sqo : qe;
    for (uint32_t k = 0; k < c.n_ops; k++) {
        bool covered; const uint32_t n = ydepth::opRef(ops[k], &covered);
        if (covered) { for (uint32_t i = 0; i < n && q + i < qe; i++) add(slotOf(L, seq, cur + i), chOfRead(fwd, qlen, q + i, reversed)); }
        else {
            const yevents::OpEvents e = yevents::opEvents(c, ops[k], cur);
            if (e.ch == (uint32_t)yevents::DELETED) for (uint32_t i = 0; i < e.len; i++) add(slotOf(L, seq, e.off + i), (uint32_t)DEL);
            else if (e.ch == (uint32_t)yevents::INSERTION && e.len) add(slotOf(L, seq, e.off), (uint32_t)INS);
        }
        cur += n; q += opQuery(ops[k]); if (q > qe) q = qe;                // (past the end nothing is added any more: q stays there)
    }
    return COUNTED;
}
}  // namespace ypileup
