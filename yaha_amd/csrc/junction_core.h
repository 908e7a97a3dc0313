// junction_core.h -- split-read breakpoint calls (-obp): where the printed alignments of a read join, as ONE set of routines compiled for the host
// (host/junctions.cpp: the reads the device did not see) and for the device (device/junction_stage.h: a wave per read behind the post-filter), so that the two
// sides cannot drift apart.  No allocation, no library calls.
//
// The contract (every layer and every test shares it):
//   Eligible records of a read: the ones printClump prints (ydepth::gate does not answer DROPPED: the record lies within one sequence), that are primary
//   (status & 0x20) and have mapQuality >= minMapq (-bpq).  The tests come in that order; only the last one counts as "skipped by MAPQ".
//   sqo and eqo are on the printed strand.  With rev = status & 1 and qlen the read's length the read-forward query interval of a record is
//     qs = rev ? qlen - 1 - eqo : sqo,   qe = rev ? qlen - 1 - sqo : eqo;
//   its reference interval rs = sro, re = sro + refLen - 1, as positions WITHIN its sequence (0-based), the sequence number from the gate.
//   The eligible records ordered by (qs, qe, print order): every consecutive pair (a, b) is one junction, the k-th pair has ordinal k;
//     side A = (seq_a, rev_a ? rs_a : re_a, rev_a ? '-' : '+'),   side B = (seq_b, rev_b ? re_b : rs_b, rev_b ? '-' : '+'),   qgap = qs_b - qe_a - 1
//   (negative: the pieces overlap on the read -- microhomology; positive: unaligned bases between them).
//   Canonical form: when (seqB, posB) < (seqA, posA) the sides are swapped and both strands flipped, so that a read from the other strand of the same molecule
//   yields the same junction.  At EQUAL (sequence, position) on both sides nothing is swapped, so the two strands of such a molecule can give two forms
//   ('+','+' from one, '-','-' from the other).  The case is rare (a piece that ends on the very base the next one starts on) and is left as it is.
//   Type: TRA when the sequences differ, else INV when the strands differ, else DEL for '+','+' and DUP for '-','-'.
//   Hard and soft clipping, SAM or -o8 output change nothing.
#pragma once
#include "depth_core.h"

namespace yjunc {

enum { ELIGIBLE = 0, SKIPPED_MAPQ = 1, DROPPED = 2, SECONDARY = 3 };       // what became of a record
enum { DEL = YGPU_JUNCTION_DEL, DUP = YGPU_JUNCTION_DUP, INV = YGPU_JUNCTION_INV, TRA = YGPU_JUNCTION_TRA };

// the sequence table and the gate in the form depth_core.h takes them (no bins here)
YDP_FN ydepth::Layout layout(const uint32_t *seqStart, const uint32_t *seqLength, uint32_t nSeqs, uint32_t minMapq)
{
    ydepth::Layout L; L.seqStart = seqStart; L.seqLength = seqLength; L.binBase = nullptr; L.nSeqs = nSeqs; L.bin = 1; L.minMapq = minMapq; return L;
}

// one eligible record as the junctions see it
struct Piece { uint32_t qs, qe, seq, rs, re, rev; };

// the eligibility tests of one record, and its piece when it passes them
YDP_FN int piece(const ydepth::Layout &L, const ygpu_clump &c, uint32_t status, uint32_t mapQuality, uint32_t qlen, Piece *p)
{
    int seq = -1; const int g = ydepth::gate(L, c, mapQuality, &seq);
    if (g == ydepth::DROPPED) return DROPPED;
    if (!(status & 0x20u)) return SECONDARY;
    if (g == ydepth::SKIPPED_MAPQ) return SKIPPED_MAPQ;
    const uint32_t rev = status & 1u;
    p->rev = rev; p->seq = (uint32_t)seq;
    p->qs = rev ? qlen - 1u - c.eqo : (uint32_t)c.sqo; p->qe = rev ? qlen - 1u - c.sqo : (uint32_t)c.eqo;
    p->rs = c.sro - L.seqStart[seq]; p->re = p->rs + c.refLen - 1u;
    return ELIGIBLE;
}

// The order of a read's eligible records as one 64-bit key: (qs, qe, print order).  Query offsets are 16-bit (ygpu_clump::sqo / eqo), a read has fewer than
// 2^24 records; keys of different records of a read differ, so "the record before mine" is the largest key below mine.
YDP_FN uint64_t orderKey(const Piece &p, uint32_t printOrder)
{
    return ((uint64_t)(p.qs & 0xFFFFu) << 40) | ((uint64_t)(p.qe & 0xFFFFu) << 24) | (uint64_t)(printOrder & 0xFFFFFFu);
}
YDP_FN uint32_t keyOrder(uint64_t key) { return (uint32_t)(key & 0xFFFFFFu); }

// the junction of two pieces that follow one another in that order, in canonical form
YDP_FN ygpu_junction make(const Piece &a, const Piece &b, uint32_t read, uint32_t ordinal)
{
    uint32_t seqA = a.seq, posA = a.rev ? a.rs : a.re, seqB = b.seq, posB = b.rev ? b.re : b.rs;
    bool minusA = a.rev != 0, minusB = b.rev != 0;
    if (seqB < seqA || (seqB == seqA && posB < posA)) {
        const uint32_t s = seqA, p = posA; const bool m = minusA;
        seqA = seqB; posA = posB; minusA = !minusB; seqB = s; posB = p; minusB = !m;
    }
    ygpu_junction j;
    j.read = read; j.ordinal = ordinal; j.seqA = seqA; j.posA = posA; j.seqB = seqB; j.posB = posB;
    j.strandA = minusA ? '-' : '+'; j.strandB = minusB ? '-' : '+';
    j.type = (uint8_t)(seqA != seqB ? TRA : minusA != minusB ? INV : minusA ? DUP : DEL); j.reserved = 0;
    j.qgap = (int32_t)b.qs - (int32_t)a.qe - 1;
    return j;
}

// All junctions of one read on one thread (the host's path): rec(k, &c, &status, &mapQuality) describes its k-th printed record, emit(j) takes the junctions in
// ordinal order.  Quadratic in the read's records -- the records of a read are few.  *skipped (may be null): records that failed the MAPQ test only.
// Returns the number of junctions.
template <class Rec, class Emit> YDP_FN uint32_t readJunctions(const ydepth::Layout &L, uint32_t nRecs, uint32_t qlen, uint32_t read, Rec rec, Emit emit, uint32_t *skipped)
{
    uint32_t nSkip = 0, nJ = 0; bool havePrev = false; uint64_t prevKey = 0; Piece prev;
    for (;;) {                                                            // the next record in the order: the smallest key above the previous one
        bool have = false; uint64_t best = 0; Piece bp;
        for (uint32_t k = 0; k < nRecs; k++) {
            const ygpu_clump *c; uint32_t status, mq; rec(k, &c, &status, &mq);
            Piece p; const int e = piece(L, *c, status, mq, qlen, &p);
            if (e == SKIPPED_MAPQ && !havePrev) nSkip++;
            if (e != ELIGIBLE) continue;
            const uint64_t key = orderKey(p, k);
            if ((!havePrev || key > prevKey) && (!have || key < best)) { have = true; best = key; bp = p; }
        }
        if (skipped && !havePrev) *skipped = nSkip;
        if (!have) break;
        if (havePrev) { emit(make(prev, bp, read, nJ)); nJ++; }
        havePrev = true; prevKey = best; prev = bp;
    }
    return nJ;
}
}  // namespace yjunc
