// eprofile_core.h -- the error profile (-oep): how good the printed alignments are -- the substitution spectrum, the lengths of insertions and deletions, the
// identity the records reach, the error rate along the read -- as ONE set of routines compiled for the host (host/eprofile.cpp: the records the device did not
// count, the writer) and for the device (device/eprofile_stage.h: a wave per clump behind the post-filter, the table in LDS), so that the two sides cannot drift
// apart.  No allocation, no library calls.
//
// The contract (every layer and every test shares it):
//   One table per run, WORDS = YGPU_EPROFILE_WORDS = 1556 words of uint64, in five sections (the enum below has their offsets).
//   The table covers the records that get printed: a clump printClump drops (it spans two sequences, host/sam.cpp) adds nothing, a record with
//   mapQuality < minMapq adds nothing -- ydepth::gate, the two-sequence test first.
//   The walk keeps the pileup's two cursors (pileup_core.h): `cur`, the reference offset, starts at c.sro and advances over M, R and D ops; `q`, the query
//   offset, starts at c.sqo and advances over M, R and I ops, strand-local as sqo / eqo are, and never passes qEnd(c, qlen); a base whose q lies past the end
//   adds nothing.
//   The reference channel at absolute offset `off` is chOfCode of the packed image's nibble there (two bases a byte, the even offset in the high nibble); an
//   offset past the image is N.  The read's channel is ypileup::chOfRead's.  Channels are A C G T N in ypileup order.
//   A PAIR is one reference base under an M or R op together with the read base over it -- whether the op is M or R is not consulted, the two channels decide
//   everything.  A pair is a MATCH when its two channels are equal and not N.
//     SUB    25 words [ref][read]   1 per pair
//     INS    65 words               1 per I op of length n >= 1, at index min(n, 65) - 1 (the last row is "65 and longer")
//     DEL    65 words               the same per D op
//     IDENT  1001 words             1 per record with cols > 0, at floor(1000 * m / cols) (64-bit): m = matches, cols = pairs + inserted bases + deleted bases,
//                                   where only the I and D ops that begin before qEnd count, each at its full length
//     POS    100 x 4 words          by position in the read as sequenced: strand-local q has the forward offset f = reversed ? qlen - 1 - q : q and the bin
//                                   f * 100 / qlen (64-bit); channel 0: 1 per pair; 1: 1 per pair that is no match; 2: 1 per I op at the q where it starts;
//                                   3: 1 per D op at min(q, qEnd - 1)
//   I and D ops reached with q >= qEnd add nothing to POS or IDENT; they still count in INS / DEL.  (Such ops only exist where the ops do not add up to their
//   clump: ygpu_inject_results can hand the stage such ops.)  Homopolymer context and base qualities are not looked at.
#pragma once
#include "pileup_core.h"

namespace yeprofile {

enum { NCH = 5, NLEN = 65, NIDENT = 1001, NBINS = 100, NPOS = 4 };
enum { SUB = 0, INS = SUB + NCH * NCH, DEL = INS + NLEN, IDENT = DEL + NLEN, POS = IDENT + NIDENT, WORDS = POS + NBINS * NPOS };
enum { POS_PAIRS = 0, POS_ERRORS = 1, POS_INS = 2, POS_DEL = 3 };
using ydepth::COUNTED; using ydepth::SKIPPED_MAPQ; using ydepth::DROPPED;
static_assert(WORDS == YGPU_EPROFILE_WORDS, "the table's sections must add up to the C-ABI's word count");

// the reference's channel at absolute offset off of the packed image (nBaseBytes bytes); past the image: N
YDP_FN uint32_t refCh(const uint8_t *bases, uint64_t nBaseBytes, uint32_t off)
{
    if ((uint64_t)(off >> 1) >= nBaseBytes) return (uint32_t)ypileup::N;
    const uint8_t b = bases[off >> 1];
    return ypileup::chOfCode((off & 1u) ? (uint32_t)(b & 0xFu) : (uint32_t)(b >> 4));
}
YDP_FN bool isMatch(uint32_t refChannel, uint32_t readChannel) { return refChannel == readChannel && refChannel != (uint32_t)ypileup::N; }
// the words of the sections
YDP_FN uint32_t subWord(uint32_t refChannel, uint32_t readChannel) { return (uint32_t)SUB + refChannel * NCH + readChannel; }
YDP_FN uint32_t lenWord(uint32_t section, uint32_t n) { return section + (n < (uint32_t)NLEN ? n : (uint32_t)NLEN) - 1u; }      // n >= 1
YDP_FN uint32_t identWord(uint64_t m, uint64_t cols) { return (uint32_t)IDENT + (uint32_t)(1000ull * m / cols); }               // m <= cols, cols > 0
// the bin of strand-local query offset q < qlen by its place in the read as sequenced (the quotient of the 64-bit rule; 32-bit where the product fits)
YDP_FN uint32_t posBin(uint32_t q, uint32_t qlen, bool reversed)
{
    const uint32_t f = reversed ? qlen - 1u - q : q;
    return qlen <= 0xFFFFFFFFu / NBINS ? f * NBINS / qlen : (uint32_t)((uint64_t)f * NBINS / qlen);
}
YDP_FN uint32_t posWord(uint32_t bin, uint32_t ch) { return (uint32_t)POS + bin * NPOS + ch; }
// what an I or D op is to the profile: its section (INS / DEL) and POS channel, or false (M, R, clips, a length of 0)
YDP_FN bool gapOp(const ygpu_clump &c, uint32_t op, uint32_t cur, uint32_t *section, uint32_t *posCh)
{
    const yevents::OpEvents e = yevents::opEvents(c, op, cur);
    if (YGPU_OP_LEN(op) == 0 || e.len == 0) return false;
    if (e.ch == (uint32_t)yevents::INSERTION) { *section = (uint32_t)INS; *posCh = (uint32_t)POS_INS; return true; }
    if (e.ch == (uint32_t)yevents::DELETED) { *section = (uint32_t)DEL; *posCh = (uint32_t)POS_DEL; return true; }
    return false;
}

// The whole walk of one record on one thread: gate, then its ops -> add(word, n).  fwd: the read's forward codes, qlen of them; reversed: status & 1 of the
// record as it is printed; bases: the packed reference image of nBaseBytes bytes.  Returns COUNTED / SKIPPED_MAPQ / DROPPED.
template <class Add> YDP_FN int walkClump(const ydepth::Layout &L, const ygpu_clump &c, const uint32_t *ops, const uint8_t *fwd, uint32_t qlen, bool reversed,
                                          uint32_t mapQuality, const uint8_t *bases, uint64_t nBaseBytes, Add add)
{
    int seq = -1; const int g = ydepth::gate(L, c, mapQuality, &seq);
    if (g != COUNTED) return g;
    const uint32_t qe = ypileup::qEnd(c, qlen); uint32_t cur = c.sro, q = c.sqo < qe ? c.sqo : qe; uint64_t m = 0, cols = 0;
    for (uint32_t k = 0; k < c.n_ops; k++) {
        bool covered; const uint32_t n = ydepth::opRef(ops[k], &covered); uint32_t section, posCh;
        if (covered) {
            for (uint32_t i = 0; i < n && q + i < qe; i++) {
                const uint32_t r = refCh(bases, nBaseBytes, cur + i), b = ypileup::chOfRead(fwd, qlen, q + i, reversed), bin = posBin(q + i, qlen, reversed);
                add(subWord(r, b), 1u); add(posWord(bin, POS_PAIRS), 1u); cols++;
                if (isMatch(r, b)) m++; else add(posWord(bin, POS_ERRORS), 1u);
            }
        } else if (gapOp(c, ops[k], cur, &section, &posCh)) {
            add(lenWord(section, YGPU_OP_LEN(ops[k])), 1u);
            if (q < qe) { cols += YGPU_OP_LEN(ops[k]); add(posWord(posBin(q < qe - 1u ? q : qe - 1u, qlen, reversed), posCh), 1u); }
        }
        cur += n; q += ypileup::opQuery(ops[k]); if (q > qe) q = qe;          // (past the end nothing is added any more: q stays there)
    }
    if (cols) add(identWord(m, cols), 1u);
    return COUNTED;
}
}  // namespace yeprofile
