// indelcall_core.h -- indel calls with genotypes (-oindel) from the run's raw indel alleles (indel_core.h), the reference and the allele pileup (pileup_core.h):
// every raw allele is left-normalised, alleles that become equal are merged, and what is left is judged at its anchor base -- as ONE set of routines compiled
// for the host (host/indelcalls.cpp: the fallback, the writer) and for the device (device/indelcall_stage.h: a wave per raw allele, a lane per merged allele),
// so that the two sides cannot drift apart.  No allocation, no library calls.  Slots, channels and the reference's codes are pileup_core.h's, keys indel_core.h's.
//
// The contract (every layer and every test shares it):
//   Input: the run's raw alleles, Key plus count, counted with a minimum length of 1 and the gate -puq.  p = slotOfKey is the event's position: the first deleted
//   base, or the base an insertion stands before.  The anchor is p - 1.
//   NOT called, counted as `skipped`: an insertion with len > KEPT (its key has no room for its last base); an allele whose p is the first slot of its sequence
//   (no anchor).  Two more rules keep every read inside the allele's own sequence, whatever a caller hands in: an allele whose p is no slot of the layout, or
//   whose length is 0, and a deletion whose last base lies past the end of its sequence are skipped too (the walk of indel_core.h makes none of these).
//   Left shift: s is the largest value with s <= S (max_shift; 0: no normalisation), s <= p - 1 - first slot of the sequence (the anchor stays inside the
//   sequence, the shift never crosses into the previous one) and, for every i < s, x == y with both in {A, C, G, T} on pileup channels (an N on either side
//   stops the shift), where
//     a deletion of length L:              x = ref[p - 1 - i], y = ref[p + L - 1 - i]
//     an insertion with bases I[0 .. L-1]: x = ref[p - 1 - i], y = I[L - 1 - (i mod L)]
//   So s is the first i at which the comparison fails -- a first-mismatch search, no loop-carried state: sameAt(i) below answers for any i on its own.
//   The normalised allele has slot p - s; a deletion keeps its length; an insertion's bases are I rotated right by s mod L: I'[j] = I[(j - s) mod L].
//   Merging: raw alleles with equal normalised keys are ONE allele; their counts add, saturated to 32 bits.
//   Depth and counts: d = row[A] + row[C] + row[G] + row[T] + row[N] + row[DEL] of the pileup at the anchor slot, in 64 bits -- the reads that cover the anchor;
//   a = the merged count; r = d > a ? d - a : 0.  Reads that carry ANOTHER indel at the same site cover the anchor without showing this allele: they count as r.
//   The model is three integer costs in 1/100 phred, which arrive in the parameter block -- no logarithm is ever taken here.  The host derives them once from
//   e = E / 1000 (-inderr E, per mille): cM = round(-1000 log10(1 - e)), cE = round(-1000 log10 e), cH = round(1000 log10 2).  A read shows the allele or does
//   not -- two states, so no e / 3.  The default E = 50 gives (22, 1301, 301) -- DEFAULT_* below.
//     PL0 = r cM + a cE,  PL1 = (r + a) cH,  PL2 = r cE + a cM
//   GT, the normalised PLs, QUAL and GQ are ysnv::judge's, with the same caps and the same tie rules: GT = the index of the smallest, ties to the lower index;
//   PLn[i] = PL[i] - min; QUAL = min(PLn[0], 999 900) / 100; GQ = min(second smallest PLn, 9 900) / 100.
//   An allele is a CALL when GT != 0, a >= min_alt, d >= min_depth and QUAL >= min_qual.
//   The record (ygpu_indel_call, include/yaha_hip.h; 64 bytes): the normalised w0, w1, w2; alt_count = a, ref_count = r, depth = d, each saturated to 32 bits;
//   qual; gq; the three normalised PLs, saturated; info = GT | the 4-bit reference code of the anchor << 4; a word that is zero.
//   The order of every output: yindel::keyLess on the normalised key.
#pragma once
#include "indel_core.h"
#include "snv_core.h"

namespace yindelcall {

enum { DEFAULT_ERR = 50, DEFAULT_CM = 22, DEFAULT_CE = 1301, DEFAULT_CH = 301, DEFAULT_SHIFT = 256, MAX_SHIFT = 65535 };
using yindel::Key;

YDP_FN uint32_t infoWord(uint32_t gt, uint32_t refCode) { return (gt & 15u) | (refCode & 15u) << 4; }
YDP_FN uint32_t infoGt(uint32_t info) { return info & 15u; }
YDP_FN uint32_t infoRefCode(uint32_t info) { return info >> 4 & 15u; }

// the reference's 4-bit code at a slot of sequence seq (no search: the caller knows the sequence), read the way ypileup::refCode reads it
YDP_FN uint32_t codeIn(const ydepth::Layout &L, const uint8_t *bases, uint64_t nBaseBytes, uint32_t seq, uint32_t slot)
{
    const uint32_t off = L.seqStart[seq] + (slot - L.binBase[seq]);
    if ((uint64_t)(off >> 1) >= nBaseBytes) return 4u;
    const uint8_t b = bases[off >> 1];
    return (off & 1u) ? (uint32_t)(b & 0xFu) : (uint32_t)(b >> 4);
}
// Is the allele judged at all?  true: *seq = its sequence, *cap = the most it may shift (max_shift and the anchor rule); false: it is `skipped`.
YDP_FN bool callable(const ydepth::Layout &L, uint64_t nSlots, const Key &k, uint32_t maxShift, uint32_t *seq, uint32_t *cap)
{
    const uint32_t p = yindel::slotOfKey(k), len = yindel::lenOfKey(k);
    if ((uint64_t)p >= nSlots || len == 0u || L.nSeqs == 0u) return false;
    const bool ins = yindel::typeOfKey(k) == (uint32_t)yindel::INS;
    if (ins && len > (uint32_t)yindel::KEPT) return false;
    const uint32_t s = ypileup::seqOfSlot(L, p), first = L.binBase[s];
    if (p <= first) return false;
    if (!ins && (uint64_t)(p - first) + len > (uint64_t)L.seqLength[s]) return false;
    const uint32_t room = p - 1u - first;
    *seq = s; *cap = maxShift < room ? maxShift : room;
    return true;
}
// the comparison of step i < cap: may the allele move one more base to the left after i moves?
YDP_FN bool sameAt(const ydepth::Layout &L, const uint8_t *bases, uint64_t nBaseBytes, uint32_t seq, const Key &k, uint32_t i)
{
    const uint32_t p = yindel::slotOfKey(k), len = yindel::lenOfKey(k);
    const uint32_t x = ypileup::chOfCode(codeIn(L, bases, nBaseBytes, seq, p - 1u - i));
    const uint32_t y = yindel::typeOfKey(k) == (uint32_t)yindel::INS ? yindel::baseOfKey(k, len - 1u - i % len)
                                                                     : ypileup::chOfCode(codeIn(L, bases, nBaseBytes, seq, p + len - 1u - i));
    return x < 4u && x == y;
}
// the shift of one allele on one thread: the first i that fails, or cap
YDP_FN uint32_t shiftOf(const ydepth::Layout &L, const uint8_t *bases, uint64_t nBaseBytes, uint32_t seq, const Key &k, uint32_t cap)
{
    uint32_t i = 0;
    while (i < cap && sameAt(L, bases, nBaseBytes, seq, k, i)) i++;
    return i;
}
// base j of the insertion moved s bases to the left: I[(j - s) mod L]
YDP_FN uint32_t rotatedBase(const Key &k, uint32_t s, uint32_t j) { const uint32_t len = yindel::lenOfKey(k); return yindel::baseOfKey(k, (j + len - s % len) % len); }
// the normalised key of an allele that moves s bases (one thread)
YDP_FN Key shifted(const Key &k, uint32_t s)
{
    const uint32_t len = yindel::lenOfKey(k), type = yindel::typeOfKey(k);
    Key o; o.w0 = yindel::word0(yindel::slotOfKey(k) - s, type, len); o.w1 = yindel::kMarker; o.w2 = yindel::kMarker;
    if (type == (uint32_t)yindel::INS) for (uint32_t j = 0; j < len && j < (uint32_t)yindel::KEPT; j++) {
        const uint64_t ch = rotatedBase(k, s, j);
        if (j < (uint32_t)yindel::PER_WORD) o.w1 |= ch << (3u * j); else o.w2 |= ch << (3u * (j - yindel::PER_WORD));
    }
    return o;
}
YDP_FN uint32_t addSat32(uint32_t a, uint32_t b) { const uint64_t v = (uint64_t)a + b; return ysnv::sat32(v); }

// The verdict on one merged allele: key (normalised), count a, the pileup row of its anchor and the reference's 4-bit code there.  Fills every word of *out
// whether or not the allele is a call -- the tests hold all of it to their oracle -- and returns whether it is one.
YDP_FN bool judge(const Key &k, uint32_t count, const uint32_t *row, uint32_t anchorCode, const ygpu_indelcall_params &P, ygpu_indel_call *out)
{
    const uint64_t d = (uint64_t)row[ypileup::A] + row[ypileup::C] + row[ypileup::G] + row[ypileup::T] + row[ypileup::N] + row[ypileup::DEL];
    const uint64_t a = count, r = d > a ? d - a : 0ull;
    uint64_t pl[3] = {r * P.cost_match + a * P.cost_error, (r + a) * P.cost_het, r * P.cost_error + a * P.cost_match};
    uint32_t gt = 0;
    if (pl[1] < pl[gt]) gt = 1;
    if (pl[2] < pl[gt]) gt = 2;
    const uint64_t least = pl[gt];
    pl[0] -= least; pl[1] -= least; pl[2] -= least;
    const uint64_t x = pl[gt == 0 ? 1 : 0], y = pl[gt == 2 ? 1 : 2], second = x < y ? x : y;
    const uint32_t qual = (uint32_t)((pl[0] < (uint64_t)ysnv::QUAL_CAP ? pl[0] : (uint64_t)ysnv::QUAL_CAP) / 100u);
    const uint32_t gq = (uint32_t)((second < (uint64_t)ysnv::GQ_CAP ? second : (uint64_t)ysnv::GQ_CAP) / 100u);
    out->w0 = k.w0; out->w1 = k.w1; out->w2 = k.w2;
    out->alt_count = count; out->ref_count = ysnv::sat32(r); out->depth = ysnv::sat32(d); out->qual = qual; out->gq = gq;
    out->pl[0] = ysnv::sat32(pl[0]); out->pl[1] = ysnv::sat32(pl[1]); out->pl[2] = ysnv::sat32(pl[2]); out->info = infoWord(gt, anchorCode); out->zero = 0u;
    return gt != 0u && a >= (uint64_t)P.min_alt && d >= (uint64_t)P.min_depth && qual >= P.min_qual;
}
// the same for an allele nobody looked its anchor up for yet: row = the pileup's row at slotOfKey(k) - 1 (the caller's), the code from the reference
YDP_FN bool judgeAt(const ydepth::Layout &L, const uint8_t *bases, uint64_t nBaseBytes, const Key &k, uint32_t count, const uint32_t *row, const ygpu_indelcall_params &P,
                    ygpu_indel_call *out)
{
    return judge(k, count, row, ypileup::refCode(L, bases, nBaseBytes, yindel::slotOfKey(k) - 1u), P, out);
}
}  // namespace yindelcall
