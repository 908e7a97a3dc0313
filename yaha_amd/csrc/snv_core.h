// snv_core.h -- SNV calls with genotypes (-osnv) from the allele pileup: what a slot's seven counts say about the sample at that reference base -- as ONE set of
// routines compiled for the host (host/snv.cpp: the fallback over the union of the sources, the writer) and for the device (device/snv_stage.h: the selection
// over an image's array), so that the two sides cannot drift apart.  No allocation, no library calls.  Slots, channels, refCh and the gate are pileup_core.h's.
//
// The contract (every layer and every test shares it):
//   A slot is judged from its row[7] and rc, the channel of the reference's own base there.  rc == N: no call.  r = row[rc]; alt = the channel among A C G T
//   other than rc with the greatest count, ties to the lowest channel number; a = row[alt]; D = A + C + G + T; other = row[N] + row[DEL] (reported, not
//   modelled; INS is not looked at).  All sums are 64 bits wide, as ypileup::nonref's are.
//   The model is three integer costs in 1/100 phred, which arrive in the parameter block -- no logarithm is ever taken here.  The host derives them once from
//   the sequencing error e = E / 1000 (-snverr E, per mille): cM = round(-1000 log10(1 - e)), a read that shows the genotype's base; cE = round(-1000
//   log10(e / 3)), a read that shows another base; cH = round(-1000 log10(1/2 - e / 3)), a read that shows one of a heterozygous genotype's two bases.
//   The default E = 100 gives (cM, cE, cH) = (46, 1477, 331) -- DEFAULT_* below.
//     PL0 = r cM + a cE        (reference / reference)
//     PL1 = (r + a) cH         (reference / alt)
//     PL2 = r cE + a cM        (alt / alt)
//   Reads that are neither r nor a cost the same in every genotype and drop out.  GT = the index of the smallest, ties to the lower index; PLn[i] = PL[i] - min;
//   QUAL = min(PLn[0], 999 900) / 100 and GQ = min(second smallest PLn, 9 900) / 100, integer divisions.
//   A slot is a CALL when GT != 0, a >= min_alt, D >= min_depth and QUAL >= min_qual (whole phred).
//   The record (ygpu_snv_call, include/yaha_hip.h; 12 uint32 = 48 bytes): slot; info = rc | alt << 4 | GT << 8 | the reference's 4-bit code << 12, so that the
//   writer needs no lookup; r; a; D and other, each saturated to 32 bits; QUAL; GQ; the three normalised PLs in 1/100 phred, each saturated to 32 bits; a word
//   that is zero.
#pragma once
#include "pileup_core.h"

namespace ysnv {

enum { DEFAULT_ERR = 100, DEFAULT_CM = 46, DEFAULT_CE = 1477, DEFAULT_CH = 331 };     // -snverr's default and the costs it gives
enum { QUAL_CAP = 999900, GQ_CAP = 9900 };

YDP_FN uint32_t sat32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }
YDP_FN uint32_t infoWord(uint32_t rc, uint32_t alt, uint32_t gt, uint32_t refCode) { return rc | alt << 4 | gt << 8 | (refCode & 15u) << 12; }
YDP_FN uint32_t infoRc(uint32_t info) { return info & 15u; }
YDP_FN uint32_t infoAlt(uint32_t info) { return info >> 4 & 15u; }
YDP_FN uint32_t infoGt(uint32_t info) { return info >> 8 & 15u; }
YDP_FN uint32_t infoRefCode(uint32_t info) { return info >> 12 & 15u; }

// The verdict on one slot whose reference channel is rc: fills every word of *out but slot and the reference's code (judgeAt's), whether or not the slot is a
// call -- the tests hold all of it to their oracle -- and returns whether it is one.  rc == N: nothing is filled.
YDP_FN bool judge(const uint32_t *row, uint32_t rc, const ygpu_snv_params &P, ygpu_snv_call *out)
{
    if (rc >= (uint32_t)ypileup::N) return false;
    uint32_t alt = rc == 0u ? 1u : 0u;
    for (uint32_t ch = alt + 1u; ch < 4u; ch++) if (ch != rc && row[ch] > row[alt]) alt = ch;
    const uint64_t r = row[rc], a = row[alt];
    const uint64_t depth = (uint64_t)row[ypileup::A] + row[ypileup::C] + row[ypileup::G] + row[ypileup::T], other = (uint64_t)row[ypileup::N] + row[ypileup::DEL];
    uint64_t pl[3] = {r * P.cost_match + a * P.cost_error, (r + a) * P.cost_het, r * P.cost_error + a * P.cost_match};
    uint32_t gt = 0;
    if (pl[1] < pl[gt]) gt = 1;
    if (pl[2] < pl[gt]) gt = 2;
    const uint64_t least = pl[gt];
    pl[0] -= least; pl[1] -= least; pl[2] -= least;
    // the second smallest of the three: the smaller of the two that are not the genotype's
    const uint64_t x = pl[gt == 0 ? 1 : 0], y = pl[gt == 2 ? 1 : 2], second = x < y ? x : y;
    const uint32_t qual = (uint32_t)((pl[0] < (uint64_t)QUAL_CAP ? pl[0] : (uint64_t)QUAL_CAP) / 100u);
    const uint32_t gq = (uint32_t)((second < (uint64_t)GQ_CAP ? second : (uint64_t)GQ_CAP) / 100u);
    out->info = infoWord(rc, alt, gt, 0u); out->ref_count = (uint32_t)r; out->alt_count = (uint32_t)a; out->depth = sat32(depth); out->other = sat32(other);
    out->qual = qual; out->gq = gq; out->pl[0] = sat32(pl[0]); out->pl[1] = sat32(pl[1]); out->pl[2] = sat32(pl[2]); out->zero = 0u;
    return gt != 0u && a >= (uint64_t)P.min_alt && depth >= (uint64_t)P.min_depth && qual >= P.min_qual;
}
// the same for a slot nobody looked the reference up for yet: an untouched slot -- nearly all of a sparse array -- leaves before the sequence table is searched
YDP_FN bool judgeAt(const ydepth::Layout &L, const uint8_t *bases, uint64_t nBaseBytes, uint32_t slot, const uint32_t *row, const ygpu_snv_params &P, ygpu_snv_call *out)
{
    if (!(row[0] | row[1] | row[2] | row[3] | row[4] | row[5] | row[6])) return false;
    const uint32_t code = ypileup::refCode(L, bases, nBaseBytes, slot);
    if (!judge(row, ypileup::chOfCode(code), P, out)) return false;
    out->slot = slot; out->info |= (code & 15u) << 12;
    return true;
}
}  // namespace ysnv
