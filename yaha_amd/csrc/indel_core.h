// indel_core.h -- indel alleles (-oid): which insertions and deletions the printed alignments carry, by position, length and inserted bases -- as ONE set of
// routines compiled for the host (host/indels.cpp: the records the device did not count, the run's alleles, the writer) and for the device
// (device/indel_stage.h: a wave per clump behind the post-filter, a lane per op, a hash table per context), so that the two sides cannot drift apart.  No
// allocation, no library calls.
//
// The contract (every layer and every test shares it):
//   The layout is -ocov's with a bin of one base (depth_core.h, ydepth::layoutBins): one SLOT per reference base, sequence by sequence in index order.
//   Alleles cover the records that get printed: a clump printClump drops (it spans two sequences, host/sam.cpp) has none, a record with
//   mapQuality < minMapq has none -- ydepth::gate, the two-sequence test first.
//   The walk keeps the pileup's two cursors (pileup_core.h): `cur`, the reference offset, starts at c.sro and advances over M, R and D ops; `q`, the query
//   offset, starts at c.sqo and advances over M, R and I ops, strand-local as sqo / eqo are; nothing is read past qEnd(c, qlen).  One record has
//     a deletion   for every D op of length len >= minLen: (slot of cur, DEL, len) -- the slot of the first deleted base.  A deletion whose bases would lie past
//                  the record's last reference base (cur + len > c.sro + c.refLen) is NOT an event.
//     an insertion for every I op of length len >= minLen: (slot of min(cur, c.sro + c.refLen - 1), INS, len, bases) -- yevents::opEvents' rule, taken from
//                  there.  bases: the channels (ypileup::chOfRead: A C G T N, reference orientation, from the FORWARD codes) of the first min(len, KEPT)
//                  inserted bases, KEPT = 42.  An insertion whose bases would lie past qEnd (q + len > qEnd) is NOT an event.
//   The two "is not an event" rules only bite on ops that do not add up to their clump (ygpu_inject_results can hand the stage such ops): they are stated here
//   so that host and device agree on them, and so that no slot leaves its record and no base is read outside its read.
//   Two insertions longer than KEPT bases with equal slot, length and first KEPT bases are ONE allele -- by contract: the key has room for 42 bases.
//   A record adds 1 per event, not per distinct allele: two equal ops in one record count 2.
//   The key is three 64-bit words, none of them ever zero (zero is the empty word of the device's table):
//     w0 = slot | type << 32 | len << 33 | 1 << 63        (type: DEL 0, INS 1; len < 2^16 -- an op's length has 16 bits, YGPU_OP_LEN)
//     w1 = bases 0 .. 20, w2 = bases 21 .. 41, 3 bits a base, the first base lowest, bit 63 set; a deletion's w1 and w2 hold that marker bit alone.
//   The order of alleles in every output: slot, then type (DEL before INS), then length, then the bases compared one by one in channel order (A C G T N).
#pragma once
#include "pileup_core.h"

namespace yindel {

enum { DEL = 0, INS = 1, KEPT = 42, PER_WORD = 21 };
using ydepth::COUNTED; using ydepth::SKIPPED_MAPQ; using ydepth::DROPPED;
static_assert(YGPU_OP_LEN(0xFFFFFFFFu) < (1u << 16), "an op's length must fit the key's 16 bits");

struct Key { uint64_t w0, w1, w2; };
constexpr uint64_t kMarker = 1ull << 63;

YDP_FN uint64_t word0(uint32_t slot, uint32_t type, uint32_t len) { return (uint64_t)slot | (uint64_t)(type & 1u) << 32 | (uint64_t)(len & 0xFFFFu) << 33 | kMarker; }
YDP_FN uint32_t slotOfKey(const Key &k) { return (uint32_t)k.w0; }
YDP_FN uint32_t typeOfKey(const Key &k) { return (uint32_t)(k.w0 >> 32) & 1u; }
YDP_FN uint32_t lenOfKey(const Key &k) { return (uint32_t)(k.w0 >> 33) & 0xFFFFu; }
YDP_FN uint32_t keptOfKey(const Key &k) { const uint32_t n = lenOfKey(k); return typeOfKey(k) == (uint32_t)INS ? (n < (uint32_t)KEPT ? n : (uint32_t)KEPT) : 0u; }
// the channel of kept base i < keptOfKey(k)
YDP_FN uint32_t baseOfKey(const Key &k, uint32_t i) { return (uint32_t)((i < (uint32_t)PER_WORD ? k.w1 >> (3u * i) : k.w2 >> (3u * (i - PER_WORD))) & 7u); }
YDP_FN bool sameKey(const Key &a, const Key &b) { return a.w0 == b.w0 && a.w1 == b.w1 && a.w2 == b.w2; }
// the order of every output (see above)
YDP_FN bool keyLess(const Key &a, const Key &b)
{
    if (slotOfKey(a) != slotOfKey(b)) return slotOfKey(a) < slotOfKey(b);
    if (typeOfKey(a) != typeOfKey(b)) return typeOfKey(a) < typeOfKey(b);
    if (lenOfKey(a) != lenOfKey(b)) return lenOfKey(a) < lenOfKey(b);
    const uint32_t n = keptOfKey(a);
    for (uint32_t i = 0; i < n; i++) { const uint32_t x = baseOfKey(a, i), y = baseOfKey(b, i); if (x != y) return x < y; }
    return false;
}
// a fixed mix of the three words (the device's table, and nothing else, depends on it: no output shows the table's order)
YDP_FN uint64_t hashKey(const Key &k)
{
    uint64_t h = k.w0 * 0x9E3779B97F4A7C15ull ^ k.w1 * 0xC2B2AE3D27D4EB4Full ^ k.w2 * 0x165667B19E3779F9ull;
    h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
    return h;
}
// the table the device keeps for a batch of `bases` bases: the smallest power of two >= 2 x bases (a batch has at most one event per two bases, so a table
// that is drained whenever more than a quarter of it is used never passes one half), at least 1024 entries
inline uint64_t tableCapacity(uint64_t bases) { uint64_t c = 1024; while (c < 2 * bases && c < (1ull << 31)) c <<= 1; return c; }

// The event of ONE op, when the walk stands at reference offset cur and (clamped) query offset q <= qe = qEnd(c, qlen): true and its key, or false.
YDP_FN bool opKey(const ydepth::Layout &L, int seq, const ygpu_clump &c, uint32_t op, uint32_t cur, uint32_t q, uint32_t qe, const uint8_t *fwd, uint32_t qlen, bool reversed,
                  uint32_t minLen, Key *out)
{
    const char code = YGPU_OP_CODE(op); const uint32_t len = YGPU_OP_LEN(op);
    if (len == 0 || len < minLen) return false;
    if (code == 'D') {
        if ((uint64_t)cur + len > (uint64_t)c.sro + c.refLen) return false;
        out->w0 = word0(ypileup::slotOf(L, seq, cur), (uint32_t)DEL, len); out->w1 = kMarker; out->w2 = kMarker;
        return true;
    }
    if (code != 'I' || q + len > qe) return false;
    const yevents::OpEvents e = yevents::opEvents(c, op, cur);
    uint64_t w1 = kMarker, w2 = kMarker; const uint32_t n = len < (uint32_t)KEPT ? len : (uint32_t)KEPT;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t ch = ypileup::chOfRead(fwd, qlen, q + i, reversed);
        if (i < (uint32_t)PER_WORD) w1 |= ch << (3u * i); else w2 |= ch << (3u * (i - PER_WORD));
    }
    out->w0 = word0(ypileup::slotOf(L, seq, e.off), (uint32_t)INS, len); out->w1 = w1; out->w2 = w2;
    return true;
}

// The whole walk of one record on one thread: gate, then its ops -> add(key), one call per event.  fwd: the read's forward codes, qlen of them; reversed:
// status & 1 of the record as it is printed.  Returns COUNTED / SKIPPED_MAPQ / DROPPED.
template <class Add> YDP_FN int walkClump(const ydepth::Layout &L, const ygpu_clump &c, const uint32_t *ops, const uint8_t *fwd, uint32_t qlen, bool reversed,
                                          uint32_t mapQuality, uint32_t minLen, Add add)
{
    int seq = -1; const int g = ydepth::gate(L, c, mapQuality, &seq);
    if (g != COUNTED) return g;
    const uint32_t qe = ypileup::qEnd(c, qlen); uint32_t cur = c.sro, q = c.sqo < qe ? c.sqo : qe;
    for (uint32_t k = 0; k < c.n_ops; k++) {
        Key key;
        if (opKey(L, seq, c, ops[k], cur, q, qe, fwd, qlen, reversed, minLen, &key)) add(key);
        cur += yevents::opRef(ops[k]); q += ypileup::opQuery(ops[k]); if (q > qe) q = qe;      // (past the end q stays there, as in the pileup's walk)
    }
    return COUNTED;
}
}  // namespace yindel
