// events_core.h -- the evidence track (-oev): where along the reference the printed alignments disagree with it or stop -- mismatched bases, deleted bases,
// insertions and clipped ends per bin -- as ONE routine compiled for the host (host/events.cpp: the records the device did not count) and for the device
// (device/events_stage.h: a wave per clump behind the post-filter), so that the two sides cannot drift apart.  No allocation, no library calls.
//
// The contract (every layer and every test shares it):
//   Bins are exactly -ocov's (depth_core.h, ydepth::layoutBins): per sequence, never across two sequences, the last bin of a sequence may be shorter, numbered
//   sequence by sequence in index order.  A caller can divide these counts by the depth of the same bin.
//   ev[bin][ch] is uint32, bin-major, NCH = 5 channels; a count that passes 2^32 - 1 wraps (not handled, as in -ocov).
//   Counts cover the records that get printed: a clump printClump drops (it spans two sequences, host/sam.cpp) adds nothing, a record with
//   mapQuality < minMapq adds nothing -- ydepth::gate, the two-sequence test first.
//   `cur` is the walk's reference offset: it starts at c.sro and advances over M, R and D ops.  One record adds
//     ch 0 mismatch    1 for every reference base under an R op, in that base's bin
//     ch 1 deleted     1 for every reference base under a D op, in that base's bin
//     ch 2 insertion   1 per I op, whatever its length, in the bin of min(cur, c.sro + c.refLen - 1): the next reference base the walk reaches
//     ch 3 clip_left   1 in the bin of c.sro when the printed CIGAR starts with a clip of at least minClip bases: c.sqo >= minClip (sam.cpp, clipFront)
//     ch 4 clip_right  1 in the bin of c.sro + c.refLen - 1 when it ends with one: qlen - 1 - c.eqo >= minClip (clipBack)
//   Hard and soft clipping count alike, and -o8 output changes nothing: the track follows what would be printed.
#pragma once
#include "depth_core.h"

namespace yevents {

enum { MISMATCH = 0, DELETED = 1, INSERTION = 2, CLIP_LEFT = 3, CLIP_RIGHT = 4, NCH = 5 };
using ydepth::COUNTED; using ydepth::SKIPPED_MAPQ; using ydepth::DROPPED;

// the bin (numbered over all sequences) of absolute reference offset `off` of sequence seq
YDP_FN uint32_t binOf(const ydepth::Layout &L, int seq, uint32_t off)
{
    const uint32_t s = L.seqStart[seq];
    return L.binBase[seq] + (off >= s ? off - s : 0u) / L.bin;
}
// reference bases an op consumes (M, R, D)
YDP_FN uint32_t opRef(uint32_t op) { bool covered; return ydepth::opRef(op, &covered); }
// What an op emits when the walk stands at reference offset cur: one event of channel ch for each of the bases [off, off + len); len 0: nothing (M, clips).
// An I is one event at the next reference base, kept inside the record.
struct OpEvents { uint32_t ch, off, len; };
YDP_FN OpEvents opEvents(const ygpu_clump &c, uint32_t op, uint32_t cur)
{
    const char code = YGPU_OP_CODE(op); OpEvents e; e.ch = 0; e.off = cur; e.len = 0;
    if (code == 'R') { e.ch = MISMATCH; e.len = YGPU_OP_LEN(op); }
    else if (code == 'D') { e.ch = DELETED; e.len = YGPU_OP_LEN(op); }
    else if (code == 'I') { const uint32_t last = c.sro + c.refLen - 1; e.ch = INSERTION; e.off = cur < last ? cur : last; e.len = 1; }
    return e;
}
// the two clip tests (the very comparisons printClump makes before it writes a clip, with minClip in place of 1)
YDP_FN bool clipLeft(const ygpu_clump &c, uint32_t minClip) { return (int)c.sqo >= (int)minClip; }
YDP_FN bool clipRight(const ygpu_clump &c, uint32_t qlen, uint32_t minClip) { return (int)qlen - 1 - (int)c.eqo >= (int)minClip; }
// events of one channel on the bases [off, off + len) of sequence seq -> add(bin, ch, events in that bin), one call per bin
template <class Add> YDP_FN void addSpan(const ydepth::Layout &L, int seq, uint32_t ch, uint32_t off, uint32_t len, Add add)
{
    while (len) {
        const uint32_t s = L.seqStart[seq], rel = off >= s ? off - s : 0u, room = L.bin - rel % L.bin, n = len < room ? len : room;
        add(L.binBase[seq] + rel / L.bin, ch, n);
        off += n; len -= n;
    }
}
// The whole walk of one record on one thread: gate, the ops' events, the two clipped ends.  Returns COUNTED / SKIPPED_MAPQ / DROPPED.
template <class Add> YDP_FN int walkClump(const ydepth::Layout &L, uint32_t minClip, const ygpu_clump &c, const uint32_t *ops, uint32_t qlen, uint32_t mapQuality, Add add)
{
    int seq = -1; const int g = ydepth::gate(L, c, mapQuality, &seq);
    if (g != COUNTED) return g;
    uint32_t cur = c.sro;
    for (uint32_t k = 0; k < c.n_ops; k++) {
        const OpEvents e = opEvents(c, ops[k], cur);
        addSpan(L, seq, e.ch, e.off, e.len, add);
        cur += opRef(ops[k]);
    }
    if (clipLeft(c, minClip)) add(binOf(L, seq, c.sro), (uint32_t)CLIP_LEFT, 1u);
    if (clipRight(c, qlen, minClip)) add(binOf(L, seq, c.sro + c.refLen - 1), (uint32_t)CLIP_RIGHT, 1u);
    return COUNTED;
}
}  // namespace yevents
