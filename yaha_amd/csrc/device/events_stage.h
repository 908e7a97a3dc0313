// events_stage.h -- the evidence track (-oev) accumulated on the device, right behind the post-filter: mismatched bases, deleted bases, insertions and clipped
// ends of the clumps that will be printed, per bin of the reference (the bins of -ocov), five uint32 channels a bin.  The printed clumps, their edit ops, the
// reads' lengths and the sequence table are all in HBM at that point; only the finished counts cross PCIe, once, at the end of the run.  What one record adds is
// ../events_core.h, the very source the host compiles for the records the device does not see (host/events.cpp).
//
// A clump gets a WAVE: the lanes take 64 ops at a time, a scan of their reference-consuming lengths across the wave gives every op its reference offset, and
// each lane emits the events of its own op -- R and D ops are short, so a lane walks its op's bins itself.  Lane 0 emits the two clipped ends.
// The query length: ygpu_out_clump carries no read number and the right clip needs qlen, so every wave finds its clump's read by a BINARY SEARCH in the
// exclusive sums of the reads' output counts (oqOutStart, n + 1 words; every lane reads the same word, so a step is one broadcast load).  The other way -- a
// wave per read that loops over the read's clumps -- would leave a chimeric read's dozens of clumps to one wave; the search keeps the balance of a wave per clump
// for at most 17 loads.  The wave of a read's first clump also counts the reads handed back unfiltered.
// The array is shared by the contexts of an index image: plain global atomicAdd on uint32 (no value returned, device scope).  With bins of more than one base
// the ops of a chunk mostly fall into the same few bins, so the wave combines them first: a loop over the chunk's distinct (channel, bin) pairs with a ballot and
// a wave sum, one atomic a pair instead of one an op.  (Only the part of an op in its first bin is combined: what an op longer than the bin's rest adds to later
// bins goes straight to memory.)  At a bin of one base nothing can be combined and the branch -- the same on every lane -- is skipped.  The counts are exact
// either way.
#pragma once
#include "track_stage.h"
#include "../events_core.h"

struct EventsArgs {
    ydepth::Layout L;
    uint32_t minClip;
    uint32_t *ev; uint32_t nBins;              // the image's array, ev[bin * NCH + channel]
    unsigned long long *stats;                 // records counted, skipped (MAPQ), dropped (two sequences), reads left to the host
};

template <bool COMBINE>
__global__ void __launch_bounds__(256) k_event_clumps(EventsArgs E, const ygpu_out_clump *fClumps, const uint32_t *fOps, const uint32_t *outStart, const uint32_t *qlens,
                                                      uint32_t nReads, uint32_t nClumps)
{
    const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= nClumps || nReads == 0) return;
    const ygpu_out_clump f = fClumps[w];
    // the read of clump w: the last r with outStart[r] <= w (reads without output repeat their neighbour's word)
    uint32_t lo = 0, hi = nReads - 1;
    while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (outStart[mid] <= w) lo = mid; else hi = mid - 1; }
    if (f.primaryCount == 0xFFFFu) {                                        // a read handed back unfiltered: the host filters it and counts what it prints
        if (lane == 0 && outStart[lo] == w) atomicAdd(E.stats + 3, 1ull);
        return;
    }
    int seq = -1;
    if (!trackGate(E.L, f, E.stats, lane, &seq)) return;
    uint32_t *const ev = E.ev; const uint32_t nBins = E.nBins;
    auto add = [ev, nBins](uint32_t b, uint32_t ch, uint32_t n) { if (b < nBins && ch < (uint32_t)yevents::NCH) atomicAdd(ev + (size_t)b * yevents::NCH + ch, n); };
    if (lane == 0) {
        if (yevents::clipLeft(f.c, E.minClip)) add(yevents::binOf(E.L, seq, f.c.sro), (uint32_t)yevents::CLIP_LEFT, 1u);
        if (yevents::clipRight(f.c, qlens[lo], E.minClip)) add(yevents::binOf(E.L, seq, f.c.sro + f.c.refLen - 1), (uint32_t)yevents::CLIP_RIGHT, 1u);
    }
    const uint32_t *ops = fOps + f.c.op_start; const uint32_t nOps = f.c.n_ops;
    uint32_t cur = f.c.sro;                                                 // (the same on every lane)
    for (uint32_t k0 = 0; k0 < nOps; k0 += 64) {
        const OpChunk c = loadOpChunk(ops, nOps, k0, lane);
        yevents::OpEvents e; e.ch = 0; e.off = cur; e.len = 0;
        if (c.k < nOps) e = yevents::opEvents(f.c, c.op, cur + c.excl);
        if (COMBINE) {
            // the op's share of its first bin, summed over the lanes of the same (channel, bin); the rest of a longer op goes its own way
            uint32_t bin0 = 0, n0 = 0;
            if (e.len) {
                const uint32_t s = E.L.seqStart[seq], rel = e.off >= s ? e.off - s : 0u, room = E.L.bin - rel % E.L.bin;
                bin0 = E.L.binBase[seq] + rel / E.L.bin; n0 = e.len < room ? e.len : room;
            }
            unsigned long long todo = __ballot(n0 != 0);
            while (todo) {
                const int l = __ffsll((long long)todo) - 1;
                const uint32_t b = (uint32_t)__shfl((int)bin0, l, 64), ch = (uint32_t)__shfl((int)e.ch, l, 64);
                const bool mine = n0 != 0 && bin0 == b && e.ch == ch;
                uint32_t sum = mine ? n0 : 0u;
#pragma unroll
                for (int s = 32; s; s >>= 1) sum += (uint32_t)__shfl_xor((int)sum, s, 64);
                if ((int)lane == l) add(b, ch, sum);
                todo &= ~__ballot(mine);
            }
            if (e.len > n0) yevents::addSpan(E.L, seq, e.ch, e.off + n0, e.len - n0, add);
        } else yevents::addSpan(E.L, seq, e.ch, e.off, e.len, add);
        cur += c.total;
    }
}
