// indel_stage.h -- indel alleles (-oid) counted on the device, right behind the post-filter: the (slot, type, length, inserted bases) of every D and I op of the
// clumps that will be printed, counted in a hash table -- the one output of the family without a dense layout.  What an event is and what its key looks like
// are ../indel_core.h, the very source the host compiles for the records the device does not see (host/indels.cpp).
//
// k_indel_clumps: a clump gets a WAVE, which opens like the other tracks (track_stage.h: the gate, then the ops 64 at a time with the scan of their reference
// lengths); one more scan across the wave -- the ops' query-consuming lengths, as k_pileup_clumps has it -- gives every op its query offset.  The wave finds its
// clump's read by the binary search in oqOutStart k_event_clumps uses, and the read's forward codes in the snapshot's own copy of them.  A lane owns an op: a
// lane whose op is an event builds its key (an insertion: at most 42 byte loads) and inserts it.
//
// The table is the CONTEXT's (draining it never races with another context): open addressing, linear probing, entries of 32 bytes {w0, w1, w2, count, zero},
// a power of two of them, all zero when empty (no key word is ever zero).  An insertion never waits for another lane: at a probed entry
// old = atomicCAS(&w0, 0, my0); neither 0 nor my0: the entry is somebody else's, probe on; otherwise the same for w1, then w2 -- a mismatch at either probes
// on; after the last match atomicAdd(&count, 1), no value returned.  Whoever turns a w0 from 0 always goes on to offer its w1 and w2, every other lane that
// passes the entry offers its own: no entry stays half-keyed, a word once set never changes, so a key meets the same answer at an entry whenever it asks, and
// two alleles that share w0 (or w0 and w1) end in different entries whatever the interleaving.  Lanes of one wave with equal keys need no special case.  No
// spinning, no locks, no LDS; ordinary global atomics.  The lane that turns a w0 from 0 adds 1 to `used`; a lane that has probed `probeLimit` entries in vain
// adds 1 to `lost` and gives up (the host then answers YGPU_EOVERFLOW).
//
// Draining: IndelDrainSel picks the occupied entries and leaves them in ascending table index, through the tile selection of select.h.
#pragma once
#include "track_stage.h"
#include "select.h"
#include "../indel_core.h"

#define YI_PROBE_LIMIT 1024u
struct IndelArgs {
    ydepth::Layout L;                          // bin 1
    uint32_t minLen;
    ygpu_indel_entry *table; uint32_t mask, probeLimit;      // capacity - 1 (a power of two of entries), entries an insertion may probe
    unsigned long long *stats;                 // records counted, skipped (MAPQ), dropped (two sequences), events, reads left to the host
    uint32_t *used, *lost;
    const uint8_t *fwd; const uint32_t *readOff;      // the snapshot's forward codes and the reads' offsets into them (n + 1 words)
};

__device__ __forceinline__ void indelInsert(const IndelArgs &A, const yindel::Key &k)
{
    uint32_t at = (uint32_t)yindel::hashKey(k) & A.mask;
    for (uint32_t p = 0; p < A.probeLimit; p++, at = (at + 1u) & A.mask) {
        ygpu_indel_entry *const e = A.table + at;
        unsigned long long old = atomicCAS((unsigned long long *)&e->w0, 0ull, (unsigned long long)k.w0);
        if (old != 0ull && old != k.w0) continue;
        if (old == 0ull) atomicAdd(A.used, 1u);
        old = atomicCAS((unsigned long long *)&e->w1, 0ull, (unsigned long long)k.w1);
        if (old != 0ull && old != k.w1) continue;
        old = atomicCAS((unsigned long long *)&e->w2, 0ull, (unsigned long long)k.w2);
        if (old != 0ull && old != k.w2) continue;
        atomicAdd(&e->count, 1u);
        return;
    }
    atomicAdd(A.lost, 1u);
}

__global__ void __launch_bounds__(256) k_indel_clumps(IndelArgs A, const ygpu_out_clump *fClumps, const uint32_t *fOps, const uint32_t *outStart, uint32_t nReads,
                                                      uint32_t nClumps)
{
    const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= nClumps || nReads == 0) return;
    const ygpu_out_clump f = fClumps[w];
    // the read of clump w: the last r with outStart[r] <= w (reads without output repeat their neighbour's word)
    uint32_t lo = 0, hi = nReads - 1;
    while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (outStart[mid] <= w) lo = mid; else hi = mid - 1; }
    if (f.primaryCount == 0xFFFFu) {                                        // a read handed back unfiltered: the host filters it and counts what it prints
        if (lane == 0 && outStart[lo] == w) atomicAdd(A.stats + 4, 1ull);
        return;
    }
    int seq = -1;
    if (!trackGate(A.L, f, A.stats, lane, &seq)) return;
    const uint32_t r0 = A.readOff[lo], qlen = A.readOff[lo + 1] - r0; const uint8_t *const fwd = A.fwd + r0;
    const bool reversed = (f.status & 1u) != 0;
    const uint32_t *ops = fOps + f.c.op_start; const uint32_t nOps = f.c.n_ops;
    const uint32_t qe = ypileup::qEnd(f.c, qlen);
    uint32_t cur = f.c.sro, q = f.c.sqo < qe ? f.c.sqo : qe, events = 0;   // (cur and q: the same on every lane)
    for (uint32_t k0 = 0; k0 < nOps; k0 += 64) {
        const OpChunk c = loadOpChunk(ops, nOps, k0, lane);
        const uint32_t qn = c.k < nOps ? ypileup::opQuery(c.op) : 0u, qIncl = waveInclSumU(qn), qTotal = (uint32_t)__shfl((int)qIncl, 63, 64);
        if (c.k < nOps && !c.covered) {                                      // D and I: the lane's own op
            const uint32_t qx = qIncl - qn, qOp = qx < qe - q ? q + qx : qe; yindel::Key key;
            if (yindel::opKey(A.L, seq, f.c, c.op, cur + c.excl, qOp, qe, fwd, qlen, reversed, A.minLen, &key)) { indelInsert(A, key); events++; }
        }
        cur += c.total; q = qTotal < qe - q ? q + qTotal : qe;               // (past the end q stays there, as in the one-thread walk)
    }
    events = waveTotalSumU(events);
    if (lane == 0 && events) atomicAdd(A.stats + 3, (unsigned long long)events);
}

// ---- draining: the occupied entries, ascending table index ------------------------------------------------------------------------------------------------------
struct IndelDrainSel {
    static constexpr uint32_t ROWS = 32, COUNT_UNROLL = 1; using Rec = NoRec;
    const ygpu_indel_entry *table; uint64_t capacity; ygpu_indel_entry *out;
    __device__ __forceinline__ bool pick(uint64_t i, Rec &) const { return i < capacity && table[i].w0 != 0ull; }
    __device__ __forceinline__ void put(uint32_t pos, uint64_t i, const Rec &) const { out[pos] = table[i]; }
};
