// pileup_stage.h -- the allele pileup (-opu) accumulated on the device, right behind the post-filter: which base the clumps that will be printed carry at every
// reference base they cover, seven uint32 channels a base (A C G T N DEL INS), and at the end of the run the selection of the slots where reads disagree with
// the reference, so that only those cross PCIe.  What one record adds and what a site is are ../pileup_core.h, the very source the host compiles for the records
// the device does not see (host/pileup.cpp).
//
// k_pileup_clumps: a clump gets a WAVE, which opens like the other tracks (track_stage.h: the gate, then the ops 64 at a time with the scan of their reference
// lengths).  Two more scans across the wave -- the ops' query-consuming lengths (M, R, I) and the lengths of the M / R ops alone -- give every op its query offset
// and the chunk's aligned BASES a numbering.  Those bases, not the ops, are dealt across the lanes in strips of 64: M runs are tens to thousands of bases long and
// a lane per op would walk them alone.  A lane finds the op that owns its base by a binary search in the inclusive sums (six shuffles) and fetches that op's
// offsets (three more); neighbouring lanes then read neighbouring bytes of the read and add to neighbouring slots.  D and I ops are short and rare: a lane each,
// as k_event_clumps has it.  The read's bases: ygpu_out_clump carries no read number, so the wave finds its clump's read by the binary search in oqOutStart
// k_event_clumps uses, then the read's forward codes in the SNAPSHOT's own copy of them (stage_out.hip: by the time this runs the context may be uploading its
// next batch) -- the forward codes alone: the reverse strand's channel follows from them (pileup_core.h chOfRead).
// The array is shared by the contexts of an index image: plain global atomicAdd on uint32 (no value returned, device scope), one per aligned base.  At one base
// a slot nothing can be combined in the wave.
//
// The end of the run: CandidateSel selects the slots with nonref >= 1 in ascending order, through the tile selection of select.h.  An untouched slot leaves
// after its seven loads; only a touched one looks the reference base up (the sequence table, then the packed image).  k_pileup_gather writes the seven counts
// of every slot of a caller's list.
#pragma once
#include "track_stage.h"
#include "select.h"
#include "../pileup_core.h"

struct PileupArgs {
    ydepth::Layout L;                          // bin 1
    uint32_t *pu; uint32_t nSlots;             // the image's array, pu[slot * NCH + channel]
    unsigned long long *stats;                 // records counted, skipped (MAPQ), dropped (two sequences), reads left to the host, counts added
    const uint8_t *fwd; const uint32_t *readOff;      // the snapshot's forward codes and the reads' offsets into them (n + 1 words)
};

__global__ void __launch_bounds__(256) k_pileup_clumps(PileupArgs P, const ygpu_out_clump *fClumps, const uint32_t *fOps, const uint32_t *outStart, uint32_t nReads,
                                                       uint32_t nClumps)
{
    const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= nClumps || nReads == 0) return;
    const ygpu_out_clump f = fClumps[w];
    // the read of clump w: the last r with outStart[r] <= w (reads without output repeat their neighbour's word)
    uint32_t lo = 0, hi = nReads - 1;
    while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (outStart[mid] <= w) lo = mid; else hi = mid - 1; }
    if (f.primaryCount == 0xFFFFu) {                                        // a read handed back unfiltered: the host filters it and counts what it prints
        if (lane == 0 && outStart[lo] == w) atomicAdd(P.stats + 3, 1ull);
        return;
    }
    int seq = -1;
    if (!trackGate(P.L, f, P.stats, lane, &seq)) return;
    const uint32_t r0 = P.readOff[lo], qlen = P.readOff[lo + 1] - r0; const uint8_t *const fwd = P.fwd + r0;
    const bool reversed = (f.status & 1u) != 0;
    uint32_t *const pu = P.pu; const uint32_t nSlots = P.nSlots; uint32_t added = 0;
    auto add = [pu, nSlots, &added](uint32_t s, uint32_t ch) { if (s < nSlots && ch < (uint32_t)ypileup::NCH) { atomicAdd(pu + (size_t)s * ypileup::NCH + ch, 1u); added++; } };
    const uint32_t *ops = fOps + f.c.op_start; const uint32_t nOps = f.c.n_ops;
    const uint32_t qe = ypileup::qEnd(f.c, qlen);
    uint32_t cur = f.c.sro, q = f.c.sqo < qe ? f.c.sqo : qe;                // (the same on every lane)
    for (uint32_t k0 = 0; k0 < nOps; k0 += 64) {
        const OpChunk c = loadOpChunk(ops, nOps, k0, lane);
        const uint32_t qn = c.k < nOps ? ypileup::opQuery(c.op) : 0u, qIncl = waveInclSumU(qn), qTotal = (uint32_t)__shfl((int)qIncl, 63, 64);
        const uint32_t bn = c.covered ? c.n : 0u, bIncl = waveInclSumU(bn), bTotal = (uint32_t)__shfl((int)bIncl, 63, 64);
        // D and I: the lane's own op
        if (c.k < nOps && !c.covered) {
            const yevents::OpEvents e = yevents::opEvents(f.c, c.op, cur + c.excl);
            if (e.ch == (uint32_t)yevents::DELETED) for (uint32_t i = 0; i < e.len; i++) add(ypileup::slotOf(P.L, seq, e.off + i), (uint32_t)ypileup::DEL);
            else if (e.ch == (uint32_t)yevents::INSERTION && e.len) add(ypileup::slotOf(P.L, seq, e.off), (uint32_t)ypileup::INS);
        }
        // M and R: the chunk's aligned bases in strips of 64, a base a lane (every lane takes part in the shuffles; a lane past the last base adds nothing)
        for (uint32_t b0 = 0; b0 < bTotal; b0 += 64) {
            const uint32_t b = b0 + lane;
            uint32_t jl = 0, jh = 63;                                        // the first lane whose inclusive sum is above b
            for (int step = 0; step < 6; step++) {
                const uint32_t mid = (jl + jh) >> 1, v = (uint32_t)__shfl((int)bIncl, (int)mid, 64);
                if (v > b) jh = mid; else jl = mid + 1;
            }
            const uint32_t j = jl < 63u ? jl : 63u;
            const uint32_t i = b - (uint32_t)__shfl((int)(bIncl - bn), (int)j, 64);
            const uint32_t ro = cur + (uint32_t)__shfl((int)c.excl, (int)j, 64) + i, qo = q + (uint32_t)__shfl((int)(qIncl - qn), (int)j, 64) + i;
            if (b < bTotal && qo < qe) add(ypileup::slotOf(P.L, seq, ro), ypileup::chOfRead(fwd, qlen, qo, reversed));
        }
        cur += c.total; q = qTotal < qe - q ? q + qTotal : qe;               // (past the end nothing is added any more: q stays there, as in the one-thread walk)
    }
    added = waveTotalSumU(added);
    if (lane == 0 && added) atomicAdd(P.stats + 4, (unsigned long long)added);
}

// ---- the candidates: slots with nonref >= 1, ascending ---------------------------------------------------------------------------------------------------------
struct CandidateSel {
    static constexpr uint32_t ROWS = 32, COUNT_UNROLL = 1; using Rec = NoRec;
    ydepth::Layout L; const uint32_t *pu; uint32_t nSlots; const uint8_t *bases; uint64_t nBaseBytes;      // the image's array and packed reference
    uint32_t *out;
    __device__ __forceinline__ bool pick(uint64_t slot64, Rec &) const
    {
        if (slot64 >= nSlots) return false;
        const uint32_t slot = (uint32_t)slot64;
        uint32_t row[ypileup::NCH];
#pragma unroll
        for (int ch = 0; ch < ypileup::NCH; ch++) row[ch] = pu[(size_t)slot * ypileup::NCH + ch];
        return ypileup::isSiteAt(L, bases, nBaseBytes, slot, row, 1u);
    }
    __device__ __forceinline__ void put(uint32_t pos, uint64_t slot, const Rec &) const { out[pos] = (uint32_t)slot; }
};
// rows[i * NCH + ch] = pu[slots[i]][ch] (zero for a slot past the array)
__global__ void __launch_bounds__(256) k_pileup_gather(const uint32_t *pu, uint32_t nSlots, const uint32_t *slots, uint32_t n, uint32_t *rows)
{
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (uint64_t)n * ypileup::NCH) return;
    const uint32_t i = (uint32_t)(idx / ypileup::NCH), ch = (uint32_t)(idx % ypileup::NCH), s = slots[i];
    rows[idx] = s < nSlots ? pu[(size_t)s * ypileup::NCH + ch] : 0u;
}
