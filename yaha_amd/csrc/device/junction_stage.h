// junction_stage.h -- split-read breakpoint calls (-obp) made on the device, right behind the post-filter: where the printed alignments of a read join.  The
// printed clumps in print order, the reads' lengths and the sequence table are all in HBM at that point; only the junctions cross PCIe, with the filtered batch,
// and they are few.  What a junction is -- eligibility, the read-forward interval, the canonical form, the type -- is ../junction_core.h, the very source the host
// compiles for the reads the device does not see (host/junctions.cpp).
//
// A read gets a WAVE, in two passes, so that the output is ordered by (read, ordinal) and the same for the same batch whatever the schedule:
//   k_junction_count   junctions of the read (eligible records - 1) into cnt[r]; an exclusive sum of cnt gives every read its place;
//   k_junction_emit    ranks the read's eligible records by (qs, qe, print order) and writes the junctions: the lane that holds rank k >= 1 writes junction k - 1.
// A read with fewer than two gathered clumps -- nearly all of them -- leaves either pass after two loads of neighbouring words.
// The ranking is an all-pairs comparison, no sort: the order of a record is one 64-bit key (junction_core.h orderKey; keys of a read are distinct), the lanes take
// the read's records 64 at a time, every lane's key visits every other lane by a shuffle, and a lane counts the keys below its own -- its rank -- and keeps the
// LARGEST of them: the record before it in the order, whose clump it then loads itself for side A.  So nothing is staged in LDS and nothing is scattered: a read
// of more than 64 records runs the same loop over pairs of chunks, the other chunk's keys made again from its clumps (loads the wave shares), and there is no cap
// beside the post-filter's own.  The kernels use no LDS and some 40 registers: blocks of 256 threads as the sibling stages', eight waves a SIMD.
// Reads handed back unfiltered (primaryCount == 0xFFFF) get no junctions here, they are counted: the host filters them and makes theirs.
#pragma once
#include "common.h"
#include "../junction_core.h"

struct JunctionArgs {
    ydepth::Layout L;                          // the sequence table and -bpq (no bins)
    const ygpu_out_clump *fClumps;             // the gathered clumps, print order
    const uint32_t *outStart, *qlens;          // exclusive sums of the reads' output counts (n + 1 words); the reads' lengths
    uint32_t nReads;
    uint32_t *cnt; const uint32_t *start;      // junctions per read (zeroed before the count pass; n + 1 words) and their exclusive sums
    ygpu_junction *out; uint32_t cap;          // the batch's junctions and how many the buffer holds
    unsigned long long *stats;                 // reads with junctions, junctions, records skipped (MAPQ), reads left to the host
};

static constexpr unsigned long long YJ_NONE = ~0ull;       // the key of a lane without an eligible record: above every key

// key (and piece) of record k of a read whose clumps start at base; YJ_NONE when there is none or it is not eligible
__device__ inline unsigned long long junctionKey(const JunctionArgs &J, uint32_t base, uint32_t k, uint32_t n, uint32_t qlen, yjunc::Piece *p, int *why)
{
    *why = -1;
    if (k >= n) return YJ_NONE;
    const ygpu_out_clump f = J.fClumps[base + k];
    *why = yjunc::piece(J.L, f.c, f.status, f.mapQuality, qlen, p);
    return *why == yjunc::ELIGIBLE ? (unsigned long long)yjunc::orderKey(*p, k) : YJ_NONE;
}

__global__ void __launch_bounds__(256) k_junction_count(JunctionArgs J)
{
    const uint32_t r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (r >= J.nReads) return;
    const uint32_t base = J.outStart[r], n = J.outStart[r + 1] - base;
    if (n < 2) return;
    if (J.fClumps[base].primaryCount == 0xFFFFu) { if (lane == 0) atomicAdd(J.stats + 3, 1ull); return; }
    const uint32_t qlen = J.qlens[r];
    uint32_t nEl = 0, nSkip = 0;
    for (uint32_t k0 = 0; k0 < n; k0 += 64) {
        yjunc::Piece p; int why; (void)junctionKey(J, base, k0 + lane, n, qlen, &p, &why);
        nEl += (uint32_t)__popcll(__ballot(why == yjunc::ELIGIBLE)); nSkip += (uint32_t)__popcll(__ballot(why == yjunc::SKIPPED_MAPQ));
    }
    if (lane != 0) return;
    if (nSkip) atomicAdd(J.stats + 2, (unsigned long long)nSkip);
    if (nEl >= 2) { J.cnt[r] = nEl - 1; atomicAdd(J.stats + 0, 1ull); atomicAdd(J.stats + 1, (unsigned long long)(nEl - 1)); }
}

__global__ void __launch_bounds__(256) k_junction_emit(JunctionArgs J)
{
    const uint32_t r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (r >= J.nReads) return;
    const uint32_t j0 = J.start[r], nj = J.start[r + 1] - j0;
    if (nj == 0) return;
    const uint32_t base = J.outStart[r], n = J.outStart[r + 1] - base, qlen = J.qlens[r];
    for (uint32_t c1 = 0; c1 < n; c1 += 64) {
        yjunc::Piece mine; int why;
        const unsigned long long myKey = junctionKey(J, base, c1 + lane, n, qlen, &mine, &why);
        uint32_t rank = 0; unsigned long long before = 0;                   // keys below mine: how many, and the largest
        for (uint32_t c2 = 0; c2 < n; c2 += 64) {
            unsigned long long key2 = myKey;
            if (c2 != c1) { yjunc::Piece other; int w2; key2 = junctionKey(J, base, c2 + lane, n, qlen, &other, &w2); }
            const uint32_t m = n - c2 < 64u ? n - c2 : 64u;
            for (uint32_t l = 0; l < m; l++) {
                const unsigned long long k = __shfl(key2, (int)l, 64);
                if (k < myKey) { rank++; before = k > before ? k : before; }
            }
        }
        if (myKey == YJ_NONE || rank == 0) continue;
        // side A: the record before mine in the order, by its print order in the key
        const ygpu_out_clump fa = J.fClumps[base + yjunc::keyOrder(before)];
        yjunc::Piece a;
        if (yjunc::piece(J.L, fa.c, fa.status, fa.mapQuality, qlen, &a) != yjunc::ELIGIBLE) continue;
        const uint32_t at = j0 + rank - 1;
        if (rank - 1 < nj && at < J.cap) J.out[at] = yjunc::make(a, mine, r, rank - 1);
    }
}
