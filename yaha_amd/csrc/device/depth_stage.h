// depth_stage.h -- read depth along the reference (-ocov) accumulated on the device, right behind the post-filter: the clumps that will be printed, their edit
// ops and the table of reference sequences are all in HBM at that point, so the coverage array is fed there and the clumps are not walked a second time on the
// host.  The walk itself is ../depth_core.h, the very source the host compiles for the records the device does not see (host/depth.cpp).
//
// The work is uneven -- a 10 kbp read has covered runs of thousands of bases, a chimeric 1 kbp read dozens of short ones -- so a clump gets a WAVE: the lanes take
// 64 ops at a time, a scan of their reference-consuming lengths across the wave gives every op its reference offset, the D ops among them (a ballot) cut the chunk
// into covered runs (neighbouring M and R ops are one run, and a run carries on into the next 64 ops), and a run's bins -- its bases at a bin of 1 -- are dealt across
// the lanes: neighbouring lanes add to neighbouring words, one atomic per (run, bin).  The array is shared by the contexts of an index image; plain global
// atomicAdd on uint32 (no value returned, device scope) makes that safe.
#pragma once
#include "track_stage.h"

struct DepthArgs {
    ydepth::Layout L;
    uint32_t *cov; uint32_t nBins;             // the image's coverage array
    unsigned long long *stats;                 // records counted, skipped (MAPQ), dropped (two sequences), reads left to the host
};

__global__ void __launch_bounds__(256) k_depth_clumps(DepthArgs D, const ygpu_out_clump *fClumps, const uint32_t *fOps, uint32_t nClumps)
{
    const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= nClumps) return;
    const ygpu_out_clump f = fClumps[w];
    if (f.primaryCount == 0xFFFFu) return;                                  // a read handed back unfiltered: the host filters it and counts what it prints
    int seq = -1;
    if (!trackGate(D.L, f, D.stats, lane, &seq)) return;
    uint32_t *const cov = D.cov; const uint32_t nBins = D.nBins;
    auto add = [cov, nBins](uint32_t b, uint32_t n) { if (b < nBins) atomicAdd(cov + b, n); };
    const uint32_t *ops = fOps + f.c.op_start; const uint32_t nOps = f.c.n_ops;
    uint32_t cur = f.c.sro, runStart = f.c.sro;                             // (the same on every lane)
    for (uint32_t k0 = 0; k0 < nOps; k0 += 64) {
        const OpChunk c = loadOpChunk(ops, nOps, k0, lane);
        unsigned long long dels = __ballot(!c.covered && c.n != 0);
        while (dels) {                                                      // every D of the chunk ends the run before it
            const int l = __ffsll((long long)dels) - 1; dels &= dels - 1;
            const uint32_t dOff = cur + (uint32_t)__shfl((int)c.excl, l, 64), dLen = (uint32_t)__shfl((int)c.n, l, 64);
            ydepth::addRun(D.L, seq, runStart, dOff - runStart, lane, 64u, add);
            runStart = dOff + dLen;
        }
        cur += c.total;
    }
    ydepth::addRun(D.L, seq, runStart, cur - runStart, lane, 64u, add);
}

// the reads the post-filter handed back unfiltered (more clumps than its stage takes): counted, so that the host's share of a run shows in the statistics
__global__ void k_depth_handed_back(const uint32_t *outCnt, const uint32_t *primCnt, uint32_t nReads, unsigned long long *stats)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < nReads && outCnt[r] != 0 && primCnt[r] == 0xFFFFu) atomicAdd(stats + 3, 1ull);
}
