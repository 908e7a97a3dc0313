// track_stage.h -- what the kernels of the binned tracks (depth_stage.h, events_stage.h) open with: a printed clump gets a wave, the gate of the record is counted
// once, and the wave takes the clump's ops 64 at a time with a scan of their reference-consuming lengths, which gives every op its reference offset.
#pragma once
#include "common.h"
#include "../depth_core.h"

// the gate of a printed clump (the same on every lane of its wave): lane 0 counts what became of the record; true = the wave goes on to walk it
__device__ __forceinline__ bool trackGate(const ydepth::Layout &L, const ygpu_out_clump &f, unsigned long long *stats, uint32_t lane, int *seq)
{
    const int g = ydepth::gate(L, f.c, f.mapQuality, seq);
    if (lane == 0) atomicAdd(stats + g, 1ull);
    return g == ydepth::COUNTED;
}
// 64 ops of a clump, one a lane (all 64 lanes call it): the lane's op (0 past the end), the reference bases it consumes and whether they are covered, and the
// sums of those lengths across the wave -- up to and including the lane, before it, and over the chunk
struct OpChunk { uint32_t k, op, n, incl, excl, total; bool covered; };
__device__ __forceinline__ OpChunk loadOpChunk(const uint32_t *ops, uint32_t nOps, uint32_t k0, uint32_t lane)
{
    OpChunk c; c.k = k0 + lane; c.op = c.k < nOps ? ops[c.k] : 0u; c.covered = false;
    c.n = c.k < nOps ? ydepth::opRef(c.op, &c.covered) : 0u;
    c.incl = waveInclSumU(c.n); c.excl = c.incl - c.n; c.total = (uint32_t)__shfl((int)c.incl, 63, 64);
    return c;
}
