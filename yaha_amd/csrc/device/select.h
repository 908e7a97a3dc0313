// select.h -- the tile selection every side output ends with: the items of an array that pass a test, written out in ascending order of their index, so that
// only those cross PCIe.  A wave takes a tile of 64 x S::ROWS neighbouring items and counts the ones its selector S picks, by ballot and population count
// (k_select_count); an exclusive sum of the tiles' counts (scan.h) places the tiles; the second pass picks again and writes every picked item at its tile's
// start plus the picked items before it in the tile -- the popcount of the ballot below the lane, the rows' totals carried along (k_select_emit).  No atomics,
// no LDS; a tile without a picked item leaves the second pass after two loads.  cnt and start hold nTiles + 2 words, the two behind the counts zero: the sum
// runs over nTiles + 1 words, so start[nTiles] is the total.  `pos < cap` keeps a store inside what the host sized from that total.
//
// A selector is a small struct passed by value: the arrays it reads, the array it writes, and
//     ROWS, COUNT_UNROLL     the tile's height; 4 where the rows' loads are worth having in flight together in the count pass, 1: the loop as it stands
//     Rec                    what pick hands to put (NoRec: nothing)
//     bool pick(i, rec)      item i passes (false at and past the array's end); fills rec
//     void put(pos, i, rec)  stores item i as the pos-th record
// The selectors live with their stages: CandidateSel (pileup_stage.h), SnvSel (snv_stage.h), IndelDrainSel (indel_stage.h), IndelMergeDrainSel and
// IndelCallSel (indelcall_stage.h).
#pragma once
#include <stdint.h>

struct TileSel { uint32_t nTiles; uint32_t *cnt; const uint32_t *start; uint32_t cap; };
struct NoRec {};

template <class S> __device__ __forceinline__ uint32_t selectRowCount(const S &s, uint32_t tile, uint32_t r, uint32_t lane)
{
    typename S::Rec rec;
    return (uint32_t)__popcll(__ballot(s.pick((uint64_t)tile * (64u * S::ROWS) + r * 64u + lane, rec)));
}
template <class S> __global__ void __launch_bounds__(256) k_select_count(S s, TileSel t)
{
    const uint32_t tile = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (tile >= t.nTiles) return;
    uint32_t n = 0;
    if constexpr (S::COUNT_UNROLL > 1) {
#pragma unroll S::COUNT_UNROLL
        for (uint32_t r = 0; r < S::ROWS; r++) n += selectRowCount(s, tile, r, lane);
    } else {
        for (uint32_t r = 0; r < S::ROWS; r++) n += selectRowCount(s, tile, r, lane);
    }
    if (lane == 0) t.cnt[tile] = n;
}
template <class S> __global__ void __launch_bounds__(256) k_select_emit(S s, TileSel t)
{
    const uint32_t tile = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (tile >= t.nTiles) return;
    uint32_t at = t.start[tile];
    if (t.start[tile + 1] == at) return;
    for (uint32_t r = 0; r < S::ROWS; r++) {
        const uint64_t i = (uint64_t)tile * (64u * S::ROWS) + r * 64u + lane;
        typename S::Rec rec; const bool is = s.pick(i, rec);
        const unsigned long long m = __ballot(is);
        const uint32_t pos = at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (is && pos < t.cap) s.put(pos, i, rec);
        at += (uint32_t)__popcll(m);
    }
}
