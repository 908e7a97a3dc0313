// snv_stage.h -- SNV calls with genotypes (-osnv) selected on the device from an image's pileup array (pileup_stage.h made it): what a call is and the record it
// leaves are ../snv_core.h, the very source the host compiles for its fallback (host/snv.cpp).
//
// k_pileup_add: one call needs the SUM of all sources before it is judged -- the host's blocks (reads handed back, runs filtered on the host) and the other
// images of a run over several devices are folded into ONE image's array first: a thread per (list entry, channel), a plain global atomicAdd (no value
// returned, device scope) where the word to add is not zero.  A slot at or past nSlots adds nothing; slots need not be distinct.
//
// k_snv_count / k_snv_emit have the shape of k_pileup_count / k_pileup_emit: a wave takes a tile of 64 x YS_TILE_ROWS neighbouring slots, counts its calls, an
// exclusive sum of the tiles' counts (scan.h) places them, and the second pass writes the records by ballot and population count in ascending slot order, no
// atomics, no LDS.  An untouched slot leaves after its loads, before the sequence table is searched.  The row loads: a lane reads the seven words of its slot,
// 28 bytes apart from its neighbour's, so one row of a tile is 1 792 contiguous bytes -- fourteen 128-byte lines, each of them touched by every one of the
// lane's loads: memory sees every line once, the vector cache sees it up to seven times.  Staging a row through LDS with 16-byte loads would make that once;
// it has not been built (DESIGN 4 says what is and is not measured).  The rows of a tile are independent, so the loop is unrolled and their loads are in flight
// together.
#pragma once
#include "pileup_stage.h"
#include "../snv_core.h"

__global__ void __launch_bounds__(256) k_pileup_add(uint32_t *pu, uint32_t nSlots, const uint32_t *slots, const uint32_t *rows, uint32_t n)
{
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (uint64_t)n * ypileup::NCH) return;
    const uint32_t i = (uint32_t)(idx / ypileup::NCH), ch = (uint32_t)(idx % ypileup::NCH), s = slots[i], v = rows[idx];
    if (s < nSlots && v) atomicAdd(pu + (size_t)s * ypileup::NCH + ch, v);
}

#define YS_TILE_ROWS YP_TILE_ROWS
#define YS_TILE YP_TILE
struct SnvArgs {
    ydepth::Layout L; const uint32_t *pu; uint32_t nSlots, nTiles; const uint8_t *bases; uint64_t nBaseBytes;      // the image's array and packed reference
    ygpu_snv_params P;
    uint32_t *cnt; const uint32_t *start; ygpu_snv_call *out; uint32_t cap;
};
__device__ __forceinline__ bool snvCall(const SnvArgs &A, uint64_t slot64, ygpu_snv_call *c)
{
    if (slot64 >= A.nSlots) return false;
    const uint32_t slot = (uint32_t)slot64;
    uint32_t row[ypileup::NCH];
#pragma unroll
    for (int ch = 0; ch < ypileup::NCH; ch++) row[ch] = A.pu[(size_t)slot * ypileup::NCH + ch];
    return ysnv::judgeAt(A.L, A.bases, A.nBaseBytes, slot, row, A.P, c);
}
__global__ void __launch_bounds__(256) k_snv_count(SnvArgs A)
{
    const uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (t >= A.nTiles) return;
    uint32_t n = 0;
#pragma unroll 4
    for (uint32_t r = 0; r < YS_TILE_ROWS; r++) { ygpu_snv_call c; n += (uint32_t)__popcll(__ballot(snvCall(A, (uint64_t)t * YS_TILE + r * 64u + lane, &c))); }
    if (lane == 0) A.cnt[t] = n;
}
__global__ void __launch_bounds__(256) k_snv_emit(SnvArgs A)
{
    const uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (t >= A.nTiles) return;
    uint32_t at = A.start[t];
    if (A.start[t + 1] == at) return;
    for (uint32_t r = 0; r < YS_TILE_ROWS; r++) {
        ygpu_snv_call c; const bool is = snvCall(A, (uint64_t)t * YS_TILE + r * 64u + lane, &c);
        const unsigned long long m = __ballot(is);
        const uint32_t pos = at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (is && pos < A.cap) {                                             // 48 bytes, 16-byte aligned: three 16-byte stores
            uint4 *const o = reinterpret_cast<uint4 *>(A.out + pos);
            o[0] = make_uint4(c.slot, c.info, c.ref_count, c.alt_count); o[1] = make_uint4(c.depth, c.other, c.qual, c.gq); o[2] = make_uint4(c.pl[0], c.pl[1], c.pl[2], 0u);
        }
        at += (uint32_t)__popcll(m);
    }
}
