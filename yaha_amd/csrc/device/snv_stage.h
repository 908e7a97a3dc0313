// snv_stage.h -- SNV calls with genotypes (-osnv) selected on the device from an image's pileup array (pileup_stage.h made it): what a call is and the record it
// leaves are ../snv_core.h, the very source the host compiles for its fallback (host/snv.cpp).
//
// k_pileup_add: one call needs the SUM of all sources before it is judged -- the host's blocks (reads handed back, runs filtered on the host) and the other
// images of a run over several devices are folded into ONE image's array first: a thread per (list entry, channel), a plain global atomicAdd (no value
// returned, device scope) where the word to add is not zero.  A slot at or past nSlots adds nothing; slots need not be distinct.
//
// SnvSel judges every slot of the array and leaves the calls' records in ascending slot order, through the tile selection of select.h, 64 x 32 slots a
// wave.  An untouched slot leaves after its loads, before the sequence table is searched.  The row loads of pick: a lane reads the seven words of its slot,
// 28 bytes apart from its neighbour's, so one row of a tile is 1 792 contiguous bytes -- fourteen 128-byte lines, each of them touched by every one of the
// lane's loads: memory sees every line once, the vector cache sees it up to seven times.  Staging a row through LDS with 16-byte loads would make that once;
// it has not been built (DESIGN 4 says what is and is not measured).  The rows of a tile are independent, so the count pass is unrolled by four and their
// loads are in flight together.
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

struct SnvSel {
    static constexpr uint32_t ROWS = CandidateSel::ROWS, COUNT_UNROLL = 4; using Rec = ygpu_snv_call;
    ydepth::Layout L; const uint32_t *pu; uint32_t nSlots; const uint8_t *bases; uint64_t nBaseBytes;      // the image's array and packed reference
    ygpu_snv_params P;
    ygpu_snv_call *out;
    __device__ __forceinline__ bool pick(uint64_t slot64, Rec &c) const
    {
        if (slot64 >= nSlots) return false;
        const uint32_t slot = (uint32_t)slot64;
        uint32_t row[ypileup::NCH];
#pragma unroll
        for (int ch = 0; ch < ypileup::NCH; ch++) row[ch] = pu[(size_t)slot * ypileup::NCH + ch];
        return ysnv::judgeAt(L, bases, nBaseBytes, slot, row, P, &c);
    }
    __device__ __forceinline__ void put(uint32_t pos, uint64_t, const Rec &c) const       // 48 bytes, 16-byte aligned: three 16-byte stores
    {
        uint4 *const o = reinterpret_cast<uint4 *>(out + pos);
        o[0] = make_uint4(c.slot, c.info, c.ref_count, c.alt_count); o[1] = make_uint4(c.depth, c.other, c.qual, c.gq); o[2] = make_uint4(c.pl[0], c.pl[1], c.pl[2], 0u);
    }
};
