// indelcall_stage.h -- indel calls with genotypes (-oindel) on the device: the run's raw indel alleles (indel_stage.h counted them, the host kept the run's
// map) are left-normalised against the image's reference, merged, and judged at their anchor base against the image's pileup array (pileup_stage.h made it).
// What the shift, the merge and a call are, and the record a call leaves, are ../indelcall_core.h, the very source the host compiles for its fallback
// (host/indelcalls.cpp).
//
// k_indel_norm: a raw allele gets a WAVE.  The wave decides -- the same on every lane -- whether the allele is judged at all and how far it may move (the cap
// and the anchor rule), then searches the first mismatch 64 steps at a time: lane l answers step i0 + l on its own (yindelcall::sameAt: two reference bases,
// or one and a base of the key; no state is carried from step to step), one ballot and a bit scan give the first step that fails, and the loop ends there or
// at the cap.  No lane walks base by base.  The bases of a moved insertion are built by the lanes -- lane j < L <= 42 takes base (j - s) mod L of the key and
// shifts it to its place -- and the two words are combined by an OR across the wave.  Lane 0 then inserts the normalised key into the merge table with the
// allele's count as the weight.
// The merge table is the context's own, made for the call: open addressing, linear probing, a power of two of at least twice the raw alleles, entries of 32
// bytes {w0, w1, w2, a 64-bit count}.  The insert is indel_stage.h's compare-and-swap on the three words; the count is a 64-bit atomic add (at most 2^32 raw
// alleles of at most 2^32 - 1 each: no wrap), saturated to 32 bits when the table is drained.  Which ENTRY a key lands in depends on who came first; the set
// of keys and every sum do not.  Draining is the indel table's with a store of its own that saturates the count (IndelMergeDrainSel).
//
// IndelCallSel: a lane per merged allele, 64 x 8 alleles a wave, through the tile selection of select.h.  The lane loads its allele and the seven words of its
// anchor's row, looks up the anchor's reference code and runs yindelcall::judge.  The kernels are small and latency-bound -- a run has thousands of alleles,
// not millions; their cost on a large run has not been measured.
#pragma once
#include "indel_stage.h"
#include "../indelcall_core.h"

struct IndelNormArgs {
    ydepth::Layout L; uint64_t nSlots; const uint8_t *bases; uint64_t nBaseBytes;      // the pileup's layout, the image's packed reference
    const ygpu_indel_entry *raw; uint32_t n, maxShift;
    ygpu_indel_entry *table; uint32_t mask;                                      // capacity - 1; the whole table may be probed (it is at most half full)
    unsigned long long *stats;                                                   // alleles that moved, alleles skipped, inserts that found no entry
    uint32_t *used;                                                              // entries turned from empty
};
__device__ __forceinline__ uint64_t waveOr64(uint64_t v)
{
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { lo |= (uint32_t)__shfl_xor((int)lo, d, 64); hi |= (uint32_t)__shfl_xor((int)hi, d, 64); }
    return (uint64_t)lo | (uint64_t)hi << 32;
}
__device__ __forceinline__ void indelMergeInsert(const IndelNormArgs &A, const yindel::Key &k, uint32_t weight)
{
    uint32_t at = (uint32_t)yindel::hashKey(k) & A.mask;
    for (uint32_t p = 0; p <= A.mask; p++, at = (at + 1u) & A.mask) {
        ygpu_indel_entry *const e = A.table + at;
        unsigned long long old = atomicCAS((unsigned long long *)&e->w0, 0ull, (unsigned long long)k.w0);
        if (old != 0ull && old != k.w0) continue;
        if (old == 0ull) atomicAdd(A.used, 1u);
        old = atomicCAS((unsigned long long *)&e->w1, 0ull, (unsigned long long)k.w1);
        if (old != 0ull && old != k.w1) continue;
        old = atomicCAS((unsigned long long *)&e->w2, 0ull, (unsigned long long)k.w2);
        if (old != 0ull && old != k.w2) continue;
        atomicAdd(reinterpret_cast<unsigned long long *>(&e->count), (unsigned long long)weight);      // (count and the word behind it: one 64-bit sum)
        return;
    }
    atomicAdd(A.stats + 2, 1ull);
}
__global__ void __launch_bounds__(256) k_indel_norm(IndelNormArgs A)
{
    const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= A.n) return;
    const ygpu_indel_entry e = A.raw[w];
    yindel::Key k; k.w0 = e.w0; k.w1 = e.w1; k.w2 = e.w2;
    uint32_t seq = 0, cap = 0;
    if (!yindelcall::callable(A.L, A.nSlots, k, A.maxShift, &seq, &cap)) { if (lane == 0) atomicAdd(A.stats + 1, 1ull); return; }      // (the same on every lane)
    uint32_t s = cap;
    for (uint32_t i0 = 0; i0 < cap; i0 += 64u) {
        const uint32_t i = i0 + lane;
        const unsigned long long bad = __ballot(i < cap && !yindelcall::sameAt(A.L, A.bases, A.nBaseBytes, seq, k, i));
        if (bad) { s = i0 + (uint32_t)__ffsll((long long)bad) - 1u; break; }
    }
    const uint32_t len = yindel::lenOfKey(k), type = yindel::typeOfKey(k);
    uint64_t p1 = 0, p2 = 0;
    if (type == (uint32_t)yindel::INS && lane < len) {                           // len <= KEPT = 42 here
        const uint64_t ch = yindelcall::rotatedBase(k, s, lane);
        if (lane < (uint32_t)yindel::PER_WORD) p1 = ch << (3u * lane); else p2 = ch << (3u * (lane - yindel::PER_WORD));
    }
    yindel::Key o; o.w0 = yindel::word0(yindel::slotOfKey(k) - s, type, len); o.w1 = waveOr64(p1) | yindel::kMarker; o.w2 = waveOr64(p2) | yindel::kMarker;
    if (lane == 0) { if (s) atomicAdd(A.stats, 1ull); indelMergeInsert(A, o, e.count); }
}

// ---- draining the merge table: indel_stage.h's pick, a store that saturates the 64-bit count ---------------------------------------------------------------------
struct IndelMergeDrainSel : IndelDrainSel {
    __device__ __forceinline__ void put(uint32_t pos, uint64_t i, const Rec &) const
    {
        ygpu_indel_entry e = table[i]; if (e.zero) { e.count = 0xFFFFFFFFu; e.zero = 0u; } out[pos] = e;
    }
};

// ---- the selection: every merged allele judged at its anchor ----------------------------------------------------------------------------------------------------
struct IndelCallSel {
    static constexpr uint32_t ROWS = 8, COUNT_UNROLL = 4; using Rec = ygpu_indel_call;
    ydepth::Layout L; const uint32_t *pu; uint32_t nSlots; const uint8_t *bases; uint64_t nBaseBytes;      // the image's array and packed reference
    const ygpu_indel_entry *alleles; uint32_t n;
    ygpu_indelcall_params P;
    ygpu_indel_call *out;
    __device__ __forceinline__ bool pick(uint64_t i, Rec &c) const
    {
        if (i >= n) return false;
        const ygpu_indel_entry e = alleles[i];
        yindel::Key k; k.w0 = e.w0; k.w1 = e.w1; k.w2 = e.w2;
        const uint32_t p = yindel::slotOfKey(k);
        if (p == 0u || p > nSlots) return false;                                 // (a normalised allele always has an anchor inside the array)
        uint32_t row[ypileup::NCH];
#pragma unroll
        for (int ch = 0; ch < ypileup::NCH; ch++) row[ch] = pu[(size_t)(p - 1u) * ypileup::NCH + ch];
        return yindelcall::judgeAt(L, bases, nBaseBytes, k, e.count, row, P, &c);
    }
    __device__ __forceinline__ void put(uint32_t pos, uint64_t, const Rec &c) const       // 64 bytes, 16-byte aligned: four 16-byte stores
    {
        uint4 *const o = reinterpret_cast<uint4 *>(out + pos);
        o[0] = make_uint4((uint32_t)c.w0, (uint32_t)(c.w0 >> 32), (uint32_t)c.w1, (uint32_t)(c.w1 >> 32));
        o[1] = make_uint4((uint32_t)c.w2, (uint32_t)(c.w2 >> 32), c.alt_count, c.ref_count);
        o[2] = make_uint4(c.depth, c.qual, c.gq, c.pl[0]); o[3] = make_uint4(c.pl[1], c.pl[2], c.info, 0u);
    }
};
