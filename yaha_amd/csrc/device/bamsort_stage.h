// bamsort_stage.h -- the coordinate order of a run's BAM records and the way of the ordered records into the deflate kernels (-obsort; ygpu_bamsort_* in
// bgzf.hip, which owns this header).  The reference writes unsorted text only; this stage has no counterpart there.
//
// The order is a stable least-significant-digit radix sort of the 64-bit keys (sequence << 32 | position), eight bits a pass, the record number as the value.
// A pass is three launches over tiles of YBS_TILE keys, a key a lane, lanes in key order:
//   k_bamsort_hist     the tile's count of every digit (LDS counters: only their SUMS are used, which no order of the additions changes) to table[digit][tile];
//   k_bamsort_sum      the exclusive sum over the table read digit-major -- where the first key of (digit, tile) goes -- by one workgroup, like k_bgzf_offsets;
//   k_bamsort_scatter  a key's place = the table's entry + the keys of its digit in the waves before its own + those in the lanes below it.  The last comes from
//                      eight ballots (the mask of the lanes with the same digit, a bit of the digit a ballot) and a population count below the lane; the
//                      first from a table in LDS that one lane per (wave, digit) -- the lowest of the mask -- fills with the mask's population with a plain
//                      store.  No atomic takes part in a rank: equal digits keep their order because lane order is key order, whatever order the hardware
//                      serves anything in.
// k_bamsort_sum also gives every record its offset in the sorted stream (the lengths read through the permutation, 64-bit sums).
// k_bam_gather: a wave a record of a window of that stream: the part of the record inside the window from its segment to the window buffer -- bytes up to the
//   destination's first dword boundary, whole dwords (the source read as aligned dwords and funnel-shifted where its alignment differs), bytes at the end.
#pragma once
#include "common.h"

#define YBS_BS 256
enum : uint32_t { YBS_TILE = YBS_BS,            // keys a scatter tile ranks
                  YBS_SUM_ITEMS = 4 };          // entries a lane of k_bamsort_sum takes a trip

__global__ void __launch_bounds__(YBS_BS) k_bamsort_iota(uint32_t *vals, uint32_t n)
{
    const uint32_t i = blockIdx.x * YBS_BS + threadIdx.x;
    if (i < n) vals[i] = i;
}

__global__ void __launch_bounds__(YBS_BS) k_bamsort_hist(const unsigned long long *keys, uint32_t n, uint32_t shift, uint32_t nTiles, uint32_t *table)
{
    __shared__ uint32_t sCount[256];
    sCount[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * YBS_TILE + threadIdx.x;
    if (i < n) atomicAdd(&sCount[(uint32_t)(keys[i] >> shift) & 255u], 1u);
    __syncthreads();
    table[(size_t)threadIdx.x * nTiles + blockIdx.x] = sCount[threadIdx.x];
}

// out[i] = the sum of v[idx ? idx[j] : j] over j < i, for i <= n (out[n]: everything; out may be v itself when idx is null).  One workgroup.
template <class OutT> __global__ void __launch_bounds__(YBS_BS) k_bamsort_sum(const uint32_t *v, const uint32_t *idx, unsigned long long n, OutT *out)
{
    __shared__ unsigned long long sWave[YBS_BS / 64];
    const uint32_t lane = (uint32_t)laneId(), wave = threadIdx.x >> 6;
    unsigned long long running = 0;
    for (unsigned long long base = 0; base < n; base += (unsigned long long)YBS_BS * YBS_SUM_ITEMS) {
        const unsigned long long i0 = base + (unsigned long long)threadIdx.x * YBS_SUM_ITEMS;
        uint32_t x[YBS_SUM_ITEMS]; unsigned long long mine = 0;
#pragma unroll
        for (uint32_t k = 0; k < YBS_SUM_ITEMS; k++) { x[k] = i0 + k < n ? v[idx ? idx[i0 + k] : i0 + k] : 0u; mine += x[k]; }
        // the wave's inclusive sum of the lanes' shares (64-bit: a run's bytes pass 2^32), then the waves in order
        unsigned long long incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)incl, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), d, 64);
            if (lane >= (uint32_t)d) incl += (unsigned long long)hi << 32 | lo;
        }
        if (lane == 63) sWave[wave] = incl;
        __syncthreads();
        unsigned long long before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < YBS_BS / 64; w++) { const unsigned long long s = sWave[w]; all += s; if (w < wave) before += s; }
        unsigned long long at = running + before + incl - mine;
#pragma unroll
        for (uint32_t k = 0; k < YBS_SUM_ITEMS; k++) { if (i0 + k < n) out[i0 + k] = (OutT)at; at += x[k]; }
        running += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) out[n] = (OutT)running;
}

__global__ void __launch_bounds__(YBS_BS) k_bamsort_scatter(const unsigned long long *keysIn, const uint32_t *valsIn, unsigned long long *keysOut, uint32_t *valsOut, uint32_t n,
                                                            uint32_t shift, uint32_t nTiles, const uint32_t *table /* after k_bamsort_sum */)
{
    __shared__ uint32_t sWaveCount[YBS_BS / 64][256];
    const uint32_t lane = (uint32_t)laneId(), wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t w = 0; w < YBS_BS / 64; w++) sWaveCount[w][threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * YBS_TILE + threadIdx.x; const bool valid = i < n;
    unsigned long long key = 0; uint32_t val = 0, digit = 0;
    if (valid) { key = keysIn[i]; val = valsIn[i]; digit = (uint32_t)(key >> shift) & 255u; }
    // the lanes of this wave that hold a key with the same digit
    unsigned long long same = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
    for (uint32_t b = 0; b < 8; b++) {
        const unsigned long long set = __builtin_amdgcn_ballot_w64((digit >> b & 1u) != 0);
        same &= (digit >> b & 1u) ? set : ~set;
    }
    const uint32_t below = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    if (valid && below == 0) sWaveCount[wave][digit] = (uint32_t)__popcll(same);      // (one lane per wave and digit: a plain store)
    __syncthreads();
    if (valid) {
        uint32_t at = table[(size_t)digit * nTiles + blockIdx.x] + below;
#pragma unroll
        for (uint32_t w = 0; w < YBS_BS / 64; w++) if (w < wave) at += sWaveCount[w][digit];
        if (at < n) { keysOut[at] = key; valsOut[at] = val; }                          // (at < n always; the check keeps a wrong table inside the arrays)
    }
}

// Window [w0, w1) of the sorted stream into win: wave r of the grid takes sorted place j0 + r, whose record perm[j] starts at stream offset offs[j], has lens[..]
// bytes and lies at addr[..] in its segment.  Segments have eight readable bytes behind their last record (the funnel's second dword).
__global__ void __launch_bounds__(YBS_BS) k_bam_gather(const uint32_t *perm, const unsigned long long *offs, const unsigned long long *addr, const uint32_t *lens, uint32_t j0,
                                                       uint32_t nRec, unsigned long long w0, unsigned long long w1, uint8_t *win)
{
    const uint32_t r = blockIdx.x * (YBS_BS / 64) + (threadIdx.x >> 6), lane = (uint32_t)laneId();
    if (r >= nRec) return;
    const uint32_t rec = perm[j0 + r];
    const unsigned long long s0 = offs[j0 + r], s1 = s0 + lens[rec];
    const unsigned long long a = s0 > w0 ? s0 : w0, b = s1 < w1 ? s1 : w1;
    if (a >= b) return;
    const uint8_t *src = (const uint8_t *)(uintptr_t)addr[rec] + (a - s0);
    uint8_t *dst = win + (a - w0);
    const uint32_t nBytes = (uint32_t)(b - a);
    uint32_t head = (uint32_t)(4u - ((uintptr_t)dst & 3u)) & 3u; if (head > nBytes) head = nBytes;
    if (lane < head) dst[lane] = src[lane];
    const uint32_t nWords = (nBytes - head) >> 2, tail = head + 4u * nWords;
    const uint8_t *s = src + head; uint32_t *d = (uint32_t *)(dst + head);
    const uint32_t mis = (uint32_t)((uintptr_t)s & 3u);
    if (mis == 0) { const uint32_t *sw = (const uint32_t *)s; for (uint32_t k = lane; k < nWords; k += 64u) d[k] = sw[k]; }
    else {
        const uint32_t *sw = (const uint32_t *)(s - mis); const uint32_t sh = 8u * mis;
        for (uint32_t k = lane; k < nWords; k += 64u) { const uint32_t lo = sw[k], hi = sw[k + 1u]; d[k] = (uint32_t)((((unsigned long long)hi << 32) | lo) >> sh); }
    }
    if (lane < nBytes - tail) dst[tail + lane] = src[tail + lane];
}
