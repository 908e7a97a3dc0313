// bgzf_stage.h -- BGZF blocks deflated on the device (-obh / -obs; the format, the codes and the checksum's algebra are ../bgzf_core.h, the source the host's
// encoder compiles as well).  Owned by bgzf.hip.  The reference writes text only (AlignOutput.c); this stage has no counterpart there.
//
// k_bgzf_deflate: one workgroup of 256 lanes per payload of up to 65 280 bytes, which it reads from global memory (word loads, funnel-shifted to the byte).
//   The payload is walked in TILES of 256 positions, a lane a position:
//     search   the lane hashes its four bytes and takes the one candidate the table in LDS holds for them (1 + position; 32 KB); the table only ever holds
//              positions of EARLIER tiles -- the lanes add their own with atomicMax after the tile's barrier -- so what a lane finds does not depend on the
//              order lanes or waves run in, and neither do the bytes written.  The candidate is extended eight bytes a step (258 at most, never past the
//              payload, never at a distance over 32 768); where that gives no match the byte before (distance 1: runs) is tried.  Positions a match of an
//              earlier tile already covers search nothing.
//     parse    greedy, left to right: wave 0 holds the tile's match lengths in four registers a lane and hops through them with v_readlane (a scalar cursor,
//              a scalar loop), setting a bit per token start.
//     bits     a token lane makes its code (literal: 8 or 9 bits; match: up to 31); the workgroup's exclusive sum of the bit lengths places it.
//   This runs TWICE.  The first pass only adds up the lengths: the size of the deflated form is known before a byte of it exists, and where the stored form is
//   not larger the block is stored (a copy) and there is no second pass.  The second pass ORs the codes into a window of LDS words (ordinary LDS atomics: two
//   tokens may share a word) and flushes the window's whole words after every tile with plain 16-bit vector stores (the deflate data starts at byte 18 of the
//   slot); the unfinished word starts the next window.  The passes see the same table states and make the same parse, and every flush is clamped to the size
//   the first pass found, so nothing can leave the block's slot of 65 536 bytes.
//   The checksum: every lane takes the CRC-32 of 1/256 of the payload with a byte table in LDS, shifts it over the bytes behind its piece (multiplication by
//   x^(8 n) modulo the polynomial, ybgzf::crcShift) and the shares are joined by exclusive or: the host never reads the payload again.
// k_bgzf_offsets: the exclusive sum of the blocks' sizes (one workgroup; a batch has a few hundred blocks).  The path's sums (scan.h through prims.hip) take
//   a context's look-back state and failure counter; this primitive has no context.
// k_bgzf_gather: every block copied from its slot to its place in the contiguous output.
#pragma once
#include "common.h"
#include "../bgzf_core.h"

#define YBZ_BS 256
// a tile adds at most 255 * 9 + 31 bits (a match covers four positions, so matches only shorten it) to at most 31 left over: 75 words
enum : uint32_t { YBZ_WIN_WORDS = 128,
                  YBZ_PAD = 16 };                  // bytes a search may read past the input's end (two words past the last compared one): the input buffer has them

// the four bytes at byte offset `off` of a word-aligned buffer
__device__ __forceinline__ uint32_t bzLoad32(const uint32_t *words, uint32_t off)
{
    const uint32_t lo = words[off >> 2], hi = words[(off >> 2) + 1u];
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> ((off & 3u) * 8u));
}
// how far the bytes at p and at c < p agree, `most` at the most
__device__ __forceinline__ uint32_t bzExtend(const uint32_t *words, uint32_t p, uint32_t c, uint32_t most)
{
    uint32_t k = 0;
    while (k < most) {
        const uint64_t x = (uint64_t)(bzLoad32(words, p + k) ^ bzLoad32(words, c + k)) | (uint64_t)(bzLoad32(words, p + k + 4u) ^ bzLoad32(words, c + k + 4u)) << 32;
        if (x) { k += (uint32_t)__builtin_ctzll(x) >> 3; break; }
        k += 8u;
    }
    return k < most ? k : most;
}
// the workgroup's exclusive sum of v (every lane calls it; sWave: four words; a barrier inside); *total: the sum over all lanes
__device__ __forceinline__ uint32_t bzExclSum(uint32_t v, uint32_t *sWave, uint32_t *total)
{
    const uint32_t incl = waveInclSumU(v); const int wave = (int)(threadIdx.x >> 6);
    if (laneId() == 63) sWave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < YBZ_BS / 64; w++) { const uint32_t s = sWave[w]; all += s; if (w < wave) before += s; }
    *total = all;
    return before + incl - v;
}

__global__ void __launch_bounds__(YBZ_BS) k_bgzf_deflate(const uint32_t *in /* the stream, word-aligned, YBZ_PAD readable bytes behind it */, unsigned long long nIn,
                                                         uint8_t *slots /* BLOCK_MAX bytes a block */, uint32_t *sizes)
{
    YD_HIGH_PRIO();
    using namespace ybgzf;
    __shared__ uint32_t sHash[HASH_SIZE];
    __shared__ uint32_t sWin[YBZ_WIN_WORDS];
    __shared__ uint32_t sCrcTab[256];
    __shared__ uint16_t sLen[YBZ_BS], sDist[YBZ_BS];
    __shared__ uint8_t  sTok[YBZ_BS];
    __shared__ uint32_t sWave[YBZ_BS / 64], sCur, sCrc;
    const uint32_t tid = threadIdx.x, lane = (uint32_t)laneId(), wave = tid >> 6;
    const unsigned long long base = (unsigned long long)blockIdx.x * PAYLOAD_MAX;
    const uint32_t n = (uint32_t)(nIn - base < PAYLOAD_MAX ? nIn - base : PAYLOAD_MAX);
    const uint32_t *words = in + base / 4u; const uint8_t *bytes = (const uint8_t *)words;
    uint8_t *dst = slots + (size_t)blockIdx.x * BLOCK_MAX;
    const uint32_t nTiles = (n + YBZ_BS - 1u) / YBZ_BS;

    // ---- the checksum ---------------------------------------------------------------------------------------------------------------------------------------------
    sCrcTab[tid] = crcEntry(tid); if (tid == 0) sCrc = 0;
    __syncthreads();
    {
        const uint32_t piece = (n + YBZ_BS - 1u) / YBZ_BS, lo = min(tid * piece, n), hi = min(lo + piece, n);
        const uint32_t share = crcShift(crc32(sCrcTab, bytes + lo, hi - lo), n - hi);
        atomicXor(&sCrc, share);
    }

    uint32_t deflated = 0;
    for (int pass = 0; pass < 2; pass++) {
        // pass 0: the tokens' bit lengths; pass 1: the bits.  Both start from an empty table and the cursor at 0.
        for (uint32_t h = tid; h < HASH_SIZE; h += YBZ_BS) sHash[h] = 0;
        if (tid < YBZ_WIN_WORDS) sWin[tid] = tid == 0 ? (uint32_t)BLOCK_HEAD : 0u;
        if (tid == 0) sCur = 0;
        uint32_t bitPos = BLOCK_HEAD_BITS;                                       // (the same value in every lane)
        __syncthreads();
        for (uint32_t tile = 0; tile < nTiles; tile++) {
            const uint32_t tileBase = tile * YBZ_BS, p = tileBase + tid, curStart = sCur;
            // search
            uint32_t len = 0, dist = 0, h = 0; const bool hashed = p + MIN_MATCH <= n;
            if (hashed) {
                h = hash4(bzLoad32(words, p));
                if (p >= curStart) {
                    const uint32_t cand = sHash[h], most = min(n - p, (uint32_t)MAX_MATCH);
                    if (cand && p - (cand - 1u) <= MAX_DIST) { len = bzExtend(words, p, cand - 1u, most); dist = p - (cand - 1u); }
                    if (len < MIN_MATCH && p >= 1u) { len = bzExtend(words, p, p - 1u, most); dist = 1u; }
                    if (len < MIN_MATCH) len = 0;
                }
            }
            sLen[tid] = (uint16_t)len; sDist[tid] = (uint16_t)(dist - 1u);         // (32 768 does not fit sixteen bits)
            __syncthreads();
            if (hashed) atomicMax(&sHash[h], p + 1u);
            // parse: wave 0, a scalar cursor
            if (UNI_B(wave == 0)) {
                uint32_t cur = uniU(curStart);
#pragma unroll
                for (uint32_t k = 0; k < YBZ_BS / 64; k++) {
                    const uint32_t L = sLen[k * 64u + lane], chunkBase = tileBase + k * 64u, chunkEnd = min(chunkBase + 64u, n);
                    uint64_t starts = 0;
                    while (UNI_B(cur < chunkEnd)) {
                        const uint32_t i = uniU(cur - chunkBase), l = (uint32_t)__builtin_amdgcn_readlane((int)L, (int)i);
                        starts |= 1ull << i; cur = uniU(cur + (l ? l : 1u));
                    }
                    sTok[k * 64u + lane] = (uint8_t)((starts >> lane) & 1u);
                }
                if (lane == 0) sCur = cur;
            }
            __syncthreads();
            // bits
            Bits t{0, 0};
            if (sTok[tid]) { const uint32_t l = sLen[tid]; t = l ? matchBits(l, (uint32_t)sDist[tid] + 1u) : literalBits(bytes[p]); }
            uint32_t total; const uint32_t at = bitPos + bzExclSum(t.n, sWave, &total);      // (a barrier inside)
            const uint32_t winBase = bitPos >> 5, newPos = bitPos + total;
            if (pass == 1) {
                if (t.n) {
                    const uint32_t w = (at >> 5) - winBase, s = at & 31u;
                    atomicOr(&sWin[w], t.v << s);
                    if (s + t.n > 32u) atomicOr(&sWin[w + 1u], t.v >> (32u - s));
                }
                __syncthreads();
                // the window's whole words leave as halves (byte 18 of the slot is no word boundary); nothing past the size pass 0 found
                const uint32_t whole = (newPos >> 5) - winBase, halfAt = 2u * winBase + tid;
                if (tid < 2u * whole && 2u * halfAt + 2u <= deflated) ((uint16_t *)(dst + HEADER))[halfAt] = (uint16_t)(sWin[tid >> 1] >> (16u * (tid & 1u)));
                const uint32_t carry = sWin[whole];
                __syncthreads();
                if (tid < YBZ_WIN_WORDS) sWin[tid] = tid == 0 ? carry : 0u;
            }
            bitPos = newPos;
            __syncthreads();
        }
        if (pass == 0) {
            deflated = deflateBytes((uint64_t)bitPos - BLOCK_HEAD_BITS);
            if (useStored(deflated, n)) break;                                   // (the same in every lane: bitPos is)
        } else {
            // the last bits and the end-of-block symbol's seven zeros: what the window still holds, byte by byte
            const uint32_t done = 4u * (bitPos >> 5);
            if (done + tid < deflated && tid < 4u * YBZ_WIN_WORDS) dst[HEADER + done + tid] = (uint8_t)(sWin[tid >> 2] >> (8u * (tid & 3u)));
        }
    }
    const bool stored = useStored(deflated, n);
    const uint32_t body = stored ? n + STORED_OVERHEAD : deflated;
    if (stored) for (uint32_t i = tid; i < n; i += YBZ_BS) dst[HEADER + STORED_OVERHEAD + i] = bytes[i];
    if (tid == 0) {
        putHeader(dst, blockBytes(body));
        if (stored) putStoredHead(dst + HEADER, n);
        putTrailer(dst + HEADER + body, sCrc, n);
        sizes[blockIdx.x] = blockBytes(body);
    }
}

// offs[b] = the bytes of the blocks before b; offs[nBlocks] = all of them.  One workgroup.
__global__ void __launch_bounds__(YBZ_BS) k_bgzf_offsets(const uint32_t *sizes, uint32_t nBlocks, unsigned long long *offs)
{
    YD_HIGH_PRIO();
    __shared__ uint32_t sWave[YBZ_BS / 64];
    unsigned long long running = 0;
    for (uint32_t b0 = 0; b0 < nBlocks; b0 += YBZ_BS) {
        const uint32_t b = b0 + threadIdx.x, v = b < nBlocks ? sizes[b] : 0u;
        uint32_t total; const uint32_t before = bzExclSum(v, sWave, &total);
        if (b < nBlocks) offs[b] = running + before;
        running += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) offs[nBlocks] = running;
}

// one workgroup a block: its bytes from its slot to their place
__global__ void __launch_bounds__(YBZ_BS) k_bgzf_gather(const uint8_t *slots, const uint32_t *sizes, const unsigned long long *offs, uint8_t *out)
{
    YD_HIGH_PRIO();
    const uint8_t *src = slots + (size_t)blockIdx.x * ybgzf::BLOCK_MAX; uint8_t *dst = out + offs[blockIdx.x];
    const uint32_t n = min(sizes[blockIdx.x], (uint32_t)ybgzf::BLOCK_MAX);
    for (uint32_t i = threadIdx.x; i < n; i += YBZ_BS) dst[i] = src[i];
}
