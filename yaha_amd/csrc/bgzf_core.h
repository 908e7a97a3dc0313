// bgzf_core.h -- BGZF blocks (-obh / -obs: BAM output): the block format, the checksum and the deflate encoder's pieces as ONE set of routines compiled for the
// host (host/bam.cpp: the header's blocks, the fallback; tests/fixtures/bgzf_driver.cpp) and for the device (device/bgzf_stage.h: a workgroup per block), so that
// the two sides cannot drift apart.  No allocation, no library calls.
//
// The contract (every layer and every test shares it):
//   A stream is cut into PAYLOADS of at most PAYLOAD_MAX = 65 280 bytes; every payload becomes one BGZF block: an 18-byte gzip header with the extra subfield
//   "BC" that holds BSIZE = block bytes - 1, ONE final raw-deflate block, and the trailer { CRC-32 of the payload, ISIZE = payload bytes }.
//   The deflate block uses the FIXED Huffman codes (BTYPE 01) over a greedy LZ77 parse: matches of MIN_MATCH = 4 to MAX_MATCH = 258 bytes at a distance of 1 to
//   MAX_DIST = 32 768, found through a hash of four bytes that remembers one earlier position per value; a match never starts before the payload's first byte.
//   The size is known before the first byte is written: the parse runs once to add up its tokens' bit lengths (deflateBytes), and only when that form is smaller
//   than the STORED one (BTYPE 00: STORED_OVERHEAD = 5 bytes and the payload itself) does it run a second time to write.  Whatever the input, a block has at
//   most HEADER + STORED_OVERHEAD + PAYLOAD_MAX + TRAILER = 65 311 bytes, inside its slot of BLOCK_MAX = 65 536.
//   Host and device parse differently (the host sees every earlier position, the device only those of earlier tiles of a workgroup's width) and so write
//   different bytes for one payload; each of them writes the same bytes for it every time.
//   The end-of-file marker is the block of an empty payload (28 bytes, putEof); the writer appends it, no encoder does.
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define YBZ_FN __host__ __device__ inline
#else
#define YBZ_FN inline
#endif

namespace ybgzf {

enum : uint32_t { PAYLOAD_MAX = 65280, BLOCK_MAX = 65536, HEADER = 18, TRAILER = 8, STORED_OVERHEAD = 5, EOF_BYTES = 28, MIN_MATCH = 4, MAX_MATCH = 258, MAX_DIST = 32768,
                  HASH_BITS = 13, HASH_SIZE = 1u << HASH_BITS };
static_assert(HEADER + STORED_OVERHEAD + PAYLOAD_MAX + TRAILER <= BLOCK_MAX, "a stored block must fit its slot");
static_assert(PAYLOAD_MAX % 4 == 0, "payloads start on a word of the stream");

YBZ_FN uint64_t blocksOf(uint64_t nIn) { return (nIn + PAYLOAD_MAX - 1) / PAYLOAD_MAX; }
YBZ_FN uint64_t bound(uint64_t nIn) { return blocksOf(nIn) * (uint64_t)BLOCK_MAX; }

// ---- CRC-32 (the zlib polynomial, reflected) -----------------------------------------------------------------------------------------------------------------
constexpr uint32_t POLY = 0xEDB88320u;
YBZ_FN uint32_t crcEntry(uint32_t i) { for (int k = 0; k < 8; k++) i = (i & 1u) ? (i >> 1) ^ POLY : i >> 1; return i; }      // entry i of the byte table
// the checksum of n bytes, as zlib.crc32 gives it; tab: crcEntry(0 .. 255)
template <class Tab> YBZ_FN uint32_t crc32(const Tab *tab, const uint8_t *p, uint32_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; i++) c = tab[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return ~c;
}
// Checksums of pieces join without a second look at the bytes: crc(A B) = crc(A) * x^(8 |B|) + crc(B) over GF(2) modulo the polynomial (bit 31 is x^0 in the
// reflected form).  mulmod: the product; xpow8: x^(8 n) by squaring.  A piece's share of the whole is crcShift(crc of the piece, bytes after it); the shares add
// up by exclusive or.
YBZ_FN uint32_t mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) { if (a & m) p ^= b; b = (b & 1u) ? (b >> 1) ^ POLY : b >> 1; }
    return p;
}
YBZ_FN uint32_t xpow8(uint32_t n)
{
    uint32_t p = 1u << 31, base = 1u << 23;                                      // x^0, x^8
    for (; n; n >>= 1) { if (n & 1u) p = mulmod(base, p); base = mulmod(base, base); }
    return p;
}
YBZ_FN uint32_t crcShift(uint32_t crc, uint32_t bytesAfter) { return mulmod(xpow8(bytesAfter), crc); }

// ---- the fixed Huffman codes: a token's bits in the order they enter the stream (the first bit lowest) ----------------------------------------------------------
struct Bits { uint32_t v, n; };
// Huffman codes go out highest bit first
YBZ_FN uint32_t rev(uint32_t v, uint32_t n) { uint32_t r = 0; for (uint32_t k = 0; k < n; k++) { r = (r << 1) | (v & 1u); v >>= 1; } return r; }
YBZ_FN uint32_t log2u(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }
YBZ_FN Bits literalBits(uint32_t b) { return b < 144u ? Bits{rev(0x30u + b, 8), 8u} : Bits{rev(0x190u + (b - 144u), 9), 9u}; }
YBZ_FN uint32_t literalLen(uint32_t b) { return b < 144u ? 8u : 9u; }
// a match of len (3 .. 258) bytes at distance dist (1 .. 32 768): length symbol, its extra bits, distance symbol, its extra bits -- 31 bits at most
YBZ_FN Bits matchBits(uint32_t len, uint32_t dist)
{
    const uint32_t l = len - 3u; uint32_t sym, e = 0;
    if (len == 258u) sym = 285u; else if (l < 8u) sym = 257u + l; else { e = log2u(l) - 2u; sym = 261u + 4u * e + ((l >> e) & 3u); }
    Bits t = sym < 280u ? Bits{rev(sym - 256u, 7), 7u} : Bits{rev(0xC0u + (sym - 280u), 8), 8u};
    t.v |= (l & ((1u << e) - 1u)) << t.n; t.n += e;
    const uint32_t d = dist - 1u; uint32_t code = d, de = 0;
    if (d >= 4u) { const uint32_t hb = log2u(d); de = hb - 1u; code = 2u * hb + ((d >> de) & 1u); }
    t.v |= rev(code, 5) << t.n; t.n += 5u;
    t.v |= (d & ((1u << de) - 1u)) << t.n; t.n += de;
    return t;
}
enum : uint32_t { BLOCK_HEAD_BITS = 3, BLOCK_HEAD = 3, END_BITS = 7 };            // BFINAL 1, BTYPE 01; the end-of-block symbol: seven zero bits
YBZ_FN uint32_t deflateBytes(uint64_t tokenBits) { return (uint32_t)((BLOCK_HEAD_BITS + tokenBits + END_BITS + 7u) >> 3); }
YBZ_FN bool useStored(uint32_t deflated, uint32_t n) { return deflated >= n + STORED_OVERHEAD; }
YBZ_FN uint32_t hash4(uint32_t fourBytes) { return (fourBytes * 2654435761u) >> (32 - HASH_BITS); }

// ---- framing -----------------------------------------------------------------------------------------------------------------------------------------------------
YBZ_FN void put16(uint8_t *w, uint32_t v) { w[0] = (uint8_t)v; w[1] = (uint8_t)(v >> 8); }
YBZ_FN void put32(uint8_t *w, uint32_t v) { put16(w, v); put16(w + 2, v >> 16); }
YBZ_FN void putHeader(uint8_t *w, uint32_t blockBytes)
{
    w[0] = 0x1F; w[1] = 0x8B; w[2] = 8; w[3] = 4; put32(w + 4, 0); w[8] = 0; w[9] = 0xFF; put16(w + 10, 6); w[12] = 'B'; w[13] = 'C'; put16(w + 14, 2);
        put16(w + 16, blockBytes - 1u);
}
YBZ_FN void putTrailer(uint8_t *w, uint32_t crc, uint32_t isize) { put32(w, crc); put32(w + 4, isize); }
YBZ_FN void putStoredHead(uint8_t *w, uint32_t n) { w[0] = 1; put16(w + 1, n); put16(w + 3, ~n); }      // BFINAL 1, BTYPE 00, LEN, NLEN
YBZ_FN uint32_t blockBytes(uint32_t body) { return HEADER + body + TRAILER; }
YBZ_FN void putEof(uint8_t *w) { putHeader(w, EOF_BYTES); w[HEADER] = BLOCK_HEAD; w[HEADER + 1] = 0; putTrailer(w + HEADER + 2, 0, 0); }

// ---- the host's encoder --------------------------------------------------------------------------------------------------------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
// what a thread keeps for its blocks (on its stack or in its own storage; 17 KB)
struct HostWork { uint16_t head[HASH_SIZE]; uint32_t crcTab[256]; bool ready = false; };
inline uint32_t load32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
// the greedy parse, left to right; head[h]: 1 + the last position whose four bytes hash to h (a payload has fewer than 2^16 positions)
template <class Sink> inline void parse(const uint8_t *src, uint32_t n, uint16_t *head, Sink &sink)
{
    for (uint32_t h = 0; h < HASH_SIZE; h++) head[h] = 0;
    for (uint32_t p = 0; p < n;) {
        uint32_t len = 0, dist = 0;
        if (p + MIN_MATCH <= n) {
            const uint32_t h = hash4(load32(src + p)), cand = head[h]; head[h] = (uint16_t)(p + 1u);
            if (cand && p - (cand - 1u) <= MAX_DIST) {
                const uint32_t c = cand - 1u, most = n - p < MAX_MATCH ? n - p : (uint32_t)MAX_MATCH; uint32_t k = 0;
                while (k < most && src[c + k] == src[p + k]) k++;
                if (k >= MIN_MATCH) { len = k; dist = p - c; }
            }
        }
        if (len) {
            sink.put(matchBits(len, dist));
            for (uint32_t q = p + 1u; q < p + len && q + MIN_MATCH <= n; q++) head[hash4(load32(src + q))] = (uint16_t)(q + 1u);
            p += len;
        } else { sink.put(literalBits(src[p])); p++; }
    }
}
struct CountSink { uint64_t bits = 0; void put(Bits t) { bits += t.n; } };
struct WriteSink {
    uint8_t *w; uint64_t acc = 0; uint32_t have = 0;
    void put(Bits t) { acc |= (uint64_t)t.v << have; have += t.n; while (have >= 8u) { *w++ = (uint8_t)acc; acc >>= 8; have -= 8u; } }
    void finish() { if (have) { *w++ = (uint8_t)acc; acc = 0; have = 0; } }
};
// one payload (n <= PAYLOAD_MAX) -> one block at dst (room for BLOCK_MAX bytes); returns its size; *stored: whether it took the stored form
inline uint32_t encodeBlock(const uint8_t *src, uint32_t n, uint8_t *dst, HostWork &W, bool *stored)
{
    if (!W.ready) { for (uint32_t i = 0; i < 256; i++) W.crcTab[i] = crcEntry(i); W.ready = true; }
    CountSink count; parse(src, n, W.head, count);
    const uint32_t deflated = deflateBytes(count.bits); const bool st = useStored(deflated, n);
    const uint32_t body = st ? n + STORED_OVERHEAD : deflated;
    putHeader(dst, blockBytes(body));
    if (st) { putStoredHead(dst + HEADER, n); for (uint32_t i = 0; i < n; i++) dst[HEADER + STORED_OVERHEAD + i] = src[i]; }
    else { WriteSink out{dst + HEADER}; out.put(Bits{BLOCK_HEAD, BLOCK_HEAD_BITS}); parse(src, n, W.head, out); out.put(Bits{0, END_BITS}); out.finish(); }
    putTrailer(dst + HEADER + body, crc32(W.crcTab, src, n), n);
    if (stored) *stored = st;
    return blockBytes(body);
}
// a whole stream: its payloads' blocks one after the other at out (room for bound(nIn) bytes); returns their bytes; no end-of-file block
inline uint64_t encodeStream(const uint8_t *in, uint64_t nIn, uint8_t *out, HostWork &W, uint64_t *nBlocks, uint64_t *nStored)
{
    uint64_t at = 0;
    for (uint64_t o = 0; o < nIn; o += PAYLOAD_MAX) {
        bool st = false; at += encodeBlock(in + o, (uint32_t)(nIn - o < PAYLOAD_MAX ? nIn - o : PAYLOAD_MAX), out + at, W, &st);
        if (nBlocks) ++*nBlocks;
        if (nStored && st) ++*nStored;
    }
    return at;
}
#endif
}  // namespace ybgzf
