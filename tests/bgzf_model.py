"""The BGZF blocks both encoders must write, bit for bit, from the written contract alone (DESIGN.md's BAM paragraph, the header comments of csrc/bgzf_core.h and
csrc/device/bgzf_stage.h) and RFC 1951 / RFC 1952: stdlib and numpy, no line of the encoders.  The code tables are the RFC's (3.2.5, 3.2.6), the two parses
are the contract's:

  host    one remembered position per 13-bit hash of four bytes; EVERY position is inserted, those inside a match too; at the cursor only that candidate is
          tried (no other distance), a match has 4 .. 258 bytes at a distance of at most 32 768 and never runs past the payload; greedy, left to right.
  device  tiles of 256 positions; while the cursor is in tile t the table maps a hash to the HIGHEST position p of the tiles before t with p + 4 <= n.  At the
          cursor the candidate is tried if it is within 32 768; if that gives fewer than 4 bytes the position before the cursor (distance 1) is; if that
          gives fewer than 4 the byte is a literal.  Greedy, left to right; a match may cross tiles.

A token is an int (a literal byte) or a tuple (length, distance).  block() frames one payload, stream() a whole input; stats() is what the coverage conditions
of tests/test_bam_cpu.py are stated in."""
import struct
import zlib
from bisect import bisect_right

import numpy as np

PAYLOAD_MAX = 65280
TILE = 256
MIN_MATCH, MAX_MATCH, MAX_DIST = 4, 258, 32768
HASH_BITS = 13

# ---- RFC 1951, 3.2.5: length and distance symbols ---------------------------------------------------------------------------------------------------------------
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]          # symbols 257 .. 285
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
# ---- RFC 1951, 3.2.6: the fixed code's lengths; 3.2.2: the codes that follow from lengths ----------------------------------------------------------------------
FIXED_LENGTHS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8                            # literal / length symbols 0 .. 287
END_OF_BLOCK = 256


def _canonical(lengths):
    """RFC 1951, 3.2.2: the code of every symbol from the code lengths."""
    count = [0] * (max(lengths) + 1)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * (max(lengths) + 2), 0
    for bits in range(1, max(lengths) + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for l in lengths:
        out.append(nxt[l]); nxt[l] += 1
    return out


def _msb_first(code, n):
    """A Huffman code enters the stream highest bit first; everything else lowest bit first.  The value whose LOWEST bit enters first."""
    return int(format(code, "0%db" % n)[::-1], 2)


_FIXED = _canonical(FIXED_LENGTHS)
_SYMBOL = [(_msb_first(c, l), l) for c, l in zip(_FIXED, FIXED_LENGTHS)]             # symbol -> (bits, count), the first bit lowest
_DIST_SYMBOL = [(_msb_first(c, 5), 5) for c in range(30)]                             # distance codes: five bits each


def literal_code(b):
    return _SYMBOL[b]


def length_symbol(length):
    return bisect_right(LEN_BASE, length) - 1                                         # (258 is symbol 285, not 284 with 31 extra)


def dist_code(dist):
    return bisect_right(DIST_BASE, dist) - 1


def match_code(length, dist):
    """(bits, count) of a match: the length symbol, its extra bits, the distance code, its extra bits."""
    i = length_symbol(length); v, n = _SYMBOL[257 + i]
    v |= (length - LEN_BASE[i]) << n; n += LEN_EXTRA[i]
    c = dist_code(dist); dv, dn = _DIST_SYMBOL[c]
    v |= dv << n; n += dn
    v |= (dist - DIST_BASE[c]) << n; n += DIST_EXTRA[c]
    return v, n


def token_code(t):
    return _SYMBOL[t] if isinstance(t, int) else match_code(*t)


# ---- the parses -------------------------------------------------------------------------------------------------------------------------------------------------
def hashes(payload):
    """The 13-bit hash of the four bytes at every position p with p + 4 <= n (a list): the little-endian word times 2654435761, its top 13 bits."""
    n = len(payload)
    if n < 4:
        return []
    b = np.frombuffer(payload, dtype=np.uint8).astype(np.uint32)
    w = b[:n - 3] | b[1:n - 2] << 8 | b[2:n - 1] << 16 | b[3:] << 24
    return ((w * np.uint32(2654435761)) >> np.uint32(32 - HASH_BITS)).tolist()


def _agree(payload, p, c, most):
    """How many of the bytes at p and at c < p agree, `most` at the most."""
    x = int.from_bytes(payload[p:p + most], "little") ^ int.from_bytes(payload[c:c + most], "little")
    return most if x == 0 else ((x & -x).bit_length() - 1) >> 3


def host_tokens(payload, info=None):
    """The host's parse.  info (a dict, optional) gains "rejected": candidates passed over because they lie more than 32 768 back."""
    payload = bytes(payload); n = len(payload); h = hashes(payload)
    head = [-1] * (1 << HASH_BITS)
    out, p, rejected = [], 0, 0
    while p < n:
        length = 0
        if p + MIN_MATCH <= n:
            c = head[h[p]]; head[h[p]] = p
            if c >= 0:
                if p - c <= MAX_DIST:
                    k = _agree(payload, p, c, min(n - p, MAX_MATCH))
                    if k >= MIN_MATCH:
                        length = k
                else:
                    rejected += 1
        if length:
            out.append((length, p - c))
            for q in range(p + 1, min(p + length, n - 3)):
                head[h[q]] = q
            p += length
        else:
            out.append(payload[p]); p += 1
    if info is not None:
        info["rejected"] = info.get("rejected", 0) + rejected
    return out


def device_tokens(payload, info=None):
    """The device's parse (info as in host_tokens)."""
    payload = bytes(payload); n = len(payload); h = hashes(payload)
    table = [-1] * (1 << HASH_BITS); filled = 0                                        # the table holds the positions below `filled`, a multiple of the tile
    out, p, rejected = [], 0, 0
    while p < n:
        start = p - p % TILE
        if filled < start:
            for q, hv in enumerate(h[filled:start], filled):                           # ascending: the highest position stays
                table[hv] = q
            filled = start
        length = dist = 0
        if p + MIN_MATCH <= n:
            most = min(n - p, MAX_MATCH)
            c = table[h[p]]
            if c >= 0:
                if p - c <= MAX_DIST:
                    length, dist = _agree(payload, p, c, most), p - c
                else:
                    rejected += 1
            if length < MIN_MATCH and p >= 1:
                length, dist = _agree(payload, p, p - 1, most), 1
        if length >= MIN_MATCH:
            out.append((length, dist)); p += length
        else:
            out.append(payload[p]); p += 1
    if info is not None:
        info["rejected"] = info.get("rejected", 0) + rejected
    return out


# ---- framing (RFC 1952 with the BGZF subfield; RFC 1951 3.2.3, 3.2.4) ----------------------------------------------------------------------------------------------
def _pack(codes):
    """(bits, count) pairs, the first bit of each lowest, laid end to end from bit 0 of byte 0; the last byte padded with zeros."""
    out, acc, have = bytearray(), 0, 0
    for v, n in codes:
        acc |= v << have; have += n
        if have >= 64:
            out += (acc & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little"); acc >>= 64; have -= 64
    out += acc.to_bytes((have + 7) // 8, "little")
    return bytes(out)


def block(payload, tokens):
    """The BGZF block of one payload (at most 65 280 bytes) whose parse is `tokens`."""
    payload = bytes(payload); n = len(payload)
    assert n <= PAYLOAD_MAX
    codes = [(1 | 1 << 1, 3)] + [token_code(t) for t in tokens] + [_SYMBOL[END_OF_BLOCK]]      # BFINAL 1, BTYPE 01 (its two bits lowest first)
    deflated = (sum(c[1] for c in codes) + 7) // 8
    if deflated >= n + 5:                                                              # stored: BFINAL 1, BTYPE 00, to the byte boundary, LEN, NLEN, the bytes
        body = b"\x01" + struct.pack("<HH", n, n ^ 0xFFFF) + payload
    else:
        body = _pack(codes)
    size = 18 + len(body) + 8
    head = struct.pack("<BBBBIBBH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6) + b"BC" + struct.pack("<HH", 2, size - 1)
    return head + body + struct.pack("<II", zlib.crc32(payload), n)


def payloads(data):
    return [data[o:o + PAYLOAD_MAX] for o in range(0, len(data), PAYLOAD_MAX)]


def stream(data, tokens_fn, cache=None):
    """The blocks of a whole input, one after the other, no end-of-file block.  cache: a dict payload -> block of the same tokens_fn, filled here."""
    out = []
    for pl in payloads(bytes(data)):
        b = cache.get(pl) if cache is not None else None
        if b is None:
            b = block(pl, tokens_fn(pl))
            if cache is not None:
                cache[pl] = b
        out.append(b)
    return b"".join(out)


def split_blocks(data):
    """The blocks of a BGZF byte string as they stand (cut by BSIZE, nothing checked: tests/bam_oracle.py blocks() is the reader)."""
    out, at = [], 0
    while at < len(data):
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        out.append(data[at:at + size]); at += size
    return out


# ---- what a parse used --------------------------------------------------------------------------------------------------------------------------------------------
def stats(payload, tokens):
    """lengths, dists, dist_codes: the sets over the matches; nine_bit: literals of nine bits; tile_bits: per tile of 256 positions, the bits of the tokens
    that START in it (block head and end-of-block symbol not counted); starts: position -> token, for the matches."""
    n = len(payload)
    st = {"lengths": set(), "dists": set(), "dist_codes": set(), "nine_bit": 0, "tile_bits": [0] * (-(-n // TILE)), "starts": {}}
    p = 0
    for t in tokens:
        st["tile_bits"][p // TILE] += token_code(t)[1]
        if isinstance(t, int):
            st["nine_bit"] += t >= 144; p += 1
        else:
            st["lengths"].add(t[0]); st["dists"].add(t[1]); st["dist_codes"].add(dist_code(t[1])); st["starts"][p] = t; p += t[0]
    assert p == n
    return st
