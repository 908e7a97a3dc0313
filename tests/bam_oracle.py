"""What -obh / -obs must write, from the specifications alone (stdlib zlib / struct): a strict reader of BGZF files, a BAM -> SAM text converter that gives
back the line the SAM writer (host/sam.cpp printClump) would have written, and the one normalisation BAM forces on a SAM line's SEQ."""
import struct
import zlib

PAYLOAD_MAX = 65280
BLOCK_MAX = 65536
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SEQ_LETTERS = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"


def blocks(data):
    """Every block of `data` (a sequence of whole BGZF blocks, no more and no less) as (payload, block bytes, stored?), each checked to the letter."""
    out, at = [], 0
    while at < len(data):
        assert len(data) - at >= 26, "a block has at least 26 bytes"
        magic, cm, flg, mtime, xfl, os_, xlen = struct.unpack_from("<HBBIBBH", data, at)
        assert (magic, cm, flg) == (0x8B1F, 8, 4), "magic and flags at %d" % at
        assert xlen == 6 and data[at + 12:at + 16] == b"BC\x02\x00", "one extra subfield BC of two bytes at %d" % at
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        assert size <= BLOCK_MAX and at + size <= len(data), "BSIZE at %d" % at
        body = data[at + 18:at + size - 8]
        d = zlib.decompressobj(-15)
        payload = d.decompress(body)
        assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b"", "the deflate data must be exactly one finished stream at %d" % at
        crc, isize = struct.unpack_from("<II", data, at + size - 8)
        assert isize == len(payload) <= PAYLOAD_MAX, "ISIZE at %d" % at
        assert crc == zlib.crc32(payload), "CRC at %d" % at
        stored = (body[0] >> 1) & 3 == 0
        assert body[0] & 1 == 1, "one FINAL deflate block at %d" % at
        if stored:
            assert len(body) == 5 + len(payload)
        out.append((payload, size, stored))
        at += size
    return out


def read_stream(data):
    """The decompressed bytes of blocks without an end-of-file marker (what ygpu_bgzf_compress returns): no block is empty."""
    bl = blocks(data)
    assert all(len(p) > 0 for p, _s, _st in bl), "an empty block inside the stream"
    return b"".join(p for p, _s, _st in bl), bl


def read_file(data):
    """The decompressed bytes of a whole BGZF file: it ends with exactly the 28-byte end-of-file block, and no other block is empty."""
    assert data[-28:] == EOF, "the file must end with the end-of-file block"
    return read_stream(data[:-28])


def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def _tag_text(raw, at):
    tag = raw[at:at + 2].decode(); typ = chr(raw[at + 2]); at += 3
    if typ in "cCsSiI":
        fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[typ]
        v = struct.unpack_from(fmt, raw, at)[0]
        return "%s:i:%d" % (tag, v), at + struct.calcsize(fmt), typ
    assert typ in "ZH", typ
    end = raw.index(b"\0", at)
    return "%s:%s:%s" % (tag, typ, raw[at:end].decode()), end + 1, typ


def bam_to_sam(raw):
    """(SAM text: the header text, then one line per record; the reference list [(name, length)]; the records' integer tag types, for the width rule)."""
    assert raw[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", raw, 4)[0]
    text = raw[8:8 + l_text].decode(); at = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, at)[0]; at += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", raw, at)[0]; at += 4
        name = raw[at:at + l_name]; at += l_name
        assert name.endswith(b"\0") and b"\0" not in name[:-1]
        refs.append((name[:-1].decode(), struct.unpack_from("<i", raw, at)[0])); at += 4
    lines, int_types = [], []
    while at < len(raw):
        size = struct.unpack_from("<i", raw, at)[0]; at += 4
        rec = raw[at:at + size]; at += size
        assert len(rec) == size, "a record is cut off"
        ref_id, pos, l_name, mapq, bin_, n_cig, flag, l_seq, next_ref, next_pos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 0)
        assert (next_ref, next_pos, tlen) == (-1, -1, 0) and 0 <= ref_id < n_ref
        p = 32
        name = rec[p:p + l_name]; p += l_name
        assert name.endswith(b"\0")
        cig = struct.unpack_from("<%dI" % n_cig, rec, p); p += 4 * n_cig
        ref_span = sum(c >> 4 for c in cig if CIGAR_OPS[c & 15] in "MDN=X")
        assert bin_ == reg2bin(pos, pos + max(1, ref_span)), "bin"
        assert sum(c >> 4 for c in cig if CIGAR_OPS[c & 15] in "MIS=X") == l_seq, "the CIGAR's query length is the sequence's"
        packed = rec[p:p + (l_seq + 1) // 2]; p += (l_seq + 1) // 2
        seq = "".join(SEQ_LETTERS[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
        if l_seq & 1:
            assert packed[-1] & 15 == 0
        q = rec[p:p + l_seq]; p += l_seq
        qual = "*" if l_seq and all(b == 0xFF for b in q) else "".join(chr(b + 33) for b in q)
        tags, kinds = [], {}
        while p < len(rec):
            t, p, typ = _tag_text(rec, p)
            tags.append(t)
            if typ in "cCsSiI":
                kinds[t[:2]] = (typ, int(t[5:]))
        assert p == len(rec)
        int_types.append(kinds)
        lines.append("\t".join([name[:-1].decode(), str(flag), refs[ref_id][0], str(pos + 1), str(mapq), "".join("%d%s" % (c >> 4, CIGAR_OPS[c & 15]) for c in cig), "*", "0", "0",
                                seq, qual] + tags))
    return text + "".join(l + "\n" for l in lines), refs, int_types


def records_of(raw):
    """The bytes of a BAM stream behind its header (the header's @PG line names the output file, the records do not)."""
    assert raw[:4] == b"BAM\1"
    at = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, at)[0]; at += 4
    for _ in range(n_ref):
        at += 4 + struct.unpack_from("<i", raw, at)[0] + 4
    return raw[at:]


def smallest_unsigned(v):
    return "C" if v < 256 else "S" if v < 65536 else "I"


def normalise_sam_seq(line):
    """A SAM record line with its SEQ as BAM can carry it: upper case, and every letter outside =ACMGRSVTWYHKDBN an N.  Header lines are returned as they are."""
    if line.startswith("@") or not line:
        return line
    f = line.split("\t")
    f[9] = "".join(c if c in SEQ_LETTERS else "N" for c in f[9].upper())
    return "\t".join(f)
