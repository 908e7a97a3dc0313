"""What -obsort must write beside its BAM, from the SAM specification (section 5, "Indexing BAM") and the contract of the option alone: a strict parser of
BAI files, the index a sorted BAM file must have (rebuilt from the file's records and its blocks' headers), the reader's region query through the index, and
the scan it must agree with.  Nothing here comes from csrc/bai_core.h."""
import struct

import bam_oracle as bo

PSEUDO_BIN = 37450
LEVEL_FIRST = (0, 1, 9, 73, 585, 4681)                                               # the first bin of every level; level 5 has the 16 384-base bins


def bin_level(b):
    return max(l for l, first in enumerate(LEVEL_FIRST) if b >= first)


def parse_bai(data):
    """[(bins, ioffset)] per sequence -- bins: [(bin, [(beg, end), ...])] as in the file -- and n_no_coor.  Checks the magic, the counts, that the bins of a
    sequence ascend strictly and that nothing trails the file."""
    assert data[:4] == b"BAI\1", "magic"
    n_ref = struct.unpack_from("<i", data, 4)[0]; at = 8
    assert n_ref >= 0
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", data, at)[0]; at += 4
        assert n_bin >= 0
        bins = []
        for _b in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, at); at += 8
            assert n_chunk > 0 and b <= PSEUDO_BIN and (not bins or b > bins[-1][0]), "bin %d after %s" % (b, bins[-1][0] if bins else None)
            chunks = [struct.unpack_from("<QQ", data, at + 16 * c) for c in range(n_chunk)]; at += 16 * n_chunk
            bins.append((b, chunks))
        n_intv = struct.unpack_from("<i", data, at)[0]; at += 4
        assert n_intv >= 0
        ioffset = list(struct.unpack_from("<%dQ" % n_intv, data, at)); at += 8 * n_intv
        refs.append((bins, ioffset))
    n_no_coor = struct.unpack_from("<Q", data, at)[0]; at += 8
    assert at == len(data), "%d bytes trail the index" % (len(data) - at)
    return refs, n_no_coor


class Bam:
    """A whole BAM file: its blocks (file offset, first uncompressed byte), its records (sequence, pos, end, bin, first and last + 1 uncompressed byte)."""

    def __init__(self, data):
        self.data = data
        raw, bl = bo.read_file(data)                                                  # (strict: framing, CRC, ISIZE, the end-of-file block)
        self.raw = raw
        self.block_at, self.block_start = [], []
        at = start = 0
        for payload, size, _stored in bl:
            self.block_at.append(at); self.block_start.append(start); at += size; start += len(payload)
        self.block_at.append(at); self.block_start.append(start)                      # the end-of-file block: where the stream's end points
        assert at + 28 == len(data) and start == len(raw)
        rec0 = len(raw) - len(bo.records_of(raw))
        self.n_ref = struct.unpack_from("<i", raw, 8 + struct.unpack_from("<i", raw, 4)[0])[0]
        self.records = []
        p = rec0
        while p < len(raw):
            size = struct.unpack_from("<i", raw, p)[0]
            ref, pos, l_name, _mapq, bin_, n_cig = struct.unpack_from("<iiBBHH", raw, p + 4)
            cig = struct.unpack_from("<%dI" % n_cig, raw, p + 36 + l_name)
            span = sum(c >> 4 for c in cig if bo.CIGAR_OPS[c & 15] in "MDN=X")
            self.records.append((ref, pos, pos + max(1, span), bin_, p, p + 4 + size))
            p += 4 + size
        assert p == len(raw)
        self.by_start = {r[4]: i for i, r in enumerate(self.records)}

    def voffset(self, u):
        """The virtual offset of uncompressed byte u: the last block that starts at or before it (a block boundary: the start of the next block; the stream's
        end: the end-of-file block)."""
        k = max(i for i, s in enumerate(self.block_start) if s <= u) if u < self.block_start[-1] else len(self.block_start) - 1
        within = u - self.block_start[k]
        assert 0 <= within < 65536
        return self.block_at[k] << 16 | within

    def upos(self, v):
        """The uncompressed byte a virtual offset names (it must name a block of the file)."""
        k = self.block_at.index(v >> 16)
        return self.block_start[k] + (v & 0xFFFF)


def expected_index(bam):
    """The index the contract gives for the file: per sequence ({bin: [(beg, end)]}, ioffset)."""
    out = []
    for ref in range(bam.n_ref):
        recs = [(i, r) for i, r in enumerate(bam.records) if r[0] == ref]
        if not recs:
            out.append(({}, [])); continue
        bins = {}
        run = [recs[0]]
        for prev, cur in zip(recs, recs[1:] + [None]):
            if cur is not None and cur[0] == prev[0] + 1 and cur[1][3] == prev[1][3]:
                run.append(cur); continue
            bins.setdefault(run[0][1][3], []).append((bam.voffset(run[0][1][4]), bam.voffset(run[-1][1][5])))
            run = [cur]
        assert PSEUDO_BIN not in bins
        bins[PSEUDO_BIN] = [(bam.voffset(recs[0][1][4]), bam.voffset(recs[-1][1][5])), (len(recs), 0)]
        n_intv = ((max(r[2] for _i, r in recs) - 1) >> 14) + 1
        io = [None] * n_intv
        for _i, r in recs:
            v = bam.voffset(r[4])
            for w in range(r[1] >> 14, ((r[2] - 1) >> 14) + 1):
                io[w] = v if io[w] is None else min(io[w], v)
        for w in range(n_intv):
            if io[w] is None:
                io[w] = io[w - 1] if w else 0
        out.append((bins, io))
    return out


def check_contract(bam_bytes, bai_bytes):
    bam = Bam(bam_bytes)
    refs, n_no_coor = parse_bai(bai_bytes)
    assert n_no_coor == 0 and len(refs) == bam.n_ref
    keys = [(r[0], r[1]) for r in bam.records]
    assert keys == sorted(keys), "the records are not in coordinate order"
    want = expected_index(bam)
    for ref, ((bins, ioffset), (wbins, wio)) in enumerate(zip(refs, want)):
        assert dict(bins) == wbins, "bins of sequence %d" % ref
        assert ioffset == wio, "linear index of sequence %d" % ref
    return bam, refs


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


def query(bam, refs, seq, beg, end):
    """The records of sequence seq that overlap [beg, end), found the way a reader finds them: the chunks of the region's bins, none that ends at or before the
    linear index's offset for beg's window, a seek to each, records until one starts at or after end."""
    bins, ioffset = refs[seq]
    if not bins:
        return []
    table = dict(bins)
    w = beg >> 14
    min_off = ioffset[w] if w < len(ioffset) else (ioffset[-1] if ioffset else 0)
    chunks = sorted(c for b in reg2bins(beg, end) if b in table and b != PSEUDO_BIN for c in table[b] if c[1] > min_off)
    out = []
    for cbeg, cend in chunks:
        u = bam.upos(cbeg); stop = bam.upos(cend)
        while u < stop:
            i = bam.by_start[u]                                                       # (a seek that does not land on a record is a KeyError)
            ref, pos, rend, _bin, _s, e = bam.records[i]
            assert ref == seq
            if pos >= end:
                return out
            if rend > beg:
                out.append(i)
            u = e
    return out


def brute(bam, seq, beg, end):
    return [i for i, r in enumerate(bam.records) if r[0] == seq and r[1] < end and r[2] > beg]
