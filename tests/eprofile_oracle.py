"""The error profile (-oep) recomputed from SAM text and the reference FASTA alone, by the rules of the issue.  Inputs are SEQ, CIGAR with its H / S clips, POS,
FLAG 16, MAPQ and the @SQ table.  A PAIR is a reference base under an M with the SEQ letter that lies over it, both as channels A C G T N (anything else: N);
a pair is a match when the two are equal and not N.  The table has 1556 words:
  SUB    25, [ref][read]   1 per pair
  INS    65                1 per I of n bases at min(n, 65) - 1
  DEL    65                the same per D
  IDENT  1001              1 per record at floor(1000 * matches / (pairs + inserted + deleted bases))
  POS    100 x 4           by the place in the read AS SEQUENCED -- the offset in SEQ plus the leading clip, counted from the other end when FLAG has 16 --,
                           bin = offset * 100 // read length: pairs, pairs that are no match, I ops (where they start), D ops (at the next read base)
The read length is the sum of the H, S, M and I lengths.  text() is the file, given once here.  Shares nothing with the product: the tests compare the command
line's file and the device's table with this."""
import re

import numpy as np

_CIG = re.compile(r"(\d+)([MIDNSHP=X])")
SUB, INS, DEL, IDENT, POS, WORDS = 0, 25, 90, 155, 1156, 1556
CHANNELS = "ACGTN"
_LUT = np.full(256, 4, dtype=np.int64)
for _i, _c in enumerate("ACGT"):
    _LUT[ord(_c)] = _i
    _LUT[ord(_c.lower())] = _i
_LUT[ord("U")] = _LUT[ord("u")] = 3                                       # (the .nib2 reads U as T)


def sq_table(lines):
    """[(name, length)] from the @SQ lines, in header order."""
    out = []
    for l in lines:
        if l.startswith("@SQ"):
            f = dict(x.split(":", 1) for x in l.split("\t")[1:])
            out.append((f["SN"], int(f["LN"])))
    return out


def read_fasta(path):
    """{name: channels of the sequence as a numpy array}; the name is the header line up to the first blank."""
    seqs, name, parts = {}, None, []

    def done():
        if name is not None:
            seqs[name] = _LUT[np.frombuffer("".join(parts).encode(), dtype=np.uint8)]
    for l in open(path):
        l = l.rstrip("\n")
        if l.startswith(">"):
            done()
            name, parts = l[1:].split()[0], []
        else:
            parts.append(l.strip())
    done()
    return seqs


def _records(lines):
    for l in lines:
        if l and not l.startswith("@"):
            yield l.split("\t")


def records(lines, Q=0):
    """(records counted, records skipped by MAPQ)"""
    mq = [int(f[4]) for f in _records(lines)]
    return sum(1 for m in mq if m >= Q), sum(1 for m in mq if m < Q)


def strands(lines):
    """(forward records, reversed records)"""
    fl = [int(f[1]) & 16 for f in _records(lines)]
    return sum(1 for x in fl if not x), sum(1 for x in fl if x)


def table(lines, ref, Q=0):
    """The 1556 words (numpy uint64) of the records with MAPQ >= Q; ref: read_fasta's result."""
    t = np.zeros(WORDS, dtype=np.uint64)
    sub = np.zeros((5, 5), dtype=np.int64); pos = np.zeros((100, 4), dtype=np.int64)
    for f in _records(lines):
        if int(f[4]) < Q:
            continue
        rev = (int(f[1]) & 16) != 0; chrom = ref[f[2]]; at = int(f[3]) - 1; seq = _LUT[np.frombuffer(f[9].encode(), dtype=np.uint8)]
        cig = [(int(n), op) for n, op in _CIG.findall(f[5])]
        assert "".join("%d%s" % c for c in cig) == f[5] and cig
        qlen = sum(n for n, op in cig if op in "HSMI")
        lead = cig[0][0] if cig[0][1] in "HS" else 0
        trail = cig[-1][0] if len(cig) > 1 and cig[-1][1] in "HS" else 0
        q, qe = lead, qlen - trail                                         # offsets in the read as SEQ shows it (the strand of the reference)
        si = lead if cig[0][1] == "S" else 0                               # ... and in SEQ itself: H is not in it
        fwd = (lambda x: qlen - 1 - x) if rev else (lambda x: x)
        m = cols = 0
        for k, (n, op) in enumerate(cig):
            if op == "M":
                c = max(0, min(n, qe - q))
                r = chrom[at:at + c]; b = seq[si:si + c]
                assert len(r) == c and len(b) == c
                np.add.at(sub, (r, b), 1)
                bins = fwd(np.arange(q, q + c, dtype=np.int64)) * 100 // qlen
                ok = (r == b) & (r != 4)
                np.add.at(pos, (bins, 0), 1); np.add.at(pos, (bins[~ok], 1), 1)
                m += int(ok.sum()); cols += c
                at += n; q += n; si += n
            elif op == "I":
                t[INS + min(n, 65) - 1] += 1
                if q < qe:
                    cols += n; pos[fwd(q) * 100 // qlen, 2] += 1
                q += n; si += n
            elif op == "D":
                t[DEL + min(n, 65) - 1] += 1
                if q < qe:
                    cols += n; pos[fwd(min(q, qe - 1)) * 100 // qlen, 3] += 1
                at += n
            else:
                assert op in "HS" and k in (0, len(cig) - 1), op
        if cols:
            t[IDENT + 1000 * m // cols] += 1
    t[SUB:SUB + 25] = sub.reshape(-1); t[POS:POS + 400] = pos.reshape(-1)
    return t


def text(t, counted, skipped, dropped=0):
    """The file.  dropped: records that span two sequences are not printed, so SAM text does not show them -- the caller says how many it expects."""
    t = [int(x) for x in t]
    out = ["#yaha error profile\trecords\t%d\tskipped_mapq\t%d\tdropped\t%d\n" % (counted, skipped, dropped), "SUB\tref\t" + "\t".join(CHANNELS) + "\n"]
    for r in range(5):
        out.append("SUB\t%s\t%s\n" % (CHANNELS[r], "\t".join(str(x) for x in t[SUB + 5 * r:SUB + 5 * r + 5])))
    for name, base in (("INS", INS), ("DEL", DEL)):
        for n in range(1, 66):
            out.append("%s\t%d%s\t%d\n" % (name, n, "+" if n == 65 else "", t[base + n - 1]))
    for i in range(1001):
        if t[IDENT + i]:
            out.append("IDENT\t%d\t%d\n" % (i, t[IDENT + i]))
    for b in range(100):
        out.append("POS\t%d\t%s\n" % (b, "\t".join(str(x) for x in t[POS + 4 * b:POS + 4 * b + 4])))
    return "".join(out)
