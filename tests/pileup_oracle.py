"""The allele pileup (-opu) recomputed from SAM text and the reference FASTA alone, by the rules of the issue.  Inputs are SEQ, CIGAR, POS, MAPQ and the @SQ
table: every reference base under an M takes the SEQ letter that lies over it (A C G T, anything else N), every base under a D counts as deleted, every I
counts once at the next reference base (kept inside the record), S and H clips are skipped -- S consumes SEQ, H does not.  A CIGAR that asks for more SEQ than
there is before the trailing clip counts what is there.  Shares nothing with the product: the tests compare the command line's file and the device's array,
candidates and gathered rows with this."""
import re

import numpy as np

_CIG = re.compile(r"(\d+)([MIDNSHP=X])")
CHANNELS = ("A", "C", "G", "T", "N", "del", "ins")
HEADER = "#chrom\tstart\tend\tref\t" + "\t".join(CHANNELS) + "\n"
_LUT = np.full(256, 4, dtype=np.int64)
for _i, _c in enumerate("ACGT"):
    _LUT[ord(_c)] = _i
    _LUT[ord(_c.lower())] = _i


def sq_table(lines):
    """[(name, length)] from the @SQ lines, in header order (= index order)."""
    out = []
    for l in lines:
        if l.startswith("@SQ"):
            f = dict(x.split(":", 1) for x in l.split("\t")[1:])
            out.append((f["SN"], int(f["LN"])))
    return out


def read_fasta(path):
    """{name: sequence} of a FASTA file; the name is the header line up to the first blank."""
    seqs, name, parts = {}, None, []
    for l in open(path):
        l = l.rstrip("\n")
        if l.startswith(">"):
            if name is not None:
                seqs[name] = "".join(parts)
            name, parts = l[1:].split()[0], []
        else:
            parts.append(l.strip())
    if name is not None:
        seqs[name] = "".join(parts)
    return seqs


def n_slots(sq):
    return sum(ln for _, ln in sq)


def _records(lines, Q):
    for l in lines:
        if l and not l.startswith("@"):
            f = l.split("\t")
            if int(f[4]) >= Q:
                yield f


def records(lines, Q=0):
    return sum(1 for _ in _records(lines, Q))


def pileup(lines, sq, Q=0):
    """pu[slot] = [A, C, G, T, N, del, ins] over all reference bases, sequence by sequence (numpy uint32, shape (n_slots, 7)), from the records with MAPQ >= Q."""
    base, length, tot = {}, {}, 0
    for name, ln in sq:
        base[name] = tot; length[name] = ln; tot += ln
    pu = np.zeros((tot, 7), dtype=np.uint32)
    for f in _records(lines, Q):
        name, start, seq = f[2], int(f[3]) - 1, np.frombuffer(f[9].encode(), dtype=np.uint8)
        cig = [(int(n), op) for n, op in _CIG.findall(f[5])]
        assert "".join("%d%s" % c for c in cig) == f[5] and cig
        last = start + sum(n for n, op in cig if op in "MD") - 1
        assert 0 <= start and last < length[name]
        b0 = base[name]
        limit = len(seq) - (cig[-1][0] if len(cig) > 1 and cig[-1][1] == "S" else 0)      # SEQ before the trailing soft clip
        pos, q = start, 0
        for k, (n, op) in enumerate(cig):
            if op == "M":
                m = max(0, min(n, limit - q))
                if m:
                    np.add.at(pu, (np.arange(b0 + pos, b0 + pos + m), _LUT[seq[q:q + m]]), 1)
                pos += n; q += n
            elif op == "D":
                pu[b0 + pos:b0 + pos + n, 5] += 1
                pos += n
            elif op == "I":
                pu[b0 + min(pos, last), 6] += 1
                q += n
            elif op == "S":
                assert k in (0, len(cig) - 1)
                q += n
            else:
                assert op == "H" and k in (0, len(cig) - 1), op
    return pu


def ref_letters(sq, fasta):
    """The reference letter of every slot as the .nib2 decodes it (upper case; U reads as T, a letter outside the IUPAC set as X), a numpy array of bytes."""
    out = []
    for name, ln in sq:
        s = fasta[name].upper().replace("U", "T")
        assert len(s) == ln, (name, len(s), ln)
        out.append(np.frombuffer(s.encode(), dtype=np.uint8))
    a = np.concatenate(out).copy()
    a[~np.isin(a, np.frombuffer(b"TCAGNBDHKMRSVWXY", dtype=np.uint8))] = ord("X")
    return a


def nonref(pu, ref):
    """Reads that disagree with the reference, per slot (int64)."""
    p = pu.astype(np.int64)
    return p[:, :6].sum(axis=1) - p[np.arange(len(p)), _LUT[ref]] + p[:, 6]


def candidates(pu, ref):
    """The slots with at least one disagreeing read, ascending (numpy uint32)."""
    return np.nonzero(nonref(pu, ref) >= 1)[0].astype(np.uint32)


def sites(pu, ref, min_alt):
    return np.nonzero(nonref(pu, ref) >= min_alt)[0]


def text(pu, sq, ref, min_alt):
    out, want = [HEADER], sites(pu, ref, min_alt)
    b0, k = 0, 0
    for name, ln in sq:
        while k < len(want) and want[k] < b0 + ln:
            s = int(want[k]); k += 1
            out.append("%s\t%d\t%d\t%s\t%s\n" % (name, s - b0, s - b0 + 1, chr(ref[s]), "\t".join(str(int(x)) for x in pu[s])))
        b0 += ln
    return "".join(out)
