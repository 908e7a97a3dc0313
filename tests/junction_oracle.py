"""Split-read breakpoint calls (-obp) recomputed from SAM text alone, by the rules of the contract (yaha_amd/csrc/junction_core.h says the same in C++; this file
shares nothing with it).  The @SQ order gives the sequence numbers, YF:H bit 0x20 marks a primary record, FLAG 0x10 the strand, the CIGAR's clips and M / I
lengths give qlen, sqo and eqo on the printed strand, its M / D lengths the reference length.  Records of a read are the consecutive lines with its name."""
import re

_CIG = re.compile(r"(\d+)([MIDNSHP=X])")
TYPES = ("DEL", "DUP", "INV", "TRA")


def sq_table(lines):
    """[(name, length)] from the @SQ lines, in header order (= index order)."""
    out = []
    for l in lines:
        if l.startswith("@SQ"):
            f = dict(x.split(":", 1) for x in l.split("\t")[1:])
            out.append((f["SN"], int(f["LN"])))
    return out


def _piece(f, seq_no, Q):
    """(qs, qe, seq, rs, re, rev) of one SAM record, or None when it is not eligible (not primary, MAPQ below Q)."""
    yf = [x[5:] for x in f[11:] if x.startswith("YF:H:")]
    assert len(yf) == 1
    if not int(yf[0], 16) & 0x20 or int(f[4]) < Q:
        return None
    cig = [(int(n), op) for n, op in _CIG.findall(f[5])]
    assert cig and "".join("%d%s" % c for c in cig) == f[5] and all(op in "MIDSH" for _n, op in cig)
    front = cig[0][0] if cig[0][1] in "SH" else 0
    back = cig[-1][0] if len(cig) > 1 and cig[-1][1] in "SH" else 0
    qal = sum(n for n, op in cig if op in "MI"); ref_len = sum(n for n, op in cig if op in "MD")
    qlen = front + qal + back; sqo = front; eqo = front + qal - 1
    rev = bool(int(f[1]) & 0x10)
    qs, qe = (qlen - 1 - eqo, qlen - 1 - sqo) if rev else (sqo, eqo)
    rs = int(f[3]) - 1
    return (qs, qe, seq_no[f[2]], rs, rs + ref_len - 1, rev)


def canonical(seq_a, pos_a, str_a, seq_b, pos_b, str_b):
    """The smaller (sequence, position) first; a swap flips both strands.  Equal positions: no swap."""
    flip = {"+": "-", "-": "+"}
    if (seq_b, pos_b) < (seq_a, pos_a):
        return seq_b, pos_b, flip[str_b], seq_a, pos_a, flip[str_a]
    return seq_a, pos_a, str_a, seq_b, pos_b, str_b


def kind(seq_a, str_a, seq_b, str_b):
    if seq_a != seq_b:
        return "TRA"
    if str_a != str_b:
        return "INV"
    return "DEL" if str_a == "+" else "DUP"


def read_junctions(pieces):
    """Junctions of one read from its eligible pieces in print order: [(seqA, posA, strandA, seqB, posB, strandB, type, qgap)], ordinal order."""
    order = sorted(range(len(pieces)), key=lambda i: (pieces[i][0], pieces[i][1], i))
    out = []
    for x, y in zip(order, order[1:]):
        a, b = pieces[x], pieces[y]
        side_a = (a[2], a[3] if a[5] else a[4], "-" if a[5] else "+")
        side_b = (b[2], b[4] if b[5] else b[3], "-" if b[5] else "+")
        c = canonical(*(side_a + side_b))
        out.append(c + (kind(c[0], c[2], c[3], c[5]), b[0] - a[1] - 1))
    return out


def junctions(lines, Q=0, with_reads=False):
    """All junctions of a SAM text, in (read, ordinal) order.  with_reads: [(read number among the reads that have records, junction)]."""
    seq_no = {name: i for i, (name, _ln) in enumerate(sq_table(lines))}
    out, cur, pieces, rno = [], None, [], -1

    def flush():
        for j in read_junctions(pieces):
            out.append((rno, j) if with_reads else j)

    for l in lines:
        if not l or l.startswith("@"):
            continue
        f = l.split("\t")
        if f[0] != cur:
            flush(); cur = f[0]; pieces = []; rno += 1
        p = _piece(f, seq_no, Q)
        if p is not None:
            pieces.append(p)
    flush()
    return out


def clusters(junc, W=10):
    """[[members]] in creation order: the junctions sorted by (seqA, strandA, seqB, strandB, posA, posB, qgap) join the first cluster of their
    (seqA, strandA, seqB, strandB) whose first member is within W on both sides, else open one.  ('+' sorts before '-'.)"""
    out = []
    for j in sorted(junc, key=lambda j: (j[0], j[2], j[3], j[5], j[1], j[4], j[7])):
        for c in out:
            f = c[0]
            if (f[0], f[2], f[3], f[5]) == (j[0], j[2], j[3], j[5]) and j[1] - f[1] <= W and abs(j[4] - f[4]) <= W:
                c.append(j); break
        else:
            out.append([j])
    return out


def text(cl, sq):
    out = []
    for c in cl:
        f = c[0]
        pa = [j[1] for j in c]; pb = [j[4] for j in c]; g = [j[7] for j in c]
        out.append("%s\t%d\t%d\t%s\t%d\t%d\t%s\t%d\t%s\t%s\t%d\t%d\n" % (sq[f[0]][0], min(pa), max(pa) + 1, sq[f[3]][0], min(pb), max(pb) + 1, f[6], len(c), f[2], f[5],
                                                                 min(g), max(g)))
    return "".join(out)


def expected(lines, Q=0, W=10):
    return text(clusters(junctions(lines, Q), W), sq_table(lines))


def by_type(junc):
    return {t: sum(1 for j in junc if j[6] == t) for t in TYPES}
