"""Indel alleles (-oid) recomputed from SAM text alone, by the rules of the issue.  Inputs are CIGAR, POS, SEQ, FLAG, MAPQ and the @SQ table: a D of at least L
bases is the allele (slot of its first base, DEL, length); an I of at least L bases is the allele (slot of the next reference base, kept inside the record, INS,
length, the first 42 inserted letters of SEQ -- A C G T, anything else N); S clips consume SEQ, H clips nothing; an I that asks for more SEQ than there is before
the trailing clip is no event.  SEQ is in reference orientation for either strand (FLAG 16 is only asserted to be consistent), so the letters are taken as they
stand.  A record counts 1 per op.  Shares nothing with the product: the tests compare the command line's file and the device's entries with this."""
import collections
import re

_CIG = re.compile(r"(\d+)([MIDNSHP=X])")
KEPT = 42
DEL, INS = 0, 1
_ORDER = {c: i for i, c in enumerate("ACGTN")}


def sq_table(lines):
    """[(name, length)] from the @SQ lines, in header order (= index order)."""
    out = []
    for l in lines:
        if l.startswith("@SQ"):
            f = dict(x.split(":", 1) for x in l.split("\t")[1:])
            out.append((f["SN"], int(f["LN"])))
    return out


def _records(lines, Q):
    for l in lines:
        if l and not l.startswith("@"):
            f = l.split("\t")
            if int(f[4]) >= Q:
                yield f


def records(lines, Q=0):
    return sum(1 for _ in _records(lines, Q))


def alleles(lines, sq, Q=0, L=1):
    """Counter {(slot, type, length, bases): records' ops} over the records with MAPQ >= Q; slot: reference bases before it in @SQ order; bases: the kept
    letters of an insertion, '' for a deletion."""
    base, length, tot = {}, {}, 0
    for name, ln in sq:
        base[name] = tot; length[name] = ln; tot += ln
    out = collections.Counter()
    for f in _records(lines, Q):
        name, start, seq = f[2], int(f[3]) - 1, f[9].upper()
        cig = [(int(n), op) for n, op in _CIG.findall(f[5])]
        assert "".join("%d%s" % c for c in cig) == f[5] and cig
        last = start + sum(n for n, op in cig if op in "MD") - 1
        assert 0 <= start and last < length[name]
        b0 = base[name]
        limit = len(seq) - (cig[-1][0] if len(cig) > 1 and cig[-1][1] == "S" else 0)      # SEQ before the trailing soft clip
        pos, q = start, 0
        for k, (n, op) in enumerate(cig):
            if op == "M":
                pos += n; q += n
            elif op == "D":
                if n >= L and pos + n <= last + 1:
                    out[(b0 + pos, DEL, n, "")] += 1
                pos += n
            elif op == "I":
                if n >= L and q + n <= limit:
                    out[(b0 + min(pos, last), INS, n, "".join(c if c in "ACGT" else "N" for c in seq[q:q + min(n, KEPT)]))] += 1
                q += n
            elif op == "S":
                assert k in (0, len(cig) - 1)
                q += n
            else:
                assert op == "H" and k in (0, len(cig) - 1), op
    return out


def order(key):
    slot, typ, n, bases = key
    return (slot, typ, n, [_ORDER[c] for c in bases])


def text(al, sq, min_count=1, times=1):
    """The file: one line per allele with count * times >= min_count, sorted by (sequence, position, DEL before INS, length, bases in the order A C G T N)."""
    starts, tot = [], 0
    for name, ln in sq:
        starts.append((tot, name)); tot += ln
    out = []
    for key in sorted(al, key=order):
        n = al[key] * times
        if n < min_count:
            continue
        slot, typ, ln, bases = key
        b0, name = [s for s in starts if s[0] <= slot][-1]
        seq = "*" if typ == DEL else bases + ("+" if ln > KEPT else "")
        out.append("%s\t%d\t%s\t%d\t%s\t%d\n" % (name, slot - b0 + 1, "INS" if typ == INS else "DEL", ln, seq, n))
    return "".join(out)


def entry_key(w0, w1, w2):
    """(slot, type, length, bases) of a device entry's three words (the key layout of the issue)."""
    assert w0 >> 63 and w1 >> 63 and w2 >> 63
    slot, typ, ln = w0 & 0xFFFFFFFF, (w0 >> 32) & 1, (w0 >> 33) & 0xFFFF
    assert (w0 >> 49) & 0x3FFF == 0
    n = min(ln, KEPT) if typ == INS else 0
    digits = [((w1 >> (3 * i)) if i < 21 else (w2 >> (3 * (i - 21)))) & 7 for i in range(n)]
    assert all(d < 5 for d in digits)
    rest1 = (w1 & ~(1 << 63)) >> (3 * min(n, 21)); rest2 = (w2 & ~(1 << 63)) >> (3 * max(0, n - 21))
    assert rest1 == 0 and rest2 == 0
    return (slot, typ, ln, "".join("ACGTN"[d] for d in digits))
