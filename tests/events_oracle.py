"""The evidence track (-oev) recomputed from SAM text alone and formatted by the rules of the issue.  POS and the clip, I and D lengths come from the CIGAR,
mismatch positions from MD:Z (the letters not inside a ^ run), MAPQ and the @SQ lengths complete the picture.  Shares nothing with the product: the tests
compare the command line's file and the device's array with this."""
import re

_CIG = re.compile(r"(\d+)([MIDNSHP=X])")
_MD = re.compile(r"(\d+)|\^([A-Za-z]+)|([A-Za-z])")
CHANNELS = ("mismatch", "deleted", "insertion", "clip_left", "clip_right")
HEADER = "#chrom\tstart\tend\t" + "\t".join(CHANNELS) + "\n"


def sq_table(lines):
    """[(name, length)] from the @SQ lines, in header order (= index order)."""
    out = []
    for l in lines:
        if l.startswith("@SQ"):
            f = dict(x.split(":", 1) for x in l.split("\t")[1:])
            out.append((f["SN"], int(f["LN"])))
    return out


def n_bins(sq, B):
    return sum((ln + B - 1) // B for _, ln in sq)


def _records(lines, Q):
    for l in lines:
        if l and not l.startswith("@"):
            f = l.split("\t")
            if int(f[4]) >= Q:
                yield f


def records(lines, Q=0):
    return sum(1 for _ in _records(lines, Q))


def events(lines, sq, B=100, Q=0, N=1):
    """ev[bin] = [mismatch, deleted, insertion, clip_left, clip_right] over all bins, sequence by sequence, from the records with MAPQ >= Q."""
    base, length, tot = {}, {}, 0
    for name, ln in sq:
        base[name] = tot; length[name] = ln; tot += (ln + B - 1) // B
    ev = [[0] * 5 for _ in range(tot)]
    for f in _records(lines, Q):
        name, start = f[2], int(f[3]) - 1
        cig = [(int(n), op) for n, op in _CIG.findall(f[5])]
        assert "".join("%d%s" % c for c in cig) == f[5] and cig
        ref_len = sum(n for n, op in cig if op in "MD")
        last = start + ref_len - 1
        assert 0 <= start and last < length[name]
        b0 = base[name]
        pos = start
        for n, op in cig:
            if op == "M":
                pos += n
            elif op == "D":
                for p in range(pos, pos + n):
                    ev[b0 + p // B][1] += 1
                pos += n
            elif op == "I":
                ev[b0 + min(pos, last) // B][2] += 1
            else:
                assert op in "SH", op
        if cig[0][1] in "SH" and cig[0][0] >= N:
            ev[b0 + start // B][3] += 1
        if len(cig) > 1 and cig[-1][1] in "SH" and cig[-1][0] >= N:
            ev[b0 + last // B][4] += 1
        md = [x[5:] for x in f[11:] if x.startswith("MD:Z:")]
        assert len(md) == 1
        pos = start; seen = 0
        for num, dele, mis in _MD.findall(md[0]):
            seen += len(num) + (len(dele) + 1 if dele else 0) + len(mis)
            if num:
                pos += int(num)
            elif dele:
                pos += len(dele)
            else:
                ev[b0 + pos // B][0] += 1
                pos += 1
        assert seen == len(md[0]) and pos == last + 1, (md[0], pos, last)
    return ev


def totals(ev):
    return [sum(b[c] for b in ev) for c in range(5)]


def text(ev, sq, B):
    out, b0 = [HEADER], 0
    for name, ln in sq:
        nb = (ln + B - 1) // B
        for b in range(nb):
            c = ev[b0 + b]
            if any(c):
                out.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % ((name, b * B, min((b + 1) * B, ln)) + tuple(c)))
        b0 += nb
    return "".join(out)
