"""The read-depth track (-ocov) recomputed from SAM text alone -- RNAME, POS, the M lengths of the CIGAR, MAPQ and the @SQ lengths -- and formatted as bedGraph by
the rules of the issue.  Shares nothing with the product: the tests compare the command line's file and the device's array with this."""
import re

_CIG = re.compile(r"(\d+)([MIDNSHP=X])")


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


def coverage(lines, sq, B=100, Q=0):
    """cov[bin] over all bins, sequence by sequence: bases under M of every record with MAPQ >= Q; D skips reference without covering it, I / S / H consume none."""
    base, length, tot = {}, {}, 0
    for name, ln in sq:
        base[name] = tot; length[name] = ln; tot += (ln + B - 1) // B
    cov = [0] * tot
    for l in lines:
        if not l or l.startswith("@"):
            continue
        f = l.split("\t")
        if int(f[4]) < Q:
            continue
        pos = int(f[3]) - 1
        for n, op in _CIG.findall(f[5]):
            n = int(n)
            if op == "M":
                assert pos + n <= length[f[2]]
                for p in range(pos, pos + n):
                    cov[base[f[2]] + p // B] += 1
                pos += n
            elif op == "D":
                pos += n
    return cov


def records(lines, Q=0):
    return sum(1 for l in lines if l and not l.startswith("@") and int(l.split("\t")[4]) >= Q)


def bedgraph(cov, sq, B):
    out, b0 = [], 0
    for name, ln in sq:
        nb = (ln + B - 1) // B
        c = cov[b0:b0 + nb]
        if B == 1:
            i = 0
            while i < ln:
                if c[i] == 0:
                    i += 1; continue
                j = i + 1
                while j < ln and c[j] == c[i]:
                    j += 1
                out.append("%s\t%d\t%d\t%d\n" % (name, i, j, c[i])); i = j
        else:
            for b in range(nb):
                if c[b]:
                    lo, hi = b * B, min((b + 1) * B, ln)
                    out.append("%s\t%d\t%d\t%.4f\n" % (name, lo, hi, c[b] / (hi - lo)))
        b0 += nb
    return "".join(out)
