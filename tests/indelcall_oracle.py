"""The indel calls (-oindel) recomputed by the rules of the issue, in plain Python on strings and integers.  An allele is (slot, type, length, bases) as
tests/indel_oracle.py makes it; the reference is one string of letters over all slots (pileup_oracle.ref_letters) with the sequences' lengths.  Normalisation
is the textbook loop, one base at a time: "while the allele's last base equals the base before it, move".  Merging is a dict.  The verdict: d = A + C + G + T +
N + del of the pileup row at the anchor, a = the merged count (saturated at 2^32 - 1), r = max(d - a, 0); PL0 = r cM + a cE, PL1 = (r + a) cH, PL2 = r cE + a cM
with cM = round(-1000 log10(1 - e)), cE = round(-1000 log10 e), cH = round(1000 log10 2); GT the smallest (ties to the lower index), QUAL = min(PL0 - least,
999900) // 100, GQ = min(second smallest - least, 9900) // 100; a call needs GT != 0, a >= min_alt, d >= min_depth, QUAL >= min_qual.
Shares nothing with the product: the tests compare the command line's file, the device's records and the shared routines' results with this."""
import math

import indel_oracle as io

DEL, INS, KEPT = io.DEL, io.INS, io.KEPT
SAT = 0xFFFFFFFF
DEFAULTS = dict(err=50, min_alt=2, min_depth=4, min_qual=20)
CODE = {"T": 0, "C": 1, "A": 2, "G": 3, "N": 4}


def costs(err=50):
    e = err / 1000.0
    return (int(math.floor(-1000.0 * math.log10(1.0 - e) + 0.5)), int(math.floor(-1000.0 * math.log10(e) + 0.5)), int(math.floor(1000.0 * math.log10(2.0) + 0.5)))


def seq_of(sq, slot):
    """(first slot, one past the last slot) of the sequence a slot lies in; sq: [(name, length)]."""
    b0 = 0
    for _name, ln in sq:
        if b0 <= slot < b0 + ln:
            return b0, b0 + ln
        b0 += ln
    return None


def normalise(key, ref, sq, max_shift):
    """(the normalised key, bases moved), or None where the allele is not called (`skipped`).  ref: a str with one letter a slot."""
    slot, typ, ln, bases = key
    span = seq_of(sq, slot)
    if span is None or ln == 0:
        return None
    first, end = span
    if typ == INS and ln > KEPT:
        return None
    if slot == first:
        return None
    if typ == DEL and slot + ln > end:
        return None
    p, moved, ins = slot, 0, bases
    while moved < max_shift and p - 1 > first:
        before = ref[p - 1]
        last = ins[-1] if typ == INS else ref[p + ln - 1]
        if before not in "ACGT" or last not in "ACGT" or before != last:
            break
        if typ == INS:
            ins = before + ins[:-1]
        p -= 1; moved += 1
    return (p, typ, ln, ins), moved


def merge(raw, ref, sq, max_shift):
    """raw: {key: count} or [(key, count)].  Returns ({normalised key: count saturated}, stats dict raw / shifted / merged / skipped)."""
    items = list(raw.items()) if isinstance(raw, dict) else list(raw)
    out, shifted, skipped = {}, 0, 0
    for key, n in items:
        r = normalise(key, ref, sq, max_shift)
        if r is None:
            skipped += 1; continue
        shifted += r[1] > 0
        out[r[0]] = out.get(r[0], 0) + n
    out = {k: min(v, SAT) for k, v in out.items()}
    return out, dict(raw=len(items), shifted=shifted, merged=len(items) - skipped - len(out), skipped=skipped)


def verdict(row, a, cst, min_alt, min_depth, min_qual):
    row = [int(x) for x in row]; cM, cE, cH = cst
    d = sum(row[:6]); r = d - a if d > a else 0
    pl = [r * cM + a * cE, (r + a) * cH, r * cE + a * cM]
    gt = pl.index(min(pl)); least = pl[gt]
    pl = [x - least for x in pl]
    qual = min(pl[0], 999900) // 100
    gq = min(sorted(pl)[1], 9900) // 100
    return dict(gt=gt, a=a, r=min(r, SAT), d=min(d, SAT), qual=qual, gq=gq, pl=[min(x, SAT) for x in pl],
                call=gt != 0 and a >= min_alt and d >= min_depth and qual >= min_qual)


def judged(merged, pu, err=50, min_alt=2, min_depth=4, min_qual=20, keep=lambda v: v["call"]):
    """[(key, verdict)] in the order of the file for the alleles `keep` accepts.  pu: rows by slot (anything indexable by slot that gives seven counts)."""
    cst = costs(err); out = []
    for key in sorted(merged, key=io.order):
        v = verdict(pu[key[0] - 1], merged[key], cst, min_alt, min_depth, min_qual)
        if keep(v):
            out.append((key, v))
    return out


def words(key):
    """The three 64-bit words of a key (the layout of the issue of -oid)."""
    slot, typ, ln, bases = key
    w0 = slot | typ << 32 | ln << 33 | 1 << 63; w1 = w2 = 1 << 63
    for i, c in enumerate(bases[:KEPT]):
        d = "ACGTN".index(c)
        if i < 21:
            w1 |= d << (3 * i)
        else:
            w2 |= d << (3 * (i - 21))
    return w0, w1, w2


def records(cl, ref):
    """The calls as the device's records: (w0, w1, w2, a, r, d, QUAL, GQ, PL0, PL1, PL2, info, 0)."""
    return [words(k) + (v["a"], v["r"], v["d"], v["qual"], v["gq"], v["pl"][0], v["pl"][1], v["pl"][2], v["gt"] | CODE.get(ref[k[0] - 1], 14) << 4, 0) for k, v in cl]


def header(sq, err=50, min_alt=2, min_depth=4, min_qual=20, shift=256, Q=0):
    h = ["##fileformat=VCFv4.2", "##source=yaha_amd -inderr %d -indmin %d -inddp %d -indqual %d -indshift %d -puq %d" % (err, min_alt, min_depth, min_qual, shift, Q),
         "##yaha_costs=<match=%d,error=%d,het=%d>" % costs(err),
         "##yaha_note=insertions and deletions only, left-normalised, one line per allele (-osnv holds the single-nucleotide variants)"]
    h += ["##contig=<ID=%s,length=%d>" % (name, ln) for name, ln in sq]
    h += ['##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads that cover the anchor base">',
          '##INFO=<ID=TYPE,Number=1,Type=String,Description="INS or DEL">',
          '##INFO=<ID=LEN,Number=1,Type=Integer,Description="Inserted or deleted bases">',
          '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
          '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality: the second smallest PL, at most 99">',
          '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Reads that cover the anchor without the allele, reads that carry it">',
          '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Normalised phred-scaled genotype likelihoods">',
          "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tyaha"]
    return "\n".join(h) + "\n"


def text(raw, pu, sq, ref, err=50, min_alt=2, min_depth=4, min_qual=20, shift=256, Q=0):
    """The VCF file: raw = indel_oracle.alleles(lines, sq, Q, 1), pu = pileup_oracle.pileup(lines, sq, Q), ref = the reference's letters as a str."""
    merged, _st = merge(raw, ref, sq, shift)
    out = [header(sq, err, min_alt, min_depth, min_qual, shift, Q)]
    starts, tot = [], 0
    for name, ln in sq:
        starts.append((tot, name)); tot += ln
    for (slot, typ, ln, bases), v in judged(merged, pu, err, min_alt, min_depth, min_qual):
        anchor = slot - 1
        b0, name = [s for s in starts if s[0] <= anchor][-1]
        if typ == INS:
            r, a = ref[anchor], ref[anchor] + bases
        else:
            r, a = ref[anchor:anchor + ln + 1], ref[anchor]
        out.append("%s\t%d\t.\t%s\t%s\t%d\tPASS\tDP=%d;TYPE=%s;LEN=%d\tGT:GQ:AD:PL\t%s:%d:%d,%d:%d,%d,%d\n" % (
            name, anchor - b0 + 1, r, a, v["qual"], v["d"], "INS" if typ == INS else "DEL", ln, "0/1" if v["gt"] == 1 else "1/1", v["gq"], v["r"], v["a"],
            v["pl"][0] // 100, v["pl"][1] // 100, v["pl"][2] // 100))
    return "".join(out)
