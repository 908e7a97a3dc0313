"""The SNV calls (-osnv) recomputed from the pileup of tests/pileup_oracle.py and the reference letters alone, by the rules of the issue, in plain Python
integers: r = the count of the reference's base, alt = the greatest of the other three of A C G T (ties to the lowest channel), D = A + C + G + T, other = N +
del; three costs in 1/100 phred from the sequencing error; PL0 = r cM + a cE, PL1 = (r + a) cH, PL2 = r cE + a cM; GT the smallest (ties to the lower index);
QUAL = min(PL0 - least, 999900) // 100, GQ = min(second smallest - least, 9900) // 100; a call needs GT != 0, a >= min_alt, D >= min_depth, QUAL >= min_qual.
Shares nothing with the product: the tests compare the command line's file, the device's records and the shared routine's verdicts with this."""
import math

import numpy as np

LETTERS = "ACGT"
DEFAULTS = dict(err=100, min_alt=2, min_depth=4, min_qual=20)
SAT = 0xFFFFFFFF


def costs(err=100):
    """(cM, cE, cH) in 1/100 phred for a sequencing error of `err` per mille."""
    e = err / 1000.0
    return (int(math.floor(-1000.0 * math.log10(1.0 - e) + 0.5)), int(math.floor(-1000.0 * math.log10(e / 3.0) + 0.5)),
            int(math.floor(-1000.0 * math.log10(0.5 - e / 3.0) + 0.5)))


def verdict(row, ref_letter, cst, min_alt, min_depth, min_qual):
    """None where the reference is not one of A C G T; otherwise a dict with everything the record holds and `call`."""
    if ref_letter not in LETTERS:
        return None
    row = [int(x) for x in row]; rc = LETTERS.index(ref_letter); cM, cE, cH = cst
    alt = None
    for ch in range(4):
        if ch != rc and (alt is None or row[ch] > row[alt]):
            alt = ch
    r, a = row[rc], row[alt]
    depth, other = sum(row[:4]), row[4] + row[5]
    pl = [r * cM + a * cE, (r + a) * cH, r * cE + a * cM]
    gt = pl.index(min(pl)); least = pl[gt]
    pl = [x - least for x in pl]
    qual = min(pl[0], 999900) // 100
    gq = min(sorted(pl)[1], 9900) // 100
    return dict(rc=rc, alt=alt, gt=gt, r=r, a=a, depth=min(depth, SAT), other=min(other, SAT), qual=qual, gq=gq, pl=[min(x, SAT) for x in pl],
                call=gt != 0 and a >= min_alt and depth >= min_depth and qual >= min_qual)


def calls(pu, ref, err=100, min_alt=2, min_depth=4, min_qual=20, keep=lambda v: v["call"]):
    """[(slot, verdict)] ascending, for the slots `keep` accepts (default: the calls).  pu: (n_slots, 7); ref: the reference's letters as bytes (ref_letters)."""
    cst = costs(err); out = []
    touched = np.nonzero(pu[:, :4].sum(axis=1) > 0)[0]            # (a call needs a >= min_alt >= 1: nothing is lost)
    for s in touched:
        v = verdict(pu[s], chr(ref[s]), cst, min_alt, min_depth, min_qual)
        if v is not None and keep(v):
            out.append((int(s), v))
    return out


def records(cl, ref):
    """The calls as the device's records: rows of twelve integers (slot, info, r, a, D, other, QUAL, GQ, PL0, PL1, PL2, 0)."""
    code = {"T": 0, "C": 1, "A": 2, "G": 3}
    return [(s, v["rc"] | v["alt"] << 4 | v["gt"] << 8 | code[chr(ref[s])] << 12, v["r"], v["a"], v["depth"], v["other"], v["qual"], v["gq"], v["pl"][0], v["pl"][1],
             v["pl"][2], 0) for s, v in cl]


def header(sq, err=100, min_alt=2, min_depth=4, min_qual=20, Q=0):
    cst = costs(err)
    h = ["##fileformat=VCFv4.2", "##source=yaha_amd -snverr %d -snvmin %d -snvdp %d -snvqual %d -puq %d" % (err, min_alt, min_depth, min_qual, Q),
         "##yaha_costs=<match=%d,error=%d,het=%d>" % cst,
         "##yaha_note=single-nucleotide variants only: insertions and deletions are not called here (-oid holds them)"]
    h += ["##contig=<ID=%s,length=%d>" % (name, ln) for name, ln in sq]
    h += ['##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads that show A, C, G or T at the site">',
          '##INFO=<ID=OT,Number=1,Type=Integer,Description="Reads that show N or a deletion at the site (not modelled)">',
          '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
          '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality: the second smallest PL, at most 99">',
          '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Reads that show A, C, G or T at the site">',
          '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Reads that show the reference base and the alternate base">',
          '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Normalised phred-scaled genotype likelihoods">',
          "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tyaha"]
    return "\n".join(h) + "\n"


def text(pu, sq, ref, err=100, min_alt=2, min_depth=4, min_qual=20, Q=0):
    """The VCF file of a pileup made with -puq Q."""
    out = [header(sq, err, min_alt, min_depth, min_qual, Q)]; cl = calls(pu, ref, err, min_alt, min_depth, min_qual)
    b0, k = 0, 0
    for name, ln in sq:
        while k < len(cl) and cl[k][0] < b0 + ln:
            s, v = cl[k]; k += 1
            out.append("%s\t%d\t.\t%s\t%s\t%d\tPASS\tDP=%d;OT=%d\tGT:GQ:DP:AD:PL\t%s:%d:%d:%d,%d:%d,%d,%d\n" % (
                name, s - b0 + 1, chr(ref[s]), LETTERS[v["alt"]], v["qual"], v["depth"], v["other"], "0/1" if v["gt"] == 1 else "1/1", v["gq"], v["depth"], v["r"], v["a"],
                v["pl"][0] // 100, v["pl"][1] // 100, v["pl"][2] // 100))
        b0 += ln
    return "".join(out)


# ---- the variant read set: two haplotypes of the first ~200 kbp of the golden genome, reads of both with sequencing errors ----------------------------------------
SEED = 20261
REGION = 200000
READ_LEN = 1000
DEPTH = 12
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def variant_reads(fasta, seed=SEED):
    """(FASTA text of the reads, planted: [(sequence name, 0-based position, reference letter, alt letter, 'hom' | 'het')]).  fasta: {name: sequence} in file
    order.  SNVs every 250 to 350 bases, alternately on both haplotypes and on the second alone; 1 kbp reads at about twelve-fold depth, half from each
    haplotype, half from each strand, with 2 % substitutions and 0.4 % insertions and deletions of one or two bases each."""
    rng = np.random.RandomState(seed); left = REGION; planted, out, n_read = [], [], 0
    for name, seq in fasta.items():
        if left < 2 * READ_LEN:
            break
        seq = seq[:left].upper(); left -= len(seq)
        hap = [list(seq), list(seq)]
        pos, k = 150, 0
        while pos < len(seq) - 150:
            refb = seq[pos]
            if refb in "ACGT":
                alt = "ACGT".replace(refb, "")[rng.randint(3)]; kind = "hom" if k % 2 == 0 else "het"; k += 1
                hap[1][pos] = alt
                if kind == "hom":
                    hap[0][pos] = alt
                planted.append((name, pos, refb, alt, kind))
            pos += int(rng.randint(250, 351))
        hap = ["".join(h) for h in hap]
        for i in range(DEPTH * len(seq) // READ_LEN):
            h = hap[i & 1]; start = int(rng.randint(0, len(seq) - READ_LEN + 1)); src = h[start:start + READ_LEN]; rd = []
            u = rng.random_sample(len(src)); v = rng.randint(0, 1 << 30, len(src)); j = 0
            while j < len(src):
                if u[j] < 0.02:
                    rd.append("ACGT".replace(src[j], "")[v[j] % 3] if src[j] in "ACGT" else src[j]); j += 1
                elif u[j] < 0.024:
                    rd.append(src[j]); rd.extend("ACGT"[(v[j] >> (2 * t)) & 3] for t in range(1 + (v[j] >> 8 & 1))); j += 1
                elif u[j] < 0.028:
                    j += 1 + (v[j] & 1)
                else:
                    rd.append(src[j]); j += 1
            rd = "".join(rd)
            if i & 2:
                rd = "".join(COMP.get(c, "N") for c in reversed(rd))
            out.append(">v%d_%s_%d_h%d\n%s\n" % (n_read, name, start, i & 1, rd)); n_read += 1
    return "".join(out), planted
