"""What the indel-call tests stand on: a crafted genome with planted runs, a directed set of raw alleles placed at the RIGHT end of those runs (so every one
must move), pileup rows for the anchors, and a variant read set with planted indels.  Everything is made with fixed seeds; nothing here knows the product --
what a set reaches is asserted by the tests on the ORACLE's result (tests/indelcall_oracle.py)."""
import numpy as np

import indelcall_oracle as ico
import snv_oracle as so

DEL, INS = ico.DEL, ico.INS
SEED = 20262
HOMO = (1, 2, 63, 64, 65, 127, 128, 129)          # homopolymer runs: the wave-step edges
INS_LEN = (2, 21, 22, 41, 42, 43)                 # unit lengths of the insertion runs (1 is the homopolymers'); 43 is skipped
DEL_LEN = (2, 64, 65, 300)                        # unit lengths of the deletion runs (1 is the homopolymers')
CAP_RUN = 64                                      # the run the caps are set around: max_shift 0, 63, 64, 65
BIG = 0xFFFFFFF0


def _other(rng, *not_these):
    left = [c for c in "ACGT" if c not in not_these]
    return left[rng.randint(len(left))]


def _filler(rng, n):
    """n random letters with no two neighbours equal (a filler never lengthens a run by more than its flank rule allows)."""
    out = []
    for _ in range(n):
        out.append(_other(rng, out[-1]) if out else "ACGT"[rng.randint(4)])
    return out


def _unit(rng, n):
    u = _filler(rng, n)
    if n > 1 and u[0] == u[-1]:
        u[-1] = _other(rng, u[0], u[-2])
    return "".join(u)


class Craft:
    """The genome, sequence by sequence, and the places of its runs: runs[name] = (first slot, one past the last slot, unit)."""

    def __init__(self, seed=SEED):
        rng = np.random.RandomState(seed)
        self.rng, self.seqs, self.runs, self._cur, self._base = rng, [], {}, [], 0

        def close(name):
            self.seqs.append((name, "".join(self._cur))); self._base += len(self._cur); self._cur = []

        def add_run(name, unit, length, gap=37):
            """A periodic run of `length` letters with period `unit`, flanked by letters that continue it on neither side."""
            run = (unit * (length // len(unit) + 1))[:length]
            before = _other(rng, unit[-1], self._cur[-1] if self._cur else "")
            after = _other(rng, unit[length % len(unit)])
            self._cur.append(before)
            r0 = self._base + len(self._cur)
            self._cur.extend(run); self._cur.append(after)
            fill = _filler(rng, gap)
            if fill[0] == after:
                fill[0] = _other(rng, after, fill[1])
            self._cur.extend(fill)
            self.runs[name] = (r0, r0 + length, unit)

        # sequence 1: background, the homopolymer runs and the short repeats
        self._cur.extend(_filler(rng, 150))
        for n in HOMO:
            add_run("homo%d" % n, "A", n)
        add_run("di7", "CA", 7); add_run("tri10", "GAT", 10); add_run("tri11", "GAT", 11)
        add_run("di8", "CA", 8)                                                  # (a whole number of units: s mod L == 0)
        self._cur.extend("GGGGNGGGG"); self.runs["broken"] = (self._base + len(self._cur) - 4, self._base + len(self._cur), "G")
        self._cur.extend(_filler(rng, 60))
        self._cur[-60] = "C"
        self._cur.extend("TTTT")                                                 # the previous sequence ends in the letters the next one starts with
        close("craft1")
        # sequence 2: starts inside a run (the anchor cap; it must not cross into sequence 1), then the insertion and deletion units
        self._cur.extend("TTTTTT"); self.runs["edge"] = (self._base, self._base + 6, "T"); self._cur.append("G"); self._cur.extend(_filler(rng, 40))
        for L in INS_LEN:
            add_run("ins%d" % L, _unit(rng, L), 2 * L + L // 2)
        add_run("ins21x2", _unit(rng, 21), 42)                                    # s mod L == 0
        for L in DEL_LEN:
            add_run("del%d" % L, _unit(rng, L), 2 * L + 5)
        close("craft2")
        # sequence 3: plain background, where the alleles of the judging cases sit
        self._cur.extend(_filler(rng, 2600))
        close("craft3")
        self.sq = [(n, len(s)) for n, s in self.seqs]
        self.ref = "".join(s for _n, s in self.seqs)
        self.first = {}
        b0 = 0
        for n, s in self.seqs:
            self.first[n] = b0; b0 += len(s)

    def fasta(self):
        return "".join(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))) for n, s in self.seqs)


def directed(g):
    """[(key, count)]: raw alleles at the right end of their runs, the merging and boundary cases, then the judging cases.  Also the names of what is what:
    returns (raw, tags) with tags[name] = index into raw."""
    raw, tags = [], {}

    def add(name, key, count=6):
        tags[name] = len(raw); raw.append((key, count))

    ref = g.ref
    for n in HOMO:
        r0, r1, _u = g.runs["homo%d" % n]
        add("homo%d_del" % n, (r1 - 1, DEL, 1, ""))
        add("homo%d_ins" % n, (r1, INS, 1, "A"))
    for name in ("di7", "di8", "tri10", "tri11"):
        r0, r1, u = g.runs[name]; L = len(u)
        add(name + "_ins", (r1, INS, L, ref[r1 - L:r1])); add(name + "_del", (r1 - L, DEL, L, ""))
    for L in INS_LEN:
        r0, r1, u = g.runs["ins%d" % L]
        add("ins%d" % L, (r1, INS, L, ref[r1 - L:r1][:ico.KEPT]))
    r0, r1, u = g.runs["ins21x2"]; add("ins21x2", (r1, INS, 21, ref[r1 - 21:r1]))
    for L in DEL_LEN:
        r0, r1, u = g.runs["del%d" % L]
        add("del%d" % L, (r1 - L, DEL, L, ""))
    # boundaries
    r0, r1, _u = g.runs["edge"]; add("edge_ins", (r1, INS, 1, "T")); add("edge_del", (r1 - 1, DEL, 1, ""))
    r0, r1, _u = g.runs["broken"]; add("broken_ins", (r1, INS, 1, "G")); add("broken_del", (r1 - 1, DEL, 1, ""))
    add("first_slot_del", (g.first["craft2"], DEL, 1, "")); add("first_slot_ins", (0, INS, 2, "AC")); add("n_in_ins", (g.runs["homo63"][1], INS, 2, "NA"))
    # merging: three offsets of one run that become one; two of one run that stay two (by length); counts that saturate
    r0, r1, _u = g.runs["homo129"]; add("merge_mid", (r0 + 50, DEL, 1, ""), 2); add("merge_left", (r0, DEL, 1, ""), 3)
    r0, r1, _u = g.runs["homo65"]; add("stay_two", (r1 - 2, DEL, 2, ""))
    r0, r1, _u = g.runs["homo127"]; raw[tags["homo127_ins"]] = (raw[tags["homo127_ins"]][0], BIG); add("saturate", (r0 + 10, INS, 1, "A"), 0x20)
    # judging: alleles in the plain background of sequence 3, one per (a, d) case (cases() below gives them their rows)
    b3 = g.first["craft3"]
    for i, (a, _d) in enumerate(JUDGE):
        p = b3 + 100 + 40 * i
        key = (p, DEL, 1 + i % 3, "") if i % 2 == 0 else (p, INS, 1 + i % 4, "".join("ACGT"[(i + j) % 4] for j in range(1 + i % 4)))
        add("judge%d" % i, key, a)
    return raw, tags


# (a, d) of the judging cases with the default costs (22, 1301, 301) and thresholds (2, 4, 20): d = 0; a > d; a = d; a heterozygote; a reference genotype; -indmin
# one below and at its value; -inddp one below and at; QUAL 19 and 20 (a heterozygote's QUAL is (1000 a - 279 r) // 100: a = 5, r = 11 and a = 4, r = 7)
JUDGE = ((5, 0), (5, 4), (5, 5), (5, 10), (5, 200), (1, 1), (2, 4), (3, 3), (4, 4), (5, 16), (4, 11), (0xFFFFFFFF, 7))


def rows_for(g, merged, tags, raw):
    """{anchor slot: seven counts} for the merged alleles: the judging cases get their d, spread over the six channels that count (INS holds a number nothing
    may look at); every other anchor is covered by twice its allele's count, at most 40."""
    rows = {}
    judge_slots = {}
    for i, (_a, d) in enumerate(JUDGE):
        key = ico.normalise(raw[tags["judge%d" % i]][0], g.ref, g.sq, 256)[0]
        judge_slots[key[0] - 1] = d
    for key, n in merged.items():
        anchor = key[0] - 1
        d = judge_slots.get(anchor, min(2 * n, 40))
        part = [d // 6] * 6
        for k in range(d % 6):
            part[k] += 1
        rows[anchor] = [a + b for a, b in zip(rows.get(anchor, [0] * 7), part + [9])]
    return rows


class RowTable:
    """Rows by slot for the oracle: zeros where nothing was set."""

    def __init__(self, rows):
        self.rows = rows

    def __getitem__(self, slot):
        return self.rows.get(int(slot), [0] * 7)


# ---- the variant read set with planted indels: snv_oracle.variant_reads' scheme (two haplotypes, reads of both, sequencing errors), extended -------------------
INDEL_REGION = 120000


def indel_reads(fasta, seed=SEED + 1):
    """(FASTA text of the reads, planted: [(name, 0-based position, 'INS' | 'DEL', length, 'hom' | 'het')]).  Indels of 1 to 12 bases every 400 to 600 bases,
    alternately on both haplotypes and on the second alone, alternately insertions and deletions, every third one a copy / removal of the bases beside it (a
    tandem duplication or the contraction of one: inside a repeat by construction); reads as in snv_oracle.variant_reads, without the random indel errors' being
    any different."""
    rng = np.random.RandomState(seed); left = INDEL_REGION; planted, out, n_read = [], [], 0
    for name, seq in fasta.items():
        if left < 2 * so.READ_LEN:
            break
        seq = seq[:left].upper(); left -= len(seq)
        edits, pos, k = [], 300, 0
        while pos < len(seq) - 300:
            ln = 1 + int(rng.randint(12)); kind = "hom" if k % 2 == 0 else "het"; typ = "INS" if (k // 2) % 2 == 0 else "DEL"
            if set(seq[pos - 14:pos + 14]) <= set("ACGT"):
                if typ == "INS":
                    bases = seq[pos - ln:pos] if k % 3 == 0 else "".join("ACGT"[x] for x in rng.randint(0, 4, ln))
                else:
                    bases = ""
                edits.append((pos, typ, ln, bases, kind)); planted.append((name, pos, typ, ln, kind)); k += 1
            pos += int(rng.randint(400, 601))
        hap = []
        for h in (0, 1):
            parts, at = [], 0
            for pos, typ, ln, bases, kind in edits:
                if h == 0 and kind == "het":
                    continue
                parts.append(seq[at:pos])
                if typ == "INS":
                    parts.append(bases); at = pos
                else:
                    at = pos + ln
            parts.append(seq[at:]); hap.append("".join(parts))
        for i in range(so.DEPTH * len(seq) // so.READ_LEN):
            h = hap[i & 1]; start = int(rng.randint(0, len(h) - so.READ_LEN + 1)); src = h[start:start + so.READ_LEN]
            u = rng.random_sample(len(src)); v = rng.randint(0, 1 << 30, len(src))
            rd = "".join(("ACGT".replace(c, "")[v[j] % 3] if c in "ACGT" else c) if u[j] < 0.01 else c for j, c in enumerate(src))
            if i & 2:
                rd = "".join(so.COMP.get(c, "N") for c in reversed(rd))
            out.append(">w%d_%s_%d_h%d\n%s\n" % (n_read, name, start, i & 1, rd)); n_read += 1
    return "".join(out), planted
