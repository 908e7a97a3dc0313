"""The gap fills between chained fragments, kernel instance by kernel instance, against the oracle: score and edit list of constructed joints, bit-exact.

launchGapFills (stage_align.hip) hands a joint to one of eight kernel instances, chosen by gapJointKey (phase_lanes.h), gapBandPacked() and two environment
switches that are read at every call: YGPU_GAP32 (the 32-bit k_gap_band<12|16> instead of the packed band kernels) and YGPU_GAP24_OFF (the banded joints of
W = 17..24 go to k_gap_lanes<32> instead of k_gap_band_pk<24>).  The joints here are built, not found, and every family is aimed at something:

  columns   k_gap_band_pk<12|16|24> (gap_band_pk.h) and, under YGPU_GAP32, k_gap_band<12|16> (gap_band_lanes.h): trace cell (y, x) is byte x of record
            y + (x >= GW / 2), so a byte in the wrong record shows only when a traceback passes through that column.  For every d = qGap - rGap in -13..13
            and every column c of the strip the best path is led from the origin (column `left`) to c -- once arriving by a deletion, once by an insertion --
            down c over a substitution and on to the end cell (column `right`); also from edge to edge of the strip (column 0 <-> W - 1).  Paths start and end
            with a gap or with matches (explicit row 0: left >= GW / 2).  The same for banded W = 25..32 (k_gap_lanes<32>: strip in LDS), for banded W > 32
            (k_gap_wave) and for the unbanded shapes of rLen <= 15 (k_gap_lanes<16>) and 16..31 (<32>) with 1..60 rows.
  limits    the shapes at YD_GROWS = 60 rows and YD_GREF = 64 reference bases, and one past them (`tooBig`: k_gap_wave); insertion runs of 55 and more (trace
            cell op | run << 2 in a byte, 0xFF the origin mark); the smallest banded joints (12 x 12, and |d| = 1 at rGap = 13).
  ties      the global mode's `>` rules: gaps inside homopolymer and dinucleotide tracts, where they can sit in many places for one score; and, under a scoring
            where two substitutions cost what an insertion and a deletion of two cost, both next to each other.
  edges     joints at reference offsets 0..4 (refAt's code 15 for the strip's columns left of the first base), joints that end on the genome's last base
            (staged reference dwords from the padding behind it), joints across a run of N.
  caps      -G 20 -I 8 (and -I 20): maxGap >= 16 keeps the band kernels, the caps bind inside them -- gapBandPkRows<GW, CAPS = true> and the cap tests of
            k_gap_band; deletions of 9..23 and insertions past 20 that the caps break up; and a list whose band classes hold ONE joint of qGap > maxGap each:
            the wave-uniform __ballot switches the whole wave to the capped instance, and its other lanes must not notice.
  packed    a scoring exactly at gapBandPacked()'s bound (64 max(MS, RC) + GO + 64 GE = 12000), where 58 rows of insertion take the scores to -7500 (as
            far as a scoring goes that the reference itself computes without overflow, see SETS) against the packed sentinel of -16000, and one a step
            past it, where the 32-bit kernels take over with nothing set in the environment.

Before anything is compared the ORACLE's results are checked for the coverage all this is about (check_coverage; a test of its own that needs no GPU).
Tie criterion used there: the `>` rules make the traceback prefer a match to a gap of the same score, which leaves a gap at the FIRST place it can sit (the
oracle's lists for the tract joints all have it there), so a joint counts as decided by a tie rule when a gap of the oracle's list could sit one position
LATER for the same score (the matched base behind it equals the gap's first base) -- the opposite preference would move it; or, under the second scoring,
when its list holds two adjacent substitutions or an insertion and a deletion of two side by side, which cost the same.

A last test sends reads with one short indel through ygpu_run under the same switches: k_p1_joints' own classification, its nDPb[2] count, the sortedVals order
and the band24 split as the pipeline makes them."""
import os
import random

import numpy as np
import pytest

import oracle
import yaha_amd as ya
from problems import batch_arrays, dp_problems_from_chain

LETTERS = "TCAG"                      # the index's base codes 0..3
COMP = {"T": "A", "A": "T", "C": "G", "G": "C"}
BW = 5
YD_GROWS, YD_GREF = 60, 64            # the last shapes the lane kernels take (phase_lanes.h)
# a gap of 13 (16) beats any run of substitutions, a substitution (4 + 3 lost) an insertion + deletion (8)
MAIN = ["-MS", "3", "-RC", "4", "-GOC", "3", "-GEC", "1"]
SETS = {
    "main": MAIN,
    "ties": ["-MS", "1", "-RC", "3", "-GOC", "1", "-GEC", "1"],                 # 2 R = -6 = I2 + D2
    "caps8": MAIN + ["-G", "20", "-I", "8"],
    "caps20": MAIN + ["-G", "20", "-I", "20"],
    # 64 * 58 + 96 + 64 * 128 = 12000.  (GE <= 128 and GO + GE <= 256: the reference's DPWorstScore is INT_MIN + 256, and beyond that `worst - GE - GE` and
    # `worst - (GO + GE)` at the edges of a banded row wrap round to a huge score -- in the oracle as in the reference, e.g. -GOC 224 -GEC 180 -- so that such
    # scorings have no expected result to compare with.  This is the scoring with the dearest gaps inside both bounds.)
    "packed_last": ["-MS", "3", "-RC", "58", "-GOC", "96", "-GEC", "128"],
    "packed_past": ["-MS", "3", "-RC", "58", "-GOC", "97", "-GEC", "128"],
}
SWITCHES = (None, "YGPU_GAP24_OFF", "YGPU_GAP32")
BAND = {"band12": 12, "band16": 16, "band24": 24}
# (banded W = 25..32 within the limits: none of the band kernels' -- k_gap_lanes<32>)


# ---- the genome ----------------------------------------------------------------------------------------------------------------------------------------
def write_genome(path):
    """~300 kbp in five sequences, seeded: random bases; a homopolymer or dinucleotide tract of 20..60 bases about every 1500; a run of ten N inside the second
    sequence.  Returns [(sequence, position, length, unit length)] of the tracts and (sequence, position, length) of the N run."""
    rng = random.Random(1955)
    tracts, nrun, seqs = [], None, []
    for k, n in enumerate((70000, 60000, 50000, 64000, 56001)):
        s = [rng.choice(LETTERS) for _ in range(n)]
        at = 600
        while at + 200 < n:
            unit = 1 + (len(tracts) & 1)
            u = rng.sample(LETTERS, unit)
            tl = rng.randint(20, 60)
            s[at:at + tl] = [u[i % unit] for i in range(tl)]
            while s[at - 1] in u:                                            # (the tract is exactly as long as recorded)
                s[at - 1] = rng.choice(LETTERS)
            while s[at + tl] == u[tl % unit]:
                s[at + tl] = rng.choice(LETTERS)
            tracts.append((k, at, tl, unit))
            at += rng.randint(1200, 1800)
        if k == 1:
            s[30000:30010] = "N" * 10
            nrun = (k, 30000, 10)
        seqs.append("".join(s))
    with open(path, "w") as f:
        for k, s in enumerate(seqs):
            f.write(">gf%d\n" % k)
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    return seqs, tracts, nrun


# ---- the problems --------------------------------------------------------------------------------------------------------------------------------------
def _other(rng, code):
    return rng.choice([c for k, c in enumerate(LETTERS) if k != code])


def banded_rule(q, r):
    return abs(q - r) + 2 * BW + 1 < r


class Builder:
    def __init__(self, nib, max_roff, seq_starts):
        self.nib, self.max_roff, self.seq_starts = nib, max_roff, seq_starts
        self.rng = random.Random(406)
        self.place = 2000
        self.items = []                                                      # (read, fields without the read's number, meta)

    def spot(self, need=100):
        """the offset of `need` plain bases (no N, no padding), 101 apart"""
        while True:
            at = self.place; self.place += 101
            assert at + need < self.max_roff - 1000, "the genome is used up"
            if (self.nib[at:at + need] < 4).all():
                return at

    def apply(self, at, steps):
        """query and reference length of a path over the reference from `at`: ('m', n) copies, ('s',) substitutes, ('i', n) inserts, ('d', n) skips"""
        rng, nib, r, q = self.rng, self.nib, at, []
        for st in steps:
            if st[0] == "m":
                q.extend(LETTERS[c] if c < 4 else rng.choice(LETTERS) for c in nib[r:r + st[1]]); r += st[1]
            elif st[0] == "s":
                q.append(_other(rng, nib[r])); r += 1
            elif st[0] == "i":
                q.extend(_other(rng, nib[r + i]) for i in range(st[1]))      # (no base that would pair with the reference behind the insertion)
            else:
                r += st[1]
        return "".join(q), r - at

    def add(self, fam, at, query, rlen, banded=None, **more):
        rng = self.rng
        qlen = len(query)
        assert qlen >= 1 and rlen >= 1 and (qlen, rlen) != (1, 1) and at >= 0 and at + rlen <= self.max_roff
        rule = banded_rule(qlen, rlen)
        assert banded is None or banded == rule, (fam, qlen, rlen, banded)
        strand = len(self.items) & 1
        pl = "".join(rng.choice(LETTERS) for _ in range(rng.randint(2, 6)))
        pr = "".join(rng.choice(LETTERS) for _ in range(max(4, 44 - qlen) + rng.randint(0, 5)))
        full = pl + query + pr
        read = "".join(COMP[c] for c in reversed(full)) if strand else full
        rc = [int(c) for c in self.nib[at:at + rlen]]
        qc = [LETTERS.index(c) for c in query]
        mm = sum(a != b for a, b in zip(qc, rc)) if qlen == rlen else -1
        meta = dict(fam=fam, q=qlen, r=rlen, d=qlen - rlen, banded=rule, strand=strand, mm=mm, qc=qc, rc=rc, at=at, **more)
        self.items.append((read, (strand, ya.DP_BANDED if rule else ya.DP_FULL, len(pl), qlen, rlen, at), meta))

    def routed(self, fam, d, ways, head, tail, qmax=YD_GROWS, rmax=YD_GREF, stretch=(5, 8), at=None, end_at=None, want_banded=True, **more):
        """A banded joint of qGap - rGap = d whose path goes from column `left` over the columns `ways` (a stretch with a substitution down each) to `right`."""
        rng = self.rng
        left, right = (BW, BW - d) if d <= 0 else (BW + d, BW)
        for attempt in range(400):
            lo, hi = stretch if attempt < 200 else (5, 5)
            steps, cur = ([("m", head)] if head else []), left
            for c in list(ways) + [None]:
                to = right if c is None else c
                if to > cur:
                    steps.append(("d", to - cur))
                elif to < cur:
                    steps.append(("i", cur - to))
                cur = to
                if c is not None:
                    n = rng.randint(lo, hi)
                    steps += [("m", n // 2), ("s",), ("m", n - n // 2 - 1)]
            q = sum(s[1] if s[0] in "mi" else 1 for s in steps if s[0] != "d")
            r = sum(s[1] if s[0] in "md" else 1 for s in steps if s[0] != "i")
            t = tail
            if want_banded:
                while not banded_rule(q + t, r + t):
                    t += 1
            if t:
                steps.append(("m", t))
            if q + t > qmax or r + t > rmax:
                continue
            where = self.spot() if at is None and end_at is None else (at if at is not None else end_at - (r + t))
            query, rlen = self.apply(where, steps)
            assert rlen == r + t and len(query) == q + t
            self.add(fam, where, query, rlen, banded=True if want_banded else None, ways=tuple(ways), **more)
            return True
        return False

    def edited(self, fam, at, rlen, qlen, **more):
        """A joint of the given shape over the reference from `at`: a copy with the net gap in two places and, where there is room, a substitution."""
        rng, nib = self.rng, self.nib
        ref = [LETTERS[c] if c < 4 else rng.choice(LETTERS) for c in nib[at:at + rlen]]
        if qlen >= rlen:
            q, extra = list(ref), qlen - rlen
            a = extra - extra // 3 if more.get("one_run") is None else extra
            for n, pos in ((a, rng.randint(0, len(q))), (extra - a, rng.randint(0, len(q)))):
                q[pos:pos] = [rng.choice(LETTERS) for _ in range(n)]
        else:
            cut = rlen - qlen
            a = cut - cut // 3
            p1 = rng.randint(0, rlen - cut)
            q = ref[:p1] + ref[p1 + a:]
            p2 = rng.randint(0, len(q) - (cut - a))
            q = q[:p2] + q[p2 + (cut - a):]
        if len(q) >= 4:
            p = rng.randrange(len(q))
            q[p] = rng.choice([c for c in LETTERS if c != q[p]])
        assert len(q) == qlen
        self.add(fam, at, "".join(q), rlen, **more)


def build_items(nib, max_roff, seq_starts, tracts, nrun):
    B = Builder(nib, max_roff, seq_starts)
    rng = B.rng
    ht = [(0, 0), (4, 0), (0, 5), (3, 4), (6, 6), (0, 9)]                    # matches in front of the first gap / behind the last: 0 = the path leaves the origin
    k = 0                                                                    # (reaches the end cell) with a gap

    # 1. columns: every column of every band width, arriving by a deletion and by an insertion; from edge to edge
    for d in range(-13, 14):
        left, W = (BW if d <= 0 else BW + d), 2 * BW + abs(d) + 1
        for c in range(W):
            for arrive in "DI":
                if arrive == "D":
                    if c == 0:
                        continue                                             # (nothing lies left of column 0 to come from)
                    ways = [c] if left < c else [rng.randrange(0, c), c]
                else:
                    if c == W - 1:
                        continue
                    ways = [c] if left > c else [rng.randrange(c + 1, W), c]
                h, t = ht[k % len(ht)]; k += 1
                assert B.routed("columns", d, ways, h, t), (d, ways)
        for ways in ([0, W - 1], [W - 1, 0]):
            h, t = ht[k % len(ht)]; k += 1
            assert B.routed("columns", d, ways, h, t), (d, ways)
        # (a gap of one base costs what a substitution costs: the steps of one column at the strip's edges want long stretches to be the best path)
        for ways in ([W - 1, W - 2], [0, 1]):
            for h, t in ((0, 0), (5, 6)):
                assert B.routed("columns", d, ways, h, t, stretch=(9, 11)), (d, ways)
    # ... banded W = 25..32 (k_gap_lanes<32>) and W > 32 (k_gap_wave)
    for d in list(range(-21, -13)) + list(range(14, 22)):
        left, W = (BW if d <= 0 else BW + d), 2 * BW + abs(d) + 1
        n = 0
        for c in (0, W - 1, left, BW, rng.randrange(W), rng.randrange(W), rng.randrange(W), rng.randrange(W)):
            h, t = ht[k % len(ht)]; k += 1
            n += B.routed("columns32", d, [c], h, t)
        assert n >= 5, (d, n)
    for d in (-30, -25, -22, 22, 24):
        for c in (0, BW, 2 * BW + abs(d)):
            assert B.routed("columnsW", d, [c], 0, 3, qmax=62, rmax=75), d
    # ... the unbanded shapes: rLen <= 15 (k_gap_lanes<16>), 16..31 (<32>), 1..60 rows
    for rlen in list(range(1, 32)) * 3:
        choices = [q for q in range(1, 61) if not banded_rule(q, rlen) and (q, rlen) != (1, 1)]
        for qlen in (rng.choice(choices), rng.choice(choices[:6] + choices[-6:])):
            B.edited("full", B.spot(), rlen, qlen)

    # 2. limits
    for rep in range(3):
        for qlen in (1, 2, 3, 11, 12, 59, 60, 61):
            for rlen in (2, 12, 13, 63, 64, 65):
                B.edited("limits", B.spot(), rlen, qlen)
        for rlen in (2, 3, 5):                                               # one insertion run of 55 and more
            B.edited("limits", B.spot(), rlen, 60, one_run=True)
        # the smallest banded joints (their d = 0 ones with enough substitutions to need a DP: an insertion and a deletion apart)
        assert B.routed("limits", 0, [BW - 2], 2, 0, qmax=12, rmax=12, stretch=(5, 5))
        assert B.routed("limits", 0, [BW + 2], 1, 0, qmax=12, rmax=12, stretch=(5, 5))
        assert B.routed("limits", -1, [BW + 3], 0, 0, qmax=12, rmax=13)
        assert B.routed("limits", 1, [BW - 2], 0, 0, qmax=14, rmax=13)

    # 3. ties: gaps inside the tracts; two substitutions beside each other (decided under the second scoring)
    for n, (sk, pos, tl, unit) in enumerate(tracts[:84]):
        t0 = seq_starts[sk] + pos
        g = 1 + n % 6
        lead = rng.randint(3, 8)
        at = t0 - lead
        rlen = min(rng.randint(g + 16, 50), YD_GREF)
        inside = min(tl, rlen - lead)                                        # tract bases inside the piece
        if not (nib[at:at + rlen] < 4).all():
            continue
        ref = [LETTERS[c] for c in nib[at:at + rlen]]
        if n % 2 and inside > g + 2:                                         # the read has lost g tract bases
            p = lead + rng.randint(1, inside - g - 1)
            q = ref[:p] + ref[p + g:]
        else:                                                                # the read has g tract bases more
            p = lead + rng.randint(min(g, inside - 1), inside - 1)
            q = ref[:p] + [LETTERS[nib[t0 + (p - lead + i) % unit]] for i in range(g)] + ref[p:]
        if len(q) <= YD_GROWS and banded_rule(len(q), rlen):
            B.add("ties_tract", at, "".join(q), rlen, banded=True)
    for n in range(48):
        d = (1, -1, 2, -2, 3, -4)[n % 6]
        at = B.spot()
        pre, post = rng.randint(5, 9), rng.randint(6, 10)
        steps = [("m", pre), ("s",), ("s",), ("m", post), ("i", d) if d > 0 else ("d", -d), ("m", rng.randint(8, 14))]
        query, rlen = B.apply(at, steps if n % 4 < 2 else steps[::-1])
        B.add("ties_rr", at, query, rlen, banded=True)

    # 4. reference edges
    for at in range(5):
        for d in (-13, -7, -3, -1, 0, 1, 2, 6, 9, 13):
            left, W = (BW if d <= 0 else BW + d), 2 * BW + abs(d) + 1
            h, t = ht[k % len(ht)]; k += 1
            assert B.routed("edge_first", d, [rng.randrange(W)], h, t, at=at), (at, d)
    for d in list(range(-13, 14)) + [-20, 17]:
        W = 2 * BW + abs(d) + 1
        h, t = ht[k % len(ht)]; k += 1
        assert B.routed("edge_last", d, [rng.randrange(W)], h, t, end_at=max_roff), d
    n0 = seq_starts[nrun[0]] + nrun[1]
    for n in range(30):
        at = n0 - rng.randint(6, 30)
        if n % 3 == 0:                                                       # the read lacks the run
            steps = [("m", n0 - at), ("d", nrun[2]), ("m", rng.randint(8, 20))]
        elif n % 3 == 1:                                                     # the read has bases of its own there, and a gap beside
            steps = [("m", n0 - at + nrun[2] + 4), ("i", 1 + n % 5), ("m", rng.randint(8, 20))]
        else:
            steps = [("m", n0 - at - 3), ("d", 2 + n % 4), ("m", nrun[2] + rng.randint(8, 20))]
        query, rlen = B.apply(at, steps)
        B.add("edge_n", at, query, rlen)

    # 5. run caps (decided under -G 20 -I 8 and -I 20): deletions of 9..13 in one run, insertions past 20, the widest swings
    for d in range(-13, -8):
        for c_from in (0, 2, BW):
            ways = [] if c_from == BW else [c_from]                          # one deletion of 9..13, plus what brought the path left of the origin
            h, t = ht[k % len(ht)]; k += 1
            assert B.routed("caps", d, ways, h or 3, t or 3), (d, ways)
    # (a long run next to a run of the other kind is only the best path when the stretch between them is long: shorter ones let the inserted bases pair up
    # with the skipped ones)
    for d in (-13, -12, -11, 11, 12, 13, -1, 0, 1):
        left, W = (BW if d <= 0 else BW + d), 2 * BW + abs(d) + 1
        for ways in ([W - 1, W - 1 - 21], [W - 1, 0], [0, W - 1]) if W > 12 else ([0, W - 1], [W - 1, 0]):
            for h, t in ((0, 0), (2, 2)):
                assert B.routed("caps", d, ways, h, t, stretch=(12, 13)), (d, ways)
    return B


def solo_items(nib, max_roff, seq_starts):
    """The list for the wave-uniform ballot: in each of the classes of W <= 12 and W <= 16, fewer than 64 joints (one wave) of which ONE has qGap > 20."""
    B = Builder(nib, max_roff, seq_starts)
    B.place = max_roff // 2
    rng = B.rng
    for dset, big in (((-1, 0, 1), 0), ((-5, -4, -3, -2, 2, 3), -3)):
        for n in range(44):
            d = dset[n % len(dset)]
            left, W = (BW if d <= 0 else BW + d), 2 * BW + abs(d) + 1
            while not B.routed("solo", d, [rng.randrange(W)], 0, 0, qmax=20, stretch=(5, 5)):
                pass
        assert B.routed("solo_big", big, [2, 9], 6, 8, stretch=(8, 8))
    return B


def finish(B, seed):
    order = list(range(len(B.items)))
    random.Random(seed).shuffle(order)                                       # a wave holds unlike joints
    return [B.items[k] for k in order]


# ---- what takes a joint, and where its path runs -------------------------------------------------------------------------------------------------------
def packed(P):
    return 64 * max(P.MScore, P.RCost) + P.GOCost + 64 * P.GECost <= 12000


def classify(P, m, switch=None):
    """The kernel instance launchGapFills gives the joint to (k_dp_classify's shortcut, gapJointKey, gapBandPacked, the two switches)."""
    q, r, banded = m["q"], m["r"], m["banded"]
    if q == r and m["mm"] * (P.MScore + P.RCost) <= P.MScore + 2 * (P.GOCost + P.GECost):
        return "diag"
    W = 2 * P.bandWidth + abs(q - r) + 1 if banded else r + 1
    if q > YD_GROWS or r > YD_GREF or W > 32:
        return "wave"
    lim = banded and P.bandWidth >= 5 and P.maxGap >= 16
    pk = packed(P) and switch != "YGPU_GAP32"
    if lim and W <= 16:
        return ("band12" if W <= 12 else "band16") + ("" if pk else "_32bit")
    if lim and W <= 24 and pk and switch != "YGPU_GAP24_OFF":
        return "band24"
    return "lanes16" if W <= 16 else "lanes32"


def replay(P, m, ops):
    """(events, score): the trace cells the list's path reads, as (kind, column) with column x = left + (reference consumed - query consumed) -- for a gap the
    column of the cell that holds the run, where it ends -- and the list's score with a run charged one opening per started maxIntron / maxGap (a run that
    leaves the origin lies in the initialised row 0 or left edge, which know no caps: one opening)."""
    d = m["d"]
    x = BW if d <= 0 else BW + d
    ev, score, qi, ri = [], 0, 0, 0
    for k, (n, c) in enumerate(ops):
        if c in "MR":
            for _ in range(n):
                assert (m["qc"][qi] == m["rc"][ri]) == (c == "M"), (m, ops)
                ev.append((c, x)); qi += 1; ri += 1
            score += n * (P.MScore if c == "M" else -P.RCost)
        elif c == "D":
            x += n; ri += n; ev.append((c, x)); score -= (1 if k == 0 else -(-n // P.maxIntron)) * P.GOCost + n * P.GECost
        else:
            x -= n; qi += n; ev.append((c, x)); score -= (1 if k == 0 else -(-n // P.maxGap)) * P.GOCost + n * P.GECost
    assert qi == m["q"] and ri == m["r"], (m, ops)
    return ev, score


def gap_could_sit_later(m, ops):
    """a gap of the list with a match behind it whose base equals the gap's first: one position on, the same operations give the same score"""
    qi = ri = 0
    for (n, c), nxt in zip(ops, ops[1:] + ((0, "-"),)):
        if c == "D":
            if nxt[1] == "M" and m["rc"][ri] == m["rc"][ri + n]:
                return True
            ri += n
        elif c == "I":
            if nxt[1] == "M" and m["qc"][qi] == m["qc"][qi + n]:
                return True
            qi += n
        else:
            qi += n; ri += n
    return False


def check_coverage(params, lists, exp):
    """What the oracle's own results have to show, or the comparison proves nothing about the kernels' columns, classes and caps.  Returns the table of the summary."""
    report = {}
    P = params["main"]
    items = lists["all"]
    res = exp["main", "all"]
    # every list is a global alignment whose score is its operations' (and every parameter set's too)
    for (name, lname), rr in exp.items():
        for (_rd, _f, m), (score, _aq, _ar, ops) in zip(lists[lname], rr):
            assert replay(params[name], m, ops)[1] == score, (name, m["fam"], m["q"], m["r"], score, ops)
    # per band instance: every column, every kind of step, both halves, both kinds of row 0, both ways out of the origin
    seen = {g: {} for g in BAND}
    count = {}
    strands = set()
    for (_rd, _f, m), (_s, _aq, _ar, ops) in zip(items, res):
        cls = classify(P, m)
        count[cls] = count.get(cls, 0) + 1
        if -13 <= m["d"] <= 13 and m["banded"]:
            strands.add((m["d"], m["strand"]))
        if cls in BAND:
            S = seen[cls]
            for kind, col in replay(P, m, ops)[0]:
                S.setdefault(kind, set()).add(col)
            left = BW if m["d"] <= 0 else BW + m["d"]
            S.setdefault("row0", set()).add(left >= BAND[cls] // 2)
            S.setdefault("first", set()).add(ops[0][1])
    for g, GW in BAND.items():
        S = seen[g]
        assert S["M"] >= set(range(GW)) and S["R"] >= set(range(GW)), (g, sorted(S["M"]), sorted(S["R"]))
        # a deletion run ends right of where it began and an insertion run left of it: no cell of column 0 holds a D, none of column GW - 1 an I
        assert S["D"] >= set(range(1, GW)), (g, sorted(S["D"]))
        assert S["I"] >= set(range(GW - 1)), (g, sorted(S["I"]))
        assert S["row0"] == {False, True} and S["first"] >= {"D", "I", "M"}, (g, S["row0"], S["first"])
        report[g] = dict(joints=count[g], **{kk: "%d..%d" % (min(S[kk]), max(S[kk])) for kk in "MRDI"})
    assert strands == {(d, s) for d in range(-13, 14) for s in (0, 1)}
    # every class the dispatch can choose, by more than a wave (the slow wave kernel: 16); and the classes the switches and the packed range bring
    for cls in ("band12", "band16", "band24", "lanes16", "lanes32"):
        assert count.get(cls, 0) > 64, (cls, count)
    assert count.get("wave", 0) >= 16, count
    report["classes"] = dict(count)
    for name, switch in (("main", "YGPU_GAP32"), ("packed_past", None)):
        c2 = {}
        for (_rd, _f, m) in items:
            c = classify(params[name], m, switch); c2[c] = c2.get(c, 0) + 1
        assert c2.get("band12_32bit", 0) > 64 and c2.get("band16_32bit", 0) > 64 and "band24" not in c2, (name, switch, c2)
    c2 = sum(classify(P, m, "YGPU_GAP24_OFF") == "lanes32" and classify(P, m) == "band24" for (_rd, _f, m) in items)
    assert c2 > 64
    assert packed(params["packed_last"]) and not packed(params["packed_past"])
    assert 64 * max(params["packed_last"].MScore, params["packed_last"].RCost) + params["packed_last"].GOCost + 64 * params["packed_last"].GECost == 12000
    # limits: an insertion run of 55 and more, under the main scoring and at the end of the packed range; the shapes at and past the lane kernels' limits
    for name in ("main", "packed_last", "packed_past"):
        runs = [n for (_rd, _f, m), (_s, _aq, _ar, ops) in zip(items, exp[name, "all"]) if m["fam"] == "limits" for n, c in ops if c == "I"]
        assert max(runs) >= 55, (name, max(runs))
    shapes = {(m["q"], m["r"]) for (_rd, _f, m) in items if m["fam"] == "limits"}
    assert shapes >= {(q, r) for q in (1, 2, 3, 11, 12, 59, 60, 61) for r in (2, 12, 13, 63, 64, 65)} | {(12, 12), (12, 13), (14, 13)}
    assert {(m["q"], m["r"]) for (_rd, _f, m) in items if m["fam"] == "limits" and classify(P, m) == "band12"} >= {(12, 12), (12, 13), (14, 13)}
    Pl = params["packed_last"]
    assert min(sc for (_rd, _f, m), (sc, _aq, _ar, _o) in zip(items, exp["packed_last", "all"]) if m["fam"] == "limits") < -(Pl.GOCost + 55 * Pl.GECost)
    # ties
    tied = sum(gap_could_sit_later(m, ops) for (_rd, _f, m), (_s, _aq, _ar, ops) in zip(items, res) if m["fam"] == "ties_tract")
    assert tied >= 20, tied
    rr = 0
    for (_rd, _f, m), (_s, _aq, _ar, ops) in zip(items, exp["ties", "all"]):
        if m["fam"] == "ties_rr":
            pairs = list(zip(ops, ops[1:]))
            rr += (2, "R") in ops or ((2, "I"), (2, "D")) in pairs or ((2, "D"), (2, "I")) in pairs
    assert rr >= 20, rr
    report["ties"] = dict(tract=tied, two_substitutions=rr)
    # reference edges
    assert {m["at"] for (_rd, _f, m) in items if m["fam"] == "edge_first" and m["banded"]} == set(range(5))
    assert sum(m["banded"] and classify(P, m) in BAND for (_rd, _f, m) in items if m["fam"] == "edge_last") >= 20
    assert sum(any(c >= 4 for c in m["rc"]) for (_rd, _f, m) in items if m["fam"] == "edge_n") >= 20
    # run caps inside the band kernels: a run of the cap's length with another behind it shows as ONE operation longer than the cap (the traceback merges
    # equal neighbours) whose second opening the score carries (checked for every list above)
    for name, need in (("caps8", {("D", 12), ("D", 16), ("D", 24), ("I", 24)}), ("caps20", {("D", 24), ("I", 24)})):
        Pc, got = params[name], set()
        for (_rd, _f, m), (_s, _aq, _ar, ops) in zip(items, exp[name, "all"]):
            cls = classify(Pc, m)
            if cls in BAND:
                got |= {(c, BAND[cls]) for n, c in ops if n > (Pc.maxIntron if c == "D" else Pc.maxGap) and c in "DI"}
        assert got >= need, (name, sorted(got))
        if name == "caps8":
            assert any(m["fam"] == "caps" and any(c == "D" and 9 <= n <= 13 for n, c in ops) for (_rd, _f, m), (_s, _aq, _ar, ops) in zip(items, exp[name, "all"]))
        # the wave of one capped lane: per class one joint of qGap > maxGap among fewer than 64
        for g in ("band12", "band16"):
            js = [m for (_rd, _f, m) in lists["solo"] if classify(Pc, m) == g]
            assert 32 < len(js) < 64 and sum(m["q"] > Pc.maxGap for m in js) == 1, (name, g, len(js))
    return report


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def genome(work, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gapfills"))
    fa = os.path.join(d, "gf.fa")
    seqs, tracts, nrun = write_genome(fa)
    ya.build_index(["-g", fa, "-L", "11"])
    return d, os.path.join(d, "gf.X11_01_65525S"), seqs, tracts, nrun


@pytest.fixture(scope="module")
def cases(genome):
    """(index, {list: reads file}, {list: items}, {set: params}, {(set, list): the oracle's results}): made once for the module."""
    d, index, seqs, tracts, nrun = genome
    probe = os.path.join(d, "probe.fa")
    with open(probe, "w") as f:
        f.write(">p\n%s\n" % seqs[0][:100])
    with ya.Session(["-x", index, "-q", probe]) as s0:
        bases, _offs, _codes = batch_arrays(s0, s0.next_batch(1))
        nib = np.empty(2 * len(bases), np.uint8); nib[0::2] = bases >> 4; nib[1::2] = bases & 15
        max_roff = int(s0.index.maxROff)
    # the sequences lie one behind the other from offset 0, padding (codes above 4) between them; the last base of the last is the genome's last
    seq_starts, at = [], 0
    for sq in seqs:
        while nib[at] > 4:
            at += 1
        seq_starts.append(at)
        assert "".join(LETTERS[c] if c < 4 else "N" for c in nib[at:at + 50]) == sq[:50]
        at += len(sq)
    assert seq_starts[0] == 0 and at == max_roff and (nib[:5] < 4).all() and nib[max_roff - 1] < 4
    lists = {"all": finish(build_items(nib, max_roff, seq_starts, tracts, nrun), 7), "solo": finish(solo_items(nib, max_roff, seq_starts), 8)}
    files, params, exp = {}, {}, {}
    for lname, items in lists.items():
        files[lname] = os.path.join(d, lname + ".fa")
        with open(files[lname], "w") as f:
            for k, (read, _fields, _m) in enumerate(items):
                f.write(">j%d\n%s\n" % (k, read))
    for name, args in SETS.items():
        for lname, items in lists.items():
            with ya.Session(["-x", index, "-q", files[lname]] + args) as s:
                b = s.next_batch(len(items) + 1)
                assert b.n_reads == len(items)
                params[name] = s.params
                exp[name, lname] = oracle.dp_batch(s.index, s.params, b, [ya.DPProblem(k, *f) for k, (_rd, f, _m) in enumerate(items)])
    return index, files, lists, params, exp


def test_the_oracle_covers_every_column_class_and_cap(cases):
    _index, _files, lists, params, exp = cases
    report = check_coverage(params, lists, exp)
    print("problems: %d + %d" % (len(lists["all"]), len(lists["solo"])))
    for key, val in report.items():
        print("coverage", key, val)


def _compare(ctx, P, items, lo, hi, exp, kernels, what):
    res, ops, _nops = ctx.dp_batch([ya.DPProblem(k, *items[k][1]) for k in range(lo, hi)], kernels)
    bad = []
    for k in range(lo, hi):
        r = res[k - lo]
        got = (r.score, r.addedQLen, r.addedRLen, tuple((ops[r.op_start + j] & 0xFFFF, chr((ops[r.op_start + j] >> 16) & 0xFF)) for j in range(r.n_ops)))
        if got != exp[k]:
            m = items[k][2]
            bad.append((items[k][1], m["fam"], classify(P, m, what[1]), m["d"], m.get("ways"), got, exp[k]))
    for b in bad[:4]:
        print("MISMATCH %r kernels %d: problem %r family %s class %s d %d ways %r\n got %r\n exp %r" % ((what, kernels) + b))
    assert not bad, "%d of %d gap fills differ from the oracle (%r, kernel family %d)" % (len(bad), hi - lo, what, kernels)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SETS))
def test_gap_fills_bit_exact_in_every_column_class_and_cap(cases, name, monkeypatch):
    index, files, lists, params, exp = cases
    check_coverage(params, lists, exp)
    for lname, items in lists.items():
        with ya.Session(["-x", index, "-q", files[lname]] + SETS[name]) as s:
            b = s.next_batch(len(items) + 1)
            P, e = s.params, exp[name, lname]
            assert P.bandWidth == BW and P.maxGap >= 16
            with ya.Context(s.index, s.params) as ctx:
                ctx.upload(b)
                for kernels, switch in ((ya.DP_KERNELS_WAVE, None),) + tuple((ya.DP_KERNELS_LANES, sw) for sw in SWITCHES):
                    for sw in SWITCHES[1:]:
                        monkeypatch.delenv(sw, raising=False)
                    if switch:
                        monkeypatch.setenv(switch, "1")
                    what = (name + "/" + lname, switch)
                    _compare(ctx, P, items, 0, 40, e, kernels, what)                         # one small call
                    _compare(ctx, P, items, 0, len(items), e, kernels, what)                 # the whole list: full waves and a last one with dead lanes
                    _compare(ctx, P, items, 40, 90, e, kernels, what)                        # and a small call again on the same context


# ---- through the whole pipeline ------------------------------------------------------------------------------------------------------------------------
def write_short_indel_reads(seqs, out, n, seed):
    """Reads of about 300 bases with ONE indel -- a deletion of 6..13, a deletion of 14..21 or an insertion of 6..21 bases -- and, on either side of it, a
    substitution nine bases off and another nearer by: the seeds stop short, the exact-match extension stops at the outer substitutions, and the joint between the
    two fragments keeps 18 query bases -- a deletion of L leaves a BANDED joint (L + 11 < 18 + L) of W = 11 + L."""
    rnd = random.Random(seed)

    def sub(s, p):
        return s[:p] + rnd.choice([c for c in "ACGT" if c != s[p]]) + s[p + 1:]
    with open(out, "w") as f:
        for i in range(n):
            g = seqs[rnd.randrange(len(seqs))]
            kind = i % 4
            L = rnd.randint(6, 13) if kind < 2 else (rnd.randint(14, 21) if kind == 2 else rnd.randint(6, 21))
            fl, fr = rnd.randint(130, 170), rnd.randint(130, 170)
            a = rnd.randrange(1000, len(g) - 1000)
            left = g[a:a + fl]
            if kind < 3:
                mid, right = "", g[a + fl + L:a + fl + L + fr]
            else:
                mid, right = "".join(rnd.choice("ACGT") for _ in range(L)), g[a + fl:a + fl + fr]
            left = sub(sub(left, fl - 9), fl - rnd.randint(1, 8))
            right = sub(sub(right, 8), rnd.randint(0, 7))
            s = (left + mid + right).replace("N", "A")
            if rnd.random() < 0.5:
                s = "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(s))
            f.write(">ind_%d_%d_%d\n%s\n" % (kind, L, i, s))


@pytest.mark.gpu
def test_short_indel_reads_through_the_pipeline_under_every_switch(genome, monkeypatch):
    from test_gpu_parity import device_pipeline
    d, index, seqs, _tracts, _nrun = genome
    reads = os.path.join(d, "indel_reads.fa")
    write_short_indel_reads(seqs, reads, 320, 33)
    with ya.Session(["-x", index, "-q", reads]) as s:                        # (the exact-match extension takes as much off qGap as off rGap: W stays)
        probs = dp_problems_from_chain(s, s.next_batch(400), limit=1 << 30)
        w24 = sum(p.mode == ya.DP_BANDED and 17 <= 2 * BW + abs(p.qLen - p.rLen) + 1 <= 24 and p.qLen <= YD_GROWS and p.rLen <= YD_GREF for p in probs)
        w32 = sum(p.mode == ya.DP_BANDED and 25 <= 2 * BW + abs(p.qLen - p.rLen) + 1 <= 32 and p.qLen <= YD_GROWS and p.rLen <= YD_GREF for p in probs)
        print("joints from the oracle's chains: %d, banded W = 17..24: %d, W = 25..32: %d" % (len(probs), w24, w32))
        assert w24 > 64 and w32 > 16
    out = {}
    for switch in SWITCHES:
        for sw in SWITCHES[1:]:
            monkeypatch.delenv(sw, raising=False)
        if switch:
            monkeypatch.setenv(switch, "1")
        out[switch] = device_pipeline(index, reads, "-osh", [])              # (asserts records and work counters against oracle.run)
    assert out[None] == out["YGPU_GAP24_OFF"] == out["YGPU_GAP32"]
    for sw in SWITCHES[1:]:
        monkeypatch.delenv(sw, raising=False)
    device_pipeline(index, reads, "-osh", ["-G", "20", "-I", "8"])
