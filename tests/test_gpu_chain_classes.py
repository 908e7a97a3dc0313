"""The chain stage (A3 + A4), region class by region class, against the oracle: reads built so that the oracle's regions hold every size at which the device
changes its copy of the algorithm, and every rule of the algorithm in every copy.

The device has five copies, chosen by k_region_classify (regions.h) from the region's fragment count: k_regions_single (1), k_chain_lanes<4|8|16> (2..4, 5..8,
9..16: chain_lanes.h), chainSmall (17..64), chainGeneral on LDS (65..512) and on the wave's HBM scratch (more than 512: chain.h).  The reads:

  ladders        an exact copy of a stretch but for n - 1 substitutions 12 bases or more apart: n fragments on one diagonal, n = every LADDER size
  indel ladders  the same with insertions and deletions of 1..maxGap bases between the stretches, and one step of maxGap + 1 in the middle (it splits the region)
  tandem repeats planted in the genome (units of 12..45 bases, 3..40 copies, some copies diverged), read with flanks, with another copy number, with
                 substitutions: fragments on diagonals a unit apart that overlap in the query -- ties, chops, second and third clumps, elimination.  A ladder in the flank
                 brings the same structure into each larger class
  short          (GADGETS) a stretch of 11 or 12 bases beside an insertion that ends in a copy of the bases before it: the chop leaves a fragment shorter than
                 wordLen at the head, at the tail and inside a chain, which is what the clean-up looks for; each behind a ladder of 0, 3, 8, 20, 70, 520 fragments
  tracts         short periodic tracts read with indels (TRACT_READS, psqo_read): a piece of the read on two diagonals at once -- the ties that the query gap
                 and the path's start decide; islands: 70 and 520 fragments of 12 bases with 32 substituted bases between them -- under -MD 30 a
                 large region whose best chain stays below minMatch, under the default -MD 50 ONE clump that the align stage splits once per island
  wrap           under -MS 4: an exact stretch of 8200 bases (score 32800) and 2, 19, 69 and 514 more fragments in its region
  strands        every read and its reverse complement

chain_model.py (a plain-Python model of the stage, equal to the oracle on all of this: test_chain_model.py) names the rules each region exercised;
test_the_oracles_regions_hold_every_class_edge_and_rule asserts the list on the ORACLE's fragments (needs no GPU).  The GPU tests then compare ygpu_seed_join,
ygpu_chain and ygpu_run with the oracle's, bit for bit, in one batch, read by read, in batches of 7, after a redo, and on two contexts in flight."""
import os
import random
import threading

import pytest

import chain_model as cm
import oracle
import yaha_amd as ya
from problems import batch_arrays
from test_gpu_phase1_lists import RC, Reads

LETTERS = "TCAG"
SETS = {"main": [], "wrap": ["-MS", "4"], "tight": ["-G", "12", "-MD", "30", "-M", "30"]}
LADDERS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 63, 64, 65, 511, 512, 513, 700)
EDGES = (1, 2, 4, 5, 8, 9, 16, 17, 64, 65, 512, 513)
LANES, BODIES = ("2-4", "5-8", "9-16"), ("lanes", "17-64", "65-512", ">512")
COUNTERS = ("fragments", "regions", "clumps_formed")
MAX_GAP, BW, WORD = 50, 5, 11                                               # the defaults (asserted on the Session's params)
N_LOCI = 36
TILE = 2048                                                                  # YD_REG_TILE (regions.h): a tile of k_region_scan; 64 = a row, 512 = a wave of it


# ---- the genome ----------------------------------------------------------------------------------------------------------------------------------------
def rand_seq(rng, n):
    return "".join(rng.choice(LETTERS) for _ in range(n))


def other(rng, c):
    return rng.choice([x for x in LETTERS if x != c])


def build_genome(path):
    """two sequences, seeded: 330 kbp of random bases (ladders), and the loci: a flank, a tandem repeat, a flank, one after the other.
    Returns ([sequences], [locus]); a locus = dict(at, pre, unit, copies, post)"""
    rng = random.Random(2024)
    plain = rand_seq(rng, 330000)
    loci, parts, at = [], [], 0
    for k in range(N_LOCI):
        unit = (12, 45, 13, 24, 31, 17, 12, 20, 38, 15, 27, 12)[k % 12] if k < 24 else rng.randint(12, 45)
        copies = (3, 6, 40, 10, 4, 25, 12, 5, 8, 33, 3, 18)[(k * 5) % 12] if k < 24 else rng.randint(3, 40)
        pre = 8300 if k % 3 == 0 else 1300
        u = rand_seq(rng, unit)
        body = [list(u) for _ in range(copies)]
        if k % 2:                                                            # diverged copies: one to three substitutions in a copy or two
            for _ in range(1 + k % 3):
                c = rng.randrange(copies)
                for _s in range(1 + rng.randrange(3)):
                    p = rng.randrange(unit)
                    body[c][p] = other(rng, body[c][p])
        rep = "".join("".join(c) for c in body)
        parts.append(rand_seq(rng, pre) + rep + rand_seq(rng, 400))
        loci.append(dict(at=at, pre=pre, unit=unit, copies=copies, post=400))
        at += len(parts[-1])
    seqs = [plain, "".join(parts), "".join("".join(tract_locus(i)) for i in sorted({t for t, _j in TRACT_READS})) + "".join(psqo_locus()) + "".join(covered_locus())]
    with open(path, "w") as f:
        for k, s in enumerate(seqs):
            f.write(">cc%d\n" % k)
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    return seqs, loci


# ---- short periodic tracts: where a piece of the read lies on two diagonals at once ------------------------------------------------------------------------
# Ties that the gap and the path's start decide (tie_gap_lose, tie_psqo_*) need two left nodes at the same distance in diagonal from a right node, on either
# side of it, that overlap in the query: a tract of period 2 g.  tract_locus(i) is a seeded tract and tract_read(i, j, 0) a seeded read over it (substitutions
# and indels inside the tract); TRACT_READS names the (tract, read) pairs that raise the events their comment names in a region of at most 12 fragments, and only
# their tracts are planted.  find_tract_reads() below is the search that found them (the model over the oracle's fragments), for the day a seed changes.  Each is there alone and with 20, 70 and 520 fragments of a ladder BEHIND it in the read, cut off from it by TRACT_DESERT substituted
# bases: more than maxDesert, so no chain joins the two, but on the same diagonal, so they are one region -- the same events in each larger class.
TRACT_POST, TRACT_DESERT = 9000, 60
TRACT_FILL = (0, 20, 70, 520)
TRACT_READS = ((280, 0),                                                     # tie_gap_lose (under -MS 4)
               (125, 7),                                                     # tie_gap_win
               (15, 12), (185, 3),                                           # tie_psqo_lose
               (185, 6),                                                     # tie_psqo_win
               (200, 2),                                                     # chop_equal_more
               (90, 8), (143, 9),                                            # chop_equal_single
               (10, 5), (17, 6),                                             # kept_end_free
               (3, 0),                                                       # best_tie_psqo, best_tie_eqo
               (63, 0), (150, 3))                                            # third_clump


def tract_locus(i):
    rng = random.Random(5000 + i)
    period = rng.choice((4, 5, 6, 8, 10, 12, 14))
    tract = list((rand_seq(rng, period) * 20)[:rng.randint(24, 70)])
    if i % 3 == 0:
        q = rng.randrange(len(tract))
        tract[q] = other(rng, tract[q])
    return rand_seq(rng, 300), "".join(tract), rand_seq(rng, TRACT_POST)


def tract_read(i, j, fill):
    pre, tract, post = tract_locus(i)
    rng = random.Random(70000 + 100 * i + j)
    body = list(tract)
    for _ in range(rng.randint(1, 3)):
        q, kind = rng.randrange(len(body)), rng.randrange(4)
        if kind == 0:
            body[q] = other(rng, body[q])
        elif kind == 1:
            del body[q:q + rng.randint(1, 16)]
        elif kind == 2:
            body[q:q] = list(rand_seq(rng, rng.randint(1, 16)))
        else:
            w = rng.randint(1, 16)
            body[q:q] = body[max(q - w, 0):q]
    m = rng.randint(15, 60)
    read = pre[len(pre) - rng.randint(15, 60):] + "".join(body) + post[:m]
    if fill:
        at = m
        read += "".join(other(rng, c) for c in post[at:at + TRACT_DESERT]); at += TRACT_DESERT
        for _ in range(fill):
            n = rng.randint(12, 14)
            read += post[at:at + n] + other(rng, post[at + n]); at += n + 1
        assert at < TRACT_POST
    return read


def find_tract_reads(workdir, n_tracts=300, n_reads=16, max_size=12, args=()):
    """the search behind TRACT_READS, kept for the day a seed or the index changes (no test calls it): plants tracts 0 .. n_tracts - 1 in a genome of their
    own, reads each with tract_read(i, j, 0) for j < n_reads, and returns {event: [(i, j), ...]} over the regions of at most max_size fragments -- the model
    over the oracle's fragments.  Run it once with args=() and once with args=("-MS", "4"), pick a pair per rare event, and let the coverage test judge."""
    fa, reads = os.path.join(workdir, "tracts.fa"), os.path.join(workdir, "tracts_reads.fa")
    with open(fa, "w") as f:
        f.write(">tracts\n" + "".join(pre + tract + post[:300] for pre, tract, post in map(tract_locus, range(n_tracts))) + "\n")
    pairs = [(i, j) for i in range(n_tracts) for j in range(n_reads)]
    with open(reads, "w") as f:
        for i, j in pairs:
            f.write(">t%d_%d\n%s\n" % (i, j, tract_read(i, j, 0)))
    ya.build_index(["-g", fa, "-L", "11"])
    found = {}
    with ya.Session(["-x", os.path.join(workdir, "tracts.X11_01_65525S"), "-q", reads] + list(args)) as s:
        _frags, (_clumps, regions) = run_model(s, s.next_batch(len(pairs) + 1))
    for r in regions:
        if 2 <= r.size <= max_size:
            for e in r.events:
                found.setdefault(e, []).append(pairs[r.rs >> 1])
    return found


def covered_locus():
    rng = random.Random(4250)
    return rand_seq(rng, 300), rand_seq(rng, 26) * 2, rand_seq(rng, 300)


def covered_read():
    """a unit of 26 bases twice in the genome, once in the read, 5 bases of the flank behind it: the flank before it with the unit is one fragment of 56 bases, the
    unit with the 5 bases another of 31 on a diagonal 26 away that brings too few new bases to pay for the gap -- a region of two, whose second fragment is long
    enough to stay but has both ends under the first one's clump (elim_covered in the class 2-4)"""
    pre, rep, post = covered_locus()
    return pre[-30:] + rep[:26] + post[:5]


def psqo_locus():
    rng = random.Random(4242)
    return rand_seq(rng, 300), rand_seq(rng, 6) * 7, rand_seq(rng, TRACT_POST)


def psqo_read(fill):
    """the read starts with the first 36 bases Z of a tract of period 6 and 42 bases: Z lies on the tract's diagonal d and on d + 6, both times as query [0, 35].
    Four bases that match nothing, then the flank from its second base on: a fragment R on d + 3, 4 query bases and 1 reference base behind Z.  Both copies of Z
    reach R with the same score at the same distance in diagonal and in query: the second loses on the path's start (tie_psqo_lose), and as the scan's first two
    nodes they tie for the best node with equal EQO (best_tie_psqo)."""
    _pre, tract, post = psqo_locus()
    rng = random.Random(4243)
    junk = [rng.choice([x for x in LETTERS if x not in (tract[36], post[0])]), rng.choice(LETTERS), rng.choice(LETTERS), other(rng, post[0])]
    read, at = tract[:36] + "".join(junk) + post[1:41], 41
    if fill:
        read += "".join(other(rng, c) for c in post[at:at + TRACT_DESERT]); at += TRACT_DESERT
        for _ in range(fill):
            n = rng.randint(12, 14)
            read += post[at:at + n] + other(rng, post[at + n]); at += n + 1
    return read


# ---- the reads -----------------------------------------------------------------------------------------------------------------------------------------
def ladder(rng, n, lo=12, hi=14):
    """n exact stretches of lo..hi bases with a substitution between one and the next (lo >= 11: each holds a seed)"""
    steps = []
    for k in range(n):
        if k:
            steps.append(("s",))
        steps.append(("m", rng.randint(lo, hi)))
    return steps


def both(items, cls, read):
    assert "N" not in read
    items.append((cls, read))
    items.append((cls, "".join(RC[c] for c in reversed(read))))


def locus_read(rng, seqs, L, fill, delta, subs, tail=60, cut=None):
    """a read across locus L: `fill` ladder fragments in the flank before the repeat, the repeat with `delta` copies more (> 0) or fewer than the genome, `subs`
    substitutions inside it, `tail` bases of the flank behind it.  cut = (unit index, bases): an indel inside the repeat that is no multiple of the unit."""
    g, u, c = seqs[1], L["unit"], L["copies"]
    r0 = L["at"] + L["pre"]                                                  # the repeat's first base
    head = []
    p = r0 - 30                                                              # 30 exact bases, then the ladder backwards
    for _ in range(fill):
        n = rng.randint(12, 14)
        head.append(g[p - n:p]); p -= n + 1
        head.append(other(rng, g[p]))
    head.append(g[p - 30:p])
    head = "".join(reversed(head)) + g[r0 - 30:r0]
    rep = g[r0:r0 + u * c]
    k = rng.randrange(1, c) if c > 1 else 0
    if delta > 0:
        rep = rep[:u * k] + rep[u * max(k - delta, 0):u * k] + rep[u * k:]
    elif delta < 0:
        rep = rep[:u * max(k + delta, 0)] + rep[u * k:]
    if cut:
        ku, nb = cut
        at = min(u * ku + u // 2, len(rep) - 1)
        rep = rep[:at] + (rand_seq(rng, nb) if nb > 0 else "") + rep[at + max(-nb, 0):]
    rep = list(rep)
    for _ in range(subs):
        q = rng.randrange(len(rep))
        rep[q] = other(rng, rep[q])
    return head + "".join(rep) + g[r0 + u * c:r0 + u * c + tail]


def plain_read(rng, ref, at, steps):
    """a read from ref[at:] by steps: ("m", n) exact bases, ("s",) a substitution, ("i", n) an insertion, ("d", n) a deletion, and ("w", g, w): an insertion of g
    bases that ends in a copy of the w bases before it -- the fragment behind it then starts w bases early in the reference and overlaps the one before it there,
    not in the query"""
    q, r = [], at
    for st in steps:
        if st[0] == "m":
            q.append(ref[r:r + st[1]]); r += st[1]
        elif st[0] == "s":
            q.append(other(rng, ref[r])); r += 1
        elif st[0] == "i":
            q.append("".join(other(rng, ref[r + i]) for i in range(st[1])))
        elif st[0] == "d":
            r += st[1]
        else:
            g, w = st[1], st[2]
            assert g > w
            junk = [rng.choice(LETTERS) for _ in range(g - w)]
            junk[0] = rng.choice([x for x in LETTERS if x != ref[r] and (g - w > 1 or x != ref[r - w - 1])])
            if g - w > 1:
                junk[-1] = other(rng, ref[r - w - 1])
            q.append("".join(junk) + ref[r - w:r])
    return "".join(q)


class PlainReads(Reads):
    """Reads of test_gpu_phase1_lists.py with plain_read's steps: each read from a fresh stretch of the first sequence, on both strands"""
    def add(self, cls, steps, lead=0, trail=0):
        body = [("m", lead)] + list(steps) + [("m", trail)]
        need = sum(st[1] if st[0] in "md" else (1 if st[0] == "s" else 0) for st in body)
        _k, a = self.spot(need + 40)
        both(self.items, cls, plain_read(self.rng, self.seqs[0], a + 20, body))


# the clean-up's rules need a fragment of the clump shorter than wordLen, which only a chop leaves: a 1- or 2-base ("w") overlap next to a stretch of 10 or 11 bases.
# With MScore 1 a fragment joins a chain over an indel of g bases only if it brings more than GOCost + g GECost new bases, so g is 1 or 2 where the short
# fragment must pay for itself; mid_kept needs two indels of more than BW bases about a fragment of at most 10 bases, which pays only under -MS 4 (the wrap set).
GADGETS = {                                                                  # name: (steps, the side of the filling ladder)
    "tail": ([("m", 40), ("w", 2, 1), ("m", 10)], "before"),
    "head": ([("m", 11), ("w", 2, 1), ("m", 40)], "after"),
    "equal_more": ([("m", 20), ("w", 2, 1), ("m", 19), ("s",), ("m", 30)], "before"),    # two fragments of 20 that overlap by one base, a third behind: chop_equal_more
    "mid_between": ([("m", 40), ("w", 6, 5), ("m", 6), ("s",), ("m", 30)], "before"),
    "mid_band": ([("m", 40), ("w", 2, 1), ("m", 10), ("d", 1), ("m", 30)], "before"),
    "mid_kept": ([("m", 40), ("w", 7, 1), ("m", 10), ("d", 6), ("m", 30)], "before"),
    "mid_far": ([("m", 200), ("w", 27, 6), ("m", 6), ("i", 26), ("m", 60)], "before"),
    "mid_far_tight": ([("m", 200), ("w", 8, 6), ("m", 6), ("i", 7), ("m", 60)], "before"),
}
GADGET_FILL = (0, 3, 8, 20, 70, 520)


FILL = {"lanes": 0, "17-64": 18, "65-512": 70, ">512": 520}


def build_reads(seqs, loci, name):
    items = []
    if name == "wrap":
        rng = random.Random(91)
        R = PlainReads(seqs, 92)
        for more in (2, 19, 69, 514):
            R.add("wrap_%d" % more, [("s",)] + ladder(rng, more), lead=8200, trail=0)
        for k in (2, 5, 7, 11):                                              # ... and behind a repeat: ties and chops beside a wrapped score
            L = loci[k]
            g = seqs[1]
            r0 = L["at"] + L["pre"]
            both(items, "wrap_rep_%d" % k, g[r0 - 1200:r0 + L["unit"] * L["copies"] + 60] )
        for gname, (steps, side) in GADGETS.items():
            for fill in GADGET_FILL if gname == "mid_kept" else GADGET_FILL[:5]:
                fl = ladder(rng, fill) + [("s",)] if fill else []
                R.add("%s_%d" % (gname, fill), steps + fl[::-1] if side == "after" else fl + steps, lead=0, trail=0)
        for i, j in TRACT_READS:
            for fill in TRACT_FILL:
                both(items, "tract%d_%d_%d" % (i, j, fill), tract_read(i, j, fill))
        for fill in TRACT_FILL:
            both(items, "psqo_%d" % fill, psqo_read(fill))
        return R.items + items
    rng = random.Random(90)
    R = PlainReads(seqs, 93)
    for n in LADDERS:
        for rep in range(2 if n in (512, 513, 64, 65) else 1):
            R.add("ladder_%d" % n, ladder(rng, n), lead=0, trail=0)
    for n in (4, 8, 16, 40, 140):                                            # indel ladders: the step of maxGap + 1 in the middle splits the region
        steps = []
        for k in range(n):
            if k == n // 2:
                steps.append(("d", MAX_GAP + 1) if n & 8 else ("i", MAX_GAP + 1))
            elif k:
                g = (1, 2, BW, BW + 1, 2 * BW, 2 * BW + 1, 12, 13, 30, MAX_GAP)[rng.randrange(10)] if k % 3 else rng.randint(1, 3)
                steps.append((rng.choice("id"), g))
            steps.append(("m", rng.randint(12, 30)))
        R.add("indel_%d" % n, steps, lead=0, trail=0)
    for gname, (steps, side) in GADGETS.items():                            # the clean-up's rules, in every class
        for fill in GADGET_FILL:
            fl = ladder(rng, fill) + [("s",)] if fill else []
            R.add("%s_%d" % (gname, fill), steps + fl[::-1] if side == "after" else fl + steps, lead=0, trail=0)
    for n in (70, 520):                                                      # islands: n fragments of 12 bases, 32 substituted bases between one and the next.  Under
        # -MD 30 no two join, and the region's best chain stays below minMatch; under the default -MD 50 they chain into ONE clump, which the align stage then splits
        # once per island -- a recursion 520 deep in the reference (the device: the save stack of align.h)
        R.add("islands_%d" % n, ([("m", 12)] + [("s",)] * 32) * n, lead=0, trail=0)
    items = R.items
    for i, j in TRACT_READS:
        for fill in TRACT_FILL:
            both(items, "tract%d_%d_%d" % (i, j, fill), tract_read(i, j, fill))
    for fill in TRACT_FILL:
        both(items, "psqo_%d" % fill, psqo_read(fill))
    both(items, "covered", covered_read())
    for k, L in enumerate(loci):                                            # tandem repeats, each brought into the classes by a ladder in the flank
        bodies = BODIES if k % 3 == 0 else BODIES[:3]
        for body in bodies:
            fill = FILL[body]
            if fill > (L["pre"] - 100) // 15:
                continue
            delta = (0, 1, -1, 2, -2)[(k + len(body)) % 5]
            subs = (0, 1, 2, 4)[(k // 2 + len(body)) % 4]
            cut = None if k % 4 else (1 + k % 3, (1, -2, 2 * BW, -BW, 7, -9)[k % 6])
            both(items, "rep%d_%s" % (k, body), locus_read(rng, seqs, L, fill, delta, subs, cut=cut))
    return items


# ---- the oracle's regions, through the model -------------------------------------------------------------------------------------------------------------
def body_of(size):
    c = cm.size_class(size)
    return "lanes" if c in LANES else c


def event_table(regions):
    """{body or lane class: {event: regions that raised it}}"""
    tab = {}
    for r in regions:
        if r.size < 2:
            continue
        for key in {body_of(r.size), cm.size_class(r.size)}:
            row = tab.setdefault(key, {})
            for e in r.events:
                row[e] = row.get(e, 0) + 1
    return tab


def print_table(title, tab):
    cols = [c for c in BODIES + LANES if c in tab]
    print(title)
    print("  %-22s" % "event" + "".join("%8s" % c for c in cols))
    for e in cm.EVENTS:
        print("  %-22s" % e + "".join("%8s" % (tab[c].get(e) or ".") for c in cols))


def run_model(s, b):
    _bases, offs, _codes = batch_arrays(s, b)
    lens = [int(offs[k + 1] - offs[k]) for k in range(b.n_reads)]
    frags = oracle.seed_join(s.index, s.params, b)
    return frags, cm.chain(s.params, frags, lens)


@pytest.fixture(scope="module")
def genome(work, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("chaincls"))
    fa = os.path.join(d, "cc.fa")
    seqs, loci = build_genome(fa)
    ya.build_index(["-g", fa, "-L", "11"])
    return d, os.path.join(d, "cc.X11_01_65525S"), seqs, loci


@pytest.fixture(scope="module")
def cases(genome):
    """{set: (reads file, number of reads, the oracle's fragments, the oracle's clumps, the model's regions)}: built once.  (That the model's clumps are the oracle's
    is asserted by the tests that rely on it: the coverage test here and test_chain_model.py.)"""
    d, index, seqs, loci = genome
    out = {}
    for name, args in SETS.items():
        items = build_reads(seqs, loci, name if name != "tight" else "main")
        path = os.path.join(d, "reads_%s.fa" % name)
        with open(path, "w") as f:
            for k, (cls, read) in enumerate(items):
                f.write(">%s_%d\n%s\n" % (cls, k, read))
        with ya.Session(["-x", index, "-q", path] + args) as s:
            b = s.next_batch(len(items) + 1)
            assert b.n_reads == len(items)
            if name == "main":
                assert (s.params.maxGap, s.params.bandWidth, s.params.wordLen) == (MAX_GAP, BW, WORD)
            frags, (clumps, regions) = run_model(s, b)
            assert clumps == model_clumps(regions)
            exp = oracle.chain(s.index, s.params, b)
        out[name] = (path, len(items), frags, exp, regions)
    return out


def model_clumps(regions):
    """the model's clumps, in creation order, from its regions"""
    return [(r.rs, c) for r in regions for c in r.clumps]


def first_difference(got, exp, regions):
    """the first clump that differs, with the region (read, strand, size, class, events) it belongs to"""
    k = next((i for i, (a, e) in enumerate(zip(got, exp)) if a != e), min(len(got), len(exp)))
    lines = ["%d clumps against %d expected, the first difference at clump %d" % (len(got), len(exp), k)]
    for who, seq in (("got", got), ("expected", exp)):
        if k < len(seq):
            reg = cm.region_of_clump(regions, seq[k])
            lines.append("%s %s\n    in %s" % (who, str(seq[k])[:400], reg.describe() if reg else "no region of the model"))
    return "\n".join(lines)


# trim_reused: a fragment that insertFragment cut at its back (subLenFromBack edits the fragment array) is a node of a later extraction of its region.  The
# reference's algorithm cannot raise it under these sets.  A fragment is cut only as a node of the extracted path.  Along a path SQO and EQO both rise strictly
# (the DP takes a pair only with lSQO < rSQO and at least one new base, and a left node that reaches beyond the right one's EQO leaves it none), the path's first
# node is never cut at its front and its last never at its back, so the clump's query span -- what setCoverage marks -- holds every node of the path, cut or not.
# The clean-up takes fragments out of the clump, but only inside the span or, at the head and the tail, fragments shorter than wordLen = 11; eliminateFragments
# then drops every unused fragment with EQO - SQO < minNonOverlap - 1 (24 and 29 here) and every one whose first and last minNonOverlap bases both touch the
# coverage: each node of the path is one or the other.  So no cut fragment is unused afterwards, in any body.  The model still looks for the event, and
# the test asserts that it never comes: if it did, this argument would be wrong.  (What the in-place edit does change on the device is a REDO of the stage on the
# same fragment array: test_redo_after_the_fragment_array_was_trimmed_in_place.)
IMPOSSIBLE = {"trim_reused"}


def check_coverage(cases):
    """the five requirements; returns the list of what is missing (empty: all there).  1 to 3 are asked of the main set.  4 and 5 are asked of the UNION of the
    three sets, as the issue allows: mid_kept, for one, pays only under -MS 4 and comes from the wrap set alone, third_clump in the lane classes from the main set
    alone -- every set goes through every GPU comparison that its name is a parameter of, and the main set through all of them."""
    missing = []
    _p, _n, _f, _e, regions = cases["main"]
    sizes = {}
    for r in regions:
        sizes.setdefault(r.size, set()).add(r.rs & 1)
    for n in EDGES:                                                          # 1. every size at which the copy changes, on both strands
        if sizes.get(n, set()) != {0, 1}:
            missing.append("no region of %d fragments on strands %s" % (n, sorted({0, 1} - sizes.get(n, set()))))
    for body in BODIES[1:]:                                                  # 2. a region of each large class across a tile boundary of k_region_scan
        if not any(body_of(r.size) == body and (r.end - 1) // TILE > r.start // TILE for r in regions):
            missing.append("no %s region spans a multiple of %d" % (body, TILE))
    for m in (64, 512):                                                      # 3. a region that starts a row, and one that starts a wave, of k_region_scan
        if not any(r.size > 1 and r.start > 0 and r.start % m == 0 and (m == 512 or r.start % 512) for r in regions):
            missing.append("no region starts at a multiple of %d%s" % (m, " that is none of 512" if m == 64 else ""))
    union = {}
    for name in SETS:
        for key, row in event_table(cases[name][4]).items():
            for e, c in row.items():
                union.setdefault(key, {})[e] = union.setdefault(key, {}).get(e, 0) + c
    for body in BODIES:                                                      # 4. every event in every body (score_wraps: in the wrap set, every body)
        for e in cm.EVENTS:
            if e in IMPOSSIBLE:
                assert not any(e in row for row in union.values()), e + " was raised: the argument above is wrong"
            elif e == "score_wraps":
                if not event_table(cases["wrap"][4]).get(body, {}).get(e):
                    missing.append("wrap set, %s: no %s" % (body, e))
            elif not union.get(body, {}).get(e):
                missing.append("%s: no %s" % (body, e))
    for c in LANES:                                                          # 5. each lane class by itself
        row = union.get(c, {})
        for what, names in (("second_clump", ["second_clump"]), ("chop", [e for e in cm.EVENTS if e.startswith("chop_")]), ("tie", [e for e in cm.EVENTS if e.startswith("tie_")]),
                            ("clean-up removal", ["mid_removed_between", "mid_removed_band", "head_removed", "tail_removed"]), ("elim_covered", ["elim_covered"]),
                            ("kept", ["kept_start_free", "kept_end_free"])):
            if not any(row.get(e) for e in names):
                missing.append("lane class %s: no %s" % (c, what))
    return missing, union


def test_the_oracles_regions_hold_every_class_edge_and_rule(cases):
    """the five requirements on the model's regions over the oracle's fragments; prints the class x event table of each set and of their union"""
    for name in SETS:
        path, n, frags, exp, regions = cases[name]
        assert model_clumps(regions) == exp, "chain_model differs from the oracle: " + first_difference(model_clumps(regions), exp, regions)
        print_table("set %s: %d reads, %d fragments, %d regions, %d clumps; regions that raised the event, by class" % (name, n, len(frags), len(regions), len(exp)),
                    event_table(regions))
    missing, union = check_coverage(cases)
    print_table("all sets", union)
    assert not missing, "%d requirements are not met:\n  " % len(missing) + "\n  ".join(missing)


# ---- the device against the oracle ---------------------------------------------------------------------------------------------------------------------------
def chain_tuples(ctx):
    cf, cs, crs, nc = ctx.chain()
    return [(crs[k], tuple((cf[i].startRefOff, cf[i].startQueryOff, cf[i].endQueryOff, cf[i].refLen) for i in range(cs[k], cs[k + 1]))) for k in range(nc)]


def compare_batch(ctx, s, b):
    """seed_join, chain and run of one uploaded batch against the oracle's; returns the number of clumps the chain stage formed"""
    exp_c = oracle.chain(s.index, s.params, b)
    f, n = ctx.seed_join()
    exp_f = oracle.seed_join(s.index, s.params, b)
    assert [(f[i].startRefOff, f[i].startQueryOff, f[i].endQueryOff, f[i].refLen, f[i].read_strand) for i in range(n)] == exp_f, "fragments differ from the oracle's"
    got_c = chain_tuples(ctx)
    if got_c != exp_c:
        _bases, offs, _codes = batch_arrays(s, b)
        _clumps, regions = cm.chain(s.params, exp_f, [int(offs[k + 1] - offs[k]) for k in range(b.n_reads)])
        raise AssertionError("the device's chains differ from the oracle's: " + first_difference(got_c, exp_c, regions))
    ctx.run()
    r = ctx.collect()
    ro, _own = oracle.run(s.index, s.params, b, threads=8)
    assert ya.result_records(r) == ya.result_records(ro), "device clump records differ from the oracle"
    got, exp = r.counters.as_dict(), ro.counters.as_dict()
    for key in COUNTERS:
        assert got[key] == exp[key], (key, got[key], exp[key])
    assert got["clumps_formed"] == len(exp_c)
    return len(exp_c)


def run_set(index, path, args, batch):
    n = 0
    with ya.Session(["-x", index, "-q", path] + args) as s:
        with ya.Context(s.index, s.params) as ctx:
            while True:
                b = s.next_batch(batch)
                if b.n_reads == 0:
                    break
                ctx.upload(b)
                compare_batch(ctx, s, b)
                n += 1
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SETS))
def test_each_set_in_one_batch(genome, cases, name):
    _d, index, _seqs, _loci = genome
    path, n, _frags, _exp, _regions = cases[name]
    assert run_set(index, path, SETS[name], n + 1) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SETS))
def test_each_set_read_by_read(genome, cases, name):
    """batches of one read: the class lists hold one region or a handful -- k_chain pops eight regions at a time and gets one, k_chain_big gets one, the lane
    kernels run a nearly empty wave"""
    _d, index, _seqs, _loci = genome
    path, n, _frags, _exp, _regions = cases[name]
    assert run_set(index, path, SETS[name], 1) == n


@pytest.mark.gpu
def test_the_main_set_in_batches_of_seven(genome, cases):
    _d, index, _seqs, _loci = genome
    path, n, _frags, _exp, _regions = cases["main"]
    assert run_set(index, path, SETS["main"], 7) == (n + 6) // 7


@pytest.mark.gpu
def test_redo_after_the_fragment_array_was_trimmed_in_place(genome, cases, monkeypatch):
    """under YGPU_CLUMP_BOUND=64 the batch overflows the first bound of the clump slots and the stage is done again, after chainGeneral has cut fragments of the
    large regions in the fragment array; then the same batch without the switch on the same context"""
    _d, index, _seqs, _loci = genome
    path, n, _frags, _exp, _regions = cases["main"]
    with ya.Session(["-x", index, "-q", path]) as s:
        b = s.next_batch(n + 1)
        with ya.Context(s.index, s.params) as ctx:
            monkeypatch.setenv("YGPU_CLUMP_BOUND", "64")
            ctx.upload(b)
            assert compare_batch(ctx, s, b) > 64
            monkeypatch.delenv("YGPU_CLUMP_BOUND")
            ctx.upload(b)
            compare_batch(ctx, s, b)


@pytest.mark.gpu
def test_the_main_set_on_two_contexts_in_flight(genome, cases):
    """two contexts of one process chain the set at the same time: a wave's arena chunks are reserved with atomics on its own context's counters"""
    _d, index, _seqs, _loci = genome
    path, n, _frags, _exp, _regions = cases["main"]
    errs = []

    def one():
        try:
            with ya.Session(["-x", index, "-q", path]) as s:
                b = s.next_batch(n + 1)
                with ya.Context(s.index, s.params) as ctx:
                    for _ in range(2):
                        ctx.upload(b)
                        compare_batch(ctx, s, b)
        except BaseException as e:                                           # (reported by the test's own thread)
            errs.append(e)
    th = [threading.Thread(target=one) for _ in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
