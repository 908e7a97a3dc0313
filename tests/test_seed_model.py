"""The seed stage's inputs (A1 + A2: stage_seed.hip, seed.h, segsort.h, wgsort.h, lookback.h), built so that the device meets every size at which it changes its
copy of the algorithm, and the proof -- on the model and the oracle, no GPU -- that they do.

seed_model.py (a plain model of the stage that keeps its intermediates) gives the same fragments as oracle.seed_join on every set below, on the golden reads and
on a few thousand short random reads; the fragments it calls dead can be dropped without changing a clump (chain_model.py on both arrays); and
test_the_inputs_reach_every_seed_stage_edge asserts, edge by edge, what the sets reach.  test_gpu_seed_edges.py then runs the same sets on the device.

The genome (seeded, about 110 kbp, indexed with -L 11 and -L 12 by this repository's indexer):
  seq 0  twelve G (code 3: the k-mer that hashes LAST, so its list ends ROA), 300 unique bases, a block X of 2 000 bases copied 26 times between unique
         spacers, 48 kbp of unique bases
  seq 1  a tandem repeat of period 5, 2 000 bases, between unique flanks;  seq 2  one of period 16
The sets (SETS): ladder, deep, wrap, link, two tiny batches, the four hit-count batches, the -H pair, the read lengths and the batch of 65 536 reads; each
builder says what it is for.  Reads are placed with the MODEL's hit counts (chance hits are counted, not assumed away), so a set that stops reaching an edge
-- another seed, another index -- fails the coverage test by name.

One edge is reached under one of the deep set's two limits only: a first-cut piece that holds a single diagonal needs a segment of more hits than the limit
on one diagonal and none elsewhere, and under a limit of 700 the chance hits of a read that long make that unreachable in a genome this size.  Under 64 the
reads of 85 bases give it."""
import os
import random

import numpy as np
import pytest

import chain_model as cm
import oracle
import seed_model as sm
import yaha_amd as ya

LETTERS = "TCAG"                                                             # the index's base codes 0..3
CODE = {c: k for k, c in enumerate(LETTERS)}
RC = {"T": "A", "A": "T", "C": "G", "G": "C"}
WORD, COPIES, XLEN, SPACER, LEAD, UNIQ = 11, 26, 2000, 150, 300, 48000
X0 = 12 + LEAD                                                               # the first copy of X
U0 = X0 + COPIES * (XLEN + SPACER)                                           # the unique bases behind the copies
LADDER_TARGETS = tuple(sorted({1, 63, 64, 65, 15873, 24576, 24577, 49152, 49153} | {hi + d for hi in sm.CLASS_HI for d in (-1, 0, 1)}))
LADDER_LOW_MAX = 12000                                                       # a second limit for the ladder set: 12 288 / 12 289 hits then take the long-segment path
DEEP_LIMITS = (64, 700)
HIT_COUNTS = (1, 8191, 8192, 8193)


def revcomp(s):
    return "".join(RC[c] for c in reversed(s))


def rand_seq(rng, n):
    """n random bases without a run of six G (so that no twelve G arise where pieces meet)"""
    out = []
    for _ in range(n):
        c = rng.choice(LETTERS)
        if c == "G" and out[-5:] == ["G"] * 5:
            c = "T"
        out.append(c)
    return "".join(out)


def other(rng, c):
    return rng.choice([x for x in LETTERS if x != c])


def build_genome(path):
    rng = random.Random(3301)
    X = rand_seq(rng, XLEN)
    s0 = "G" * 12 + "T" + rand_seq(rng, LEAD - 1) + "".join(X + rand_seq(rng, SPACER) for _ in range(COPIES)) + rand_seq(rng, UNIQ)
    s1 = rand_seq(rng, 500) + "CATGA" * 400 + rand_seq(rng, 500)
    s2 = rand_seq(rng, 500) + "TCCAGATTGCAAGTCA" * 125 + rand_seq(rng, 500)
    assert s0[X0:X0 + XLEN] == X and s0[U0 - SPACER - XLEN:U0 - SPACER] == X and s0.find("G" * 11, 2) < 0
    with open(path, "w") as f:
        for k, s in enumerate((s0, s1, s2)):
            f.write(">sd%d\n" % k)
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    return [s0, s1, s2], X


def make_batch(reads):
    """a ygpu_read_batch of the reads (the host's encoding: code = place in LETTERS) and the arrays it points into"""
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    codes = np.frombuffer("".join(reads).translate(str.maketrans(LETTERS, "\0\1\2\3")).encode("latin-1"), dtype=np.uint8).copy()
    if not len(codes):
        codes = np.zeros(1, dtype=np.uint8)
    return ya.ReadBatch(len(reads), codes.ctypes.data, offs.ctypes.data), (codes, offs)


class SeedSet:
    """one batch: its reads, the session that gives its index and params, and -- worked out once -- the model's view and the oracle's fragments"""

    def __init__(self, name, reads, session, args=(), limits=(sm.SEGSORT_MAX,), index=None):
        self.name, self.reads, self.s, self.args, self.limits, self.index = name, reads, session, list(args), limits, index
        self.batch, self._keep = make_batch(reads)
        self._model = self._oracle = None
        self._cov = {}

    @property
    def lens(self):
        return [len(r) for r in self.reads]

    @property
    def model(self):
        if self._model is None:
            self._model = sm.Batch(sm.Index(self.s.index), self.s.params, self._keep[0], self._keep[1])
        return self._model

    @property
    def oracle_frags(self):
        if self._oracle is None:
            self._oracle = oracle.seed_join(self.s.index, self.s.params, self.batch)
        return self._oracle

    def coverage(self, seg_max=sm.SEGSORT_MAX):
        if seg_max not in self._cov:
            self._cov[seg_max] = sm.Coverage(sm.Index(self.s.index), self.model, seg_max)
        return self._cov[seg_max]


# ---- placing reads by the model's counts ---------------------------------------------------------------------------------------------------------------------
class Counter:
    """hit counts of single reads under one index and params"""

    def __init__(self, session):
        self.ix, self.P = sm.Index(session.index), session.params

    def strands(self, read):
        codes = [CODE[c] for c in read]
        return [sm.strand_model(self.ix, self.P, sm.strand_codes(codes, st), st) for st in (0, 1)]

    def kmer_counts(self, read):
        """the hits every k-mer of the read's forward strand brings (a k-mer's count does not depend on what follows it in the read)"""
        out = [0] * max(len(read) - self.ix.word + 1, 0)
        for i, s, cnt in sm.kept_kmers(self.ix, self.P, [CODE[c] for c in read])[0]:
            out[i] = sm.effective_list(self.ix, i, s, cnt)[0]
        return out

    def total(self, read):
        return sum(self.kmer_counts(read)) + sum(self.kmer_counts(revcomp(read)))


def ladder_read(cnt, X, uniq, target, tail_at):
    """a prefix of X and a unique tail whose forward strand has exactly `target` hits: about 26 a base inside X, about one a base in the tail"""
    a = min(XLEN, 10 + target // COPIES + 1)
    while a >= 0:
        read = X[:a] + uniq[tail_at:tail_at + 150]
        total = 0
        for i, c in enumerate(cnt.kmer_counts(read)):
            total += c
            if total == target and i + WORD >= a:
                return read[:i + WORD]
            if total > target:
                break
        a -= 1
    raise AssertionError("no ladder read of %d hits" % target)


def build_ladder(cnt, seqs, X):
    """segments that fill a shape of the workgroup sort exactly, one short of full and one past it, for each of the twelve shapes; 15 873 and the sizes at
    which k_seg_split changes its bucket count; segments of 1 and 63..65 hits.  Every other read is reverse-complemented: the segment is then its strand 1."""
    uniq = seqs[0][U0:]
    reads = []
    for k, t in enumerate(LADDER_TARGETS):
        r = ladder_read(cnt, X, uniq, t, 1000 + 37 * k)
        reads.append(revcomp(r) if k & 1 else r)
    return reads


def build_deep(cnt, seqs, X):
    """under YGPU_SEGSORT_MAX = 64 and 700: exact reads of 1 kbp (one diagonal above the limit: the copy of a one-diagonal piece), exact reads of 85 bases
    (under 64 the whole segment is one diagonal: a first-cut piece of one diagonal), reads inside the tandem repeats (tens of neighbouring diagonals above
    the limit: several levels of k_seg_split_range) and a read across the start of the genome behind 40 junk bases (wrapped diagonals in a long segment: the
    clamp of k_seg_split)"""
    rng = random.Random(3302)
    s0, s1, s2 = seqs
    reads = [s0[U0 + 3000:U0 + 4000], revcomp(s0[U0 + 9000:U0 + 10000]), s0[U0 + 15000:U0 + 15800]]
    reads += [s0[U0 + a:U0 + a + 85] for a in (20000, 21000, 22000, 23000)] + [s0[U0 + a:U0 + a + 760] for a in (24000, 26000)]
    reads += [s1[700:1700], s2[804:1804], revcomp(s2[1000:1500])]
    reads.append(rand_seq(rng, 40) + s0[:1000])
    return reads


def build_wrap(cnt, seqs, X):
    """a junk prefix of p bases, then the first bases of the first sequence: every k-mer's query offset exceeds its reference offset, so its diagonal wraps;
    the unique ones' whole lists wrap (the walk goes on into the next list), the twelve G's list is the last of ROA (the walk meets the array's end)"""
    rng = random.Random(3303)
    reads = []
    for p in (1, 40, 5000):
        r = rand_seq(rng, p) + seqs[0][:200]
        reads += [r, revcomp(r)]
    # ... and behind 2 100 junk bases nearly the whole of X: more than 49 152 hits, sixteen buckets in k_seg_split, the first copy's diagonals wrap into the last
    r = rand_seq(rng, 2100) + X[:1990]
    return reads + [r, revcomp(r)]


def isolated(cnt, rng, seqs, gaps=()):
    """a read of junk that carries 11-base matches, each flanked by mismatches (a single hit): the first at a seeded place, the next ones so that their diagonals
    lie gaps[k] behind the one before.  Retried until the model finds exactly these hits in the read and nothing else."""
    s0 = seqs[0]
    while True:
        a = U0 + rng.randrange(2000, UNIQ - 4000)
        read, q, places = [], 20, []
        read.append(rand_seq(rng, 19) + other(rng, s0[a - 1]))
        places.append((a, q))
        read.append(s0[a:a + WORD])
        for g in gaps:
            fill = rng.randint(3, 9)
            q2 = q + WORD + fill
            b = a + (q2 - q) + g                                             # diag(b) = b - q2 = diag(a) + g
            read.append(other(rng, s0[a + WORD]) + rand_seq(rng, fill - 2) + other(rng, s0[b - 1]))
            read.append(s0[b:b + WORD])
            places.append((b, q2))
            a, q = b, q2
        read.append(other(rng, s0[a + WORD]) + rand_seq(rng, 19))
        read = "".join(read)
        S0, S1 = cnt.strands(read)
        if S0.sorted == sorted((ro - q, q) for ro, q in places) and not S1.hits:
            return read, places


class LinkBuilder:
    """a batch whose hits are counted as it grows, so that a read's hit can be put on a chosen multiple of 64, 512 or 8 192 of the batch-wide hit order"""

    def __init__(self, cnt, seqs, seed):
        self.cnt, self.seqs, self.rng, self.reads, self.H = cnt, seqs, random.Random(seed), [], 0

    def add(self, read):
        self.reads.append(read)
        self.H += self.cnt.total(read)

    def filler(self, take):
        """an exact read with `take` hits on its two strands together"""
        s0 = self.seqs[0]
        for _ in range(200):
            a, n = U0 + self.rng.randrange(100, UNIQ - 9000), take + WORD - 1
            for _fit in range(8):
                if n < WORD or n > 8900:
                    break
                h = self.cnt.total(s0[a:a + n])
                if h == take:
                    self.reads.append(s0[a:a + n])
                    self.H += take
                    return
                n -= h - take
        raise AssertionError("no filler of %d hits" % take)

    def pad(self, target):
        assert target >= self.H, (target, self.H)
        while self.H < target:
            need = target - self.H
            self.filler(need if need <= 7000 else 6000)

    def place(self, level, read, mark):
        """the read behind fillers, so that the hit `mark` of its own sorted hits is the first behind a multiple of `level` (and of no larger level)"""
        B = (self.H + mark) // level * level
        while B < self.H + mark or (level == sm.ROW and B % sm.WAVE == 0) or (level == sm.WAVE and B % sm.TILE == 0):
            B += level
        self.pad(B - mark)
        self.add(read)
        return B


def build_link(cnt, seqs, X):
    """what links a hit to its neighbours, at every kind of boundary of k_frag_scan_build: random reads (their chance hits are the dead singles), two isolated
    hits exactly maxGap diagonals apart (both kept) and maxGap + 1 apart (both dead), exact reads; fillers bring each of the five BOUNDARY_EVENTS onto a
    multiple of 64, of 512 and of 8 192 hits.  Short reads from inside X give the set more kept fragments than a context's array holds after a tiny batch
    (seed_model.frag_room_after): behind one, the set is written as far as the room goes and run again."""
    G = cnt.P.maxGap
    L = LinkBuilder(cnt, seqs, 3304)
    rng = L.rng
    s0 = seqs[0]
    for _ in range(150):
        L.add(rand_seq(rng, 100))
    for _ in range(230):                                                     # 26 kept fragments each: more than the array holds after a tiny batch
        a = rng.randrange(XLEN - 30)
        L.add(X[a:a + 30])
    for level in (sm.ROW, sm.WAVE, sm.TILE):
        a = U0 + rng.randrange(100, UNIQ - 500)
        exact = s0[a:a + 60]                                                 # frag_across: hit 25 of a fragment of 50 is the first behind the boundary
        S0, _S1 = cnt.strands(exact)
        L.place(level, exact, S0.sorted.index((a, 25)))
        pair, _places = isolated(cnt, rng, seqs, gaps=(G + 1,))             # dead_before (and behind): the boundary between two singles maxGap + 1 apart
        L.place(level, pair, 1)
        single, _places = isolated(cnt, rng, seqs)                           # dead_behind, with the (read, strand) before it ending on the boundary
        L.place(level, single, 0)
        a = U0 + rng.randrange(100, UNIQ - 500)
        L.place(level, s0[a:a + 40], 0)                                      # rs_change
        pair, _places = isolated(cnt, rng, seqs, gaps=(G,))                  # near_not_joined: two singles exactly maxGap apart, one on each side
        L.place(level, pair, 1)
        a = U0 + rng.randrange(100, UNIQ - 500)
        broken = s0[a:a + 30] + other(rng, s0[a + 30]) + s0[a + 31:a + 61]   # ... and two fragments of one diagonal
        S0, _S1 = cnt.strands(broken)
        L.place(level, broken, S0.sorted.index((a, 31)))
        trio, _places = isolated(cnt, rng, seqs, gaps=(G, G + 1))            # kept, kept, dead in one (read, strand)
        L.add(trio)
    return L.reads


def build_hit_count(n):
    def build(cnt, seqs, X):
        L = LinkBuilder(cnt, seqs, 3305 + n)
        if n == 1:
            L.add(isolated(cnt, L.rng, seqs)[0])
        else:
            L.pad(n)
        assert L.H == n
        return L.reads
    return build


def build_exact2(cnt, seqs, X):
    """two exact reads of 30 bases: a tiny batch whose fragments are KEPT (the one fragment of the one-hit batch is a dead single, so with the drop on that
    batch leaves a fresh context's array empty)"""
    s0 = seqs[0]
    return [s0[U0 + 700:U0 + 730], revcomp(s0[U0 + 1700:U0 + 1730])]


def build_maxhits(cnt, seqs, X):
    """a stretch of X whose every k-mer has exactly 26 hits: all kept under -H 26, all dropped under -H 25"""
    counts = cnt.kmer_counts(X)
    for a in range(len(counts) - 40):
        if all(c == COPIES for c in counts[a:a + 40]):
            return [X[a:a + 50], revcomp(X[a:a + 50])]
    raise AssertionError("no stretch of X whose k-mers all have %d hits" % COPIES)


def build_lengths(cnt, seqs, X):
    """reads of wordLen - 1, wordLen and 32 000 bases (the largest query offset of a hit: 31 989, the largest end of a fragment: 31 999), each on both strands"""
    s0 = seqs[0]
    reads = [s0[U0 + 100:U0 + 110], s0[U0 + 200:U0 + 211], s0[U0 + 5000:U0 + 37000]]
    return reads + [revcomp(r) for r in reads]


def build_many(cnt, seqs, X):
    """65 536 reads of about 30 bases; the last ones come from the genome, on both strands, so that (read, strand) 131 071 -- all seventeen key bits set -- has hits"""
    rng = random.Random(3306)
    bases = "".join(rng.choice(LETTERS) for _ in range(65536 * 31 + 64))
    reads, at = [], 0
    for k in range(65536 - 64):
        n = 28 + (k & 3)
        reads.append(bases[at:at + n]); at += n
    for k in range(64):
        a = U0 + 400 * k
        r = seqs[0][a:a + 30 + (k & 3)]
        reads.append(revcomp(r) if k & 1 else r)
    return reads


# name: (builder, session arguments, the limits of the workgroup sort it is run under, the index's word length)
SETS = {
    "ladder": (build_ladder, [], (sm.SEGSORT_MAX, LADDER_LOW_MAX), 11),
    "deep": (build_deep, [], DEEP_LIMITS, 11),
    "wrap": (build_wrap, [], (sm.SEGSORT_MAX,), 11),
    "wrap12": (build_wrap, [], (sm.SEGSORT_MAX,), 12),
    "link": (build_link, [], (sm.SEGSORT_MAX,), 11),
    "link_M11": (build_link, ["-M", "11"], (sm.SEGSORT_MAX,), 11),
    "exact2": (build_exact2, [], (sm.SEGSORT_MAX,), 11),
    "hits1": (build_hit_count(1), [], (sm.SEGSORT_MAX,), 11),
    "hits8191": (build_hit_count(8191), [], (sm.SEGSORT_MAX,), 11),
    "hits8192": (build_hit_count(8192), [], (sm.SEGSORT_MAX,), 11),
    "hits8193": (build_hit_count(8193), [], (sm.SEGSORT_MAX,), 11),
    "H26": (build_maxhits, ["-H", "26"], (sm.SEGSORT_MAX,), 11),
    "H25": (build_maxhits, ["-H", "25"], (sm.SEGSORT_MAX,), 11),
    "lengths": (build_lengths, [], (sm.SEGSORT_MAX,), 11),
    "many": (build_many, [], (sm.SEGSORT_MAX,), 11),
}
SETS_KEY = pytest.StashKey()


@pytest.fixture(scope="session")
def seedsets(request, work, tmp_path_factory):
    """{name: SeedSet}.  Built once a run and kept with pytest's config, since test_gpu_seed_edges.py imports this fixture and a fixture counts once for every
    module that names it.  The sessions stay open until the run ends: the sets' params and index views are theirs."""
    stash = request.config.stash
    if SETS_KEY not in stash:
        stash[SETS_KEY] = build_sets(request.config, str(tmp_path_factory.mktemp("seedsets")))
    return stash[SETS_KEY]


def build_sets(config, d):
    fa = os.path.join(d, "sd.fa")
    seqs, X = build_genome(fa)
    index = {}
    for L in (11, 12):
        ya.build_index(["-g", fa, "-L", str(L)])
        index[L] = os.path.join(d, "sd.X%d_01_65525S" % L)
    dummy = os.path.join(d, "one.fa")
    with open(dummy, "w") as f:
        f.write(">one\n%s\n" % seqs[0][U0:U0 + 50])
    sessions, built, sets = {}, {}, {}
    for name, (builder, args, limits, L) in SETS.items():
        key = (L, tuple(args))
        if key not in sessions:
            sessions[key] = ya.Session(["-x", index[L], "-q", dummy] + args)
            config.add_cleanup(sessions[key].close)
        s = sessions[key]
        assert s.params.wordLen == L
        if builder not in built:                                             # (the reads are placed under the defaults at -L 11, whatever the set is run with)
            built[builder] = builder(Counter(sessions[(11, ())]), seqs, X)
        sets[name] = SeedSet(name, built[builder], s, args, limits, index[L])
    return sets


def first_difference(got, exp, what):
    k = next((i for i, (a, e) in enumerate(zip(got, exp)) if a != e), min(len(got), len(exp)))
    return "%s: %d fragments against %d, the first difference at %d: %r against %r" % (what, len(got), len(exp), k, got[k:k + 1], exp[k:k + 1])


# ---- the model against the oracle ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_the_model_equals_the_oracle_on_the_built_sets(seedsets, name):
    S = seedsets[name]
    assert S.model.frags == S.oracle_frags, first_difference(S.model.frags, S.oracle_frags, name)
    ro, _own = oracle.run(S.s.index, S.s.params, S.batch, threads=8)
    got = ro.counters.as_dict()
    assert (got["hits"], got["fragments"], got["kmer_lookups"]) == (S.model.n_hits, len(S.model.frags), S.model.lookups)


def session_batch_model(s, b):
    from problems import batch_arrays
    _bases, offs, codes = batch_arrays(s, b)
    return sm.Batch(sm.Index(s.index), s.params, codes, offs), [int(offs[k + 1] - offs[k]) for k in range(b.n_reads)]


@pytest.mark.parametrize("reads,extra", [("r1k.fa", []), ("rchim.fa", ["-H", "20"]), ("r100.fa", [])])
def test_the_model_equals_the_oracle_on_the_golden_reads(work, index11, reads, extra):
    with ya.Session(["-x", index11, "-q", os.path.join(work, reads)] + extra) as s:
        b = s.next_batch(150)
        m, lens = session_batch_model(s, b)
        exp = oracle.seed_join(s.index, s.params, b)
        assert len(exp) > 300 and m.frags == exp, first_difference(m.frags, exp, reads)
        assert_dead_is_safe(s.params, exp, m, lens)


def test_the_model_equals_the_oracle_on_random_short_reads(work, index11, tmp_path):
    """copies of stretches of the golden genome with substitutions, indels and runs of N, on both strands, 11 to 150 bases"""
    from problems import read_fasta
    rng = random.Random(3307)
    _names, seqs = read_fasta(os.path.join(work, "genome_small.fa"))
    path, n = os.path.join(str(tmp_path), "short.fa"), 3000
    with open(path, "w") as f:
        for k in range(n):
            g = seqs[rng.randrange(len(seqs))]
            a = rng.randrange(len(g) - 200)
            r = list(g[a:a + rng.randint(11, 150)])
            for _ in range(rng.randrange(4)):
                p = rng.randrange(len(r))
                r[p:p + rng.randrange(2)] = rng.choice(("A", "C", "G", "T", "N", "NNN", "", "ACGTTGCA"))
            f.write(">s%d\n%s\n" % (k, "".join(r) if len(r) >= 11 else g[a:a + 40]))
    with ya.Session(["-x", index11, "-q", path]) as s:
        b = s.next_batch(n + 1)
        assert b.n_reads == n
        m, lens = session_batch_model(s, b)
        exp = oracle.seed_join(s.index, s.params, b)
        assert len(exp) > 3000 and m.frags == exp, first_difference(m.frags, exp, "short reads")
        assert_dead_is_safe(s.params, exp, m, lens)


# ---- dropping the dead fragments changes no clump -------------------------------------------------------------------------------------------------------------
def assert_dead_is_safe(P, oracle_frags, model, lens):
    assert model.frags == oracle_frags
    whole, _regions = cm.chain(P, oracle_frags, lens)
    kept, _regions = cm.chain(P, [f for f, d in zip(oracle_frags, model.dead) if not d], lens)
    assert whole == kept, "dropping the model's dead fragments changes the clumps"
    if P.wordLen >= P.minMatch:
        assert not any(model.dead)


@pytest.mark.parametrize("name", list(SETS))
def test_dropping_the_dead_fragments_changes_no_clump(seedsets, name):
    S = seedsets[name]
    assert_dead_is_safe(S.s.params, S.oracle_frags, S.model, S.lens)


# ---- what the sets reach --------------------------------------------------------------------------------------------------------------------------------------
def diag_counts(S):
    out = {}
    for d, _q in S.hits:
        out[d] = out.get(d, 0) + 1
    return out


def missing_edges(sets):
    """the coverage list, edge by edge: the names of what the sets no longer reach (empty: all there)"""
    miss = []

    def need(ok, what):
        if not ok:
            miss.append(what)
    # ladder: the twelve shapes filled exactly, one short and one past; the bucket steps of k_seg_split
    lad = sets["ladder"]
    cov = lad.coverage()
    sizes = {}
    for rs, n in cov.seg_hits.items():
        sizes.setdefault(n, set()).add(rs)
    for t in LADDER_TARGETS:
        need(t in sizes, "ladder: no segment of %d hits" % t)
    need({rs & 1 for t in LADDER_TARGETS if t > 1024 for rs in sizes.get(t, ())} == {0, 1}, "ladder: long segments on both strands")
    for n, nb in ((15873, 4), (24576, 4), (24577, 8), (49152, 8), (49153, 16)):
        need(any(cov.plans[rs]["nb"] == nb for rs in sizes.get(n, ()) if rs in cov.plans), "ladder: %d hits cut into %d buckets" % (n, nb))
    low = lad.coverage(LADDER_LOW_MAX)
    for n, nb in ((12288, 2), (12289, 4)):
        need(any(low.plans[rs]["nb"] == nb for rs in sizes.get(n, ()) if rs in low.plans), "ladder under a limit of %d: %d hits cut into %d buckets" % (LADDER_LOW_MAX, n, nb))
    # deep: levels of k_seg_split_range, one-diagonal pieces at the first cut, at an even and at an odd level, wrapped diagonals clamped into the last bucket
    deep = sets["deep"]
    for limit in DEEP_LIMITS:
        cov = deep.coverage(limit)
        need(max(cov.max_on_diag.values()) > limit, "deep, limit %d: no diagonal holds more than the limit" % limit)
        need(any(len(p["levels"]) >= 3 for p in cov.plans.values()), "deep, limit %d: no segment needs three levels of k_seg_split_range" % limit)
        copies = {lv & 1 for p in cov.plans.values() for lv in p["copies"]}
        need(copies == {0, 1}, "deep, limit %d: one-diagonal pieces at even and at odd levels (found %s)" % (limit, sorted(copies)))
        need(any(p["clamped"] and p["nb"] > 1 for p in cov.plans.values()), "deep, limit %d: no wrapped diagonal clamped into the last of several buckets" % limit)
        crowded = [rs for rs in cov.plans if sum(1 for n in diag_counts(deep.model.strands[rs]).values() if n > limit) >= 20]
        need(crowded, "deep, limit %d: no segment with twenty diagonals above the limit (a tandem repeat)" % limit)
    need(any(p["first_single"] for limit in DEEP_LIMITS for p in deep.coverage(limit).plans.values()), "deep: no first-cut piece of one diagonal")
    # wrap: wrapping diagonals, lists that wrap whole, the end of ROA; at -L 11 (the bit table of k_kmer_lookup exact) and -L 12 (it aliases)
    for name in ("wrap", "wrap12"):
        cov = sets[name].coverage()
        need(cov.wrapped > 0, name + ": no hit whose diagonal wraps")
        need(cov.all_wrap > 0 and cov.foreign > 0, name + ": no k-mer whose whole list wraps (entries of the next list)")
        need(cov.clamped > 0, name + ": no walk that meets the end of ROA")
        need(any(p["nb"] == 16 and p["clamped"] for p in cov.plans.values()), name + ": no wrapped diagonal clamped into the last of sixteen buckets")
        for p, r in zip((1, 40, 5000), sets[name].reads[::2]):
            need(len(r) == p + 200, name + ": prefix of %d" % p)
    need(sets["wrap12"].s.params.wordLen == 12, "wrap12: an index of -L 12 (4^12 k-mers on the 2^22 bits of the table)")
    # link: the five events at the three kinds of boundary; kept and dead pairs
    link = sets["link"]
    cov = link.coverage()
    for level in (sm.ROW, sm.WAVE, sm.TILE):
        for e in sm.BOUNDARY_EVENTS:
            need(cov.events.get((level, e)), "link: no %s at a multiple of %d" % (e, level))
    G = link.s.params.maxGap
    pairs = {"kept": 0, "dead": 0, "half": 0}
    for S in link.model.strands:
        for k in range(len(S.frags) - 1):
            if S.nhits[k] == 1 and S.nhits[k + 1] == 1:
                gap = ((S.frags[k + 1][0] - S.frags[k + 1][1]) - (S.frags[k][0] - S.frags[k][1])) & sm.U32
                if gap == G and not S.dead[k] and not S.dead[k + 1]:
                    pairs["kept"] += 1
                if gap == G + 1 and S.dead[k] and S.dead[k + 1]:
                    pairs["dead"] += 1
                if gap == G + 1 and S.dead[k + 1] and not S.dead[k]:
                    pairs["half"] += 1
    need(pairs["kept"] >= 3, "link: two single hits exactly maxGap diagonals apart, both kept")
    need(pairs["dead"] >= 3, "link: two single hits maxGap + 1 diagonals apart, both dead")
    need(pairs["half"] >= 3, "link: a single hit maxGap + 1 behind one that a third keeps alive")
    need(sum(link.model.dead) > 100, "link: fewer than a hundred dead singles")
    need(not any(sets["link_M11"].model.dead) and len(sets["link_M11"].model.frags) == len(link.model.frags), "link under -M 11: every fragment kept")
    for n in HIT_COUNTS:
        need(sets["hits%d" % n].model.n_hits == n, "a batch of %d hits" % n)
    # the fragment array's room: the link set behind a tiny batch does not fit, with every fragment kept and with the dead ones dropped
    tiny, two = sets["hits1"], sets["exact2"]
    need(len(tiny.model.frags) == 1 and len(tiny.model.kept) == 0, "hits1: one fragment, a dead single")
    need(len(link.model.frags) > sm.frag_room_after(len(tiny.model.frags)), "link: more fragments than the array holds after the one-hit batch")
    need(0 < len(two.model.kept) < 100 and len(link.model.kept) > sm.frag_room_after(len(two.model.kept)),
         "link: more kept fragments than the array holds after the two exact reads")
    # small edges
    need(sets["H26"].coverage().at_max >= 80 and sets["H26"].model.n_hits >= 80 * COPIES, "-H 26: k-mers with exactly maxHits hits, kept")
    need(sets["H25"].coverage().over_max >= 80 and sets["H25"].model.n_hits == sets["H26"].model.n_hits - 80 * COPIES, "-H 25: k-mers with maxHits + 1 hits, dropped")
    ln = sets["lengths"]
    need(sorted(set(ln.lens)) == [WORD - 1, WORD, 32000], "lengths: reads of 10, 11 and 32 000 bases")
    need(ln.coverage().max_qo == 32000 - WORD and ln.coverage().max_eqo == 31999, "lengths: query offset 31 989 and fragment end 31 999")
    need(all(ln.coverage().seg_hits.get(rs, 0) == 0 for rs in (0, 1, 6, 7)) and ln.coverage().seg_hits.get(2) == 1 and ln.coverage().seg_hits.get(9) == 1,
         "lengths: no hit from 10 bases, one from 11")
    many = sets["many"]
    need(len(many.reads) == 65536 and many.coverage().max_rs == 131071, "many: (read, strand) 131 071 has hits")
    need(many.coverage().seg_hits.get(131071, 0) >= 20 and many.coverage().seg_hits.get(131068, 0) >= 20, "many: exact reads on both strands among the last")
    return miss


def test_the_inputs_reach_every_seed_stage_edge(seedsets):
    for name in SETS:
        S = seedsets[name]
        print("%-9s %6d reads %7d hits %6d fragments %6d dead" % (name, len(S.reads), S.model.n_hits, len(S.model.frags), sum(S.model.dead)))
    for limit in DEEP_LIMITS:
        cov = seedsets["deep"].coverage(limit)
        print("deep, limit %d: levels %r; plans %r" % (limit, cov.cut_levels, {rs: (p["nb"], p["first_single"], p["levels"], sorted(set(p["copies"]))) for rs, p in cov.plans.items()}))
    miss = missing_edges(seedsets)
    assert not miss, "%d edges are not reached:\n  " % len(miss) + "\n  ".join(miss)


@pytest.mark.parametrize("name,edge", [("ladder", "ladder: no segment of 15872 hits"), ("link", "link: two single hits maxGap + 1 diagonals apart, both dead"),
                                       ("link", "link: more kept fragments than the array holds after the two exact reads"),
                                       ("wrap", "wrap: no walk that meets the end of ROA"), ("deep", "deep: no first-cut piece of one diagonal")])
def test_a_set_without_its_construction_fails_by_the_edges_name(seedsets, name, edge):
    """the coverage list names what is lost: each set once without the reads that bring the named edge"""
    S = seedsets[name]
    if name == "ladder":
        reads = [r for r, t in zip(S.reads, LADDER_TARGETS) if t != 15872]
    elif name == "link" and "array holds" in edge:
        reads = [r for r in S.reads if len(r) != 30]                         # (without the short reads from inside X)
    elif name == "link":
        cov = S.coverage()
        B = cov.events[(sm.TILE, "dead_before")]
        owners = {rs >> 1 for rs, base in cov.seg_base.items() for b in B if base <= b - 1 < base + cov.seg_hits[rs]}
        reads = [r for k, r in enumerate(S.reads) if k not in owners]
    elif name == "wrap":
        reads = [r[:-200] + r[-188:] if k % 2 == 0 else r[:188] + r[200:] for k, r in enumerate(S.reads[:6])] + S.reads[6:]     # (without the twelve G)
    else:
        reads = [r for r in S.reads if len(r) != 85]
    less = dict(seedsets)
    less[name] = SeedSet(name, reads, S.s, S.args, S.limits, S.index)
    assert edge in missing_edges(less)
