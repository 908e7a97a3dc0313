"""GPU tier: k_ext_rows_pk (ext_lanes_pk.h) at the edges of what surrounds its recurrence -- the stream windows, the reference's end, the refill schedule.

The packed rows kernel reads a query code and a reference base a pass from two per-lane shift registers that are refilled with aligned dwords every 8th
pass, excludes the columns left of the matrix in a problem's first ten rows, and feeds code 15 once the reference is used up.  The problems here are the
smallest at which any of that can go wrong, on genomes of a few kbp made for the purpose, forward and reverse, on both strands:
  * 1, 2, 7 .. 12, 16 and 17 rows (the strip's left columns become real over rows 1 .. 10; a refill every 8th pass; the record block's edge);
  * a reference that ends inside the strip: cut by the genome's end after 10 .. 30 bases on genomes of every length modulo 8 (so that the end falls before,
    at and behind the end of the window's first partial dword: 11 + c1 - 1, 11 + c1, 11 + c1 + 1 bases for every c1 = 1 .. 8), cut by offset 0 after
    10 .. 30 bases, and in the middle of a longer problem;  ten bases leave no query row at all: a zero-work problem, between real ones;
  * every start phase 0 .. 7 of the reference offset and of the query's position inside a dword of eight packed codes;
  * runs of N in the reference and in the query; a homopolymer and a dinucleotide tract with a gap whose place is a tie;
  * several hundred problems of 1 .. 200 rows in one call, shuffled, zero-work ones among them: every wave loads a pool, lanes finish in the middle of a
    block, the last waves drain;
  * a whole run (ygpu_run) of 16 000 short reads with the rows launch held to 64 workgroups: more extensions than lanes, so every lane takes one problem
    after another (shared blocks, the idle record slot), refill rounds of every size occur, the pool is reloaded and ends without a problem lie between
    the others; records, and the extension's calls, rows, cells and touched bases, against the oracle's.  (ygpu_dp_batch_ex sizes its launch by the
    problems, marks every problem valid and returns no rows or cells: these classes need the whole run.)
Score, both lengths (the row and the column of the maximum) and the edit list of every problem equal the oracle's, with the lane kernels and with their
careful instantiation.  Before anything is compared the ORACLE's results are checked for the classes the test is about."""
import os
import random

import numpy as np
import pytest

import oracle
import yaha_amd as ya
from problems import batch_arrays

pytestmark = pytest.mark.gpu

LETTERS = "TCAG"                      # the index's base codes 0..3
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
BAND = 10                             # columns left and right of the origin
# inside the packed kernel's limits (MS * longest read <= 15 000, RC + X + GO + 21 GE <= 4 000)
SCORING = ["-MS", "3", "-RC", "4", "-GOC", "3", "-GEC", "1", "-X", "40"]
ROWS = (1, 2, 7, 8, 9, 10, 11, 12, 16, 17)
END_BASES = tuple(range(10, 31))


def _rand(rng, n):
    return "".join(rng.choice(LETTERS) for _ in range(n))


def _other(rng, base):
    return rng.choice([c for c in LETTERS if c != base])


def _revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def make_genome(rng, tail):
    """~4.6 kbp: random sequence with a run of N, a homopolymer and a dinucleotide tract at known places; `tail` = its length modulo 8."""
    parts = [_rand(rng, 1000), "N" * 6, _rand(rng, 394), "A" * 80, _rand(rng, 320), "AC" * 40, _rand(rng, 2720 + tail)]
    g = "".join(parts)
    marks = {"n_run": 1000, "homo": 1400, "dinuc": 1800}
    assert len(g) % 8 == tail
    return g, marks


class Builder:
    """Collects reads and problems.  An extension consumes the reference upwards from r_off (forward) or downwards (reverse); its query is written in that order."""

    def __init__(self, genome, rng):
        self.g, self.rng, self.reads, self.probs = genome, rng, [], []

    def ref(self, rev, r_off, n):
        """n reference bases in consumption order (fewer at the genome's ends)."""
        return self.g[max(r_off - n + 1, 0):r_off + 1][::-1] if rev else self.g[r_off:r_off + n]

    def add(self, rev, r_off, query, kind, strand=0, phase=0):
        rng = self.rng
        query = query.replace("N", "A") if kind[0] != "query_n" else query
        pre = _rand(rng, phase)
        body = (pre + query[::-1]) if rev else (pre + query)
        body += _rand(rng, (-len(body)) % 8 + 8)                             # (every read a multiple of eight codes: the phase is the problem's own)
        q_off = phase + len(query) - 1 if rev else phase
        self.probs.append(((len(self.reads), strand, ya.DP_EXT_REV if rev else ya.DP_EXT_FWD, q_off, len(query), 0, r_off), kind))
        self.reads.append(_revcomp(body) if strand else body)               # (strand 1: the query lies on the read's reverse complement)

    def copy_of(self, rev, r_off, n, subst=()):
        q = list(self.ref(rev, r_off, n))
        q += list(_rand(self.rng, n - len(q)))                               # beyond the genome's end: anything
        for k in subst:
            if k < len(q) and q[k] in LETTERS:
                q[k] = _other(self.rng, q[k])
        return "".join(q)


def main_problems(genome, marks, rng):
    b = Builder(genome, rng)
    place = [2200]

    def spot(rev, n):
        at = place[0]; place[0] += 7                                         # (7: walks through every phase modulo 8)
        if place[0] > len(genome) - 500:
            place[0] = 2200
        return at + n + BAND if rev else at
    for strand in (0, 1):
        for rev in (False, True):
            for n in ROWS:                                                   # query length
                r_off = spot(rev, n)
                b.add(rev, r_off, b.copy_of(rev, r_off, n), ("rows", n), strand)
            for ph in range(8):                                              # start phases: reference offset and query offset, independently
                for qph in (ph, (ph + 3) % 8):
                    r_off = 2400 + 16 * ph + ph + (40 if rev else 0)
                    b.add(rev, r_off, b.copy_of(rev, r_off, 21, subst=(13,)), ("phase", r_off % 8, qph), strand, phase=qph)
    for rev in (False, True):
        # runs of N: in the reference (the query carries real bases there), and in the query
        r_off = marks["n_run"] + (25 if rev else -20)
        b.add(rev, r_off, b.copy_of(rev, r_off, 50), ("ref_n",))
        r_off = 3000 + (60 if rev else 0)
        q = b.copy_of(rev, r_off, 50); b.add(rev, r_off, q[:20] + "NNN" + q[23:], ("query_n",))
        # ties: a homopolymer with a base missing from the query, a dinucleotide tract with a unit missing; unique sequence behind both
        for name, unit in (("homo", 1), ("dinuc", 2)):
            r_off = marks[name] + (95 if rev else -15)
            q = b.copy_of(rev, r_off, 110)
            b.add(rev, r_off, q[:40] + q[40 + unit:], ("tie", name))
        # the reference ends in the middle of a longer problem (the genome's end going up, offset 0 going down)
        for n in (40, 45, 77):
            r_off = n - 1 if rev else len(genome) - n
            b.add(rev, r_off, b.copy_of(rev, r_off, 60, subst=(31,)), ("ref_end_mid", n))
        for n in END_BASES:                                                  # cut by offset 0 / the genome's end inside the first windows
            r_off = n - 1 if rev else len(genome) - n
            b.add(rev, r_off, b.copy_of(rev, r_off, 24), ("ref_end", n))
    # mixed lengths, 1 .. 200 rows, some with a substitution, and zero-work problems (ten reference bases: no row) between them
    for k in range(330):
        rev = bool(k & 1); n = 1 + (k * 37) % 200 if k % 5 else 1 + k % 9
        if k % 11 == 0:
            b.add(rev, 9 if rev else len(genome) - 10, _rand(rng, 12), ("zero",))
            continue
        r_off = 1500 + (k * 13) % 2000 + (n + BAND if rev else 0)
        b.add(rev, r_off, b.copy_of(rev, r_off, n, subst=(n // 2,) if k % 3 == 0 and n > 8 else ()), ("mixed", n), strand=(k >> 1) & 1, phase=k % 8)
    order = list(range(len(b.probs)))
    random.Random(5).shuffle(order)
    return [b.reads[k] for k in order], [((new,) + b.probs[k][0][1:], b.probs[k][1]) for new, k in enumerate(order)]


def end_problems(genome, rng):
    """The genome's end after 10 .. 30 bases, forward, and offset 0 going down; a few ordinary problems around them."""
    b = Builder(genome, rng)
    for n in END_BASES:
        b.add(False, len(genome) - n, b.copy_of(False, len(genome) - n, 24), ("ref_end", n))
        b.add(True, n - 1, b.copy_of(True, n - 1, 24), ("ref_end", n))
        b.add(bool(n & 1), 600 + 9 * n, b.copy_of(bool(n & 1), 600 + 9 * n, 9 + n), ("mixed", 9 + n))
    return b.reads, b.probs


def prepare(tmp, genome, reads):
    """index and read file of one genome: returns the session's arguments."""
    fa = os.path.join(tmp, "g.fa")
    with open(fa, "w") as f:
        f.write(">g\n")
        for k in range(0, len(genome), 60):
            f.write(genome[k:k + 60] + "\n")
    ya.build_index(["-g", fa, "-L", "11"])
    idx = [os.path.join(tmp, n) for n in os.listdir(tmp) if n.startswith("g.X11_")][0]
    path = os.path.join(tmp, "reads.fa")
    with open(path, "w") as f:
        for k, r in enumerate(reads):
            f.write(">q%d\n%s\n" % (k, r))
    return ["-x", idx, "-q", path] + SCORING


def oracle_results(args, genome, reads, probs):
    with ya.Session(args) as s:
        b = s.next_batch(len(reads) + 1)
        assert b.n_reads == len(reads)
        assert int(s.index.maxROff) == len(genome), "the reference clamp is not where the problems were built for"
        bases, offs, codes = batch_arrays(s, b)
        info = {"offs": np.array(offs), "codes": np.array(codes), "nib": np.stack([bases >> 4, bases & 15], 1).reshape(-1)[:len(genome)].copy()}
        return oracle.dp_batch(s.index, s.params, b, [ya.DPProblem(*f) for f, _k in probs]), info


def check_end_classes(probs, exp, genome_len):
    """a reference of n bases leaves n - 10 query rows: the oracle's extension has to run into that clamp, and ten bases leave nothing."""
    seen = {}
    for (f, kind), (score, aq, ar, ops) in zip(probs, exp):
        if kind[0] == "ref_end":
            n = kind[1]
            assert aq <= max(n - BAND, 0), (f, kind, (score, aq, ar))
            if n == BAND:
                assert (score, aq, ar, ops) == (0, 0, 0, ()), (f, kind, (score, aq, ar, ops))
            seen.setdefault((f[2], n), aq)
        if kind[0] == "zero":
            assert (score, aq, ar, ops) == (0, 0, 0, ())
    for mode in (ya.DP_EXT_FWD, ya.DP_EXT_REV):
        assert {n for (m, n) in seen if m == mode} == set(END_BASES)
        full = [n for (m, n), aq in seen.items() if m == mode and BAND < n <= 24 + BAND and aq == n - BAND]
        assert len(full) >= 8, ("the oracle's extensions stop short of the reference's end", mode, seen)


def check_main_classes(probs, exp, info, genome_len):
    check_end_classes(probs, exp, genome_len)
    rows = {}
    phases, tie_gaps, strands = set(), set(), set()
    for (f, kind), (score, aq, ar, ops) in zip(probs, exp):
        read, strand, mode, q_off, q_len, _rl, r_off = f
        if kind[0] == "rows":
            assert score > 0 and aq == kind[1], (f, kind, (score, aq, ar))
            rows.setdefault((strand, mode), set()).add(aq)
        elif kind[0] == "phase":
            assert score > 0 and aq == q_len
            nibble = int(info["offs"][read]) + q_off                          # (the strand's code array starts at the read's offset: q_off indexes it)
            phases.add((mode, r_off % 8, nibble % 8))
            strands.add(strand)
        elif kind[0] == "ref_n":
            lo, hi = (r_off - 49, r_off + 1) if mode == ya.DP_EXT_REV else (r_off, r_off + 50)
            assert (info["nib"][lo:hi] >= 4).sum() >= 6 and score > 0 and aq > 30, (f, (score, aq, ar, ops))
        elif kind[0] == "query_n":
            at = int(info["offs"][read])
            assert (info["codes"][at:at + 64] >= 4).sum() >= 3 and score > 0 and aq > 30, (f, (score, aq, ar, ops))
        elif kind[0] == "tie":
            assert score > 0 and aq == q_len, (f, kind, (score, aq, ar, ops))
            tie_gaps.add((kind[1], mode, bool({c for _n, c in ops} & set("ID"))))
        elif kind[0] == "ref_end_mid":
            top = min(q_len, kind[1] - BAND)                                 # (77 bases: all 60 rows, the last ones with columns beyond the end)
            assert score > 0 and top - 6 <= aq <= top, (f, kind, (score, aq, ar))
    for strand in (0, 1):
        for mode in (ya.DP_EXT_FWD, ya.DP_EXT_REV):
            assert rows[(strand, mode)] == set(ROWS), (strand, mode, rows)
    assert strands == {0, 1}
    for mode in (ya.DP_EXT_FWD, ya.DP_EXT_REV):
        assert {r for (m, r, _q) in phases if m == mode} == set(range(8)) and {q for (m, _r, q) in phases if m == mode} == set(range(8)), phases
        for name in ("homo", "dinuc"):
            assert (name, mode, True) in tie_gaps, tie_gaps
    lens = sorted(aq for (f, kind), (_s, aq, _ar, _o) in zip(probs, exp) if kind[0] == "mixed")
    assert len(probs) > 256 + 128 and lens[0] == 1 and lens[-1] >= 190 and len(set(lens)) > 100
    assert sum(1 for _f, kind in probs if kind[0] == "zero") >= 20


def compare(ctx, probs, exp, kernels):
    res, ops, _nops = ctx.dp_batch([ya.DPProblem(*f) for f, _k in probs], kernels)
    bad = []
    for k, e in enumerate(exp):
        r = res[k]
        got = (r.score, r.addedQLen, r.addedRLen, tuple((ops[r.op_start + j] & 0xFFFF, chr((ops[r.op_start + j] >> 16) & 0xFF)) for j in range(r.n_ops)))
        if got != e:
            bad.append((probs[k], got, e))
    for b in bad[:4]:
        print("MISMATCH kernels %d: %r\n got %r\n exp %r" % ((kernels,) + b))
    assert not bad, "%d of %d extensions differ from the oracle (kernel family %d)" % (len(bad), len(probs), kernels)


def run_device(args, probs, exp, kernels, slices):
    assert "YGPU_EXT32" not in os.environ                                    # (the packed family, not its 32-bit twin)
    with ya.Session(args) as s:
        b = s.next_batch(len(probs) + 1)
        assert s.params.bandWidth == 5 and s.params.maxGap >= 21 and s.params.maxIntron >= 21      # (the packed kernel's conditions)
        with ya.Context(s.index, s.params) as ctx:
            ctx.upload(b)
            for sl in slices:
                compare(ctx, probs[sl], exp[sl], kernels)


@pytest.fixture(scope="module")
def main_case(tmp_path_factory):
    rng = random.Random(11)
    genome, marks = make_genome(rng, 3)
    reads, probs = main_problems(genome, marks, rng)
    args = prepare(str(tmp_path_factory.mktemp("rows_edges")), genome, reads)
    exp, info = oracle_results(args, genome, reads, probs)
    return args, probs, exp, info, len(genome)


def test_the_oracle_shows_every_class(main_case):
    _args, probs, exp, info, glen = main_case
    check_main_classes(probs, exp, info, glen)


@pytest.mark.parametrize("kernels", [ya.DP_KERNELS_LANES, ya.DP_KERNELS_LANES_CAREFUL])
def test_rows_edges_bit_exact(main_case, kernels):
    args, probs, exp, info, glen = main_case
    check_main_classes(probs, exp, info, glen)
    # everything at once (more than 128 problems a launch, every wave with a pool of 64), then one wave's worth, then a handful on the same context
    run_device(args, probs, exp, kernels, [slice(None), slice(0, 70), slice(70, 75)])


@pytest.mark.parametrize("tail", range(8))
def test_reference_end_at_every_dword_phase(tmp_path, tail):
    rng = random.Random(100 + tail)
    genome, _marks = make_genome(rng, tail)
    reads, probs = end_problems(genome, rng)
    args = prepare(str(tmp_path), genome, reads)
    exp, _info = oracle_results(args, genome, reads, probs)
    check_end_classes(probs, exp, len(genome))
    run_device(args, probs, exp, ya.DP_KERNELS_LANES, [slice(None)])


# ---- the whole run: many more extensions than the rows launch has lanes ---------------------------------------------------------------------------------
ROWS_BLOCKS = 64                                                             # the smallest launch ygpu_run takes (YGPU_ROWS_BLOCKS): 64 workgroups of 256 lanes
RUN_COUNTERS = ("clumps_scored", "dp_ext_calls", "dp_ext_rows", "dp_ext_cells", "dp_gap_calls", "perfect_ext_bases", "ref_bases_touched", "ops_out")


def run_reads(genome, rng, n):
    """Short reads off the plain part of the genome: an exact core that holds the seeds, and at either end a piece of 0 .. 100 bases with a substitution every
    8th base -- no seed fits, so the piece is an X-drop extension of about that many rows (none where the piece is empty: an end without a problem)."""
    out = []
    for k in range(n):
        left, right = (rng.choice((0, 1, 2, 7, 8, 9, 12, 17, 30, 60, 100)) for _ in range(2))
        core = rng.randint(30, 50)
        a = rng.randrange(2000, len(genome) - 300)
        s = list(genome[a:a + left + core + right])
        for j in range(left - 1, -1, -8):
            s[j] = _other(rng, s[j])
        for j in range(left + core, len(s), 8):
            s[j] = _other(rng, s[j])
        s = "".join(s)
        out.append(_revcomp(s) if k & 1 else s)
    return out


@pytest.fixture(scope="module")
def run_case(tmp_path_factory):
    rng = random.Random(31)
    genome, _marks = make_genome(rng, 5)
    reads = run_reads(genome, rng, 16000)
    args = prepare(str(tmp_path_factory.mktemp("rows_run")), genome, reads)[:4]      # (default scoring: the benchmark's kernels)
    return args, len(reads)


def test_whole_run_with_more_extensions_than_lanes(run_case, monkeypatch):
    """ygpu_run with the rows launch held to 64 workgroups: every lane takes one problem after another (shared blocks, the idle record slot), refill rounds of
    every size occur, the pool is reloaded many times and the last waves drain; ends without a problem lie between the others.  Records and the
    extension's work counters -- calls, rows, cells, touched bases -- against the oracle's."""
    args, n_reads = run_case
    assert "YGPU_EXT32" not in os.environ
    monkeypatch.setenv("YGPU_ROWS_BLOCKS", str(ROWS_BLOCKS))
    with ya.Session(args) as s:
        b = s.next_batch(n_reads + 1)
        assert b.n_reads == n_reads
        assert s.params.bandWidth == 5 and s.params.maxGap >= 21 and s.params.maxIntron >= 21      # (the packed kernel's conditions)
        ro, _own = oracle.run(s.index, s.params, b, threads=8)
        exp = ro.counters.as_dict()
        print("oracle:", {k: exp[k] for k in RUN_COUNTERS})
        lanes = ROWS_BLOCKS * 256
        assert exp["dp_ext_calls"] > lanes + lanes // 4, "no more problems than lanes: no lane has to take a second one"
        assert exp["dp_ext_calls"] < 2 * exp["clumps_scored"], "every end has a problem: none is left out between the others"
        assert exp["dp_ext_rows"] > 20 * exp["dp_ext_calls"]                  # (long and short ones mixed)
        with ya.Context(s.index, s.params) as ctx:
            ctx.upload(b)
            ctx.run()
            r = ctx.collect()
            got = r.counters.as_dict()
            print("device:", {k: got[k] for k in RUN_COUNTERS})
            assert ya.result_records(r) == ya.result_records(ro), "device clump records differ from the oracle"
            for key in RUN_COUNTERS:
                assert got[key] == exp[key], (key, got[key], exp[key])
