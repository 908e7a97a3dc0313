"""Phase 1's edit lists, root class by root class, against the oracle: reads built by planting edits between exact seeds, so that the oracle's chains hold every kind
of root the two phase-1 kernels tell apart (phase_lanes.h).

k_p1_roots finishes a root that has no DP joint by itself -- one fragment, or joints of one op (D, I, R) or a pure diagonal whose ops come from a 64-bit mismatch
mask -- and leaves the others to k_p1_assemble, which takes them from a compact list after the gap fills.  The classes:

  single    roots of one fragment
  one-op    roots whose joints are all R, all D, all I
  diagonal  an equal-length gap of every g from 2 up to what the scoring's shortcut admits with stretches too short for a seed; the gap's first and last base
            differ (the exact-match extensions stop there), and one variant has two mismatches side by side (run merging in put)
  long      under -G 200 and cheap mismatches: diagonals of 63, 64, 65 and 100 bases (the mask, its last bit, the path without a mask)
  DP        joints whose op lists have exactly 13, 14 and 15 ops (the joint record holds 14), short and long ones, odd and even, and (under -G 200) a short
            list with an op longer than the record's length field: a deletion of 70
  mixed     a DP joint, a diagonal and one-op joints in one root
  ends      end extensions that reach read offset 0, the read's last base, reference offset 0 and the genome's last base, and end extensions of length zero
  strands   every class on both
  batches   fewer than 64 roots, and 64 k + 1 (partial waves in the compact list)

test_the_oracles_chains_hold_every_class asserts all this on the ORACLE's chains (needs no GPU); the GPU tests then compare ygpu_run with oracle.run: records,
and the work counters including gap calls, rows, cells and touched bases."""
import os
import random

import numpy as np
import pytest

import oracle
import yaha_amd as ya
from problems import COMP as CODE_COMP, batch_arrays
from test_gpu_gap_fills import LETTERS, write_genome

RC = {"T": "A", "A": "T", "C": "G", "G": "C"}
SETS = {"main": [], "cheap": ["-RC", "1", "-GOC", "9", "-GEC", "3", "-G", "200", "-MD", "200"]}
SWITCHES = (None, "YGPU_GAP32", "YGPU_GAP24_OFF")
COUNTERS = ("kmer_lookups", "hits", "fragments", "regions", "clumps_formed", "clumps_scored", "dp_ext_calls", "dp_gap_calls", "dp_gap_rows", "dp_gap_cells", "splits",
            "ops_out", "perfect_ext_bases", "ref_bases_touched")
N_INLINE = 14                                                                # YD_JINL (phase_lanes.h)
SEED_GAP = 10                                                                # the longest exact stretch that holds no seed at -L 11


def other(rng, c):
    return rng.choice([x for x in LETTERS if x != c])


def diag_steps(g, k, adjacent=False):
    """an equal-length gap of g bases with k substitutions: the first and the last base, the rest spread; adjacent: the second base too"""
    pos = {0, g - 1} if g > 1 else {0}
    if adjacent and g > 2:
        pos.add(1)
    inner = sorted(round((g - 1) * i / (k - 1)) for i in range(1, k - 1)) if k > 2 else []
    pos |= set(inner)
    steps, run = [], 0
    for t in range(g):
        if t in pos:
            if run:
                steps.append(("m", run)); run = 0
            steps.append(("s",))
        else:
            run += 1
    assert run == 0
    return steps


def min_subs(g):
    """the fewest substitutions with which diag_steps leaves no exact stretch that could hold a seed"""
    k = 2 if g > 1 else 1
    while max([st[1] for st in diag_steps(g, k) if st[0] == "m"] or [0]) > SEED_GAP:
        k += 1
    return k


class Reads:
    def __init__(self, seqs, seed):
        self.seqs, self.rng, self.items, self.at = seqs, random.Random(seed), [], 2100

    def spot(self, need):
        """a stretch of plain bases in the first sequence, clear of its tracts' neighbourhood by chance only: the oracle is the judge of what came out"""
        s = self.seqs[0]
        while True:
            a = self.at; self.at += need + 37
            assert a + need + 100 < len(s), "the genome is used up"
            if "N" not in s[a:a + need]:
                return 0, a

    def add(self, cls, steps, where=None, lead=40, trail=40):
        rng = self.rng
        body = [("m", lead)] + list(steps) + [("m", trail)]
        need = sum(st[1] if st[0] in "md" else (1 if st[0] == "s" else 0) for st in body)
        k, a = where(need) if where else self.spot(need)
        ref, r, q = self.seqs[k], a, []
        for st in body:
            if st[0] == "m":
                q.append(ref[r:r + st[1]]); r += st[1]
            elif st[0] == "s":
                q.append(other(rng, ref[r])); r += 1
            elif st[0] == "i":
                q.append("".join(other(rng, ref[r + i]) for i in range(st[1])))
            else:
                r += st[1]
        read = "".join(q)
        assert "N" not in read
        self.items.append((cls, read))                                       # both strands of every case
        self.items.append((cls, "".join(RC[c] for c in reversed(read))))


def build_reads(seqs, mmax, long_set):
    R = Reads(seqs, 77 if long_set else 76)
    rng = R.rng
    R.add("single", [("m", 150)])
    R.add("only_R", [("s",), ("m", 45), ("s",), ("m", 38), ("s",)])
    R.add("only_D", [("d", 3), ("m", 45), ("d", 7), ("m", 38), ("d", 1)])
    R.add("only_I", [("i", 2), ("m", 45), ("i", 6), ("m", 38), ("i", 1)])
    g = 2
    while True:
        k = min_subs(g)
        if k > mmax:
            break
        R.add("diag", diag_steps(g, k))
        if g > 2 and max(k, 3) <= mmax:
            R.add("diag_adj", diag_steps(g, max(k, 3), adjacent=True))
        g += 1
    if long_set:
        for g in (63, 64, 65, 100):
            R.add("diag_long", diag_steps(g, max(min_subs(g), 8)), lead=60, trail=60)
        R.add("dp_longop", [("s",), ("m", 6), ("d", 70), ("m", 5), ("s",)], lead=330, trail=330)    # (flanks that outweigh the gap: shorter ones are not chained)
    for n in range(1, 9):                                                # DP joints: an indel with substitutions about it, lists of 2n + 1 ops and so on
        steps = []
        for _ in range(n):
            steps += [("s",), ("m", rng.randint(3, 6))]
        R.add("dp", steps + [("i", 2) if n & 1 else ("d", 2)] + [("m", 4), ("s",)])
        R.add("dp", steps + [("d", 2) if n & 1 else ("i", 2)] + [("m", 4), ("s",), ("m", 3), ("s",), ("s",), ("m", 2), ("d", 1), ("m", 4), ("s",)])
        # (a gap starts and ends with an op that is no match, and matches alternate with the rest: an even count needs two such ops side by side)
        R.add("dp", steps + [("s",), ("i", 3) if n & 1 else ("d", 3), ("m", 5), ("s",)])
    for n in (4, 5, 6):                                                      # aimed at lists of 2 n + 4 = 12, 14, 16 ops, whatever the scoring
        for gap in (("i", 2), ("d", 2), ("i", 4), ("d", 4)):
            R.add("dp", [("s",), ("m", 6)] * n + [("s",), gap, ("m", 6), ("s",)])
    R.add("dp", [("s",), ("m", 4), ("d", 9), ("m", 5), ("s",)])
    R.add("dp", [("i", 3), ("m", 4), ("s",)])
    R.add("mixed", [("s",), ("m", 5), ("i", 2), ("m", 40), ("s",), ("m", 5), ("s",), ("m", 40), ("d", 4), ("m", 40), ("s",), ("m", 36), ("i", 3), ("m", 4), ("s",)])
    R.add("mixed", [("s",), ("s",), ("m", 40), ("s",), ("m", 4), ("d", 3), ("m", 40), ("i", 5)])
    # ends: a mismatch right at either end of the seeds' reach (zero-length end extensions), reads that run to the genome's first and last base
    R.add("ends_zero", [("m", 60)], lead=0, trail=0)
    R.add("ends_blocked", [("s",), ("m", 80), ("s",)], lead=3, trail=3)
    R.add("ends_ref0", [("s",), ("m", 50)], where=lambda need: (0, 0), lead=45)
    R.add("ends_reflast", [("m", 50), ("s",)], where=lambda need: (len(seqs) - 1, len(seqs[-1]) - need), trail=45)
    return R.items


# ---- the oracle's chains, as k_p1_roots sees them ------------------------------------------------------------------------------------------------------
def root_classes(s, b, nib):
    """per root of the oracle's chain stage: (joint kinds, details) after the exact-match extensions of AlignHelpers.c:216-232 and AlignExtFrag.cpp:76-107"""
    P = s.params
    _bases, offs, codes = batch_arrays(s, b)
    max_roff = int(s.index.maxROff)
    out = []
    for rs, frags in oracle.chain(s.index, P, b):
        read, strand = rs >> 1, rs & 1
        q = codes[int(offs[read]):int(offs[read + 1])]
        if strand:
            q = np.array([CODE_COMP[c] for c in q[::-1]], np.uint8)
        qlen = len(q)
        fr = [list(f[:4]) for f in frags]                                    # sro, sqo, eqo, refLen
        joints, cur = [], fr[0]
        for nxt in fr[1:]:
            ero = cur[0] + cur[3] - 1
            gap = min(max(nxt[1] - cur[2] - 1, 0), max(nxt[0] - ero - 1, 0))
            c = 0
            while c < gap and q[nxt[1] - 1 - c] == nib[nxt[0] - 1 - c]:
                c += 1
            nxt[1] -= c; nxt[0] -= c; nxt[3] += c; gap -= c
            c = 0
            while c < gap and q[cur[2] + 1 + c] == nib[ero + 1 + c]:
                c += 1
            cur[2] += c; cur[3] += c
            ero = cur[0] + cur[3] - 1
            qg, rg = max(nxt[1] - cur[2] - 1, 0), max(nxt[0] - ero - 1, 0)
            kind, mism = "N", ()
            if qg == 0 and rg == 0:
                kind = "N"
            elif qg == 0:
                kind = "D"
            elif rg == 0:
                kind = "I"
            elif qg == 1 and rg == 1:
                kind = "R"
            else:
                kind = "DP"
                if qg == rg:
                    mism = tuple(t for t in range(qg) if q[cur[2] + 1 + t] != nib[ero + 1 + t])
                    if len(mism) * (P.MScore + P.RCost) <= P.MScore + 2 * (P.GOCost + P.GECost):
                        kind = "DIAG"
            joints.append(dict(kind=kind, q=qg, r=rg, mism=mism, qOff=cur[2] + 1, rOff=ero + 1))
            cur = nxt
        sro, sqo, eqo = fr[0][0], fr[0][1], cur[2]
        ero = cur[0] + cur[3] - 1
        back_len = min(sqo, sro)
        m = 0
        while m < back_len and q[sqo - 1 - m] == nib[sro - 1 - m]:
            m += 1
        forw_len = min(qlen - 1 - eqo, max_roff - ero)
        f = 0
        while f < forw_len and q[eqo + 1 + f] == nib[ero + 1 + f]:
            f += 1
        out.append(dict(read=read, strand=strand, n=len(fr), joints=joints, back=(back_len, m), forw=(forw_len, f), sqo=sqo - m, sro=sro - m, eqo=eqo + f, ero=ero + f,
                        qlen=qlen))
    return out, max_roff


def check_classes(name, roots, max_roff, dp_ops, mmax):
    """every class of the module's docstring is in the oracle's chains; returns a summary"""
    def has(pred):
        return {r["strand"] for r in roots if pred(r)}
    both = {0, 1}
    kinds = lambda r: [j["kind"] for j in r["joints"]]
    rep = {}
    assert has(lambda r: r["n"] == 1) == both
    for k in "RDI":
        assert has(lambda r: r["n"] > 1 and set(kinds(r)) == {k}) == both, k
    diag = [(j, r["strand"]) for r in roots for j in r["joints"] if j["kind"] == "DIAG"]
    gs = {}
    for j, st in diag:
        gs.setdefault(j["q"], set()).add(st)
        assert j["mism"][0] == 0 and j["mism"][-1] == j["q"] - 1              # (the exact-match extensions stopped at them)
    gmax = max(g for g in range(2, 400) if min_subs(g) <= mmax)
    assert all(gs.get(g) == both for g in range(2, gmax + 1)), (name, str(sorted(gs.items())), gmax)
    assert {st for j, st in diag if 1 in j["mism"] and j["q"] > 2} == both    # adjacent mismatches: one R op of two
    rep["diagonals"] = "g = 2..%d on both strands, %d joints" % (gmax, len(diag))
    if name == "cheap":
        for g in (63, 64, 65, 100):
            assert gs.get(g) == both, (g, sorted(gs))
        assert {r["strand"] for r in roots for j in r["joints"] if j["kind"] == "DP" and any(j is jj and max(n for n, _c in ops) > 64 for jj, ops in dp_ops)} == both, \
            "no DP op longer than 64"
        assert any(len(ops) <= N_INLINE and max(n for n, _c in ops) > 64 for _j, ops in dp_ops), "no list that is short enough for the record but for one op's length"
    nops = {}
    for j, ops in dp_ops:
        nops[len(ops)] = nops.get(len(ops), 0) + 1
    # the gap fills keep a list of at most N = 14 ops, none longer than 64, inside the joint record (JF_INLINE, phase_lanes.h): lists of N - 1, N and N + 1 ops whose
    # ops all fit the length field, short and long ones, odd and even; the GPU tests run under YGPU_GAP32 and YGPU_GAP24_OFF too, so every gap kernel writes some
    fits = {len(ops) for _j, ops in dp_ops if max(n for n, _c in ops) <= 64}
    assert {N_INLINE - 1, N_INLINE, N_INLINE + 1} <= fits, sorted(fits)
    assert len(nops) >= 8 and min(nops) <= 3 and max(nops) > N_INLINE + 1 and sum(1 for k in nops if k % 2 == 0) >= 2, sorted(nops.items())
    rep["DP joints by ops"] = sorted(nops.items())
    assert has(lambda r: "DP" in kinds(r) and "DIAG" in kinds(r) and set(kinds(r)) & set("RDI")) == both
    assert has(lambda r: "DP" not in kinds(r) and r["n"] > 1) == both and has(lambda r: "DP" in kinds(r)) == both
    # (A forward end extension longer than zero that runs to the read's last base cannot be planted: a fragment ends where its last seed ends, an exact tail of
    # 11 bases or more holds a seed of its own and so belongs to the fragment, and a shorter exact tail lies behind a mismatch, where the extension stops at once.
    # Reads that END on their last fragment's last base are here, and forward extensions longer than zero occur inside reads -- the summary counts them; it is the
    # backward extension, whose fragments start at the seeds' sampled offsets, that walks to offset 0.)
    assert any(r["sqo"] == 0 and r["back"][1] > 0 for r in roots) and any(r["eqo"] == r["qlen"] - 1 for r in roots)
    rep["end extensions"] = "backward > 0: %d roots, forward > 0: %d" % (sum(r["back"][1] > 0 for r in roots), sum(r["forw"][1] > 0 for r in roots))
    assert any(r["sro"] == 0 for r in roots) and any(r["ero"] == max_roff - 1 for r in roots), "no root reaches the reference's first / last base"
    assert any(r["back"][0] > 0 and r["back"][1] == 0 for r in roots) and any(r["forw"][0] > 0 and r["forw"][1] == 0 for r in roots)
    rep["roots"] = "%d, %d with a DP joint" % (len(roots), sum("DP" in kinds(r) for r in roots))
    return rep


@pytest.fixture(scope="module")
def genome(work, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("p1lists"))
    fa = os.path.join(d, "gf.fa")
    seqs, _tracts, _nrun = write_genome(fa)
    ya.build_index(["-g", fa, "-L", "11"])
    return d, os.path.join(d, "gf.X11_01_65525S"), seqs


@pytest.fixture(scope="module")
def cases(genome):
    """{set: (reads file, number of reads, the oracle's roots, summary)}: built and checked once"""
    d, index, seqs = genome
    out = {}
    for name, args in SETS.items():
        probe = os.path.join(d, "probe_%s.fa" % name)
        with open(probe, "w") as f:
            f.write(">p\n%s\n" % seqs[0][:100])
        with ya.Session(["-x", index, "-q", probe] + args) as s0:
            P = s0.params
            mmax = (P.MScore + 2 * (P.GOCost + P.GECost)) // (P.MScore + P.RCost)
        items = build_reads(seqs, mmax, name == "cheap")
        path = os.path.join(d, "reads_%s.fa" % name)
        with open(path, "w") as f:
            for k, (cls, read) in enumerate(items):
                f.write(">%s_%d\n%s\n" % (cls, k, read))
        with ya.Session(["-x", index, "-q", path] + args) as s:
            b = s.next_batch(len(items) + 1)
            assert b.n_reads == len(items)
            bases, _o, _c = batch_arrays(s, b)
            nib = np.empty(2 * len(bases), np.uint8); nib[0::2] = bases >> 4; nib[1::2] = bases & 15
            roots, max_roff = root_classes(s, b, nib)
            dpj = [(r, j) for r in roots for j in r["joints"] if j["kind"] == "DP"]
            probs = [ya.DPProblem(r["read"], r["strand"], ya.DP_BANDED if abs(j["q"] - j["r"]) + 2 * s.params.bandWidth + 1 < j["r"] else ya.DP_FULL, j["qOff"], j["q"],
                                  j["r"], j["rOff"]) for r, j in dpj]
            res = oracle.dp_batch(s.index, s.params, b, probs)
            dp_ops = [(j, ops) for (_r, j), (_s, _aq, _ar, ops) in zip(dpj, res)]
        out[name] = (path, len(items), roots, check_classes(name, roots, max_roff, dp_ops, mmax))
    return out


def test_the_oracles_chains_hold_every_class(cases):
    for name, (_path, n, _roots, rep) in cases.items():
        print("set %s: %d reads" % (name, n))
        for key, val in rep.items():
            print("  ", key, val)


def run_and_compare(index, path, args, batch):
    n = 0
    with ya.Session(["-x", index, "-q", path] + args) as s:
        with ya.Context(s.index, s.params) as ctx:
            while True:
                b = s.next_batch(batch)
                if b.n_reads == 0:
                    break
                ctx.upload(b)
                ctx.run()
                r = ctx.collect()
                ro, _own = oracle.run(s.index, s.params, b, threads=8)
                assert ya.result_records(r) == ya.result_records(ro), "device clump records differ from the oracle"
                got, exp = r.counters.as_dict(), ro.counters.as_dict()
                print("counters", {k: (got[k], exp[k]) for k in COUNTERS})
                for key in COUNTERS:
                    assert got[key] == exp[key], (key, got[key], exp[key])
                n += 1
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("name", list(SETS))
def test_phase1_lists_match_the_oracle(genome, cases, name, switch, monkeypatch):
    _d, index, _seqs = genome
    path, n, roots, _rep = cases[name]
    for sw in SWITCHES[1:]:
        monkeypatch.delenv(sw, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    run_and_compare(index, path, SETS[name], n + 1)                          # the whole list in one batch


@pytest.mark.gpu
def test_partial_waves_in_the_compact_list(genome, cases):
    """batches of fewer than 64 roots and of 64 k + 1: the root counts are the oracle's"""
    _d, index, _seqs = genome
    path, n, roots, _rep = cases["main"]
    per_read = {}
    for r in roots:
        per_read[r["read"]] = per_read.get(r["read"], 0) + 1
    upto = np.cumsum([per_read.get(k, 0) for k in range(n)])
    small = int(np.searchsorted(upto, 40))                                   # reads that give about 40 roots
    assert 0 < upto[small - 1] < 64
    k65 = [int(i) + 1 for i in range(n) if upto[i] > 64 and upto[i] % 64 == 1]
    assert k65, "no prefix of the reads gives 64 k + 1 roots"
    assert run_and_compare(index, path, SETS["main"], small) >= 2
    run_and_compare(index, path, SETS["main"], k65[0])
