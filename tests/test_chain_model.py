"""chain_model.py (the plain-Python model of the chain stage that reports the rules it used) equals the oracle, clump for clump: on the four golden calls of
test_seed_join_and_chain_bit_exact, on every set that test_gpu_chain_classes.py builds, and on a few thousand short random reads (the oracle exports no entry
that takes fragments, so the fragment lists come from reads: copies of stretches of the golden genome with substitutions, indels and doubled pieces).
CPU tier: the oracle and host code only."""
import os
import random

import pytest

import oracle
import yaha_amd as ya
from problems import read_fasta
from test_gpu_chain_classes import SETS, cases, first_difference, genome, model_clumps, run_model  # noqa: F401  (fixtures)


def model_equals_oracle(s, b):
    frags, (clumps, regions) = run_model(s, b)
    exp = oracle.chain(s.index, s.params, b)
    assert clumps == exp, first_difference(clumps, exp, regions)
    assert sum(len(r.clumps) for r in regions) == len(exp) and sum(r.size for r in regions) == len(frags)
    return regions


@pytest.mark.parametrize("reads,extra", [("r1k.fa", []), ("rchim.fa", ["-H", "20"]), ("r100.fa", []), ("r10k.fa", [])])
def test_the_model_equals_the_oracle_on_the_golden_calls(work, index11, reads, extra):
    with ya.Session(["-x", index11, "-q", os.path.join(work, reads)] + extra) as s:
        regions = model_equals_oracle(s, s.next_batch(500))
        assert len(regions) > 5000


@pytest.mark.parametrize("name", list(SETS))
def test_the_model_equals_the_oracle_on_the_built_sets(cases, name):
    """(the `cases` fixture of test_gpu_chain_classes.py ran both, once; the comparison is made here, and again by the coverage test before it trusts the events)"""
    _path, n, frags, exp, regions = cases[name]
    got = model_clumps(regions)
    assert n > 0 and exp and got == exp, first_difference(got, exp, regions)
    assert sum(r.size for r in regions) == len(frags)


@pytest.mark.parametrize("extra", [[], ["-G", "12", "-MD", "30", "-M", "30"], ["-MS", "4", "-M", "15"]])
def test_the_model_equals_the_oracle_on_random_short_reads(work, index11, tmp_path, extra):
    rng = random.Random(4711 + len(extra))
    _names, seqs = read_fasta(os.path.join(work, "genome_small.fa"))
    path = os.path.join(str(tmp_path), "short.fa")
    n = 1500
    with open(path, "w") as f:
        for k in range(n):
            g = seqs[rng.randrange(len(seqs))]
            a = rng.randrange(len(g) - 400)
            r = list(g[a:a + rng.randint(40, 300)])
            for _ in range(rng.randrange(6)):
                p = rng.randrange(len(r))
                kind = rng.randrange(4)
                if kind == 0:
                    r[p] = rng.choice("ACGT")
                elif kind == 1:
                    del r[p:p + rng.randint(1, 14)]
                elif kind == 2:
                    r[p:p] = [rng.choice("ACGT") for _ in range(rng.randint(1, 14))]
                else:                                                        # a piece doubled in place: fragments that overlap in the reference
                    w = rng.randint(3, 40)
                    r[p:p] = r[max(p - w, 0):p]
            seq = "".join(r).replace("N", "A")
            f.write(">s%d\n%s\n" % (k, seq if len(seq) >= 30 else g[a:a + 60].replace("N", "A")))
    with ya.Session(["-x", index11, "-q", path] + extra) as s:
        b = s.next_batch(n + 1)
        assert b.n_reads == n
        regions = model_equals_oracle(s, b)
        assert sum(1 for r in regions if r.size > 1) > 200
