"""GPU tier: the tile selection (device/select.h: k_select_count / k_select_emit over a selector -- a wave counts the items of a tile that pass, an exclusive
sum of the tiles' counts places them, the second pass writes them by ballot and population count) at the edges of lanes, rows and tiles, for every
instantiation: the pileup's candidates (CandidateSel), the indel table's drain (IndelDrainSel), the merge table's drain (IndelMergeDrainSel) and the indel
calls (IndelCallSel).  The SNV calls (SnvSel) get the same edges in test_gpu_snv.py.  Every comparison is with the oracles of the outputs themselves:
tests/pileup_oracle.py, tests/indel_oracle.py and tests/indelcall_oracle.py."""
import os

import numpy as np
import pytest

import indel_oracle as io
import indelcall_oracle as ico
import pileup_oracle as po
import yaha_amd as ya
from test_gpu_indels import _first_seq, _got, _run_cases, _session, _want

pytestmark = pytest.mark.gpu

CH = "ACGT"


@pytest.fixture(scope="module")
def genome(work):
    return po.read_fasta(os.path.join(work, "genome_small.fa"))


def test_candidates_at_the_edges_of_lanes_rows_and_tiles(work, index11, genome):
    """Rows folded with pileup_add into an enabled, empty array; the candidates are the oracle's slots with nonref >= 1, in order."""
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout", "-opu", "unused.tsv"]) as s:
        sq = po.sq_table(s.header().split("\n")); ref = po.ref_letters(sq, genome)
        n = po.n_slots(sq); assert n % 64 != 0 and n > 3 * 2048 and len(sq) >= 2
        is_base = np.isin(ref, np.frombuffer(b"ACGT", dtype=np.uint8))
        model = np.zeros((n, 7), dtype=np.uint32)

        def row(slot, other, depth=3):
            """`depth` reads of the reference base of a slot (other = 0: no candidate) or of the base `other` places behind it."""
            assert is_base[slot], slot
            r = [0] * 7; r[(CH.index(chr(ref[slot])) + other) % 4] = depth
            return r

        def fold(ctx, slots, rows):
            ctx.pileup_add(slots, rows)
            for sl, r in zip(slots, rows):
                if sl < n:
                    model[sl] += np.array(r, dtype=np.uint32)

        with ya.Context(s.index, s.params) as a:
            a.set_postfilter(s); a.pileup_enable(s)
            assert len(a.pileup_candidates()) == 0                                                 # an empty array has no candidates
            # the edges of waves, rows and tiles, the last slot, the two sides of a sequence boundary; tile 2 (slots 4096 .. 6143) stays empty
            first2 = sq[0][1]
            edge = [0, 63, 64, 2047, 2048, 2049, 6144, n - 1, first2 - 1, first2]
            assert all(is_base[e] for e in edge) and len(set(edge)) == len(edge)
            fold(a, edge, [row(e, 1) for e in edge])
            # a row of a tile where all 64 lanes pass (tile 5, its third row)
            full = list(range(5 * 2048 + 128, 5 * 2048 + 192)); assert is_base[full].all()
            fold(a, full, [row(e, 1 + e % 3, 1 + e % 4) for e in full])
            # touched slots that are no candidates: reads of the reference base alone, beside the edges
            plain = [x for x in (1, 62, 65, 2046, 2050, 6145, n - 2) if is_base[x]]; assert len(plain) >= 4 and not set(plain) & set(edge)
            fold(a, plain, [row(x, 0) for x in plain])
            # slots at and past the array add nothing
            fold(a, [n, n + 1, n + 63, 0xFFFFFFFF], [row(0, 1)] * 4)
            want = po.candidates(model, ref)
            got = a.pileup_candidates()
            assert got.dtype == np.uint32 and np.array_equal(got, want)
            assert sorted(edge + full) == want.tolist() and not any(4096 <= x < 6144 for x in want.tolist())
            arr, _st = a.pileup_collect()
            assert np.array_equal(arr, model)
            assert np.array_equal(a.pileup_candidates(), want)                                     # a second selection on the same array


@pytest.mark.parametrize("capacity", [2048, 4096], ids=["one_tile", "two_tiles"])
def test_indel_drain_of_one_and_two_tiles(work, index11, tmp_path, capacity):
    """The injected batch of test_gpu_indels.py into a table of exactly one and of two tiles of 2 048 entries; the drained multiset is the oracle's."""
    rng = np.random.RandomState(5); rd = lambda k: "".join(rng.choice(list("ACGT"), k)); M, I, D = "MID"
    p21, tail = rd(21), rd(9)
    other = lambda c: "ACGT"[("ACGT".index(c) + 1) % 4]
    ins = (p21 + tail, p21 + other(tail[0]) + tail[1:], other(p21[0]) + p21[1:] + tail)
    reads = ["A" * 64 + rd(100), rd(300)] + [rd(50) + ins[k % 3] + rd(50) for k in range(60)]
    with _session(index11, tmp_path, reads) as s:
        s0, l0 = _first_seq(s); assert l0 > 21000
        with ya.Context(s.index, s.params) as ctx:
            ctx.set_postfilter(s); ctx.indels_enable(s, capacity=capacity)
            ops130 = [(M, 1), (D, 1)] * 31 + [(M, 1), (I, 2), (I, 3)] + [(M, 1), (D, 2)] * 32 + [(M, 100)]
            cases = {0: [(s0 + 1000, 0, 163, 0x00, [(I, 1)] * 64 + [(M, 100)])],
                     1: [(s0 + 3000, 0, sum(k for c, k in ops130 if c in "MRI") - 1, 0x01, ops130)]}
            for k in range(60):
                cases[2 + k] = [(s0 + 20000, 0, 129, k & 1, [(M, 50), (I, 30), (M, 50)])]
            want, n_rec = _want(s, [_run_cases(s, ctx, 62, cases)])
            assert n_rec == 62 and 64 < len(want) < capacity // 2 and want[(1000, io.INS, 1, "A")] == 64
            assert ctx.indels_size() == len(want)
            entries, st = ctx.indels_collect()
            assert _got(entries) == want and st["events"] == sum(want.values()) and st["events_lost"] == 0
            again, st2 = ctx.indels_collect()                                                      # collect returns them once
            assert again == [] and ctx.indels_size() == 0 and st2["events"] == 0


def _raw_alleles(ref, sq, count, first=1000):
    """[(key, 6)]: `count` alleles, deletions and insertions in turn, at distinct anchors that no allele can leave (the base before differs from the allele's
    last base), so that none moves and none merges."""
    n = len(ref); step = 200; assert first + count * step < n
    ends = np.cumsum([ln for _name, ln in sq]); raw = []; p = first
    for i in range(count):
        while True:                                                                                # (a stretch of N is walked through)
            ln = 1 + i % 3
            inside = np.searchsorted(ends, p - 1, side="right") == np.searchsorted(ends, p + ln, side="right")
            if inside and all(c in "ACGT" for c in ref[p - 1:p + ln]) and ref[p - 1] != ref[p + ln - 1]:
                break
            p += 1
        assert p + ln < n
        if i % 2 == 0:
            raw.append(((p, ico.DEL, ln, ""), 6))
        else:
            bases = "".join(CH[(i + j) % 4] for j in range(ln - 1)) + CH[(CH.index(ref[p - 1]) + 1 + i % 3) % 4]
            raw.append(((p, ico.INS, ln, bases), 6))
        p += step
    return raw


def _alleles(ctx):
    return [(io.entry_key(e.w0, e.w1, e.w2), e.count) for e in ctx.indelcall_alleles()]


def _rows(got):
    return [tuple(int(x) for x in r) for r in got.tolist()]


def test_merge_drain_and_indel_calls_over_three_tiles_and_a_partly_filled_one(work, index11, genome):
    """1 100 raw alleles that neither move nor merge: a merge table of two drain tiles, three tiles of 512 alleles for the calls, the last row of the last tile
    partly filled; rows folded at the anchors decide which alleles call.  Then 37 alleles: one tile, one partly filled row."""
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout", "-oindel", "unused.vcf"]) as s:
        sq = po.sq_table(s.header().split("\n")); ref = po.ref_letters(sq, genome).tobytes().decode()
        n = len(ref); N = 1100; assert N > 2 * 512 and N % 64 != 0
        raw = _raw_alleles(ref, sq, N)
        merged, mst = ico.merge(raw, ref, sq, 256)
        assert len(merged) == N and mst == dict(raw=N, shifted=0, merged=0, skipped=0)
        keys = sorted(merged, key=io.order)
        # which alleles get a depth that calls (d = a = 6): the first, the 512th, the 513th and the last in key order, every third elsewhere -- but none of
        # a stretch in between, where the anchors stay bare (d = 0) or are covered by 200 reads of the reference (the genotype is 0/0)
        calling = {0, 511, 512, N - 1} | {k for k in range(N) if k % 3 == 1 and not 100 <= k < 400}
        model = np.zeros((n, 7), dtype=np.uint32); slots, rows = [], []
        for k, key in enumerate(keys):
            d = 6 if k in calling else 200 if 100 <= k < 400 and k % 2 else 0
            if d:
                slots.append(key[0] - 1); rows.append([d // 6 + (j < d % 6) for j in range(6)] + [9])
        assert len(set(slots)) == len(slots)
        with ya.Context(s.index, s.params) as a:
            a.set_postfilter(s); a.pileup_enable(s)
            got_n, st = a.indelcall_normalize([ico.words(k) + (c,) for k, c in raw])
            want_alleles = [(k, merged[k]) for k in keys]
            assert (got_n, st) == (N, mst) and _alleles(a) == want_alleles
            assert len(a.indel_calls(s)) == 0                                                      # an empty array: no depth anywhere
            a.pileup_add(slots, rows); model[slots] += np.array(rows, dtype=np.uint32)
            want = ico.judged(merged, model)
            called = {keys.index(k) for k, _v in want}
            assert called == calling and not any(100 <= k < 400 for k in called)
            got = a.indel_calls(s)
            assert got.dtype.names == ya.INDEL_CALL_FIELDS and got.itemsize == 64 and _rows(got) == ico.records(want, ref)
            assert _alleles(a) == want_alleles                                                     # the alleles are still there
            # fewer than 64 raw alleles: one tile, partly filled -- the rows stay in the array
            few = raw[:37]; m2, st2 = ico.merge(few, ref, sq, 256)
            got_n, st = a.indelcall_normalize([ico.words(k) + (c,) for k, c in few])
            assert (got_n, st) == (37, st2) and _alleles(a) == [(k, m2[k]) for k in sorted(m2, key=io.order)]
            want2 = ico.judged(m2, model)
            assert 0 < len(want2) < 37 and _rows(a.indel_calls(s)) == ico.records(want2, ref)
