"""GPU tier: the allele pileup (-opu) accumulated on the device behind the post-filter (device/pileup_stage.h: a wave per printed clump, the aligned bases
dealt across the lanes, global atomics into one seven-channel array per index image; the candidate slots selected on the device at the end).  Every
comparison is with tests/pileup_oracle.py, which recomputes the pileup from SAM text and the reference FASTA alone; the tier runs with YGPU_CHECK_STATE on
(conftest.py), so every ygpu_run / ygpu_postfilter here also checks the state words."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import pileup_oracle as po
import yaha_amd as ya
from conftest import golden_lines, strip_pg

pytestmark = pytest.mark.gpu

SETS = [("rchim_default", "rchim.fa"), ("r1k_default", "r1k.fa"), ("r10k_default", "r10k.fa"), ("rq_default", "rq.fq")]
# sites of the golden lines at -pumin 1 and 2 (the issue's table); no set has a site at 3
SITES = {"rchim_default": (3487, 21), "r1k_default": (2691, 23), "r10k_default": (4951, 24), "rq_default": (1704, 15)}


def _cli(index11, reads, out, extra=(), oflag="-osh", env=None):
    p = subprocess.run([ya.CLI_PATH, "-x", index11, "-q", reads, oflag, "stdout", "-opu", out] + list(extra), env=dict(os.environ, YAHA_STATS="1", **(env or {})),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    assert "state check" not in err, err[-2000:]                                       # YGPU_CHECK_STATE stays silent (a dirty word also fails the run)
    st = json.loads([l for l in err.split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])
    return p.stdout.decode(), open(out).read(), st


@functools.lru_cache(maxsize=None)
def _ref(fasta):
    return po.read_fasta(fasta)


@functools.lru_cache(maxsize=None)
def _oracle(name, fasta, Q=0):
    """(array, @SQ table, reference letters) of a golden set: computed once, shared, never written to."""
    lines = golden_lines(name); sq = po.sq_table(lines)
    pu = po.pileup(lines, sq, Q); pu.setflags(write=False)
    return pu, sq, po.ref_letters(sq, _ref(fasta))


def _expected(name, fasta, min_alt, Q=0):
    pu, sq, ref = _oracle(name, fasta, Q)
    return po.text(pu, sq, ref, min_alt)


@pytest.mark.parametrize("name,reads", SETS)
def test_command_line_table_is_counted_by_the_kernel_and_equals_the_oracle(work, index11, tmp_path, name, reads):
    out = str(tmp_path / "pu.tsv"); lines = golden_lines(name); q = os.path.join(work, reads); fasta = os.path.join(work, "genome_small.fa")
    pu, sq, ref = _oracle(name, fasta)
    assert (pu.sum(axis=0) > 0).all()                                                   # all seven channels are exercised by every set
    assert (len(po.sites(pu, ref, 1)), len(po.sites(pu, ref, 2)), len(po.sites(pu, ref, 3))) == SITES[name] + (0,)
    for extra, N in ((["-pumin", "1", "-ctx", "1", "-batch", "9"], 1), (["-pumin", "2", "-ctx", "2", "-batch", "17"], 2), (["-pumin", "1", "-ctx", "3", "-batch", "33"], 1),
                     (["-pumin", "2", "-ctx", "1", "-batch", "33"], 2), (["-pumin", "1", "-ctx", "2", "-batch", "9"], 1), (["-pumin", "2", "-ctx", "3", "-batch", "17"], 2)):
        sam, got, st = _cli(index11, q, out, extra)
        assert strip_pg(sam) == lines, (name, extra)
        assert got == _expected(name, fasta, N), (name, extra)
        assert got.count("\n") - 1 == SITES[name][N - 1] > 0, (name, extra)             # an empty table proves nothing
        # the kernel did the counting, not the host's fallback
        assert st["pileup_device_records"] == po.records(lines) > 0 and st["pileup_host_records"] == 0, (extra, st)
        assert st["pileup_bases"] == po.n_slots(sq) and st["pileup_counted"] == int(pu.sum())
        assert st["pileup_candidates"] == SITES[name][0] and st["pileup_sites"] == SITES[name][N - 1]
    # the host's post-filter by option: the host counts everything, and the same file
    sam, got, st = _cli(index11, q, out, ["-pumin", "1", "-dpf", "N"])
    assert strip_pg(sam) == lines and got == _expected(name, fasta, 1)
    assert st["pileup_device_records"] == 0 and st["pileup_host_records"] == po.records(lines) > 0


def test_command_line_deeper_set_and_the_mapping_quality_gate(work, index11, tmp_path):
    out = str(tmp_path / "pu.tsv"); fasta = os.path.join(work, "genome_small.fa")
    # split reads at five-fold coverage: a depth of up to 21, 24 sites where three reads disagree
    pu, sq, ref = _oracle("rsv_default", fasta)
    assert int(pu[:, :6].sum(axis=1).max()) == 21 and len(po.sites(pu, ref, 3)) == 24
    sam, got, st = _cli(index11, os.path.join(work, "rsv.fa"), out, ["-pumin", "3"])
    assert strip_pg(sam) == golden_lines("rsv_default") and got == _expected("rsv_default", fasta, 3) and got.count("\n") == 25
    assert st["pileup_host_records"] == 0 and st["pileup_sites"] == 24 and st["pileup_counted"] == int(pu.sum())
    # a read with one clump is printed with MAPQ 250 (GraphPath.cpp:907-916): -puq 251 counts no such record, -puq 250 counts them
    lines = golden_lines("r1k_default"); q = os.path.join(work, "r1k.fa")
    n250 = po.records(lines, 250); assert 0 < n250 and po.records(lines, 251) < n250
    for Q in (251, 250):
        _sam, got, st = _cli(index11, q, out, ["-pumin", "1", "-puq", str(Q)])
        assert got == _expected("r1k_default", fasta, 1, Q) and st["pileup_device_records"] == po.records(lines, Q) and st["pileup_host_records"] == 0
    assert _expected("r1k_default", fasta, 1, 251) != _expected("r1k_default", fasta, 1, 250)


def test_command_line_other_paths(work, index11, tmp_path):
    out = str(tmp_path / "pu.tsv"); q = os.path.join(work, "rchim.fa"); fasta = os.path.join(work, "genome_small.fa"); lines = golden_lines("rchim_default")
    want = _expected("rchim_default", fasta, 1)
    for oflag in ("-oss", "-o8"):
        _sam, got, st = _cli(index11, q, out, ["-pumin", "1"], oflag=oflag)
        assert got == want and st["pileup_host_records"] == 0
    # reads of more than three clumps come back unfiltered (the hand-over path of the device stage): the host counts exactly those, the device the rest
    sam, got, st = _cli(index11, q, out, ["-pumin", "1"], env={"YGPU_OQC_MAX": "3"})
    assert strip_pg(sam) == lines and got == want
    assert st["pileup_host_records"] > 0 and st["pileup_device_records"] > 0 and st["pileup_host_records"] + st["pileup_device_records"] == po.records(lines)
    assert st["pileup_counted"] == int(_oracle("rchim_default", fasta)[0].sum())
    # two index images (the same device twice): candidates of both, the union, a gather on both
    sam, got, st = _cli(index11, q, out, ["-pumin", "1", "-gpus", "2", "-ctx", "2", "-batch", "25"], env={"YAHA_DEVICES": "0,0"})
    assert strip_pg(sam) == lines and got == want
    assert st["pileup_host_records"] == 0 and st["pileup_device_records"] == po.records(lines) and all(n > 0 for n in st["reads_per_device"])
    # beside the other tracks: each file equals the one from its own run
    cov, ev, bp = (str(tmp_path / f) for f in ("cov.bg", "ev.tsv", "bp.bedpe"))
    alone = {}
    for opt, f in (("-ocov", cov), ("-oev", ev), ("-obp", bp)):
        p = subprocess.run([ya.CLI_PATH, "-x", index11, "-q", q, "-osh", "stdout", opt, f], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0
        alone[f] = open(f).read(); os.remove(f)
    sam, got, st = _cli(index11, q, out, ["-pumin", "1", "-ocov", cov, "-oev", ev, "-obp", bp])
    assert strip_pg(sam) == lines and got == want and all(alone.values())
    assert all(open(f).read() == alone[f] for f in (cov, ev, bp))
    assert st["pileup_host_records"] == st["events_host_records"] == st["depth_host_records"] == 0 and st["pileup_device_records"] == st["events_device_records"] > 0


def _oracle_array(header, texts, fasta, Q=0):
    sq = po.sq_table(header.split("\n"))
    lines = [l for t in texts for l in t.split("\n")]
    return po.pileup(lines, sq, Q), po.ref_letters(sq, _ref(fasta)), po.records(lines, Q)


def test_abi_batches_accumulate_and_contexts_of_an_image_share_one_array(work, index11):
    fasta = os.path.join(work, "genome_small.fa")
    with ya.Session(["-x", index11, "-q", os.path.join(work, "rchim.fa"), "-osh", "stdout", "-opu", "unused.tsv"]) as s:
        with ya.Context(s.index, s.params) as a:
            with pytest.raises(RuntimeError, match="ygpu_set_postfilter"):              # enable needs the post-filter
                a.pileup_enable(s)
            with pytest.raises(RuntimeError):
                a.pileup_collect()
            a.set_postfilter(s); a.pileup_enable(s)
            with ya.Context(s.index, s.params, parent=a) as b:
                b.set_postfilter(s); b.pileup_enable(s)
                texts = []
                for k, ctx in enumerate((a, a, b, a, b)):
                    rb = s.next_batch(40)
                    assert rb.n_reads > 0
                    ctx.upload(rb); ctx.run()
                    texts.append(s.emit_filtered(ctx.postfilter()))
                    want, ref, n_rec = _oracle_array(s.header(), texts, fasta)
                    got, st = ctx.pileup_collect()
                    assert got.shape == want.shape and got.dtype == np.uint32 and np.array_equal(got, want), k
                    assert st["records_counted"] == n_rec and st["reads_left_to_host"] == 0 and st["counts_added"] == int(want.sum())
                # both contexts see the same array, and every channel has something in it
                ga, _ = a.pileup_collect(); gb, _ = b.pileup_collect()
                assert np.array_equal(ga, gb) and (ga.sum(axis=0) > 0).all()
                # the candidates: the oracle's slots with nonref >= 1, ascending; the gather at them, and at a list with untouched slots mixed in
                cand = a.pileup_candidates()
                assert cand.dtype == np.uint32 and len(cand) > 0 and np.array_equal(cand, po.candidates(want, ref)) and np.array_equal(cand, b.pileup_candidates())
                assert np.array_equal(a.pileup_gather(cand), want[cand])
                untouched = np.nonzero(want.sum(axis=1) == 0)[0][:500].astype(np.uint32)
                mixed = np.unique(np.concatenate([cand[::3], untouched, np.array([0, len(want) - 1], dtype=np.uint32)]))
                assert len(untouched) == 500 and np.array_equal(b.pileup_gather(mixed), want[mixed])
                assert a.pileup_gather(np.zeros(0, dtype=np.uint32)).shape == (0, 7)
                # a sibling that is parked gives up nothing of the image's
                b.park()
                gp, _ = a.pileup_collect()
                assert np.array_equal(gp, ga) and np.array_equal(a.pileup_candidates(), cand)
                # ... and the parked sibling itself still answers for the image: the array, the selection and the gather (its work buffers went with its arenas)
                gq, stq = b.pileup_collect()
                assert np.array_equal(gq, want) and stq["counts_added"] == int(want.sum())
                assert np.array_equal(b.pileup_candidates(), po.candidates(want, ref))
                assert np.array_equal(b.pileup_gather(mixed), want[mixed]) and np.array_equal(b.pileup_gather(cand), want[cand])
            # a second enable with another min_mapq on the same image is refused
            with ya.Session(["-x", index11, "-q", os.path.join(work, "rchim.fa"), "-osh", "stdout", "-opu", "unused.tsv", "-puq", "1"]) as s2:
                with pytest.raises(RuntimeError):
                    a.pileup_enable(s2)


def _seq_table(s):
    p = ya.PileupParams()
    assert ya.lib().yaha_session_pileup_params(s._h, C.byref(p)) == 0
    st = C.cast(p.seq_start, C.POINTER(C.c_uint32)); ln = C.cast(p.seq_length, C.POINTER(C.c_uint32))
    return [(int(st[i]), int(ln[i])) for i in range(p.n_seqs)], p


def _qlens(rb):
    off = C.cast(rb.offsets, C.POINTER(C.c_uint64))
    return [int(off[i + 1] - off[i]) for i in range(rb.n_reads)]


def _batch(n_reads, per_read):
    """per_read[i] = list of (sro, sqo, eqo, status, ops) for read i; the ResultBatch ygpu_inject_results takes (and the arrays that keep it alive)."""
    recs, ops, starts = [], [], [0]
    for i in range(n_reads):
        for sro, sqo, eqo, status, o in per_read.get(i, []):
            rlen = sum(n for c, n in o if c in "MRD")
            recs.append((sro, sqo, eqo, rlen, 30, eqo - sqo + 1, sum(n for c, n in o if c == "M"), sum(n for c, n in o if c == "R"), sum(n for c, n in o if c in "ID"), status, 0, len(ops), len(o)))
            ops.extend(n | (ord(c) << 16) for c, n in o)
        starts.append(len(recs))
    cs = (C.c_uint32 * len(starts))(*starts); cl = (ya.Clump * max(1, len(recs)))(*[ya.Clump(*r) for r in recs]); op = (C.c_uint32 * max(1, len(ops)))(*ops)
    r = ya.ResultBatch(); r.n_reads = n_reads; r.clump_start = cs; r.clumps = cl; r.ops = op; r.n_clumps = len(recs); r.n_ops = len(ops)
    return r, (cs, cl, op)


def test_synthetic_clumps_through_the_stage(work, index11):
    M, R, I, D = "MRID"; fasta = os.path.join(work, "genome_small.fa")
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout", "-opu", "unused.tsv"]) as s:
        seqs, p = _seq_table(s)
        assert p.min_mapq == 0 and len(seqs) >= 2
        (s0, l0), (s1, l1) = seqs[0], seqs[1]
        with ya.Context(s.index, s.params) as ctx:
            ctx.set_postfilter(s); ctx.pileup_enable(s)
            rb = s.next_batch(12); assert rb.n_reads == 12
            ql = _qlens(rb); assert min(ql) > 700
            ctx.upload(rb)
            # (ops consume exactly eqo - sqo + 1 query bases, except in the last case)
            cases = {
                0: [(s0 + 100, 0, 199, 0x00, [(M, 120), (R, 5), (M, 75)])],                            # a forward clump ...
                1: [(s0 + 100, 0, 199, 0x01, [(M, 120), (R, 5), (M, 75)])],                            # ... and a reversed one over the same slots
                2: [(s0 + 2000, 3, 3 + 499, 0x01, [(M, 3), (R, 1)] * 40 + [(D, 2), (I, 3), (M, 337)])],      # more than 64 ops: the run of M and R ops starts in one chunk and ends in the next
                3: [(s0 + 5000, 0, 649, 0x00, [(M, 2), (I, 1)] * 50 + [(M, 3)] * 13 + [(M, 461)])],    # 114 ops, the I ops cut the M runs; the last M op alone is seven strips long
                4: [(s0 + 9000, 10, 10 + 299, 0x00, [(M, 31), (R, 2), (M, 267)])],                     # an M run longer than 64 bases that crosses a strip edge (bases 33 .. 299)
                5: [(s0 + 12000, 0, 120, 0x01, [(M, 96), (I, 3), (D, 4), (M, 20), (I, 2)])],           # an I directly before a D, an I as the last op
                6: [(s1 + l1 - 17, 0, 15, 0x00, [(M, 10), (R, 1), (M, 5), (D, 1)])],                   # ends on the last base of a sequence
                7: [(s0 + l0 - 10, 50, 69, 0x00, [(M, 5), (R, 15)])],                                  # spans two sequences: not printed, counts nothing
                8: [(s0 + 15000, 5, 5 + 99, 0x01, [(M, 60), (I, 5), (M, 80)])],                        # ops that ask for 145 query bases of a clump that has 100: nothing past eqo
            }
            r, _keep = _batch(12, cases)
            ctx.inject_results(r)
            text = s.emit_filtered(ctx.postfilter())                                                # (YGPU_CHECK_STATE: a fault or a dirty state word fails this call)
            want, ref, n_rec = _oracle_array(s.header(), [text], fasta)
            assert n_rec == 8                                                                       # all but the clump across two sequences are printed
            got, st = ctx.pileup_collect()
            assert np.array_equal(got, want)
            assert got[:, 5].sum() == 2 + 4 + 1 and got[:, 6].sum() == 1 + 50 + 2 + 1
            assert got[:, :5].sum() == 200 + 200 + (160 + 337) + (100 + 39 + 461) + 300 + 116 + 16 + (60 + 35)
            assert st == {"records_counted": 8, "records_skipped_mapq": 0, "records_dropped_two_sequences": 1, "reads_left_to_host": 0, "counts_added": int(want.sum())}
            # the forward and the reversed clump over the same slots: two bases a slot, and the reversed one is not the forward one again
            b0 = 100                                                                                # (slot of s0 + 100: the first sequence's slots start at 0)
            assert (got[b0:b0 + 200, :5].sum(axis=1) == 2).all() and (got[b0:b0 + 200, :5].max(axis=1) == 1).any()
            assert np.array_equal(ctx.pileup_candidates(), po.candidates(want, ref))
