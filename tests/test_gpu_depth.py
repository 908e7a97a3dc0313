"""GPU tier: the read-depth track (-ocov) accumulated on the device behind the post-filter (device/depth_stage.h: a wave per printed clump, global atomics into
one coverage array per index image).  Every comparison is with tests/depth_oracle.py, which recomputes depth from SAM text alone; the tier runs with
YGPU_CHECK_STATE on (conftest.py), so every ygpu_run / ygpu_postfilter here also checks the state words."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import depth_oracle as do
import events_oracle as eo
import yaha_amd as ya
from conftest import golden_lines, strip_pg

pytestmark = pytest.mark.gpu

SETS = [("rchim_default", "rchim.fa"), ("r1k_default", "r1k.fa"), ("r10k_default", "r10k.fa"), ("rq_default", "rq.fq")]


def _cli(index11, reads, out, extra=(), oflag="-osh"):
    p = subprocess.run([ya.CLI_PATH, "-x", index11, "-q", reads, oflag, "stdout", "-ocov", out] + list(extra), env=dict(os.environ, YAHA_STATS="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    assert "state check" not in err, err[-2000:]                                       # YGPU_CHECK_STATE stays silent (a dirty word also fails the run)
    st = json.loads([l for l in err.split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])
    return p.stdout.decode(), open(out).read(), st


def _expected(name, B, Q=0):
    lines = golden_lines(name); sq = do.sq_table(lines)
    return do.bedgraph(do.coverage(lines, sq, B, Q), sq, B)


@pytest.mark.parametrize("name,reads", SETS)
def test_command_line_track_is_counted_by_the_kernel_and_equals_the_oracle(work, index11, tmp_path, name, reads):
    out = str(tmp_path / "cov.bg"); lines = golden_lines(name); q = os.path.join(work, reads)
    for extra, B, Q in ((["-covbin", "1"], 1, 0), (["-covbin", "37", "-ctx", "1"], 37, 0), (["-ctx", "3", "-batch", "17"], 100, 0), (["-covq", "10"], 100, 10),
                        (["-covbin", "37", "-covq", "200", "-batch", "9"], 37, 200)):
        sam, got, st = _cli(index11, q, out, extra)
        assert strip_pg(sam) == lines, (name, extra)
        assert got == _expected(name, B, Q), (name, extra)
        # the kernel did the counting, not the host's fallback
        assert st["depth_device_records"] == do.records(lines, Q) > 0 and st["depth_host_records"] == 0, (extra, st)
        assert st["depth_bins"] == do.n_bins(do.sq_table(lines), B) and st["depth_covered_bases"] == sum(do.coverage(lines, do.sq_table(lines), B, Q))
    # the host's post-filter by option: the reverse, and the same file
    sam, got, st = _cli(index11, q, out, ["-covbin", "37", "-dpf", "N"])
    assert strip_pg(sam) == lines and got == _expected(name, 37)
    assert st["depth_device_records"] == 0 and st["depth_host_records"] == do.records(lines) > 0


def test_command_line_other_formats_and_the_handed_back_reads(work, index11, tmp_path, monkeypatch):
    out = str(tmp_path / "cov.bg"); q = os.path.join(work, "rchim.fa"); want = _expected("rchim_default", 37)
    for oflag in ("-oss", "-o8"):
        _sam, got, st = _cli(index11, q, out, ["-covbin", "37"], oflag=oflag)
        assert got == want and st["depth_host_records"] == 0
    # reads of more than three clumps come back unfiltered (the hand-over path of the device stage): the host counts exactly those, the device the rest
    monkeypatch.setenv("YGPU_OQC_MAX", "3")
    sam, got, st = _cli(index11, q, out, ["-covbin", "37"])
    assert strip_pg(sam) == golden_lines("rchim_default") and got == want
    assert st["depth_host_records"] > 0 and st["depth_device_records"] > 0 and st["depth_host_records"] + st["depth_device_records"] == do.records(golden_lines("rchim_default"))


def _oracle_array(header, texts, B, Q=0):
    sq = do.sq_table(header.split("\n"))
    lines = [l for t in texts for l in t.split("\n")]
    return np.array(do.coverage(lines, sq, B, Q), dtype=np.uint32), do.records(lines, Q), do.records(lines, 0)


def test_abi_batches_accumulate_and_contexts_of_an_image_share_one_array(work, index11):
    B = 37
    with ya.Session(["-x", index11, "-q", os.path.join(work, "rchim.fa"), "-osh", "stdout", "-ocov", "unused.bg", "-covbin", str(B)]) as s:
        with ya.Context(s.index, s.params) as a:
            a.set_postfilter(s); a.depth_enable(s)
            with ya.Context(s.index, s.params, parent=a) as b:
                b.set_postfilter(s); b.depth_enable(s)
                texts = []
                for k, ctx in enumerate((a, a, b, a, b)):
                    rb = s.next_batch(40)
                    assert rb.n_reads > 0
                    ctx.upload(rb); ctx.run()
                    texts.append(s.emit_filtered(ctx.postfilter()))
                    want, n_rec, _ = _oracle_array(s.header(), texts, B)
                    got, st = ctx.depth_collect()
                    assert got.shape == want.shape and np.array_equal(got, want), k
                    assert st["records_counted"] == n_rec and st["reads_left_to_host"] == 0
                # both contexts see the same array
                ga, _ = a.depth_collect(); gb, _ = b.depth_collect()
                assert np.array_equal(ga, gb) and ga.sum() > 0
                # a sibling that is parked gives up nothing of the image's
                b.park()
                gp, _ = a.depth_collect()
                assert np.array_equal(gp, ga)
            # a second enable with other parameters on the same image is refused
            with ya.Session(["-x", index11, "-q", os.path.join(work, "rchim.fa"), "-osh", "stdout", "-ocov", "unused.bg", "-covbin", "50"]) as s2:
                with pytest.raises(RuntimeError):
                    a.depth_enable(s2)


def test_depth_and_evidence_arrays_of_an_image_are_two_arrays_with_their_own_bins(work, index11):
    """Both kinds on the contexts of one image, with different bin sizes (37 and 50): the arrays live in one registry and one struct, so a key that did not tell
    the kinds apart, or one array serving both, shows as a wrong length or wrong counts.  Exact against the two oracles after every batch."""
    q = os.path.join(work, "rchim.fa"); BD, BE, CLIP = 37, 50, 3

    def session(covbin, evbin):
        return ya.Session(["-x", index11, "-q", q, "-osh", "stdout", "-ocov", "x", "-covbin", str(covbin), "-oev", "y", "-evbin", str(evbin), "-evclip", str(CLIP)])

    with session(BD, BE) as s:
        sq = do.sq_table(s.header().split("\n"))
        with ya.Context(s.index, s.params) as a:
            a.set_postfilter(s); a.depth_enable(s); a.events_enable(s)
            with ya.Context(s.index, s.params, parent=a) as b:
                b.set_postfilter(s); b.depth_enable(s); b.events_enable(s)
                lines = []
                for k, ctx in enumerate((a, a, b, a, b)):
                    rb = s.next_batch(40)
                    assert rb.n_reads > 0
                    ctx.upload(rb); ctx.run()
                    lines += s.emit_filtered(ctx.postfilter()).split("\n")
                    cov, _ = ctx.depth_collect(); ev, _ = ctx.events_collect()
                    assert np.array_equal(cov, np.array(do.coverage(lines, sq, BD, 0), dtype=np.uint32)), k
                    assert np.array_equal(ev, np.array(eo.events(lines, sq, BE, 0, CLIP), dtype=np.uint32).reshape(-1, 5)), k
                (ca, _), (cb, _), (ea, _), (eb, _) = a.depth_collect(), b.depth_collect(), a.events_collect(), b.events_collect()
                assert len(ca) == do.n_bins(sq, BD) != do.n_bins(sq, BE) == len(ea)
                assert np.array_equal(ca, cb) and np.array_equal(ea, eb)
                assert ca.sum() > 0 and all(t > 0 for t in ea.sum(axis=0)), (ca.sum(), ea.sum(axis=0))
                # a second enable of either kind with the OTHER kind's bin size is refused, and leaves the other kind's array alone
                with session(BE, BE) as s2:
                    with pytest.raises(RuntimeError, match="ygpu_depth_enable.*other parameters"):
                        a.depth_enable(s2)
                assert np.array_equal(a.events_collect()[0], ea) and np.array_equal(a.depth_collect()[0], ca)
                with session(BD, BD) as s3:
                    with pytest.raises(RuntimeError, match="ygpu_events_enable.*other parameters"):
                        a.events_enable(s3)
                assert np.array_equal(a.depth_collect()[0], ca) and np.array_equal(a.events_collect()[0], ea)


# (the sessions below take -covbin / -covq from their arguments, and those need -ocov; a session never writes the file)
def _seq_table(s):
    p = ya.DepthParams()
    assert ya.lib().yaha_session_depth_params(s._h, C.byref(p)) == 0
    st = C.cast(p.seq_start, C.POINTER(C.c_uint32)); ln = C.cast(p.seq_length, C.POINTER(C.c_uint32))
    return [(int(st[i]), int(ln[i])) for i in range(p.n_seqs)], p


def _batch(n_reads, per_read):
    """per_read[i] = list of (sro, sqo, eqo, ops) for read i; the ResultBatch ygpu_inject_results takes (and the arrays that keep it alive)."""
    recs, ops, starts = [], [], [0]
    for i in range(n_reads):
        for sro, sqo, eqo, o in per_read.get(i, []):
            rlen = sum(n for c, n in o if c in "MRD")
            recs.append((sro, sqo, eqo, rlen, 30, eqo - sqo + 1, sum(n for c, n in o if c == "M"), sum(n for c, n in o if c == "R"), sum(n for c, n in o if c in "ID"), 0, 0, len(ops), len(o)))
            ops.extend(n | (ord(c) << 16) for c, n in o)
        starts.append(len(recs))
    cs = (C.c_uint32 * len(starts))(*starts); cl = (ya.Clump * max(1, len(recs)))(*[ya.Clump(*r) for r in recs]); op = (C.c_uint32 * max(1, len(ops)))(*ops)
    r = ya.ResultBatch(); r.n_reads = n_reads; r.clump_start = cs; r.clumps = cl; r.ops = op; r.n_clumps = len(recs); r.n_ops = len(ops)
    return r, (cs, cl, op)


@pytest.mark.parametrize("B", [1, 100])
def test_synthetic_clumps_through_the_stage(work, index11, B):
    M, R, I, D = "MRID"
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout", "-ocov", "unused.bg", "-covbin", str(B)]) as s:
        seqs, _p = _seq_table(s)
        big = max(range(len(seqs)), key=lambda i: seqs[i][1]); assert seqs[big][1] > 31000 and len(seqs) >= 2
        (s0, l0), (s1, l1) = seqs[0], seqs[1]
        with ya.Context(s.index, s.params) as ctx:
            ctx.set_postfilter(s); ctx.depth_enable(s)
            rb = s.next_batch(10); assert rb.n_reads == 10
            ctx.upload(rb)
            cases = {
                0: [(s0 + 95, 0, 19, [(M, 20)])],                                                   # a run crossing a bin edge
                1: [(s1 + l1 - 17, 0, 16, [(M, 10), (R, 1), (M, 6)])],                              # ends on the last, short bin of a sequence
                2: [(s0 + l0 - 10, 0, 19, [(M, 20)])],                                              # spans two sequences: not printed, counts nothing
                3: [(s0 + 300, 0, 126, [(M, 40), (D, 30), (M, 10), (I, 7), (R, 2), (M, 68)])],      # D and I in the middle
                4: [(seqs[big][0] + 500, 0, 99, [(M, 30000)])],                                     # one run of 30 000 bases: the load-balance case
                5: [(s0 + 2000, 0, 499, [(M, 3), (R, 1)] * 100 + [(D, 2), (M, 100)])],              # more ops than the wave has lanes, a D in the fourth chunk
                6: [(s0 + 5000, 0, 99, [(M, 50), (D, 5)] * 70 + [(M, 50)])],                        # many runs
            }
            r, _keep = _batch(10, cases)
            ctx.inject_results(r)
            text = s.emit_filtered(ctx.postfilter())
            want, n_rec, _ = _oracle_array(s.header(), [text], B)
            assert n_rec == 6                                                                       # all but the clump across two sequences are printed
            got, st = ctx.depth_collect()
            assert np.array_equal(got, want)
            assert int(got.sum()) == 20 + 17 + 120 + 30000 + 400 + 100 + 71 * 50
            assert st == {"records_counted": 6, "records_skipped_mapq": 0, "records_dropped_two_sequences": 1, "reads_left_to_host": 0}
            # a read with more clumps than the stage takes is handed back: counted as such, nothing of it counted on the device
            many = [(s0 + 1000 + 40 * k, (k * 7) % 900, (k * 7) % 900 + 29, [(M, 30)]) for k in range(1800)]
            r2, _keep2 = _batch(10, {7: many})
            ctx.inject_results(r2)
            f = ctx.postfilter()
            assert f.n_clumps == 1800 and f.clumps[0].primaryCount == 0xFFFF
            assert len(s.emit_filtered(f)) > 0
            got2, st2 = ctx.depth_collect()
            assert np.array_equal(got2, want)
            assert st2 == {"records_counted": 6, "records_skipped_mapq": 0, "records_dropped_two_sequences": 1, "reads_left_to_host": 1}


def test_the_mapping_quality_gate_on_the_device(work, index11):
    # a read with one clump is printed with MAPQ 250 (GraphPath.cpp:907-916): -covq 251 gates every such record, -covq 250 none
    for Q, counted in ((251, 0), (250, 3)):
        with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout", "-ocov", "unused.bg", "-covbin", "10", "-covq", str(Q)]) as s:
            seqs, _p = _seq_table(s)
            with ya.Context(s.index, s.params) as ctx:
                ctx.set_postfilter(s); ctx.depth_enable(s)
                rb = s.next_batch(4); ctx.upload(rb)
                r, _keep = _batch(4, {k: [(seqs[0][0] + 100 * k + 7, 0, 49, [("M", 50)])] for k in range(3)})
                ctx.inject_results(r)
                text = s.emit_filtered(ctx.postfilter())
                want, n_rec, n_all = _oracle_array(s.header(), [text], 10, Q)
                assert n_all == 3 and n_rec == counted
                got, st = ctx.depth_collect()
                assert np.array_equal(got, want) and int(got.sum()) == 50 * counted
                assert st["records_counted"] == counted and st["records_skipped_mapq"] == 3 - counted


def test_enable_needs_the_postfilter_and_room(work, index11):
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout"]) as s:
        with ya.Context(s.index, s.params) as ctx:
            with pytest.raises(RuntimeError, match="ygpu_set_postfilter"):
                ctx.depth_enable(s)
            with pytest.raises(RuntimeError):
                ctx.depth_collect()
