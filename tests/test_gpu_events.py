"""GPU tier: the evidence track (-oev) accumulated on the device behind the post-filter (device/events_stage.h: a wave per printed clump, global atomics into one
five-channel array per index image).  Every comparison is with tests/events_oracle.py, which recomputes the track from SAM text alone; the tier runs with
YGPU_CHECK_STATE on (conftest.py), so every ygpu_run / ygpu_postfilter here also checks the state words."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import events_oracle as eo
import yaha_amd as ya
from conftest import golden_lines, strip_pg

pytestmark = pytest.mark.gpu

SETS = [("rchim_default", "rchim.fa"), ("r1k_default", "r1k.fa"), ("r10k_default", "r10k.fa"), ("rq_default", "rq.fq")]


def _cli(index11, reads, out, extra=(), oflag="-osh"):
    p = subprocess.run([ya.CLI_PATH, "-x", index11, "-q", reads, oflag, "stdout", "-oev", out] + list(extra), env=dict(os.environ, YAHA_STATS="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    assert "state check" not in err, err[-2000:]                                       # YGPU_CHECK_STATE stays silent (a dirty word also fails the run)
    st = json.loads([l for l in err.split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])
    return p.stdout.decode(), open(out).read(), st


def _events(name, B, Q=0, N=1):
    lines = golden_lines(name); sq = eo.sq_table(lines)
    return eo.events(lines, sq, B, Q, N), sq


def _expected(name, B, Q=0, N=1):
    ev, sq = _events(name, B, Q, N)
    return eo.text(ev, sq, B)


@pytest.mark.parametrize("name,reads", SETS)
def test_command_line_track_is_counted_by_the_kernel_and_equals_the_oracle(work, index11, tmp_path, name, reads):
    out = str(tmp_path / "ev.tsv"); lines = golden_lines(name); q = os.path.join(work, reads)
    for extra, B, Q, N in ((["-evbin", "1"], 1, 0, 1), (["-evbin", "37", "-ctx", "1"], 37, 0, 1), (["-ctx", "3", "-batch", "17"], 100, 0, 1), (["-evq", "10"], 100, 10, 1),
                           (["-evbin", "37", "-evq", "200", "-batch", "9"], 37, 200, 1), (["-evclip", "20", "-ctx", "2", "-batch", "33"], 100, 0, 20)):
        sam, got, st = _cli(index11, q, out, extra)
        assert strip_pg(sam) == lines, (name, extra)
        ev, sq = _events(name, B, Q, N)
        assert all(t > 0 for t in eo.totals(ev)), (name, extra, eo.totals(ev))             # an empty channel proves nothing
        assert got == eo.text(ev, sq, B), (name, extra)
        # the kernel did the counting, not the host's fallback
        assert st["events_device_records"] == eo.records(lines, Q) > 0 and st["events_host_records"] == 0, (extra, st)
        assert st["events_bins"] == eo.n_bins(sq, B) and st["events_counted"] == sum(eo.totals(ev))
    # the host's post-filter by option: the reverse, and the same file
    sam, got, st = _cli(index11, q, out, ["-evbin", "37", "-dpf", "N"])
    assert strip_pg(sam) == lines and got == _expected(name, 37)
    assert st["events_device_records"] == 0 and st["events_host_records"] == eo.records(lines) > 0


def test_command_line_other_formats_both_tracks_and_the_handed_back_reads(work, index11, tmp_path, monkeypatch):
    out = str(tmp_path / "ev.tsv"); q = os.path.join(work, "rchim.fa"); want = _expected("rchim_default", 37)
    for oflag in ("-oss", "-o8"):
        _sam, got, st = _cli(index11, q, out, ["-evbin", "37"], oflag=oflag)
        assert got == want and st["events_host_records"] == 0
    # the direct-atomics variant of the kernel (the measurement switch): the same counts
    monkeypatch.setenv("YGPU_EVENTS_DIRECT", "1")
    _sam, got, st = _cli(index11, q, out, ["-evbin", "37"])
    assert got == want and st["events_host_records"] == 0
    monkeypatch.delenv("YGPU_EVENTS_DIRECT")
    # both tracks at once, each counted by its own kernel; the depth file is what a run without -oev writes
    cov = str(tmp_path / "cov.bg"); cov2 = str(tmp_path / "cov2.bg")
    _sam, got, st = _cli(index11, q, out, ["-evbin", "37", "-ocov", cov, "-covbin", "37"])
    assert got == want and st["events_host_records"] == 0 and st["depth_host_records"] == 0 and st["depth_device_records"] == st["events_device_records"] > 0
    p = subprocess.run([ya.CLI_PATH, "-x", index11, "-q", q, "-osh", "stdout", "-ocov", cov2, "-covbin", "37"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and open(cov).read() == open(cov2).read() != ""
    # reads of more than three clumps come back unfiltered (the hand-over path of the device stage): the host counts exactly those, the device the rest
    monkeypatch.setenv("YGPU_OQC_MAX", "3")
    sam, got, st = _cli(index11, q, out, ["-evbin", "37"])
    assert strip_pg(sam) == golden_lines("rchim_default") and got == want
    assert st["events_host_records"] > 0 and st["events_device_records"] > 0 and st["events_host_records"] + st["events_device_records"] == eo.records(golden_lines("rchim_default"))


def _oracle_array(header, texts, B, Q=0, N=1):
    sq = eo.sq_table(header.split("\n"))
    lines = [l for t in texts for l in t.split("\n")]
    return np.array(eo.events(lines, sq, B, Q, N), dtype=np.uint32).reshape(-1, 5), eo.records(lines, Q), eo.records(lines, 0)


def test_abi_batches_accumulate_and_contexts_of_an_image_share_one_array(work, index11):
    B = 37
    with ya.Session(["-x", index11, "-q", os.path.join(work, "rchim.fa"), "-osh", "stdout", "-oev", "unused.tsv", "-evbin", str(B), "-evclip", "3"]) as s:
        with ya.Context(s.index, s.params) as a:
            a.set_postfilter(s); a.events_enable(s)
            with ya.Context(s.index, s.params, parent=a) as b:
                b.set_postfilter(s); b.events_enable(s)
                texts = []
                for k, ctx in enumerate((a, a, b, a, b)):
                    rb = s.next_batch(40)
                    assert rb.n_reads > 0
                    ctx.upload(rb); ctx.run()
                    texts.append(s.emit_filtered(ctx.postfilter()))
                    want, n_rec, _ = _oracle_array(s.header(), texts, B, 0, 3)
                    got, st = ctx.events_collect()
                    assert got.shape == want.shape and got.dtype == np.uint32 and np.array_equal(got, want), k
                    assert st["records_counted"] == n_rec and st["reads_left_to_host"] == 0
                # both contexts see the same array, and every channel has something in it
                ga, _ = a.events_collect(); gb, _ = b.events_collect()
                assert np.array_equal(ga, gb) and (ga.sum(axis=0) > 0).all()
                # a sibling that is parked gives up nothing of the image's
                b.park()
                gp, _ = a.events_collect()
                assert np.array_equal(gp, ga)
            # a second enable with other parameters on the same image is refused
            for other in (["-evbin", "50", "-evclip", "3"], ["-evbin", str(B), "-evclip", "4"], ["-evbin", str(B), "-evclip", "3", "-evq", "1"]):
                with ya.Session(["-x", index11, "-q", os.path.join(work, "rchim.fa"), "-osh", "stdout", "-oev", "unused.tsv"] + other) as s2:
                    with pytest.raises(RuntimeError):
                        a.events_enable(s2)


# (the sessions below take -evbin / -evq / -evclip from their arguments, and those need -oev; a session never writes the file)
def _seq_table(s):
    p = ya.EventsParams()
    assert ya.lib().yaha_session_events_params(s._h, C.byref(p)) == 0
    st = C.cast(p.seq_start, C.POINTER(C.c_uint32)); ln = C.cast(p.seq_length, C.POINTER(C.c_uint32))
    return [(int(st[i]), int(ln[i])) for i in range(p.n_seqs)], p


def _qlens(rb):
    off = C.cast(rb.offsets, C.POINTER(C.c_uint64))
    return [int(off[i + 1] - off[i]) for i in range(rb.n_reads)]


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
    N = 6
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout", "-oev", "unused.tsv", "-evbin", str(B), "-evclip", str(N)]) as s:
        seqs, p = _seq_table(s)
        assert (p.bin, p.min_mapq, p.min_clip) == (B, 0, N)
        big = max(range(len(seqs)), key=lambda i: seqs[i][1]); assert seqs[big][1] > 31000 and len(seqs) >= 2
        (s0, l0), (s1, l1) = seqs[0], seqs[1]
        with ya.Context(s.index, s.params) as ctx:
            ctx.set_postfilter(s); ctx.events_enable(s)
            rb = s.next_batch(12); assert rb.n_reads == 12
            ql = _qlens(rb); assert min(ql) > 600
            ctx.upload(rb)
            cases = {
                0: [(s0 + 90, 0, ql[0] - 1, [(M, 7), (R, 6), (M, 10)])],                            # an R run across a bin edge, no clips
                1: [(s1 + l1 - 17, 0, ql[1] - 1, [(M, 10), (R, 1), (M, 5), (D, 1)])],               # ends on the last, short bin of a sequence
                2: [(s0 + l0 - 10, 50, 99, [(M, 5), (R, 15)])],                                     # spans two sequences: not printed, counts nothing
                3: [(s0 + 300, 0, ql[3] - 1, [(M, 96), (I, 3), (D, 4), (M, 20), (I, 2)])],          # an I directly before a D, an I as the last op
                4: [(seqs[big][0] + 500, 0, ql[4] - 1, [(M, 30000)])],                              # 30 000 matching bases: no event at all
                5: [(s0 + 2000, 0, ql[5] - 1, [(M, 3), (R, 1)] * 100 + [(D, 2), (I, 3), (M, 100)])],      # more ops than the wave has lanes; R, D and I in the fourth chunk
                6: [(s0 + 5000, 0, ql[6] - 1, [(M, 50), (D, 5)] * 70 + [(M, 50)])],                 # 70 short D runs
                7: [(s0 + 9000, N - 1, ql[7] - 1 - (N - 1), [(M, 50)])],                            # clips of N - 1 on both sides: no event
                8: [(s0 + 9100, N, ql[8] - 1 - N, [(M, 50)])],                                      # clips of exactly N: one each
                9: [(s0 + 9200, N, ql[9] - 1 - (N - 1), [(M, 50)])],                                # left only
                10: [(s0 + 9300, N - 1, ql[10] - 1 - N, [(M, 50)])],                                # right only
            }
            r, _keep = _batch(12, cases)
            ctx.inject_results(r)
            text = s.emit_filtered(ctx.postfilter())
            want, n_rec, _ = _oracle_array(s.header(), [text], B, 0, N)
            assert n_rec == 10                                                                      # all but the clump across two sequences are printed
            got, st = ctx.events_collect()
            assert np.array_equal(got, want)
            assert got.sum(axis=0).tolist() == [6 + 1 + 100, 1 + 4 + 2 + 350, 2 + 1, 2, 2]
            assert st == {"records_counted": 10, "records_skipped_mapq": 0, "records_dropped_two_sequences": 1, "reads_left_to_host": 0}
            # a read with more clumps than the stage takes is handed back: counted as such, nothing of it counted on the device
            many = [(s0 + 1000 + 40 * k, (k * 7) % 500 + 10, (k * 7) % 500 + 39, [(M, 20), (R, 2), (M, 8)]) for k in range(1800)]
            r2, _keep2 = _batch(12, {7: many})
            ctx.inject_results(r2)
            f = ctx.postfilter()
            assert f.n_clumps == 1800 and f.clumps[0].primaryCount == 0xFFFF
            assert len(s.emit_filtered(f)) > 0
            got2, st2 = ctx.events_collect()
            assert np.array_equal(got2, want)
            assert st2 == {"records_counted": 10, "records_skipped_mapq": 0, "records_dropped_two_sequences": 1, "reads_left_to_host": 1}


def test_the_mapping_quality_gate_on_the_device(work, index11):
    # a read with one clump is printed with MAPQ 250 (GraphPath.cpp:907-916): -evq 251 gates every such record, -evq 250 none
    for Q, counted in ((251, 0), (250, 3)):
        with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout", "-oev", "unused.tsv", "-evbin", "10", "-evq", str(Q)]) as s:
            seqs, _p = _seq_table(s)
            with ya.Context(s.index, s.params) as ctx:
                ctx.set_postfilter(s); ctx.events_enable(s)
                rb = s.next_batch(4); ctx.upload(rb)
                r, _keep = _batch(4, {k: [(seqs[0][0] + 100 * k + 7, 5, 54, [("M", 20), ("R", 3), ("D", 2), ("M", 25)])] for k in range(3)})
                ctx.inject_results(r)
                text = s.emit_filtered(ctx.postfilter())
                want, n_rec, n_all = _oracle_array(s.header(), [text], 10, Q)
                assert n_all == 3 and n_rec == counted
                got, st = ctx.events_collect()
                assert np.array_equal(got, want) and got.sum(axis=0).tolist() == [3 * counted, 2 * counted, 0, counted, counted]
                assert st["records_counted"] == counted and st["records_skipped_mapq"] == 3 - counted


def test_enable_needs_the_postfilter(work, index11):
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout"]) as s:
        with ya.Context(s.index, s.params) as ctx:
            with pytest.raises(RuntimeError, match="ygpu_set_postfilter"):
                ctx.events_enable(s)
            with pytest.raises(RuntimeError):
                ctx.events_collect()
