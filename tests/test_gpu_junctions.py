"""GPU tier: split-read breakpoint calls (-obp) made on the device behind the post-filter (device/junction_stage.h: a wave per read counts its eligible records, an
exclusive sum places the junctions, a second pass ranks the records and writes them).  Every comparison is with tests/junction_oracle.py, which recomputes the
junctions, the clusters and the file from SAM text alone; the tier runs with YGPU_CHECK_STATE on (conftest.py).

One case of the issue cannot be built: "all primary, with a tie in qs".  The post-filter accepts node j behind node i on a path only when SQO_j - SQO_i >= -MNO, and
the device stage insists on -MNO >= 1 (oqc_core.h, ygpu_set_postfilter), so two primary records of a read never start on the same read-forward base.  The long read
below therefore has its pieces' starts all different; the (qs, qe, print order) tie-break is exercised where it can occur, on the shared routine
(tests/test_junctions_cpu.py::test_the_shared_routine_on_hand_made_records_with_ties)."""
import ctypes as C
import json
import os
import subprocess

import pytest

import junction_oracle as jo
import yaha_amd as ya
from conftest import golden_lines, strip_pg

pytestmark = pytest.mark.gpu


def _cli(index11, reads, out, extra=(), oflag="-osh", env=None):
    e = dict(os.environ, YAHA_STATS="1"); e.update(env or {})
    p = subprocess.run([ya.CLI_PATH, "-x", index11, "-q", reads, oflag, "stdout", "-obp", out] + list(extra), env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    assert "state check" not in err, err[-2000:]                                       # YGPU_CHECK_STATE stays silent (a dirty word also fails the run)
    st = json.loads([l for l in err.split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])
    return p.stdout.decode(), open(out).read(), st


def _reads_with_junctions(lines, Q=0):
    return len({r for r, _j in jo.junctions(lines, Q, with_reads=True)})


RUNS = [  # golden set, reads, the set's own options, extra options, output flag, -bpq, -bpw
    ("rsv_default", "rsv.fa", [], [], "-osh", 0, 10),
    ("rsv_default", "rsv.fa", [], ["-ctx", "1", "-batch", "17", "-bpw", "0"], "-osh", 0, 0),
    ("rsv_default", "rsv.fa", [], ["-ctx", "3", "-batch", "40", "-bpq", "30"], "-osh", 30, 10),
    ("rsv_default", "rsv.fa", [], ["-batch", "33"], "-oss", 0, 10),
    ("rsv_default", "rsv.fa", [], ["-ctx", "2"], "-o8", 0, 10),
    ("rsv_OQC_FBS", "rsv.fa", ["-OQC", "Y", "-FBS", "Y"], ["-batch", "64"], "-osh", 0, 10),
    ("rchim_default", "rchim.fa", [], [], "-osh", 0, 10),
    ("rchim_default", "rchim.fa", [], ["-ctx", "2", "-batch", "9", "-bpq", "30", "-bpw", "0"], "-osh", 30, 0),
]


@pytest.mark.parametrize("name,reads,gext,extra,oflag,Q,W", RUNS)
def test_command_line_junctions_are_made_by_the_kernels_and_the_file_equals_the_oracle(work, index11, tmp_path, name, reads, gext, extra, oflag, Q, W):
    out = str(tmp_path / "bp.bedpe"); lines = golden_lines(name)
    sam, got, st = _cli(index11, os.path.join(work, reads), out, gext + extra, oflag=oflag)
    if oflag == "-osh":
        assert strip_pg(sam) == lines
    junc = jo.junctions(lines, Q); cl = jo.clusters(junc, W)
    # every type is there, whatever the gates, and rsv has clusters of several reads: an empty class proves nothing
    assert all(v > 0 for v in jo.by_type(junc).values()), jo.by_type(junc)
    if name.startswith("rsv") and W:
        assert any(len(c) >= 2 for c in cl)
    assert got == jo.text(cl, jo.sq_table(lines))
    # the kernels made them, not the host's routine
    assert st["bp_host_reads"] == 0 and st["bp_device_reads"] == _reads_with_junctions(lines, Q) > 0, st
    assert st["bp_junctions"] == len(junc) and st["bp_clusters"] == len(cl)


@pytest.mark.parametrize("name,reads", [("rsv_default", "rsv.fa"), ("rchim_default", "rchim.fa")])
def test_command_line_host_filter_and_handed_back_reads_give_the_same_file(work, index11, tmp_path, name, reads):
    out = str(tmp_path / "bp.bedpe"); lines = golden_lines(name); want = jo.expected(lines); q = os.path.join(work, reads)
    # the host's post-filter by option: the device makes nothing, the file is the same
    sam, got, st = _cli(index11, q, out, ["-dpf", "N"])
    assert strip_pg(sam) == lines and got == want
    assert st["bp_device_reads"] == 0 and st["bp_host_reads"] == _reads_with_junctions(lines) > 0
    # reads of more than three clumps come back unfiltered (the hand-over path of the device stage): the host makes exactly theirs, the device the rest
    sam, got, st = _cli(index11, q, out, ["-batch", "50"], env={"YGPU_OQC_MAX": "3"})
    assert strip_pg(sam) == lines and got == want
    assert st["bp_host_reads"] > 0 and st["bp_device_reads"] > 0 and st["bp_host_reads"] + st["bp_device_reads"] == _reads_with_junctions(lines)


# ---- the ABI on injected clump lists ---------------------------------------------------------------------------------------------------------------------------
def _params(s):
    p = ya.JunctionParams()
    assert ya.lib().yaha_session_junction_params(s._h, C.byref(p)) == 0
    st = C.cast(p.seq_start, C.POINTER(C.c_uint32)); ln = C.cast(p.seq_length, C.POINTER(C.c_uint32))
    return [(int(st[i]), int(ln[i])) for i in range(p.n_seqs)], p


def _qlens(rb):
    off = C.cast(rb.offsets, C.POINTER(C.c_uint64))
    return [int(off[i + 1] - off[i]) for i in range(rb.n_reads)]


def _batch(n_reads, per_read, ql):
    """per_read[i] = list of (reference offset, qs, qe, reversed, score) in READ-FORWARD query coordinates, all-match pieces; the ResultBatch ygpu_inject_results takes."""
    recs, ops, starts = [], [], [0]
    for i in range(n_reads):
        for sro, qs, qe, rev, score in per_read.get(i, []):
            n = qe - qs + 1
            sqo, eqo = (ql[i] - 1 - qe, ql[i] - 1 - qs) if rev else (qs, qe)
            recs.append((sro, sqo, eqo, n, score, n, n, 0, 0, 1 if rev else 0, 0, len(ops), 1))
            ops.append(n | (ord("M") << 16))
        starts.append(len(recs))
    cs = (C.c_uint32 * len(starts))(*starts); cl = (ya.Clump * max(1, len(recs)))(*[ya.Clump(*r) for r in recs]); op = (C.c_uint32 * max(1, len(ops)))(*ops)
    r = ya.ResultBatch(); r.n_reads = n_reads; r.clump_start = cs; r.clumps = cl; r.ops = op; r.n_clumps = len(recs); r.n_ops = len(ops)
    return r, (cs, cl, op)


def _tuple(j):
    return (j.seqA, j.posA, chr(j.strandA), j.seqB, j.posB, chr(j.strandB), ya.JUNCTION_TYPES[j.type], j.qgap)


def _check_against_text(got, st, header, text, Q, n_reads):
    """The device's junctions of a batch against the oracle over the text the batch prints; returns them grouped by read."""
    lines = header.split("\n") + text.split("\n")
    want = jo.junctions(lines, Q, with_reads=True)
    # (read, ordinal) order, ordinals 0, 1, 2 ... within a read
    keys = [(j.read, j.ordinal) for j in got]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and all(j.read < n_reads and j.reserved == 0 for j in got)
    by_read = {}
    for j in got:
        by_read.setdefault(j.read, []).append(_tuple(j))
        assert j.ordinal == len(by_read[j.read]) - 1
    want_groups = {}
    for r, j in want:
        want_groups.setdefault(r, []).append(j)
    # (the oracle numbers the reads that print something; the device the reads of the batch: the same order)
    assert [by_read[r] for r in sorted(by_read)] == [want_groups[r] for r in sorted(want_groups)]
    assert st["reads_with_junctions"] == len(by_read) and st["junctions"] == len(got) and st["reads_left_to_host"] == 0
    return by_read


def test_abi_junctions_of_injected_batches_equal_the_oracle(work, index11):
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r10k.fa"), "-osh", "stdout", "-obp", "unused.bedpe", "-bpq", "250"]) as s:
        seqs, p = _params(s)
        assert p.min_mapq == 250 and len(seqs) >= 2
        big = max(range(len(seqs)), key=lambda i: seqs[i][1]); B0, BL = seqs[big]; assert BL > 31000
        oth = [i for i in range(len(seqs)) if i != big][0]; O0, OL = seqs[oth]; assert OL > 2000
        (s0, l0) = seqs[0]; assert l0 > 3400
        with ya.Context(s.index, s.params) as ctx:
            ctx.set_postfilter(s); ctx.junctions_enable(s)
            rb = s.next_batch(10); assert rb.n_reads == 10
            ql = _qlens(rb); assert min(ql) > 8000
            ctx.upload(rb)
            L = 70                                                                             # the long read: 70 pieces of 60 bases, 100 apart on the read, shuffled on the reference
            cases = {
                0: [(B0 + 1000, 0, 299, False, 300), (B0 + 5000, 300, 699, False, 400)],                       # a deletion, read from the forward strand
                1: [(B0 + 5000, 0, 399, True, 400), (B0 + 1000, 400, 699, True, 300)],                         # the same two pieces read from the other strand
                2: [(B0 + 9000, 400, 799, False, 400), (B0 + 2000, 0, 449, False, 450), (B0 + 20000, 850, 1300, True, 451)],      # three pieces: overlap, gap, an inversion
                3: [(B0 + 3000, 0, 499, False, 500), (O0 + 100, 500, 999, False, 500)],                        # two sequences
                4: [(s0 + 500, 0, 299, False, 300), (s0 + l0 - 10, 300, 359, False, 60), (s0 + 3000, 360, 700, True, 341)],      # the middle piece spans two sequences
                5: [(B0 + 11000, 0, 299, False, 300), (B0 + 12000, 300, 599, False, 300), (B0 + 13000, 600, 899, False, 300),
                    (B0 + 25000, 300, 599, False, 280)],                                               # a rival of the second piece: that one's MAPQ falls below 250
                6: [(B0 + 15000, 100, 4000, False, 3901)],                                                 # one piece
                7: [(B0 + 1000 + 400 * ((37 * k) % L), 100 * k + (k % 3), 100 * k + 59 + (k % 3), (k % 5) == 2, 60) for k in range(L)],
            }
            r, _keep = _batch(10, cases, ql)
            for Q in (250, 0):                                                                  # (a second enable replaces the parameters)
                p.min_mapq = Q
                assert ya.lib().ygpu_junctions_enable(ctx._h, C.byref(p)) == 0
                ctx.inject_results(r)
                text = s.emit_filtered(ctx.postfilter())
                got, st = ctx.junctions_collect()
                by_read = _check_against_text(got, st, s.header(), text, Q, 10)
                recs = [l.split("\t") for l in text.split("\n") if l]
                names = []
                for f in recs:
                    if f[0] not in names:
                        names.append(f[0])
                assert len(names) == 8                                                          # reads 0 .. 7 print, in order
                prim = lambda i: [f for f in recs if f[0] == names[i] and int([x for x in f if x.startswith("YF:H:")][0][5:], 16) & 0x20]
                # the same molecule from both strands: one junction each, the same one
                assert by_read[0] == by_read[1] == [(big, 1299, "+", big, 5000, "+", "DEL", 0)]
                assert by_read[2] == [(big, 2449, "+", big, 9000, "+", "DEL", -50), (big, 9399, "+", big, 20450, "-", "INV", 50)]
                assert [j[6] for j in by_read[3]] == ["TRA"]
                # the piece across two sequences is not printed: its neighbours join each other, with the unaligned bases between them
                assert len(prim(4)) == 2 and len(by_read[4]) == 1 and by_read[4][0][6:] == ("INV", 60)
                # the second piece's mapping quality is below 250, the others' is not: at -bpq 250 the first joins the third
                mq = [int(f[4]) for f in prim(5)]
                assert len(mq) == 3 and sorted(mq)[0] < 250 and sorted(mq)[1:] == [250, 250]
                assert len(by_read[5]) == (1 if Q == 250 else 2) and st["records_skipped_mapq"] == (1 if Q == 250 else 0)
                if Q == 250:
                    assert by_read[5] == [(big, 11299, "+", big, 13000, "+", "DEL", 300)]
                assert 6 not in by_read
                # more records than the wave has lanes, all primary, in a read-forward order that is not the reference's
                assert len(prim(7)) == L > 64 and len(by_read[7]) == L - 1
                assert len({j[6] for j in by_read[7]}) >= 3
                # handed out as often as asked, until the next ygpu_postfilter
                again, st2 = ctx.junctions_collect()
                assert [_tuple(j) for j in again] == [_tuple(j) for j in got] and st2 == st
            # a batch without any clump: no junctions, and the previous batch's are gone
            r0, _keep0 = _batch(10, {}, ql)
            ctx.inject_results(r0)
            assert s.emit_filtered(ctx.postfilter()) == ""
            got, st = ctx.junctions_collect()
            assert got == [] and st["junctions"] == 0
            # a read with more clumps than the stage takes is handed back: counted, no junction of it on the device
            many = [(B0 + 1000 + 40 * k, 4 * k, 4 * k + 29, False, 30) for k in range(1800)]
            r2, _keep2 = _batch(10, {0: cases[0], 3: many}, ql)
            ctx.inject_results(r2)
            f = ctx.postfilter()
            assert f.n_clumps == 1802 and f.clumps[2].primaryCount == 0xFFFF
            got, st = ctx.junctions_collect()
            assert [_tuple(j) for j in got] == [(big, 1299, "+", big, 5000, "+", "DEL", 0)] and got[0].read == 0
            assert st == {"reads_with_junctions": 1, "junctions": 1, "records_skipped_mapq": 0, "reads_left_to_host": 1}


def test_enable_needs_the_postfilter_and_collect_needs_enable(work, index11):
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout"]) as s:
        with ya.Context(s.index, s.params) as ctx:
            with pytest.raises(RuntimeError, match="ygpu_set_postfilter"):
                ctx.junctions_enable(s)
            with pytest.raises(RuntimeError, match="ygpu_junctions_enable"):
                ctx.junctions_collect()
            ctx.set_postfilter(s); ctx.junctions_enable(s)
            with pytest.raises(RuntimeError, match="ygpu_postfilter"):                          # enabled, but no batch has been filtered yet
                ctx.junctions_collect()
