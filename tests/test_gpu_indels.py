"""GPU tier: indel alleles (-oid) counted on the device behind the post-filter (device/indel_stage.h: a wave per printed clump, a lane per op, a hash table
per context filled with compare-and-swap on the key's three words; drained by count / exclusive sums / emit).  Every comparison is with
tests/indel_oracle.py, which recomputes the alleles from SAM text alone; the tier runs with YGPU_CHECK_STATE on (conftest.py), so every ygpu_run /
ygpu_postfilter here also checks the state words.

One case of the issue is built with insertions where it says deletions: equal deletions cannot meet in one clump (a D op moves the reference cursor, so the
next D has another slot), equal insertions can (an I op does not) -- 64 one-base insertions in a run of one letter are the 64 lanes with one key."""
import collections
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import indel_oracle as io
import yaha_amd as ya
from conftest import golden_lines, strip_pg

pytestmark = pytest.mark.gpu

SETS = [("rsv_default", "rsv.fa"), ("rchim_default", "rchim.fa"), ("r10k_default", "r10k.fa")]
OPS = {"rsv_default": 1458, "rchim_default": 621, "r10k_default": 905}


def _cli(index11, reads, out, extra=(), env=None):
    p = subprocess.run([ya.CLI_PATH, "-x", index11, "-q", reads, "-osh", "stdout", "-oid", out] + list(extra), env=dict(os.environ, YAHA_STATS="1", **(env or {})),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    assert "state check" not in err, err[-2000:]                                       # YGPU_CHECK_STATE stays silent (a dirty word also fails the run)
    st = json.loads([l for l in err.split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])
    return p.stdout.decode(), open(out).read(), st


@functools.lru_cache(maxsize=None)
def _oracle(name, Q=0, L=1):
    lines = golden_lines(name); sq = io.sq_table(lines)
    return io.alleles(lines, sq, Q, L), sq


def _expected(name, min_count=1, Q=0, L=1, times=1):
    al, sq = _oracle(name, Q, L)
    return io.text(al, sq, min_count, times)


@pytest.mark.parametrize("name,reads", SETS)
def test_command_line_file_is_counted_by_the_kernel_and_equals_the_oracle(work, index11, tmp_path, name, reads):
    out = str(tmp_path / "id.tsv"); lines = golden_lines(name); q = os.path.join(work, reads)
    want = _expected(name)
    assert want.count("\n") == OPS[name]
    for extra in (["-ctx", "1", "-batch", "9"], ["-ctx", "2", "-batch", "17"], ["-ctx", "3", "-batch", "33"]):
        sam, got, st = _cli(index11, q, out, ["-idmin", "1"] + extra)
        assert strip_pg(sam) == lines, (name, extra)
        assert got == want, (name, extra)
        assert st["indel_host_records"] == 0 and st["indel_device_records"] == io.records(lines) > 0 and st["indel_lost"] == 0, (extra, st)
        assert st["indel_events"] == st["indel_alleles"] == st["indel_lines"] == OPS[name]


def _doubled(work, tmp_path):
    src = open(os.path.join(work, "rsv.fa")).read().split(">")[1:]
    path = str(tmp_path / "rsv2.fa")
    with open(path, "w") as f:
        for rec in src:
            head, _, body = rec.partition("\n")
            f.write(">%s_a\n%s>%s_b\n%s" % (head.split()[0], body, head.split()[0], body))
    return path


def test_command_line_doubled_input(work, index11, tmp_path):
    out = str(tmp_path / "id.tsv"); reads = _doubled(work, tmp_path)
    _sam, got, st = _cli(index11, reads, out, ["-idmin", "2"])
    assert got == _expected("rsv_default", 2, times=2) and got.count("\n") == 1458
    assert st["indel_host_records"] == 0 and st["indel_events"] == 2 * 1458 and st["indel_alleles"] == 1458 and st["indel_lost"] == 0
    _sam, got, st = _cli(index11, reads, out, ["-idmin", "3"])
    assert got == "" and st["indel_lines"] == 0 and st["indel_alleles"] == 1458
    _sam, got, st = _cli(index11, reads, out, ["-idlen", "2", "-ctx", "2", "-batch", "40"])
    assert got == _expected("rsv_default", 2, L=2, times=2) and got.count("\n") == 1004 and st["indel_host_records"] == 0


def test_command_line_other_paths(work, index11, tmp_path):
    out = str(tmp_path / "id.tsv"); q = os.path.join(work, "rchim.fa"); lines = golden_lines("rchim_default"); want = _expected("rchim_default")
    # the host's post-filter by option: the formatters count everything
    sam, got, st = _cli(index11, q, out, ["-idmin", "1", "-dpf", "N"])
    assert strip_pg(sam) == lines and got == want and st["indel_device_records"] == 0 and st["indel_host_records"] == io.records(lines)
    # reads of more than three clumps come back unfiltered: the host counts exactly those, the device the rest
    sam, got, st = _cli(index11, q, out, ["-idmin", "1", "-batch", "50"], env={"YGPU_OQC_MAX": "3"})
    assert strip_pg(sam) == lines and got == want
    assert st["indel_host_records"] > 0 and st["indel_device_records"] > 0 and st["indel_host_records"] + st["indel_device_records"] == io.records(lines)
    # two index images (the same device twice), two contexts each: four tables
    sam, got, st = _cli(index11, q, out, ["-idmin", "1", "-gpus", "2", "-ctx", "2", "-batch", "25"], env={"YAHA_DEVICES": "0,0"})
    assert strip_pg(sam) == lines and got == want
    assert st["indel_host_records"] == 0 and st["indel_device_records"] == io.records(lines) and all(n > 0 for n in st["reads_per_device"])
    # a run without the option has none of the keys, and the same alignments
    p = subprocess.run([ya.CLI_PATH, "-x", index11, "-q", q, "-osh", "stdout"], env=dict(os.environ, YAHA_STATS="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and strip_pg(p.stdout.decode()) == lines and "indel_" not in p.stderr.decode()


# ---- the stage on injected batches ------------------------------------------------------------------------------------------------------------------------------
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


def _first_seq(s):
    p = ya.IndelParams()
    assert ya.lib().yaha_session_indel_params(s._h, C.byref(p)) == 0 and p.capacity == 0 and p.min_length == 1
    return int(C.cast(p.seq_start, C.POINTER(C.c_uint32))[0]), int(C.cast(p.seq_length, C.POINTER(C.c_uint32))[0])


def _session(index11, tmp_path, reads, name="reads.fa", extra=()):
    path = str(tmp_path / name)
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write(">r%d\n%s\n" % (i, r))
    return ya.Session(["-x", index11, "-q", path, "-osh", "stdout", "-oid", "unused.tsv"] + list(extra))


def _want(s, texts, L=1):
    lines = [l for t in texts for l in t.split("\n")]
    return io.alleles(lines, io.sq_table(s.header().split("\n")), 0, L), io.records(lines)


def _got(entries):
    out = collections.Counter()
    for e in entries:
        key = io.entry_key(e.w0, e.w1, e.w2)
        assert key not in out and e.zero == 0 and e.count > 0                             # an allele has ONE entry
        assert (e.slot, {"DEL": 0, "INS": 1}[e.type], e.length, e.bases) == key          # (the binding's own decoding agrees)
        out[key] = e.count
    return out


def _run_cases(s, ctx, n_reads, cases):
    rb = s.next_batch(n_reads); assert rb.n_reads == n_reads
    ctx.upload(rb)
    r, _keep = _batch(n_reads, cases)
    ctx.inject_results(r)
    return s.emit_filtered(ctx.postfilter())                                             # (YGPU_CHECK_STATE: a fault or a dirty state word fails this call)


def test_abi_equal_keys_chunk_edges_and_shared_words(work, index11, tmp_path):
    rng = np.random.RandomState(5); rd = lambda n: "".join(rng.choice(list("ACGT"), n)); M, R, I, D = "MRID"
    p21, tail = rd(21), rd(9)
    other = lambda c: "ACGT"[("ACGT".index(c) + 1) % 4]
    ins_a = p21 + tail; ins_b = p21 + other(tail[0]) + tail[1:]; ins_c = other(p21[0]) + p21[1:] + tail      # a / b: equal w0 and w1, another w2; a / c: equal w0, another w1
    reads = ["A" * 64 + rd(100),                                                          # 0: 64 one-base insertions of one letter: 64 lanes, one key
             rd(300)]                                                                     # 1: 130 ops
    reads += [rd(50) + (ins_a, ins_b, ins_c)[k % 3] + rd(50) for k in range(60)]         # 2 .. 61: three alleles at one slot in many records at once
    with _session(index11, tmp_path, reads * 2) as s:
        s0, l0 = _first_seq(s); assert l0 > 21000
        with ya.Context(s.index, s.params) as ctx:
            with pytest.raises(RuntimeError, match="ygpu_set_postfilter"):
                ctx.indels_enable(s)
            with pytest.raises(RuntimeError):
                ctx.indels_size()
            ctx.set_postfilter(s)
            with pytest.raises(RuntimeError, match="power of two"):
                ctx.indels_enable(s, capacity=48)
            ctx.indels_enable(s)
            assert ctx.indels_size() == 0 and ctx.indels_collect()[0] == []
            ops130 = [(M, 1), (D, 1)] * 31 + [(M, 1), (I, 2), (I, 3)] + [(M, 1), (D, 2)] * 32 + [(M, 100)]      # the insertions are op 63 and op 64
            assert len(ops130) == 130 and ops130[63] == (I, 2) and ops130[64] == (I, 3)
            cases = {0: [(s0 + 1000, 0, 163, 0x00, [(I, 1)] * 64 + [(M, 100)])],
                     1: [(s0 + 3000, 0, sum(n for c, n in ops130 if c in "MRI") - 1, 0x01, ops130)]}
            for k in range(60):
                cases[2 + k] = [(s0 + 20000, 0, 129, k & 1, [(M, 50), (I, 30), (M, 50)])]   # (odd reads reversed: their inserted bases are the reverse complement)
            texts = [_run_cases(s, ctx, 62, cases)]
            want, n_rec = _want(s, texts)
            assert n_rec == 62 and want[(1000, io.INS, 1, "A")] == 64
            assert {want[(20050, io.INS, 30, x)] for x in (ins_a, ins_b, ins_c)} == {10}      # the even reads; the odd ones carry the reverse complements
            used = ctx.indels_size()
            assert used == len(want)
            # a second batch with the same records: the entries survive and accumulate
            texts.append(_run_cases(s, ctx, 62, cases))
            assert ctx.indels_size() == used and _want(s, texts)[0] == collections.Counter({k: 2 * v for k, v in want.items()})
            entries, st = ctx.indels_collect()
            got = _got(entries)
            assert got == collections.Counter({k: 2 * v for k, v in want.items()})
            assert st == {"records_counted": 124, "records_skipped_mapq": 0, "records_dropped_two_sequences": 0, "events": 2 * sum(want.values()), "reads_left_to_host": 0,
                          "events_lost": 0}
            # collect returns them once
            assert ctx.indels_size() == 0
            again, st2 = ctx.indels_collect()
            assert again == [] and st2["events"] == 0 and st2["records_counted"] == 0


def test_abi_small_capacity_drains_and_overflow_is_an_error_not_a_fault(work, index11, tmp_path):
    rng = np.random.RandomState(6); rd = lambda n: "".join(rng.choice(list("ACGT"), n)); M, D = "MD"
    reads = [rd(200) for _ in range(8)]
    forty = lambda: [(M, 3), (D, 1)] * 40 + [(M, 80)]                                     # 40 distinct deletions, 200 query bases
    with _session(index11, tmp_path, reads) as s:
        s0, _l0 = _first_seq(s)
        with ya.Context(s.index, s.params) as ctx:
            ctx.set_postfilter(s); ctx.indels_enable(s, capacity=64)
            got, texts, lost, drains = collections.Counter(), [], 0, 0
            for b in range(3):
                texts.append(_run_cases(s, ctx, 1, {0: [(s0 + 5000 + 1000 * b, 0, 199, 0x00, forty())]}))
                if ctx.indels_size() > 16:
                    entries, st = ctx.indels_collect(); got.update(_got(entries)); lost += st["events_lost"]; drains += 1
            entries, st = ctx.indels_collect(); got.update(_got(entries)); lost += st["events_lost"]
            want, n_rec = _want(s, texts)
            assert n_rec == 3 and len(want) == 120 and got == want and lost == 0 and drains == 3
        with ya.Context(s.index, s.params) as ctx:
            ctx.set_postfilter(s); ctx.indels_enable(s, capacity=16)
            with pytest.raises(RuntimeError, match=r"ygpu_postfilter failed: -4 .*-oid"):       # YGPU_EOVERFLOW, the option named
                _run_cases(s, ctx, 1, {0: [(s0 + 9000, 0, 199, 0x00, forty())]})
            assert ctx.indels_size() == 16
            entries, st = ctx.indels_collect()
            assert len(entries) == 16 and st["events_lost"] == 40 - 16 > 0 and st["events"] == 40
            # ... and the context serves the next batch
            text = _run_cases(s, ctx, 1, {0: [(s0 + 9500, 0, 199, 0x00, [(M, 50), (D, 7), (M, 150)])]})
            entries, st = ctx.indels_collect()
            want, _n = _want(s, [text])
            assert _got(entries) == want and len(want) == 1 and st["events_lost"] == 0


def test_a_context_without_the_stage_copies_and_launches_nothing(work, index11, tmp_path):
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout"]) as s:
        caps = []
        for enable in (False, True):
            with ya.Context(s.index, s.params) as ctx:
                ctx.set_postfilter(s)
                if enable:
                    ctx.indels_enable(s, capacity=1 << 16)
                rb = s.next_batch(20); assert rb.n_reads == 20
                ctx.upload(rb); ctx.run(); ctx.postfilter()
                prof = ctx.arena_profile()
                caps.append([int(prof.cap[k]) for k in range(prof.n - 15, prof.n)])      # the pileup's seven buffers, then the indel stage's eight
                if not enable:
                    with pytest.raises(RuntimeError, match="ygpu_indels_enable"):
                        ctx.indels_collect()
                else:
                    entries, st = ctx.indels_collect()
                    assert st["records_counted"] > 0 and st["events"] == sum(e.count for e in entries) > 0
        assert caps[0] == [0] * 15                                                        # no snapshot copy of the bases, no table, no statistics
        assert caps[1][0] > 0 and caps[1][1] > 0 and caps[1][7] == 32 << 16 and caps[1][2:7] == [0] * 5
