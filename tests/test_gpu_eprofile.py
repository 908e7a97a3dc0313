"""GPU tier: the error profile (-oep) counted on the device behind the post-filter (device/eprofile_stage.h: a persistent grid, a wave per printed clump, the
table of 1556 counters in LDS for a workgroup's whole share of the batch, added to the context's table once per workgroup).  The command line is compared
with tests/eprofile_oracle.py, which recomputes the file from SAM text and the reference FASTA alone; the stage itself with the one-thread walk of
yaha_amd/csrc/eprofile_core.h (tests/fixtures/eprofile_driver.cpp) on clumps injected through ygpu_inject_results.  The tier runs with YGPU_CHECK_STATE on
(conftest.py), so every ygpu_run / ygpu_postfilter here also checks the state words."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import eprofile_oracle as eo
import yaha_amd as ya
from conftest import golden_lines, strip_pg
from test_eprofile_cpu import drive

pytestmark = pytest.mark.gpu


def _cli(index11, reads, args, env=None):
    p = subprocess.run([ya.CLI_PATH, "-x", index11, "-q", reads] + list(args), env=dict(os.environ, YAHA_STATS="1", **(env or {})), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    assert "state check" not in err, err[-2000:]                                       # YGPU_CHECK_STATE stays silent (a dirty word also fails the run)
    return p.stdout.decode(), json.loads([l for l in err.split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])


@functools.lru_cache(maxsize=None)
def _ref(fasta):
    return eo.read_fasta(fasta)


# ---- (a) the command line against the oracle --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,reads", [("rchim_default", "rchim.fa"), ("rsv_default", "rsv.fa"), ("rq_default", "rq.fq")])
def test_command_line_file_is_counted_by_the_kernel_and_equals_the_oracle(work, index11, tmp_path, name, reads):
    out = str(tmp_path / "ep.tsv"); lines = golden_lines(name); q = os.path.join(work, reads)
    t = eo.table(lines, _ref(os.path.join(work, "genome_small.fa")))
    want = eo.text(t, *eo.records(lines))
    assert t[eo.SUB:eo.SUB + 25].sum() > 0 and t[eo.INS:eo.INS + 130].sum() > 0 and min(eo.strands(lines)) > 0
    sam, st = _cli(index11, q, ["-osh", "stdout", "-oep", out], env={"YAHA_HOST_EPROFILE": "1"})
    host = open(out).read()
    assert strip_pg(sam) == lines and host == want and st["eprofile_device_records"] == 0 and st["eprofile_host_records"] == eo.records(lines)[0]
    for extra in (["-ctx", "1"], ["-ctx", "3", "-batch", "17"]):
        os.remove(out)
        sam, st = _cli(index11, q, ["-osh", "stdout", "-oep", out] + extra)
        got = open(out).read()
        assert strip_pg(sam) == lines, (name, extra)
        assert got == want, (name, extra)
        assert got == host
        # the kernel did the counting, not the host's walk
        assert st["eprofile_device_records"] == eo.records(lines)[0] > 0 and st["eprofile_host_records"] == 0, (extra, st)
        assert st["eprofile_pairs"] == int(t[eo.SUB:eo.SUB + 25].sum()) and st["eprofile_indels"] == int(t[eo.INS:eo.INS + 130].sum())


# ---- (b) the stage on injected batches --------------------------------------------------------------------------------------------------------------------------
M, R, I, D = "MRID"
LETTER = "TCAGNBDHKMRSVWXY"                                                     # the 4-bit codes (drive() takes letters)


def _inject(ctx, reads, per_read):
    """reads: the batch's reads as lists of 4-bit codes; per_read[i] = list of (sro, sqo, eqo, status, ops).  Uploads the reads, places the clumps as the
    hot path's results and returns what the post-filter makes of them."""
    codes = np.array([c for r in reads for c in r], dtype=np.uint8); off = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    rb = ya.ReadBatch(); rb.n_reads = len(reads); rb.codes = codes.ctypes.data; rb.offsets = off.ctypes.data
    ctx.upload(rb)
    recs, ops, starts = [], [], [0]
    for i in range(len(reads)):
        for sro, sqo, eqo, status, o in per_read.get(i, []):
            rlen = sum(n for c, n in o if c in "MRD"); assert rlen < 65536
            recs.append((sro, sqo, eqo, rlen, 30, min(65535, eqo - sqo + 1), 0, 0, 0, status, 0, len(ops), len(o)))
            ops.extend(n | (ord(c) << 16) for c, n in o)
        starts.append(len(recs))
    cs = (C.c_uint32 * len(starts))(*starts); cl = (ya.Clump * max(1, len(recs)))(*[ya.Clump(*r) for r in recs]); op = (C.c_uint32 * max(1, len(ops)))(*ops)
    r = ya.ResultBatch(); r.n_reads = len(reads); r.clump_start = cs; r.clumps = cl; r.ops = op; r.n_clumps = len(recs); r.n_ops = len(ops)
    ctx.inject_results(r)
    return ctx.postfilter()                                                              # (YGPU_CHECK_STATE: a fault or a dirty state word fails this call)


def _walk(tmp_path, Q, seqs, image, reads, f):
    """The one-thread walk of the core on the filtered batch f: (what became of each record, the table, the reads handed back unfiltered)."""
    clumps, handed = [], 0
    for i in range(f.n_reads):
        k0, k1 = f.clump_start[i], f.clump_start[i + 1]
        if k1 > k0 and f.clumps[k0].primaryCount == 0xFFFF:
            handed += 1; continue
        for k in range(k0, k1):
            oc = f.clumps[k]; c = oc.c
            ops = [(chr((f.ops[c.op_start + j] >> 16) & 0xFF), f.ops[c.op_start + j] & 0xFFFF) for j in range(c.n_ops)]
            assert c.refLen == sum(n for x, n in ops if x in "MRD")
            clumps.append((i, c.sro, c.sqo, c.eqo, oc.mapQuality, oc.status & 1, ops))
    res, t = drive(tmp_path, Q, seqs, "@" + image, ["".join(LETTER[c] for c in r) for r in reads], clumps)
    return res, t, handed


def test_synthetic_clumps_through_the_stage(work, index11, tmp_path, monkeypatch):
    monkeypatch.setenv("YGPU_OQC_MAX", "3")                                      # a read of more than three clumps is handed back unfiltered
    rng = np.random.RandomState(3); Q = 100
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout", "-oep", "unused.tsv", "-epq", str(Q)]) as s:
        p = ya.EProfileParams()
        assert ya.lib().yaha_session_eprofile_params(s._h, C.byref(p)) == 0 and p.min_mapq == Q and p.n_seqs >= 2
        st_ = C.cast(p.seq_start, C.POINTER(C.c_uint32)); ln_ = C.cast(p.seq_length, C.POINTER(C.c_uint32))
        seqs = [(int(st_[i]), int(ln_[i])) for i in range(p.n_seqs)]; (s0, l0), (s1, l1) = seqs[0], seqs[1]
        assert l0 > 60000
        # the packed reference as the device has it: for the walk (a file) and for reads that match it
        packed = np.ctypeslib.as_array(C.cast(s.index.bases, C.POINTER(C.c_uint8)), shape=(int(s.index.n_base_bytes),)).copy()
        image = str(tmp_path / "image.bin"); packed.tofile(image)
        ref = np.empty(2 * len(packed), dtype=np.uint8); ref[0::2] = packed >> 4; ref[1::2] = packed & 15
        exact = lambda off, n: [int(x) for x in ref[off:off + n]]                # the reference's own codes there
        wrong = lambda off, n: [(int(x) + 1) & 3 if x < 4 else 0 for x in ref[off:off + n]]      # another base at every place
        comp = lambda r: [x ^ 2 if x < 4 else x for x in reversed(r)]            # reverse complement of codes (T0 C1 A2 G3)
        rd = lambda n: [int(x) for x in rng.randint(0, 4, n)]
        run130 = [(M, 1), (D, 1)] * 31 + [(M, 1), (I, 2), (I, 3)] + [(M, 1), (R, 1)] * 32 + [(M, 100)]
        assert len(run130) == 130
        qsum = lambda o: sum(n for c, n in o if c in "MRI")
        long_ops = [(M, 4097), (I, 1), (M, 63), (I, 64), (M, 64), (I, 65), (M, 65), (I, 1000), (M, 1), (D, 1), (M, 700), (D, 64), (M, 300), (D, 65), (M, 200), (D, 1000), (M, 5000)]
        reads, cases = [], {}

        def case(read, clumps):
            cases[len(reads)] = clumps; reads.append(read)
        case(exact(s0 + 1000, 300), [(s0 + 1000, 0, 299, 0x00, [(M, 300)])])                                   # identity exactly 1000, one op
        case(comp(exact(s0 + 2000, 300)), [(s0 + 2000, 0, 299, 0x01, [(M, 300)])])                             # ... a reversed record
        case(wrong(s0 + 3000, 200), [(s0 + 3000, 0, 199, 0x00, [(R, 200)])])                                   # identity exactly 0
        case(rd(50), [(s0 + 3500, 5, 30, 0x00, [])])                                                           # no ops
        case(rd(63 * 2), [(s0 + 4000, 0, 125, 0x01, [(M, 1), (R, 1)] * 31 + [(M, 64)])])                       # 63 ops
        case(rd(64 * 2), [(s0 + 4500, 0, 127, 0x00, [(M, 1), (R, 1)] * 32)])                                   # 64 ops
        case(rd(65 * 2), [(s0 + 5000, 0, 129, 0x01, [(M, 1), (R, 1)] * 32 + [(M, 66)])])                       # 65 ops
        case(rd(qsum(run130)), [(s0 + 5500, 0, qsum(run130) - 1, 0x00, run130)])                               # 130 ops, I ops at the chunk's edge
        case(rd(qsum(long_ops)), [(s0 + 10000, 0, qsum(long_ops) - 1, 0x00, long_ops)])                        # M runs of 4097 / 63 / 64 / 65 / 1, I and D of 1 / 64 / 65 / 1000
        case(rd(qsum(long_ops)), [(s0 + 30000, 0, qsum(long_ops) - 1, 0x01, long_ops)])                        # ... reversed
        case(rd(100), [(s0 + 6000, 10, 39, 0x00, [(M, 20), (I, 5), (M, 40), (I, 3), (D, 2), (M, 5)])])         # ops that overrun eqo
        case(rd(45), [(s0 + 6500, 10, 60, 0x01, [(M, 50), (D, 3)])])                                           # eqo past the read's last base
        case([2], [(s0 + 7000, 0, 0, 0x00, [(M, 1)])])                                                         # a read of one base
        case([4, 5, 0, 1, 2, 3, 4, 15] * 10, [(s0 + 7500, 0, 79, 0x00, [(M, 80)]),])                           # N and ambiguity codes in the read
        case(rd(150), [(s0 + l0 - 10, 50, 69, 0x00, [(M, 5), (R, 15)])])                                       # spans two sequences: not printed
        case(rd(120), [(s0 + 8000, 0, 119, 0x00, [(M, 120)]), (s0 + 9000, 0, 119, 0x00, [(M, 120)])])          # two equal clumps: one record, with a low MAPQ
        case(rd(400), [(s0 + 40000 + 500 * k, 100 * k, 100 * k + 99, 0x00, [(M, 100)]) for k in range(4)])     # four clumps: handed back
        n_at = np.nonzero((ref[s1:s1 + l1 - 60] >= 4))[0]; assert len(n_at)
        case(rd(60), [(s1 + max(0, int(n_at[0]) - 20), 0, 59, 0x00, [(M, 60)])])                               # N in the reference (the second sequence has some)
        special = len(reads)
        # enough records that every wave of the persistent grid (256 workgroups of four) takes more than two
        for k in range(2300):
            a, b, c, d = (int(x) for x in rng.randint(1, 30, 4)); ops = [(M, a), (R, 1), (M, b), (I, c % 4 + 1), (M, d), (D, b % 5 + 1), (M, 20)]
            case(rd(qsum(ops) + 7), [(s0 + 100 + 23 * k, 3, 3 + qsum(ops) - 1, k & 1, ops)])
        assert len(reads) > 2 * 256 * 4 + special
        with ya.Context(s.index, s.params) as ctx:
            with pytest.raises(RuntimeError, match="ygpu_set_postfilter"):              # enable needs the post-filter
                ctx.eprofile_enable(s)
            with pytest.raises(RuntimeError, match="ygpu_eprofile_enable"):
                ctx.eprofile_collect()
            ctx.set_postfilter(s); ctx.eprofile_enable(s)
            t0, st0 = ctx.eprofile_collect()
            assert t0.dtype == np.uint64 and len(t0) == ya.EPROFILE_WORDS == eo.WORDS and not t0.any() and not any(st0.values())
            f = _inject(ctx, reads, cases)
            res, want, handed = _walk(tmp_path, Q, seqs, image, reads, f)
            # the walk first: it reaches what the cases are there for
            assert res.count(2) == 1 and res.count(1) == 1 and handed == 1 and res.count(0) == len(reads) - 3
            assert want[eo.INS:eo.INS + 4].sum() >= 2300 and want[eo.INS + 63] == 2 and want[eo.INS + 64] == 4 and want[eo.DEL + 63] == 2 and want[eo.DEL + 64] == 4
            assert want[eo.IDENT + 1000] >= 2 and want[eo.IDENT] >= 1 and int(want[eo.IDENT:eo.IDENT + 1001].sum()) == res.count(0) - 1      # (all but the record without ops)
            sub = want[eo.SUB:eo.SUB + 25].reshape(5, 5); pos = want[eo.POS:eo.POS + 400].reshape(100, 4)
            assert (sub[:4, :4] > 0).all() and sub[:, 4].sum() >= 40 and sub[4].sum() > 0
            assert (pos[:, 0] > 0).all() and pos[:, 1].sum() > 0 and pos[:, 2].sum() == want[eo.INS:eo.INS + 65].sum() - 1 and pos[:, 3].sum() == want[eo.DEL:eo.DEL + 65].sum() - 2
            got, st = ctx.eprofile_collect()
            assert np.array_equal(got, want), np.nonzero(got != want)
            assert st == {"records_counted": res.count(0), "records_skipped_mapq": 1, "records_dropped_two_sequences": 1, "reads_left_to_host": 1}
            # once more with fewer clumps than workgroups: one workgroup, two of its waves without a clump; the table goes on counting
            few = {0: cases[0], 1: cases[7]}
            f2 = _inject(ctx, [reads[0], reads[7]], few)
            res2, want2, handed2 = _walk(tmp_path, Q, seqs, image, [reads[0], reads[7]], f2)
            assert res2 == [0, 0] and handed2 == 0 and want2.any()
            got2, st2 = ctx.eprofile_collect()
            assert np.array_equal(got2, want + want2) and st2["records_counted"] == res.count(0) + 2
            # an empty batch launches nothing and changes nothing
            _inject(ctx, [reads[0]], {})
            got3, st3 = ctx.eprofile_collect()
            assert np.array_equal(got3, got2) and st3 == st2


# ---- (c) two contexts of one image --------------------------------------------------------------------------------------------------------------------------------
def test_two_contexts_of_one_image_sum_to_the_single_context_table(work, index11):
    fasta = os.path.join(work, "genome_small.fa"); args = ["-x", index11, "-q", os.path.join(work, "rchim.fa"), "-osh", "stdout", "-oep", "unused.tsv"]
    order = (0, 0, 1, 0, 1)
    with ya.Session(args) as s:
        with ya.Context(s.index, s.params) as a:
            a.set_postfilter(s); a.eprofile_enable(s)
            with ya.Context(s.index, s.params, parent=a) as b:
                b.set_postfilter(s); b.eprofile_enable(s)
                texts = []
                for k in order:
                    ctx = (a, b)[k]; rb = s.next_batch(40); assert rb.n_reads > 0
                    ctx.upload(rb); ctx.run(); texts.append(s.emit_filtered(ctx.postfilter()))
                (ta, sa), (tb, sb) = a.eprofile_collect(), b.eprofile_collect()
                header = s.header()
    assert ta.any() and tb.any() and not np.array_equal(ta, tb)                          # the tables are the contexts' own
    with ya.Session(args) as s:
        with ya.Context(s.index, s.params) as one:
            one.set_postfilter(s); one.eprofile_enable(s)
            for _k in order:
                rb = s.next_batch(40); one.upload(rb); one.run(); one.postfilter()
            t1, s1 = one.eprofile_collect()
    assert np.array_equal(ta + tb, t1) and {k: sa[k] + sb[k] for k in sa} == s1
    lines = [l for t in texts for l in t.split("\n")]
    assert np.array_equal(t1, eo.table(lines, _ref(fasta))) and s1["records_counted"] == eo.records(lines)[0] > 0 and s1["reads_left_to_host"] == 0
    assert header.startswith("@HD")


# ---- (d) all six side outputs in one run --------------------------------------------------------------------------------------------------------------------------
def test_all_six_side_outputs_in_one_run(work, index11, tmp_path):
    q = os.path.join(work, "rchim.fa")
    side = [("-ocov", "cov"), ("-oev", "ev"), ("-opu", "pu"), ("-obp", "bp"), ("-oid", "id"), ("-oep", "ep")]
    opts = lambda d, kinds: [x for o, n in kinds for x in ((o, os.path.join(d, n)) + (("-idmin", "1") if o == "-oid" else ()))]
    alone = {}
    for o, n in side:
        d = str(tmp_path / ("alone_" + n)); os.makedirs(d)
        _cli(index11, q, ["-osh", os.path.join(d, "out.sam")] + opts(d, [(o, n)]))
        alone[n] = open(os.path.join(d, n), "rb").read()
        assert alone[n], n
    d = str(tmp_path / "all"); os.makedirs(d)
    _sam, st = _cli(index11, q, ["-osh", os.path.join(d, "out.sam"), "-ctx", "3", "-batch", "17"] + opts(d, side))
    for _o, n in side:
        assert open(os.path.join(d, n), "rb").read() == alone[n], n
    assert strip_pg(open(os.path.join(d, "out.sam")).read()) == golden_lines("rchim_default")
    keys = ["depth_device_records", "events_device_records", "pileup_device_records", "bp_device_reads", "indel_device_records", "eprofile_device_records"]
    assert all(st[k] > 0 for k in keys) and st["eprofile_host_records"] == 0, st
    assert [k for k in st if k.startswith("eprofile_")] == list(st)[-4:]                 # the profile's keys stand last: the other outputs' order is as it was
