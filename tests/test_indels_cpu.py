"""CPU tier: indel alleles (-oid FILE, -idmin N, -idlen L, -idq Q): the insertions and deletions the printed records carry, by position, length and inserted
bases.  The command line is built with the test double for the device (tests/fixtures/oracle_device.cpp, as tests/test_pileup_cpu.py does, here without a
sanitizer) -- it has no ygpu_indels_* entry points, so the formatter threads count every record (host/indels.cpp looks them up weakly); the device stage is
proven by tests/test_gpu_indels.py.  The check is exact and independent of the product: the file is a pure function of the SAM text, recomputed by
tests/indel_oracle.py from the reference's golden lines."""
import functools
import glob
import json
import os
import subprocess

import numpy as np
import pytest

import indel_oracle as io
from conftest import ROOT, golden_lines, strip_pg

HOST = os.path.join(ROOT, "yaha_amd", "csrc", "host")
SRCS = sorted(glob.glob(os.path.join(HOST, "*.cpp"))) + [os.path.join(ROOT, "yaha_amd", "csrc", "main.cpp"), os.path.join(ROOT, "tests", "fixtures", "oracle_device.cpp"),
                                                          os.path.join(ROOT, "oracle", "hotpath.cpp")]
SETS = [("rsv_default", "rsv.fa"), ("rchim_default", "rchim.fa"), ("rq_default", "rq.fq"), ("r10k_default", "r10k.fa")]
# indel ops of the golden lines (the issue's figures): every one is an allele of its own, the longest op
OPS = {"rsv_default": (1458, 19), "rchim_default": (621, 16), "rq_default": (293, 15), "r10k_default": (905, 22)}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("indels")), "yaha_double")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-o", out] + SRCS)
    return out


def _run(exe, args, env=None):
    e = dict(os.environ, YAHA_KEEP_TEARDOWN="1"); e.update(env or {})
    return subprocess.run([exe] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@functools.lru_cache(maxsize=None)
def _oracle(name, Q=0, L=1):
    """(alleles, @SQ table) of a golden set: computed once, shared."""
    lines = golden_lines(name); sq = io.sq_table(lines)
    return io.alleles(lines, sq, Q, L), sq


def _expected(name, min_count=1, Q=0, L=1, times=1):
    al, sq = _oracle(name, Q, L)
    return io.text(al, sq, min_count, times)


def _id_run(exe, index11, reads, out, extra=(), env=None):
    p = _run(exe, ["-x", index11, "-q", reads, "-osh", "stdout", "-oid", out] + list(extra), env=env)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p, open(out).read()


def _stats(p):
    return json.loads([l for l in p.stderr.decode().split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])


@pytest.mark.parametrize("name,reads", SETS)
def test_file_equals_the_oracle_and_the_sam_is_undisturbed(exe, work, index11, tmp_path, name, reads):
    out = str(tmp_path / "id.tsv"); al, _sq = _oracle(name)
    # what the comparison stands on: the issue's figures for this set -- every op an allele of its own, both types, insertions on both strands
    assert (sum(al.values()), len(al), max(k[2] for k in al)) == (OPS[name][0], OPS[name][0], OPS[name][1])
    assert {k[1] for k in al} == {io.DEL, io.INS} and max(al.values()) == 1
    want = _expected(name)
    assert want.count("\n") == OPS[name][0]
    for extra in (["-idmin", "1"], ["-idmin", "1", "-batch", "9"], ["-idmin", "1", "-batch", "33"], ["-idmin", "1", "-ctx", "1"], ["-idmin", "1", "-ctx", "3", "-batch", "33"]):
        p, got = _id_run(exe, index11, os.path.join(work, reads), out, extra, env={"YAHA_STATS": "1"})
        assert strip_pg(p.stdout.decode()) == golden_lines(name), (name, extra)
        assert got == want, (name, extra)
        st = _stats(p)
        assert st["indel_device_records"] == 0 and st["indel_host_records"] == io.records(golden_lines(name)) and st["indel_events"] == st["indel_alleles"] == st["indel_lines"] == OPS[name][0]
        assert st["indel_lost"] == 0 and st["indel_drains"] == 0
    # the default -idmin is 2: no allele of the goldens is carried by two records
    _p, got = _id_run(exe, index11, os.path.join(work, reads), out)
    assert got == ""
    # -idlen and -idq
    _p, got = _id_run(exe, index11, os.path.join(work, reads), out, ["-idmin", "1", "-idlen", "2"])
    assert got == _expected(name, L=2) and 0 < got.count("\n") < OPS[name][0]
    _p, got = _id_run(exe, index11, os.path.join(work, reads), out, ["-idmin", "1", "-idq", "200"])
    assert got == _expected(name, Q=200) and 0 < got.count("\n") < OPS[name][0]


def _doubled(work, tmp_path):
    """Every read of rsv.fa twice, under two names."""
    src = open(os.path.join(work, "rsv.fa")).read().split(">")[1:]
    path = str(tmp_path / "rsv2.fa")
    with open(path, "w") as f:
        for rec in src:
            head, _, body = rec.partition("\n")
            f.write(">%s_a\n%s>%s_b\n%s" % (head.split()[0], body, head.split()[0], body))
    return path, len(src)


def test_a_doubled_input_doubles_every_count(exe, work, index11, tmp_path):
    out = str(tmp_path / "id.tsv"); reads, n = _doubled(work, tmp_path)
    single = _expected("rsv_default")
    assert single.count("\n") == 1458 and all(l.endswith("\t1") for l in single.split("\n")[:-1])
    p, got = _id_run(exe, index11, reads, out, ["-idmin", "2"], env={"YAHA_STATS": "1"})
    assert got == _expected("rsv_default", 2, times=2) and got.count("\n") == 1458 and all(l.endswith("\t2") for l in got.split("\n")[:-1])
    assert [l.rsplit("\t", 1)[0] for l in got.split("\n")] == [l.rsplit("\t", 1)[0] for l in single.split("\n")]
    st = _stats(p)
    assert st["indel_events"] == 2 * 1458 and st["indel_alleles"] == st["indel_lines"] == 1458 and st["indel_host_records"] == 2 * io.records(golden_lines("rsv_default"))
    _p, got = _id_run(exe, index11, reads, out)                               # (the default is 2)
    assert got == _expected("rsv_default", 2, times=2)
    p, got = _id_run(exe, index11, reads, out, ["-idmin", "3"], env={"YAHA_STATS": "1"})
    assert got == "" and _stats(p)["indel_lines"] == 0 and _stats(p)["indel_alleles"] == 1458


def test_argument_errors_and_what_stays_unchanged_without_the_option(exe, work, index11, tmp_path):
    reads = os.path.join(work, "rchim.fa"); out = str(tmp_path / "id.tsv"); base = ["-x", index11, "-q", reads]; fasta = os.path.join(work, "genome_small.fa")
    sam = str(tmp_path / "x.sam")
    for bad in (["-g", fasta, "-oid", out], base + ["-idmin", "2"], base + ["-idlen", "2"], base + ["-idq", "3"], base + ["-oid", out, "-idmin", "0"],
                base + ["-oid", out, "-idlen", "0"], base + ["-oid", out, "-idq", "256"], base + ["-oid", out, "-idq", "-1"], base + ["-oid", "stdout"],
                base + ["-osh", "stdout", "-oid", "stdout"], base + ["-osh", sam, "-oid", "stdout", "-ocov", "stdout"], base + ["-osh", sam, "-oid", "stdout", "-oev", "stdout"],
                base + ["-osh", sam, "-oid", "stdout", "-obp", "stdout"], base + ["-osh", sam, "-oid", "stdout", "-opu", "stdout"]):
        p = _run(exe, bad)
        assert p.returncode == 2, (bad, p.returncode, p.stderr.decode()[-300:])
        assert not os.path.exists(out)
    plain = _run(exe, base + ["-osh", "stdout"], env={"YAHA_STATS": "1"})
    wid = _run(exe, base + ["-osh", "stdout", "-oid", out, "-idmin", "1", "-idlen", "2", "-idq", "3"], env={"YAHA_STATS": "1"})
    assert plain.returncode == 0 and wid.returncode == 0
    pg = lambda p: [l for l in p.stdout.decode().split("\n") if l.startswith("@PG")]
    assert len(pg(plain)) == 1 and "-oid" not in pg(plain)[0] and "-id" not in pg(plain)[0]
    assert pg(wid)[0] == pg(plain)[0] + " -oid " + out + " -idmin 1 -idlen 2 -idq 3"
    assert strip_pg(plain.stdout.decode()) == strip_pg(wid.stdout.decode()) == golden_lines("rchim_default")
    a, b = _stats(plain), _stats(wid)
    new = {"indel_device_records", "indel_host_records", "indel_events", "indel_alleles", "indel_lines", "indel_drains", "indel_lost"}
    assert not (new & set(a)) and set(b) - set(a) == new
    assert open(out).read() == _expected("rchim_default", 1, 3, 2) != ""
    # the alignments in a file, the alleles on standard output
    p = _run(exe, base + ["-osh", sam, "-oid", "stdout", "-idmin", "1"])
    assert p.returncode == 0 and p.stdout.decode() == _expected("rchim_default")
    assert strip_pg(open(sam).read()) == golden_lines("rchim_default")
    # beside the other tracks: their files are what a run without -oid writes
    cov, ev, bp, pu = (str(tmp_path / f) for f in ("cov.bg", "ev.tsv", "bp.bedpe", "pu.tsv"))
    others = ["-ocov", cov, "-oev", ev, "-obp", bp, "-opu", pu, "-pumin", "1"]
    alone = _run(exe, base + ["-osh", "stdout"] + others)
    assert alone.returncode == 0
    want = [open(f).read() for f in (cov, ev, bp, pu)]
    for f in (cov, ev, bp, pu, out):
        os.remove(f)
    both = _run(exe, base + ["-osh", "stdout"] + others + ["-oid", out, "-idmin", "1"])
    assert both.returncode == 0
    assert [open(f).read() for f in (cov, ev, bp, pu)] == want and all(want) and open(out).read() == _expected("rchim_default")
    assert strip_pg(both.stdout.decode()) == golden_lines("rchim_default")


# ---- the shared walk on hand-made records (tests/fixtures/indel_driver.cpp) ---------------------------------------------------------------------------------------
CODE = {"T": 0, "C": 1, "A": 2, "G": 3, "N": 4, "K": 8, "R": 10, "Y": 15}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def _drive(tmp_path, Q, L, seqs, clumps):
    exe = str(tmp_path / "indel_driver")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "fixtures", "indel_driver.cpp")])
    text = "%d %d %d\n" % (Q, L, len(seqs)) + "".join("%d %d\n" % s for s in seqs)
    for sro, sqo, eqo, mq, rev, ops, read in clumps:
        ref_len = sum(n for c, n in ops if c in "MRD")
        text += "%d %d %d %d %d %d %d %s %s\n" % (sro, ref_len, sqo, eqo, mq, rev, len(ops), " ".join("%s %d" % (c, n) for c, n in ops), "".join("%x" % CODE[c] for c in read))
    p = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().split("\n"); res, events = [], []
    for l in lines[:len(clumps)]:
        f = l.split(); res.append(int(f[0])); mine = []
        for e in f[1:]:
            slot, typ, ln, bases, w0, w1, w2 = e.split(":")
            key = (int(slot), int(typ), int(ln), "" if bases == "*" else "".join("ACGTN"[int(d)] for d in bases))
            assert io.entry_key(int(w0, 16), int(w1, 16), int(w2, 16)) == key      # the three words are the issue's layout
            mine.append(key)
        events.append(mine)
    assert lines[len(clumps)].split()[0] == "order"
    return res, events, [int(x) for x in lines[len(clumps)].split()[1:]]


def _by_hand(Q, L, seqs, clumps):
    """Op by op, from the definition in the issue; the reverse strand is spelled out as a string first."""
    base, tot, res, events = [], 0, [], []
    for _s, ln in seqs:
        base.append(tot); tot += ln
    for sro, sqo, eqo, mq, rev, ops, read in clumps:
        ref_len = sum(n for c, n in ops if c in "MRD")
        inside = [i for i, (s, ln) in enumerate(seqs) if s <= sro < s + ln and sro + ref_len - 1 < s + ln]
        if not inside:
            res.append(2); events.append([]); continue
        if mq < Q:
            res.append(1); events.append([]); continue
        i = inside[0]; strand = "".join(COMP.get(c, "N") for c in reversed(read)) if rev else "".join(c if c in "ACGT" else "N" for c in read)
        slot = lambda off: base[i] + off - seqs[i][0]
        qe = min(eqo + 1, len(read)); cur, q, mine = sro, min(sqo, qe), []
        for c, n in ops:
            if c in "MR":
                cur += n; q = min(q + n, qe)
            elif c == "D":
                if n >= L and cur + n <= sro + ref_len:
                    mine.append((slot(cur), 0, n, ""))
                cur += n
            elif c == "I":
                if n >= L and q + n <= qe:
                    mine.append((slot(min(cur, sro + ref_len - 1)), 1, n, strand[q:q + min(n, 42)]))
                q = min(q + n, qe)
        res.append(0); events.append(mine)
    return res, events


def test_the_shared_walk_on_hand_made_records(tmp_path):
    rng = np.random.RandomState(11)
    seqs = [(0, 1000), (1000, 250), (1300, 333)]
    rd = lambda n, extra="": "".join(rng.choice(list("ACGT" + extra), n))
    M, R, I, D = "MRID"
    with_n = rd(20) + "ACNNGTKRY" + rd(31)                                               # an N and ambiguity codes inside an insertion (query 20 .. 28)
    long_rd = rd(400)
    clumps = [
        (100, 0, 59, 250, 0, [(M, 20), (I, 9), (M, 31)], with_n),                        # 0: a forward insertion with N / ambiguity codes
        (100, 0, 59, 250, 1, [(M, 20), (I, 9), (M, 31)], with_n),                        # 1: the same clump reversed: the inserted bases in reference orientation
        (400, 2, 103, 250, 0, [(M, 100), (I, 2)], rd(110)),                              # 2: an insertion as the last op: the slot is clamped to 499, not 500
        (300, 0, 118, 250, 1, [(M, 96), (I, 3), (D, 4), (M, 20)], rd(119)),              # 3: an I directly before a D: both at the D's first base (396)
        (500, 0, 200, 250, 0, [(M, 10), (I, 41), (M, 10), (I, 42), (M, 10), (I, 43), (M, 45)], long_rd[:201]),      # 4: lengths 41, 42 and 43
        (500, 0, 202, 250, 0, [(M, 10), (I, 41), (M, 10), (I, 42), (M, 10), (I, 45), (M, 45)], long_rd[:155] + rd(48)),   # 5: 45 bases with the same first 42 (another length: another allele)
        (700, 0, 39, 250, 0, [(M, 10), (D, 1), (M, 10), (I, 1), (M, 5), (D, 2), (M, 4), (I, 2), (M, 8)], rd(40)),     # 6: 1-base ops (dropped by -idlen 2) beside 2-base ops
        (1400, 0, 29, 9, 0, [(M, 10), (D, 3), (M, 20)], rd(30)),                         # 7: the MAPQ gate (Q = 10 below)
        (1400, 0, 29, 10, 0, [(M, 10), (D, 3), (M, 20)], rd(30)),                        # 8
        (1240, 0, 19, 250, 0, [(M, 5), (D, 3), (M, 15)], rd(20)),                        # 9: spans two sequences: dropped
        (600, 10, 39, 250, 0, [(M, 20), (I, 5), (M, 10), (I, 5), (M, 40)], rd(45)),      # 10: ops that overrun eqo: the first I fits (q 30 .. 34), the second (q 45) does not
        (800, 0, 29, 250, 0, [(M, 28), (I, 5)], rd(30)),                                 # 11: an insertion that starts inside and ends past eqo: no event
        (820, 5, 60, 250, 1, [(M, 20), (I, 30), (M, 6)], rd(40)),                        # 12: eqo past the read's last base: the insertion would leave the read
        (900, 0, 35, 250, 0, [(M, 10), (I, 3), (I, 3), (M, 10), (D, 4), (M, 10)], rd(10) + "TTT" + "TTT" + rd(20)),      # 13: two equal ops in one record: counted twice
        (1233, 0, 15, 250, 1, [(M, 10), (R, 1), (M, 4), (D, 2)], rd(16)),                # 14: a deletion that ends on the last base of a sequence
    ] + [(10, 0, 199, 250, 0, [(M, 1), (D, 1)] * 70 + [(I, 2), (M, 128)], rd(200))]      # 15: more than 64 ops
    for Q, L in ((0, 1), (10, 1), (0, 2), (10, 3)):
        got_res, got_ev, order = _drive(tmp_path, Q, L, seqs, clumps)
        want_res, want_ev = _by_hand(Q, L, seqs, clumps)
        assert got_res == want_res and got_ev == want_ev, (Q, L)
        flat = [e for ev in want_ev for e in ev]
        assert [flat[i] for i in order] == sorted(flat, key=io.order)                     # keyLess is the file's order
    res, ev = _by_hand(10, 1, seqs, clumps)
    assert res == [0, 0, 0, 0, 0, 0, 0, 1, 0, 2, 0, 0, 0, 0, 0, 0]
    comp = "".join(COMP.get(c, "N") for c in reversed(with_n))
    assert ev[0] == [(120, 1, 9, "ACNNGTNNN")] and ev[1] == [(120, 1, 9, comp[20:29])] and ev[1][0][3] != ev[0][0][3]
    assert ev[2] == [(499, 1, 2, ev[2][0][3])] and ev[3][0][0] == ev[3][1][0] == 396
    assert [(e[2], len(e[3])) for e in ev[4]] == [(41, 41), (42, 42), (43, 42)] and [(e[2], len(e[3])) for e in ev[5]] == [(41, 41), (42, 42), (45, 42)]
    assert ev[4][2][3] == ev[5][2][3] and ev[4][2] != ev[5][2] and ev[4][:2] == ev[5][:2]
    assert len(ev[6]) == 4 and len(_by_hand(0, 2, seqs, clumps)[1][6]) == 2
    assert len(ev[10]) == 1 and ev[11] == [] and ev[12] == []
    assert ev[13][0] == ev[13][1] == (910, 1, 3, "TTT") and len(ev[13]) == 3
    assert ev[14] == [(1248, 0, 2, "")] and len(ev[15]) == 71
