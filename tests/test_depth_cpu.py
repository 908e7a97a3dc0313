"""CPU tier: the read-depth track (-ocov FILE, -covbin B, -covq Q).  The command line is built with the test double for the device (tests/fixtures/oracle_device.cpp,
as tests/test_pipeline_cpu.py does) -- it has no ygpu_depth_* entry points, so the host's accumulator counts every record here (host/depth.cpp looks them up weakly);
the device stage is proven by tests/test_gpu_depth.py.  The check is exact and independent of the product: depth is a pure function of the SAM text, recomputed by
tests/depth_oracle.py from the reference's golden lines."""
import glob
import json
import os
import subprocess

import pytest

import depth_oracle as do
from conftest import ROOT, golden_lines, strip_pg

HOST = os.path.join(ROOT, "yaha_amd", "csrc", "host")
SRCS = sorted(glob.glob(os.path.join(HOST, "*.cpp"))) + [os.path.join(ROOT, "yaha_amd", "csrc", "main.cpp"), os.path.join(ROOT, "tests", "fixtures", "oracle_device.cpp"),
                                                          os.path.join(ROOT, "oracle", "hotpath.cpp")]
SETS = [("rchim_default", "rchim.fa"), ("r1k_default", "r1k.fa"), ("r10k_default", "r10k.fa"), ("rq_default", "rq.fq")]


def _build(tmp, san):
    exe = os.path.join(tmp, "yaha_" + san.replace(",", "_"))
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=" + san, "-fno-omit-frame-pointer", "-pthread", "-o", exe] + SRCS)
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("depth"))
    return {"tsan": _build(d, "thread"), "asan": _build(d, "address,undefined")}


def _run(exe, args, env=None):
    e = dict(os.environ, YAHA_KEEP_TEARDOWN="1", TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    e.update(env or {})
    return subprocess.run([exe] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def _clean(p):
    err = p.stderr.decode()
    assert "ThreadSanitizer" not in err and "AddressSanitizer" not in err and "runtime error:" not in err, err[-4000:]


def _expected(name, B, Q=0):
    lines = golden_lines(name); sq = do.sq_table(lines)
    return do.bedgraph(do.coverage(lines, sq, B, Q), sq, B)


def _cov_run(exe, index11, reads, out, extra=(), oflag="-osh", env=None):
    p = _run(exe, ["-x", index11, "-q", reads, oflag, "stdout", "-ocov", out] + list(extra), env=env)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    _clean(p)
    return p, open(out).read()


@pytest.mark.parametrize("name,reads", SETS)
def test_bedgraph_equals_the_oracle_and_the_sam_is_undisturbed(exes, work, index11, tmp_path, name, reads):
    out = str(tmp_path / "cov.bg")
    for extra, B, Q in ((["-covbin", "1"], 1, 0), (["-covbin", "37"], 37, 0), ([], 100, 0), (["-covbin", "100", "-covq", "10"], 100, 10),
                        (["-covbin", "37", "-covq", "200"], 37, 200)):
        p, got = _cov_run(exes["asan"], index11, os.path.join(work, reads), out, extra)
        assert strip_pg(p.stdout.decode()) == golden_lines(name), (name, extra)
        assert got == _expected(name, B, Q), (name, extra)
        assert got, "an empty track proves nothing"
    # the mapping-quality gate removes something, or the cases above show nothing (-covq 10: a record of MAPQ 1 in r1k, one of MAPQ 0 in rq; 200: records everywhere)
    if name in ("r1k_default", "rq_default"):
        assert _expected(name, 100, 10) != _expected(name, 100, 0)
    assert _expected(name, 37, 200) != _expected(name, 37, 0)


def test_under_the_thread_sanitizer_with_many_contexts(exes, work, index11, tmp_path):
    out = str(tmp_path / "cov.bg")
    p, got = _cov_run(exes["tsan"], index11, os.path.join(work, "rchim.fa"), out, ["-covbin", "1", "-t", "3", "-gpus", "2", "-ctx", "2", "-batch", "29"], env={"YTEST_DEVICES": "2", "YAHA_CPUS": "6"})
    assert strip_pg(p.stdout.decode()) == golden_lines("rchim_default")
    assert got == _expected("rchim_default", 1)


def test_the_track_does_not_depend_on_batching_filter_side_or_output_format(exes, work, index11, tmp_path):
    out = str(tmp_path / "cov.bg"); reads = os.path.join(work, "rchim.fa")
    want = _expected("rchim_default", 37)
    for extra, oflag, env in ((["-batch", "5"], "-osh", {}), (["-batch", "61"], "-osh", {}), ([], "-osh", {}), (["-dpf", "N", "-batch", "61"], "-osh", {}), (["-dpf", "Y", "-batch", "61"], "-osh", {}),
                              (["-batch", "61"], "-osh", {"YTEST_RAW_ABOVE": "3"}), (["-batch", "61"], "-osh", {"YAHA_HOST_OQC": "1"}), (["-batch", "61"], "-oss", {}), (["-batch", "61"], "-o8", {})):
        _p, got = _cov_run(exes["asan"], index11, reads, out, ["-covbin", "37"] + extra, oflag=oflag, env=env)
        assert got == want, (extra, oflag, env)
    # -OQC N prints other records (duplicate removal only): the track follows what is printed
    _p, got = _cov_run(exes["asan"], index11, reads, out, ["-covbin", "37", "-OQC", "N"])
    assert got == _expected("rchim_OQCN", 37) and got != want


def test_argument_errors_and_what_stays_unchanged_without_the_option(exes, work, index11, tmp_path):
    reads = os.path.join(work, "rchim.fa"); out = str(tmp_path / "cov.bg"); base = ["-x", index11, "-q", reads]
    for bad in (["-g", os.path.join(work, "genome_small.fa"), "-ocov", out], base + ["-covbin", "10"], base + ["-covq", "3"], base + ["-ocov", out, "-covbin", "0"],
                base + ["-ocov", "stdout"], base + ["-osh", "stdout", "-ocov", "stdout"]):
        p = _run(exes["asan"], bad)
        _clean(p)
        assert p.returncode == 2, (bad, p.returncode, p.stderr.decode()[-300:])
        assert not os.path.exists(out)
    plain = _run(exes["asan"], base + ["-osh", "stdout"], env={"YAHA_STATS": "1"})
    cov = _run(exes["asan"], base + ["-osh", "stdout", "-ocov", out, "-covbin", "50", "-covq", "2"], env={"YAHA_STATS": "1"})
    assert plain.returncode == 0 and cov.returncode == 0
    pg = lambda p: [l for l in p.stdout.decode().split("\n") if l.startswith("@PG")]
    assert len(pg(plain)) == 1 and "-ocov" not in pg(plain)[0] and "-cov" not in pg(plain)[0]
    assert pg(cov)[0] == pg(plain)[0] + " -ocov " + out + " -covbin 50 -covq 2"
    st = lambda p: json.loads([l for l in p.stderr.decode().split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])
    a, b = st(plain), st(cov)
    new = {"depth_bins", "depth_device_records", "depth_host_records", "depth_covered_bases"}
    assert not (new & set(a)) and set(b) - set(a) == new
    lines = golden_lines("rchim_default"); sq = do.sq_table(lines)
    assert b["depth_bins"] == do.n_bins(sq, 50) and b["depth_device_records"] == 0 and b["depth_host_records"] == do.records(lines, 2)
    assert b["depth_covered_bases"] == sum(do.coverage(lines, sq, 50, 2))
    # the alignments in a file, the track on standard output
    sam = str(tmp_path / "out.sam")
    p = _run(exes["asan"], base + ["-osh", sam, "-ocov", "stdout"])
    assert p.returncode == 0 and p.stdout.decode() == _expected("rchim_default", 100)
    assert strip_pg(open(sam).read()) == golden_lines("rchim_default")


def _drive(tmp_path, B, Q, seqs, clumps):
    exe = str(tmp_path / "depth_driver")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "fixtures", "depth_driver.cpp")])
    text = "%d %d %d\n" % (B, Q, len(seqs)) + "".join("%d %d\n" % s for s in seqs)
    for sro, ref_len, mq, ops in clumps:
        text += "%d %d %d %d %s\n" % (sro, ref_len, mq, len(ops), " ".join("%s %d" % (c, n) for c, n in ops))
    p = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().split("\n")
    return [tuple(int(x) for x in l.split()) for l in lines[:len(clumps)]], [int(x) for x in lines[len(clumps)].split()[1:]]


def _by_hand(B, Q, seqs, clumps):
    """Base by base, from the definition: which absolute reference offsets a clump covers, then into which bin each falls."""
    base, tot = [], 0
    for _s, ln in seqs:
        base.append(tot); tot += (ln + B - 1) // B
    cov = [0] * tot; res = []
    for sro, ref_len, mq, ops in clumps:
        inside = [i for i, (s, ln) in enumerate(seqs) if s <= sro < s + ln and sro + ref_len - 1 < s + ln]
        if not inside:
            res.append((2, 0)); continue
        if mq < Q:
            res.append((1, 0)); continue
        i = inside[0]; pos = sro; n_cov = 0
        for c, n in ops:
            if c in "MR":
                for p in range(pos, pos + n):
                    cov[base[i] + (p - seqs[i][0]) // B] += 1
                n_cov += n
            if c in "MRD":
                pos += n
        res.append((0, n_cov))
    return res, cov


@pytest.mark.parametrize("B", [1, 7, 100])
def test_the_shared_walk_on_hand_made_clumps(tmp_path, B):
    seqs = [(0, 1000), (1000, 250), (1300, 333)]      # (a gap between the second and the third: starts are whatever the genome file says)
    M, R, I, D = "MRID"
    clumps = [
        (95, 20, 250, [(M, 20)]),                                             # a run crossing a bin edge (B = 100: 5 + 15)
        (1233, 17, 250, [(M, 10), (R, 1), (M, 6)]),                           # ends on the last base of the second sequence: its last, short bin
        (1240, 20, 250, [(M, 20)]),                                           # spans two sequences: dropped, counts nothing
        (990, 20, 250, [(M, 20)]),                                            # the same at the first boundary
        (300, 150, 250, [(M, 40), (D, 30), (M, 10), (I, 7), (R, 2), (M, 68)]),      # D and I in the middle
        (1400, 50, 9, [(M, 50)]),                                             # the MAPQ gate (Q = 10 below)
        (1400, 50, 10, [(M, 50)]),
        (1600, 33, 255, [(M, 33)]),                                           # the last base of the last sequence
        (1250, 5, 250, [(M, 5)]),                                             # starts in the gap between two sequences: dropped
        (10, 400, 250, [(M, 1), (R, 1)] * 100 + [(D, 1), (M, 199)]),          # many short ops, then one long run
    ]
    for Q in (0, 10):
        got_res, got_cov = _drive(tmp_path, B, Q, seqs, clumps)
        want_res, want_cov = _by_hand(B, Q, seqs, clumps)
        assert got_res == want_res
        assert got_cov == want_cov
    assert [r[0] for r in _by_hand(B, 10, seqs, clumps)[0]] == [0, 0, 2, 2, 0, 1, 0, 0, 2, 0]
    if B == 100:
        c = _by_hand(B, 0, seqs, clumps)[1]
        assert c[0] == 5 + 90 and c[1] == 15 + 100 and c[12] == 17 + 0      # bins 0 and 1 also hold the last clump's bases; bin 12 = [1200, 1250) of the second sequence
