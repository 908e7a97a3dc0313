"""CPU tier: split-read breakpoint calls (-obp FILE, -bpq Q, -bpw W).  The command line is built with the test double for the device
(tests/fixtures/oracle_device.cpp, as tests/test_depth_cpu.py does) -- it has no ygpu_junctions_* entry points, so the host makes every junction here
(host/junctions.cpp looks them up weakly) with the routines the device stage compiles too (yaha_amd/csrc/junction_core.h); the device stage is proven by
tests/test_gpu_junctions.py.  The check is exact and independent of the product: the file is a pure function of the SAM text, recomputed by
tests/junction_oracle.py from the reference's golden lines."""
import ctypes as C
import glob
import json
import os
import re
import subprocess

import pytest

import junction_oracle as jo
from conftest import ROOT, golden_lines, strip_pg

HOST = os.path.join(ROOT, "yaha_amd", "csrc", "host")
SRCS = sorted(glob.glob(os.path.join(HOST, "*.cpp"))) + [os.path.join(ROOT, "yaha_amd", "csrc", "main.cpp"), os.path.join(ROOT, "tests", "fixtures", "oracle_device.cpp"),
                                                          os.path.join(ROOT, "oracle", "hotpath.cpp")]


# ---- the oracle on hand-written SAM lines ------------------------------------------------------------------------------------------------------------------
HDR = ["@HD\tVN:1.0", "@SQ\tSN:chrA\tLN:10000", "@SQ\tSN:chrB\tLN:5000"]


def _rec(name, flag, chrom, pos, cigar, primary=True, mapq=60):
    return "\t".join([name, str(flag), chrom, str(pos), str(mapq), cigar, "*", "0", "0", "*", "*", "AS:i:0", "NM:i:0", "MD:Z:0", "YF:H:%02X" % ((0x20 if primary else 0) | (1 if flag & 16 else 0))])


def test_oracle_forward_and_reverse_reads_of_one_deletion_give_the_same_junction():
    # a 100-base molecule: its first 40 bases at chrA:1000..1039, the other 60 at chrA:1500..1559 (a deletion of 460 bases)
    fwd = [_rec("f", 0, "chrA", 1001, "40M60H"), _rec("f", 0, "chrA", 1501, "40H60M")]
    # the same molecule read from the other strand: on the printed (reverse) strand the first 40 bases of the molecule are the LAST 40 of the read
    rev = [_rec("r", 16, "chrA", 1501, "40H60M"), _rec("r", 16, "chrA", 1001, "40M60H")]
    jf, jr = jo.junctions(HDR + fwd), jo.junctions(HDR + rev)
    assert jf == [(0, 1039, "+", 0, 1500, "+", "DEL", 0)]
    assert jr == jf
    # print order does not matter either, and soft clips are hard clips
    assert jo.junctions(HDR + fwd[::-1]) == jf
    assert jo.junctions(HDR + [_rec("f", 0, "chrA", 1001, "40M60S"), _rec("f", 0, "chrA", 1501, "40S60M")]) == jf


def test_oracle_types_overlap_gap_and_the_gates():
    two = lambda a, b: jo.junctions(HDR + [a, b])
    # DUP: the second piece lies BEFORE the first on the reference, same strand -> swapped, both strands flipped
    assert two(_rec("d", 0, "chrA", 2001, "50M50H"), _rec("d", 0, "chrA", 1801, "50H50M")) == [(0, 1800, "-", 0, 2049, "-", "DUP", 0)]
    # INV: the second piece on the other strand (on the printed strand it is the read's first 50 bases: read-forward 50..99)
    assert two(_rec("i", 0, "chrA", 2001, "50M50H"), _rec("i", 16, "chrA", 3001, "50M50H")) == [(0, 2049, "+", 0, 3049, "-", "INV", 0)]
    # TRA: two sequences; the @SQ order decides which side comes first
    assert two(_rec("t", 0, "chrB", 101, "50M50H"), _rec("t", 0, "chrA", 7001, "50H50M")) == [(0, 7000, "-", 1, 149, "-", "TRA", 0)]
    # overlap (microhomology) and gap on the read; I counts for the read, D for the reference
    assert two(_rec("o", 0, "chrA", 1001, "45M55H"), _rec("o", 0, "chrA", 1501, "40H60M"))[0][7] == -5
    assert two(_rec("g", 0, "chrA", 1001, "30M70H"), _rec("g", 0, "chrA", 1501, "40H60M"))[0][7] == 10
    assert two(_rec("x", 0, "chrA", 1001, "20M2I18M5D10M50H"), _rec("x", 0, "chrA", 1501, "50H50M")) == [(0, 1000 + 20 + 18 + 5 + 10 - 1, "+", 0, 1500, "+", "DEL", 0)]
    # three pieces: two junctions in read order; a secondary record and one below -bpq join nothing, and their neighbours join each other
    three = [_rec("m", 0, "chrA", 101, "30M70H"), _rec("m", 0, "chrA", 501, "30H30M40H"), _rec("m", 0, "chrA", 901, "60H40M")]
    assert [j[:2] + j[3:5] for j in jo.junctions(HDR + three)] == [(0, 129, 0, 500), (0, 529, 0, 900)]
    sec = three[:1] + [_rec("m", 0, "chrA", 501, "30H30M40H", primary=False)] + three[2:]
    assert [j[:2] + j[3:5] + j[7:] for j in jo.junctions(HDR + sec)] == [(0, 129, 0, 900, 30)]
    low = three[:1] + [_rec("m", 0, "chrA", 501, "30H30M40H", mapq=7)] + three[2:]
    assert len(jo.junctions(HDR + low, Q=7)) == 2 and [j[:2] + j[3:5] for j in jo.junctions(HDR + low, Q=8)] == [(0, 129, 0, 900)]
    # one record, or records of different reads: no junction
    assert jo.junctions(HDR + three[:1]) == [] and jo.junctions(HDR + [three[0], three[1].replace("m\t", "n\t", 1)]) == []


def test_oracle_clusters_and_text():
    j = lambda pa, pb, gap=0, sa="+", sb="+": (0, pa, sa, 0, pb, sb, jo.kind(0, sa, 0, sb), gap)
    junc = [j(1000, 5000), j(1004, 4995, -3), j(1010, 5010, 2), j(1011, 5000), j(1000, 5011), j(1005, 5000, sa="-", sb="-"), j(1020, 5000)]
    cl = jo.clusters(junc, 10)
    # sorted: + + group first: (1000,5000) opens; (1000,5011) is 11 away on side B: opens; (1004,4995) joins the first; (1010,5010) joins the first (both within 10 of
    # ITS first member); (1011,5000) is 11 past the first cluster's first posA but within 10 of the second's (1000 -> 11: no) -> opens; (1020,5000) joins that one
    assert [[(m[1], m[4]) for m in c] for c in cl] == [[(1000, 5000), (1004, 4995), (1010, 5010)], [(1000, 5011)], [(1011, 5000), (1020, 5000)], [(1005, 5000)]]
    sq = [("chrA", 10000)]
    assert jo.text(cl, sq) == ("chrA\t1000\t1011\tchrA\t4995\t5011\tDEL\t3\t+\t+\t-3\t2\n" "chrA\t1000\t1001\tchrA\t5011\t5012\tDEL\t1\t+\t+\t0\t0\n"
                               "chrA\t1011\t1021\tchrA\t5000\t5001\tDEL\t2\t+\t+\t0\t0\n" "chrA\t1005\t1006\tchrA\t5000\t5001\tDUP\t1\t-\t-\t0\t0\n")
    assert len(jo.clusters(junc, 0)) == 7


def test_oracle_on_the_goldens_gives_the_figures_of_the_issue():
    fig = {}
    for name in ("rchim_default", "rsv_default", "rsv_OQC_FBS", "r1k_default", "r10k_default", "rq_default"):
        junc = jo.junctions(golden_lines(name))
        fig[name] = (len(junc), jo.by_type(junc), len(jo.clusters(junc, 10)))
    tra = lambda t, de, i, du: {"TRA": t, "DEL": de, "INV": i, "DUP": du}
    assert fig["rchim_default"] == (114, tra(50, 43, 16, 5), 114)
    assert fig["rsv_default"] == (386, tra(108, 86, 143, 49), 120) and fig["rsv_OQC_FBS"] == fig["rsv_default"]
    assert fig["r1k_default"][0] == 1 and fig["r10k_default"][0] == 2 and fig["rq_default"][0] == 15
    junc = jo.junctions(golden_lines("rchim_default"))
    assert sum(1 for j in junc if j[7] < 0) == 40 and sum(1 for j in junc if j[7] > 0) == 24
    junc = jo.junctions(golden_lines("rsv_default")); cl = jo.clusters(junc, 10)
    assert sum(1 for c in cl if len(c) >= 2) == 86 and max(len(c) for c in cl) == 7 and len(jo.clusters(junc, 0)) == 173
    j30 = jo.junctions(golden_lines("rsv_default"), Q=30)
    assert len(j30) == 369 and len(jo.clusters(j30, 10)) == 119
    # the secondary records of the FBS set are printed and join nothing
    sec = lambda name: sum(1 for l in golden_lines(name) if l and not l.startswith("@") and not int(re.search(r"YF:H:([0-9A-F]+)", l).group(1), 16) & 0x20)
    assert sec("rsv_OQC_FBS") == 7 and sec("rsv_default") == 0
    # one read of r10k has three records: two junctions of one read
    assert [r for r, _j in jo.junctions(golden_lines("r10k_default"), with_reads=True)][0:2] == [jo.junctions(golden_lines("r10k_default"), with_reads=True)[0][0]] * 2


# ---- the struct the junctions cross the C-ABI in -----------------------------------------------------------------------------------------------------------
def test_the_junction_record_layout(tmp_path):
    import yaha_amd as ya
    want = [("read", 0, 4), ("ordinal", 4, 4), ("seqA", 8, 4), ("posA", 12, 4), ("seqB", 16, 4), ("posB", 20, 4), ("strandA", 24, 1), ("strandB", 25, 1), ("type", 26, 1),
            ("reserved", 27, 1), ("qgap", 28, 4)]
    assert C.sizeof(ya.Junction) == 32
    assert [(n, getattr(ya.Junction, n).offset, getattr(ya.Junction, n).size) for n, _o, _s in want] == want
    assert C.sizeof(ya.JunctionParams) == 24 and ya.JunctionParams.seq_start.offset == 8 and ya.JunctionParams.seq_length.offset == 16
    # ... and the header's own view of it, through the C compiler
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yaha_hip.h"\n#define F(f) printf("%s %zu %zu\\n", #f, offsetof(ygpu_junction, f), sizeof(((ygpu_junction *)0)->f));\n'
                   'int main(void) { printf("size %zu\\n", sizeof(ygpu_junction)); F(read) F(ordinal) F(seqA) F(posA) F(seqB) F(posB) F(strandA) F(strandB) F(type) F(reserved) F(qgap)\n'
                   'printf("params %zu %zu %zu\\n", sizeof(ygpu_junction_params), offsetof(ygpu_junction_params, seq_start), offsetof(ygpu_junction_params, seq_length));\n'
                   'printf("types %d %d %d %d\\n", YGPU_JUNCTION_DEL, YGPU_JUNCTION_DUP, YGPU_JUNCTION_INV, YGPU_JUNCTION_TRA); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    out = subprocess.check_output([exe]).decode().split("\n")
    assert out[0] == "size 32" and out[1:12] == ["%s %d %d" % w for w in want] and out[12] == "params 24 8 16" and out[13] == "types 0 1 2 3"
    assert ya.JUNCTION_TYPES == ("DEL", "DUP", "INV", "TRA")


# ---- the host path through the pipeline's test double, under the sanitizers -----------------------------------------------------------------------------------
def _build(tmp, san):
    exe = os.path.join(tmp, "yaha_" + san.replace(",", "_"))
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=" + san, "-fno-omit-frame-pointer", "-pthread", "-o", exe] + SRCS)
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("junctions"))
    return {"tsan": _build(d, "thread"), "asan": _build(d, "address,undefined")}


def _run(exe, args, env=None):
    e = dict(os.environ, YAHA_KEEP_TEARDOWN="1", TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    e.update(env or {})
    return subprocess.run([exe] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def _clean(p):
    err = p.stderr.decode()
    assert "ThreadSanitizer" not in err and "AddressSanitizer" not in err and "runtime error:" not in err, err[-4000:]


def _bp_run(exe, index11, reads, out, extra=(), oflag="-osh", env=None):
    p = _run(exe, ["-x", index11, "-q", reads, oflag, "stdout", "-obp", out] + list(extra), env=env)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    _clean(p)
    return p, open(out).read()


_stats = lambda p: json.loads([l for l in p.stderr.decode().split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])


@pytest.mark.parametrize("name,reads,gext", [("rchim_default", "rchim.fa", []), ("rsv_default", "rsv.fa", []), ("rsv_OQC_FBS", "rsv.fa", ["-OQC", "Y", "-FBS", "Y"])])
def test_file_equals_the_oracle_and_the_sam_is_undisturbed(exes, work, index11, tmp_path, name, reads, gext):
    out = str(tmp_path / "bp.bedpe"); lines = golden_lines(name)
    for extra, Q, W in (([], 0, 10), (["-bpw", "0"], 0, 0), (["-bpq", "30"], 30, 10), (["-bpq", "30", "-bpw", "25", "-batch", "7"], 30, 25)):
        p, got = _bp_run(exes["asan"], index11, os.path.join(work, reads), out, gext + extra, env={"YAHA_STATS": "1"})
        assert strip_pg(p.stdout.decode()) == lines, (name, extra)
        junc = jo.junctions(lines, Q); cl = jo.clusters(junc, W)
        assert got == jo.text(cl, jo.sq_table(lines)), (name, extra)
        # every type is there, whatever the gates: an empty class proves nothing
        assert all(v > 0 for v in jo.by_type(junc).values()), (name, extra)
        st = _stats(p)
        assert st["bp_junctions"] == len(junc) and st["bp_clusters"] == len(cl) == got.count("\n") and st["bp_device_reads"] == 0
        assert st["bp_host_reads"] == len({r for r, _j in jo.junctions(lines, Q, with_reads=True)}) > 0
    if name.startswith("rsv"):
        assert any(len(c) >= 2 for c in jo.clusters(jo.junctions(lines), 10))


def test_under_the_thread_sanitizer_with_many_contexts(exes, work, index11, tmp_path):
    out = str(tmp_path / "bp.bedpe")
    p, got = _bp_run(exes["tsan"], index11, os.path.join(work, "rsv.fa"), out, ["-t", "3", "-gpus", "2", "-ctx", "2", "-batch", "29"], env={"YTEST_DEVICES": "2", "YAHA_CPUS": "6"})
    assert strip_pg(p.stdout.decode()) == golden_lines("rsv_default")
    assert got == jo.expected(golden_lines("rsv_default"))


def test_the_file_does_not_depend_on_batching_filter_side_threads_or_output_format(exes, work, index11, tmp_path):
    out = str(tmp_path / "bp.bedpe"); reads = os.path.join(work, "rsv.fa")
    want = jo.expected(golden_lines("rsv_default"), 0, 10)
    for extra, oflag, env in ((["-batch", "5"], "-osh", {}), (["-batch", "61"], "-osh", {}), (["-dpf", "N", "-batch", "61"], "-osh", {}), (["-t", "3", "-batch", "61"], "-osh", {"YAHA_CPUS": "6"}),
                              (["-batch", "61"], "-osh", {"YTEST_RAW_ABOVE": "3"}), (["-batch", "61"], "-osh", {"YAHA_HOST_OQC": "1"}), (["-batch", "61"], "-oss", {}), (["-batch", "61"], "-o8", {})):
        _p, got = _bp_run(exes["asan"], index11, reads, out, extra, oflag=oflag, env=env)
        assert got == want, (extra, oflag, env)


def test_argument_errors_and_what_stays_unchanged_without_the_option(exes, work, index11, tmp_path):
    reads = os.path.join(work, "rchim.fa"); out = str(tmp_path / "bp.bedpe"); base = ["-x", index11, "-q", reads]
    for bad in (["-g", os.path.join(work, "genome_small.fa"), "-obp", out], base + ["-bpq", "10"], base + ["-bpw", "3"], base + ["-obp", out, "-bpw", "-1"], base + ["-obp", out, "-bpq", "256"],
                base + ["-obp", "stdout"], base + ["-osh", "stdout", "-obp", "stdout"], base + ["-osh", str(tmp_path / "x.sam"), "-obp", "stdout", "-ocov", "stdout"]):
        p = _run(exes["asan"], bad)
        _clean(p)
        assert p.returncode == 2, (bad, p.returncode, p.stderr.decode()[-300:])
        assert not os.path.exists(out)
    plain = _run(exes["asan"], base + ["-osh", "stdout"], env={"YAHA_STATS": "1"})
    bp = _run(exes["asan"], base + ["-osh", "stdout", "-obp", out, "-bpq", "2", "-bpw", "7"], env={"YAHA_STATS": "1"})
    assert plain.returncode == 0 and bp.returncode == 0
    pg = lambda p: [l for l in p.stdout.decode().split("\n") if l.startswith("@PG")]
    assert len(pg(plain)) == 1 and "-obp" not in pg(plain)[0] and "-bp" not in pg(plain)[0]
    assert pg(bp)[0] == pg(plain)[0] + " -obp " + out + " -bpq 2 -bpw 7"
    new = {"bp_device_reads", "bp_host_reads", "bp_junctions", "bp_clusters"}
    assert not (new & set(_stats(plain))) and set(_stats(bp)) - set(_stats(plain)) == new
    assert open(out).read() == jo.expected(golden_lines("rchim_default"), 2, 7)
    # the alignments in a file, the calls on standard output
    sam = str(tmp_path / "out.sam")
    p = _run(exes["asan"], base + ["-osh", sam, "-obp", "stdout"])
    assert p.returncode == 0 and p.stdout.decode() == jo.expected(golden_lines("rchim_default"))
    assert strip_pg(open(sam).read()) == golden_lines("rchim_default")
    # beside the two tracks: their files are what a run without -obp writes
    cov, ev = str(tmp_path / "cov.bg"), str(tmp_path / "ev.tsv")
    alone = _run(exes["asan"], base + ["-osh", "stdout", "-ocov", cov, "-oev", ev])
    assert alone.returncode == 0
    cov_alone, ev_alone = open(cov).read(), open(ev).read(); os.remove(cov); os.remove(ev); os.remove(out)
    both = _run(exes["asan"], base + ["-osh", "stdout", "-ocov", cov, "-oev", ev, "-obp", out])
    assert both.returncode == 0
    _clean(both)
    assert open(cov).read() == cov_alone != "" and open(ev).read() == ev_alone != "" and open(out).read() == jo.expected(golden_lines("rchim_default"))
    assert strip_pg(both.stdout.decode()) == golden_lines("rchim_default")


# ---- the routine host and device share, on hand-made records ---------------------------------------------------------------------------------------------------
def test_the_shared_routine_on_hand_made_records_with_ties(tmp_path):
    """Ties in qs and in (qs, qe) cannot come out of the post-filter (two primaries of a read start at least -MNO >= 1 bases apart), so the (qs, qe, print order)
    rule is checked here, on the routine itself, against the oracle's own ordering."""
    exe = str(tmp_path / "junction_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "fixtures", "junction_driver.cpp")])
    seqs = [(0, 10000), (10000, 5000), (15200, 3000)]                  # (a gap before the third: starts are whatever the genome file says)
    P, R = 0x20, 0x01
    # per read: qlen, [(sro, refLen, sqo, eqo, status, mapQuality)]
    reads = [
        (100, [(1000, 40, 0, 39, P, 60), (1500, 60, 40, 99, P, 60)]),                                              # forward
        (100, [(1500, 60, 40, 99, P | R, 60), (1000, 40, 0, 39, P | R, 60)]),                                      # the same molecule, other strand
        (300, [(4000, 50, 100, 149, P, 60), (2000, 50, 100, 159, P, 60), (3000, 50, 100, 149, P, 60), (10100, 50, 0, 49, P, 60)]),      # ties: in qs, and in (qs, qe) -> print order
        (200, [(9990, 30, 0, 29, P, 60), (100, 50, 30, 79, P, 60), (16000, 50, 80, 129, P | R, 9), (15300, 50, 130, 179, P, 60), (700, 20, 180, 199, 0, 60)]),
        (100, [(5000, 100, 0, 99, P, 60)]),
        (100, []),
        (500, [(2000 + 50 * ((7 * k) % 90), 4, 5 * k, 5 * k + 3, P | (R if k % 4 == 1 else 0), 60) for k in range(90)]),      # more records than a wave has lanes
    ]
    for Q in (0, 10):
        text = "%d %d\n" % (Q, len(seqs)) + "".join("%d %d\n" % s for s in seqs)
        for qlen, recs in reads:
            text += "%d %d\n" % (qlen, len(recs)) + "".join("%d %d %d %d %d %d\n" % r for r in recs)
        p = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        got, lines = [], p.stdout.decode().split("\n")
        for l in lines:
            if l.startswith("read "):
                got.append((int(l.split()[1]), [])); continue
            if l:
                f = l.split(); assert int(f[0]) == len(got[-1][1])
                got[-1][1].append((int(f[1]), int(f[2]), f[3], int(f[4]), int(f[5]), f[6], jo.TYPES[int(f[7])], int(f[8])))
        want = []
        for qlen, recs in reads:
            pieces, skipped = [], 0
            for sro, rl, sqo, eqo, status, mq in recs:
                inside = [i for i, (s, ln) in enumerate(seqs) if s <= sro < s + ln and sro + rl - 1 < s + ln]
                if not inside or not status & P:
                    continue
                if mq < Q:
                    skipped += 1; continue
                rev = bool(status & R); s = seqs[inside[0]][0]
                qs, qe = (qlen - 1 - eqo, qlen - 1 - sqo) if rev else (sqo, eqo)
                pieces.append((qs, qe, inside[0], sro - s, sro - s + rl - 1, rev))
            want.append((skipped, jo.read_junctions(pieces)))
        assert got == want
    # by hand: the two strands agree; the tied records come out as (100..149 print 0), (100..149 print 2), (100..159), after the piece at 0..49 on the second sequence
    assert want[0][1] == want[1][1] == [(0, 1039, "+", 0, 1500, "+", "DEL", 0)]
    assert [j[:2] + j[3:5] for j in want[2][1]] == [(0, 4000, 1, 149), (0, 3000, 0, 4049), (0, 2000, 0, 3049)]
    # Q = 10: the record across two sequences (9990 + 30 > 10000), the secondary one and the one of MAPQ 9 join nothing
    assert want[3] == (1, [(0, 149, "+", 2, 100, "+", "TRA", 50)])
    assert want[4] == (0, []) and want[5] == (0, []) and len(want[6][1]) == 89
