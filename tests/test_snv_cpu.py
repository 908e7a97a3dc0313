"""CPU tier: SNV calls with genotypes (-osnv FILE, -snverr E, -snvmin N, -snvdp D, -snvqual Q, gate -puq): the VCF of the sites the pileup genotypes as 0/1 or
1/1.  The command line is built with the test double for the device (tests/fixtures/oracle_device.cpp, as tests/test_pileup_cpu.py does) -- it has no
ygpu_pileup_* / ygpu_snv_* entry points, so the host counts every record and ysnv's routine runs on the host over the host's own candidates; the device stage is
proven by tests/test_gpu_snv.py.  The check is exact and independent of the product: the file is a pure function of the run's SAM text and the reference
FASTA, recomputed by tests/pileup_oracle.py and tests/snv_oracle.py.  The reads are a variant set made here with a fixed seed (snv_oracle.variant_reads): the
golden reads are simulated from the reference itself and hold no variants."""
import ctypes as C
import glob
import json
import os
import subprocess

import pytest

import pileup_oracle as po
import snv_oracle as so
from conftest import ROOT, strip_pg

HOST = os.path.join(ROOT, "yaha_amd", "csrc", "host")
SRCS = sorted(glob.glob(os.path.join(HOST, "*.cpp"))) + [os.path.join(ROOT, "yaha_amd", "csrc", "main.cpp"), os.path.join(ROOT, "tests", "fixtures", "oracle_device.cpp"),
                                                          os.path.join(ROOT, "oracle", "hotpath.cpp")]
SET2 = dict(err=50, min_alt=3, min_depth=6, min_qual=30)
SET2_ARGS = ["-snverr", "50", "-snvmin", "3", "-snvdp", "6", "-snvqual", "30", "-puq", "10"]
SNV_KEYS = ["snv_calls", "snv_het", "snv_hom", "snv_on_device", "snv_folded_slots"]


def _build(tmp, san):
    exe = os.path.join(tmp, "yaha_" + san.replace(",", "_"))
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=" + san, "-fno-omit-frame-pointer", "-pthread", "-o", exe] + SRCS)
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("snv"))
    return {"tsan": _build(d, "thread"), "asan": _build(d, "address,undefined")}


def _run(exe, args, env=None):
    e = dict(os.environ, YAHA_KEEP_TEARDOWN="1", TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    e.update(env or {})
    return subprocess.run([exe] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def _clean(p):
    err = p.stderr.decode()
    assert "ThreadSanitizer" not in err and "AddressSanitizer" not in err and "runtime error:" not in err, err[-4000:]


def _stats(p):
    return json.loads([l for l in p.stderr.decode().split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])


def _pg(p):
    return [l for l in p.stdout.decode().split("\n") if l.startswith("@PG")]


@pytest.fixture(scope="module")
def variants(work, tmp_path_factory):
    """The variant reads in a file, what was planted, and the reference."""
    fasta = po.read_fasta(os.path.join(work, "genome_small.fa"))
    text, planted = so.variant_reads(fasta)
    path = str(tmp_path_factory.mktemp("snvreads") / "variants.fa")
    open(path, "w").write(text)
    return path, planted, fasta


@pytest.fixture(scope="module")
def base_run(exes, index11, variants, tmp_path_factory):
    """The default run under ASan / UBSan: its SAM text, its file, its stats -- and the oracle's pileups of that SAM text (Q = 0 and 10), made once."""
    out = str(tmp_path_factory.mktemp("snvbase") / "calls.vcf")
    p = _run(exes["asan"], ["-x", index11, "-q", variants[0], "-osh", "stdout", "-osnv", out], env={"YAHA_STATS": "1"})
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    _clean(p)
    lines = p.stdout.decode().split("\n"); sq = po.sq_table(lines); ref = po.ref_letters(sq, variants[2])
    pus = {Q: po.pileup(lines, sq, Q) for Q in (0, 10)}
    for a in pus.values():
        a.setflags(write=False)
    return dict(p=p, lines=lines, sq=sq, ref=ref, pu=pus, got=open(out).read())


def test_the_oracle_finds_what_the_comparison_stands_on(base_run, variants):
    """Asserted on the ORACLE's result over the run's own SAM text, before anything of the product is compared with it."""
    pu, ref, sq = base_run["pu"][0], base_run["ref"], base_run["sq"]
    cl = so.calls(pu, ref)
    assert sum(1 for _s, v in cl if v["gt"] == 1) >= 20 and sum(1 for _s, v in cl if v["gt"] == 2) >= 20
    assert {chr(ref[s]) for s, _v in cl} == set("ACGT")
    # a slot that -snvqual alone removes: a genotype, enough alt reads, enough depth, too little QUAL
    only_qual = so.calls(pu, ref, keep=lambda v: v["gt"] != 0 and v["a"] >= 2 and v["depth"] >= 4 and v["qual"] < 20)
    assert len(only_qual) >= 1
    assert so.text(pu, sq, ref) != so.text(base_run["pu"][10], sq, ref, Q=10, **SET2)
    # how many planted sites the model finds is a property of the model: printed, not asserted
    base, tot = {}, 0
    for name, ln in sq:
        base[name] = tot; tot += ln
    called = {s: v for s, v in cl}
    for kind, gt in (("hom", 2), ("het", 1)):
        sites = [base[n] + pos for n, pos, _r, _a, k in variants[1] if k == kind]
        print("planted %s: %d, called: %d, with the planted genotype: %d" % (kind, len(sites), sum(s in called for s in sites),
                                                                          sum(s in called and called[s]["gt"] == gt for s in sites)))
    print("calls: %d, at no planted site: %d" % (len(cl), len(set(called) - {base[n] + pos for n, pos, _r, _a, _k in variants[1]})))


def test_file_equals_the_oracle_and_the_sam_is_undisturbed(exes, index11, variants, base_run, tmp_path):
    out = str(tmp_path / "calls.vcf"); sq, ref = base_run["sq"], base_run["ref"]
    want = so.text(base_run["pu"][0], sq, ref)
    assert base_run["got"] == want and want.count("\n") - want.count("\n#") > 40
    plain = _run(exes["asan"], ["-x", index11, "-q", variants[0], "-osh", "stdout"])
    assert plain.returncode == 0 and strip_pg(plain.stdout.decode()) == strip_pg(base_run["p"].stdout.decode())
    st = _stats(base_run["p"]); cl = so.calls(base_run["pu"][0], ref)
    assert st["snv_calls"] == len(cl) and st["snv_het"] == sum(v["gt"] == 1 for _s, v in cl) and st["snv_hom"] == sum(v["gt"] == 2 for _s, v in cl)
    assert st["snv_on_device"] == 0 and st["snv_folded_slots"] == 0
    # the second option set, with the pileup's gate
    p = _run(exes["asan"], ["-x", index11, "-q", variants[0], "-osh", "stdout", "-osnv", out] + SET2_ARGS)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    _clean(p)
    want2 = so.text(base_run["pu"][10], sq, ref, Q=10, **SET2)
    assert open(out).read() == want2 and want2 != want and want2.count("0/1") >= 1 and want2.count("1/1") >= 1
    assert strip_pg(p.stdout.decode()) == strip_pg(base_run["p"].stdout.decode())


def test_the_file_does_not_depend_on_batching_threads_or_the_filter_side(exes, index11, variants, base_run, tmp_path):
    out = str(tmp_path / "calls.vcf")
    for exe, extra, env in (("asan", ["-batch", "61"], {}), ("asan", ["-dpf", "N", "-batch", "300"], {}), ("asan", ["-t", "3", "-batch", "300"], {"YAHA_CPUS": "6"}),
                            ("tsan", ["-t", "3", "-gpus", "2", "-ctx", "2", "-batch", "97"], {"YTEST_DEVICES": "2", "YAHA_CPUS": "6"})):
        p = _run(exes[exe], ["-x", index11, "-q", variants[0], "-osh", "stdout", "-osnv", out] + extra, env=env)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        _clean(p)
        assert open(out).read() == base_run["got"], (extra, env)
        assert strip_pg(p.stdout.decode()) == strip_pg(base_run["p"].stdout.decode()), (extra, env)


def test_argument_errors_and_what_stays_unchanged_without_the_option(exes, work, index11, variants, base_run, tmp_path):
    reads = os.path.join(work, "rchim.fa"); out = str(tmp_path / "calls.vcf"); pu = str(tmp_path / "pu.tsv"); base = ["-x", index11, "-q", reads]
    sam = str(tmp_path / "x.sam")
    for bad in (["-g", os.path.join(work, "genome_small.fa"), "-osnv", out], base + ["-snverr", "100"], base + ["-snvmin", "2"], base + ["-snvdp", "4"],
                base + ["-snvqual", "20"], base + ["-puq", "3"], base + ["-pumin", "2"], base + ["-osnv", out, "-pumin", "2"], base + ["-osnv", out, "-snvmin", "0"],
                base + ["-osnv", out, "-snvdp", "0"], base + ["-osnv", out, "-snverr", "0"], base + ["-osnv", out, "-snverr", "501"], base + ["-osnv", out, "-snvqual", "-1"],
                base + ["-osnv", "stdout"], base + ["-osh", "stdout", "-osnv", "stdout"], base + ["-osh", sam, "-osnv", "stdout", "-opu", "stdout"],
                base + ["-osh", sam, "-osnv", "stdout", "-oep", "stdout"], base + ["-osh", sam, "-osnv", "stdout", "-ocov", "stdout"]):
        p = _run(exes["asan"], bad)
        _clean(p)
        assert p.returncode == 3, (bad, p.returncode, p.stderr.decode()[-300:])
        assert not os.path.exists(out) and not os.path.exists(pu)
    plain = _run(exes["asan"], base + ["-osh", "stdout"], env={"YAHA_STATS": "1"})
    snv = _run(exes["asan"], base + ["-osh", "stdout", "-osnv", out, "-snvmin", "1", "-puq", "2"], env={"YAHA_STATS": "1"})
    assert plain.returncode == 0 and snv.returncode == 0
    assert len(_pg(plain)) == 1 and "snv" not in _pg(plain)[0] and "-pu" not in _pg(plain)[0]
    assert _pg(snv)[0] == _pg(plain)[0] + " -osnv " + out + " -snverr 100 -snvmin 1 -snvdp 4 -snvqual 20"
    a, b = _stats(plain), _stats(snv)
    assert not [k for k in a if "snv" in k or "pileup" in k] and [k for k in b if k not in a] == SNV_KEYS
    # the alignments in a file, the calls on standard output
    p = _run(exes["asan"], base + ["-osh", sam, "-osnv", "stdout"])
    assert p.returncode == 0 and p.stdout.decode().startswith("##fileformat=VCFv4.2\n##source=yaha_amd -snverr 100 -snvmin 2 -snvdp 4 -snvqual 20 -puq 0\n")
    assert strip_pg(open(sam).read()) == strip_pg(plain.stdout.decode())
    # -opu beside it: the same pileup table as alone, the same calls as alone, the pileup's keys before the calls', @PG with the calls' part last
    v = ["-x", index11, "-q", variants[0], "-osh", "stdout"]
    alone = _run(exes["asan"], v + ["-opu", pu, "-pumin", "3"], env={"YAHA_STATS": "1"})
    assert alone.returncode == 0
    table = open(pu).read(); os.remove(pu)
    both = _run(exes["asan"], v + ["-opu", pu, "-pumin", "3", "-osnv", out], env={"YAHA_STATS": "1"})
    assert both.returncode == 0
    _clean(both)
    assert open(pu).read() == table and table.count("\n") > 40 and open(out).read() == base_run["got"]
    assert table == po.text(base_run["pu"][0], base_run["sq"], base_run["ref"], 3)
    assert _pg(both)[0] == _pg(alone)[0] + " -osnv " + out + " -snverr 100 -snvmin 2 -snvdp 4 -snvqual 20"
    assert [k for k in _stats(both) if k not in _stats(alone)] == SNV_KEYS
    assert strip_pg(both.stdout.decode()) == strip_pg(base_run["p"].stdout.decode())


def test_default_costs(work, index11):
    """(46, 1477, 331) at the default -snverr 100: what the oracle derives, what the session hands the device, what the header states."""
    import yaha_amd as ya
    assert so.costs(100) == (46, 1477, 331)
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout", "-osnv", "unused.vcf"]) as s:
        p = ya.SnvParams()
        assert ya.lib().yaha_session_snv_params(s._h, C.byref(p)) == 0
        assert (p.cost_match, p.cost_error, p.cost_het, p.min_alt, p.min_depth, p.min_qual) == (46, 1477, 331, 2, 4, 20)
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout", "-osnv", "unused.vcf"] + SET2_ARGS) as s:
        p = ya.SnvParams()
        assert ya.lib().yaha_session_snv_params(s._h, C.byref(p)) == 0
        assert (p.cost_match, p.cost_error, p.cost_het, p.min_alt, p.min_depth, p.min_qual) == so.costs(50) + (3, 6, 30)
    assert C.sizeof(ya.SnvParams) == 32 and len(ya.SNV_CALL_FIELDS) * 4 == 48


@pytest.mark.parametrize("params", [None, so.costs(50) + (3, 6, 30), so.costs(100) + (1, 1, 0), (46, 1477, 331, 12, 24, 90)])
def test_the_shared_routine_on_every_small_row(tmp_path, params):
    """tests/fixtures/snv_driver.cpp: every reference channel, every (r, x, y, other) in 0 .. 12 -- every tie and both sides of every threshold."""
    exe = str(tmp_path / "snv_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "fixtures", "snv_driver.cpp")])
    p = subprocess.run([exe] + [str(x) for x in (params or ())], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().split("\n")
    assert lines[0] == "defaults 100 46 1477 331"
    cst, (min_alt, min_depth, min_qual) = (params[:3], params[3:]) if params else ((46, 1477, 331), (2, 4, 20))
    k = 1; n_calls = 0; seen = set()
    for rc in range(5):
        for r in range(13):
            for x in range(13):
                for y in range(13):
                    for other in range(13):
                        row = [0, 0, 0, 0, other, other // 2, 3]
                        if rc < 4:
                            row[rc] = r
                            for ch, val in zip([c for c in range(4) if c != rc], (x, y, x * y % 5)):
                                row[ch] = val
                        else:
                            row[:3] = [r, x, y]
                        v = so.verdict(row, "ACGTN"[rc], cst, min_alt, min_depth, min_qual)
                        if v is None:
                            want = "%d %d %d %d %d none 0" % (rc, r, x, y, other)
                        else:
                            want = "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d" % (rc, r, x, y, other, v["call"], v["rc"], v["alt"], v["gt"], v["r"], v["a"], v["depth"],
                                                                                             v["other"], v["qual"], v["gq"], v["pl"][0], v["pl"][1], v["pl"][2])
                            n_calls += v["call"]; seen.add((v["gt"], v["call"]))
                        assert lines[k] == want, (k, lines[k], want)
                        k += 1
    assert k == 1 + 5 * 13 ** 4 and lines[k] == "" and n_calls > 0 and {(1, True), (2, True)} <= seen
    assert params is not None or seen == {(0, False), (1, False), (1, True), (2, False), (2, True)}
