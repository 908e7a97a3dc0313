"""CPU tier: indel calls with genotypes (-oindel FILE, -inderr E, -indmin N, -inddp D, -indqual Q, -indshift S, gate -puq): the run's raw indel alleles
left-normalised, merged and judged at their anchor base, written as VCF.  Two layers are held to tests/indelcall_oracle.py here: the shared core
(yaha_amd/csrc/indelcall_core.h) through the stand-alone driver tests/fixtures/indelcall_driver.cpp, built with ASan / UBSan, on the whole directed set of
tests/indelcall_sets.py; and the command line built with the test double for the device (tests/fixtures/oracle_device.cpp: no ygpu_indelcall_* entry points,
so the host's routine runs) on a variant read set with planted indels.  The device stage is proven by tests/test_gpu_indelcalls.py."""
import ctypes as C
import glob
import json
import os
import subprocess

import pytest

import indel_oracle as io
import indelcall_oracle as ico
import indelcall_sets as S
import pileup_oracle as po
from conftest import ROOT, strip_pg

HOST = os.path.join(ROOT, "yaha_amd", "csrc", "host")
SRCS = sorted(glob.glob(os.path.join(HOST, "*.cpp"))) + [os.path.join(ROOT, "yaha_amd", "csrc", "main.cpp"), os.path.join(ROOT, "tests", "fixtures", "oracle_device.cpp"),
                                                          os.path.join(ROOT, "oracle", "hotpath.cpp")]
KEYS = ["indel_calls", "indel_call_het", "indel_call_hom", "indel_call_on_device", "indel_call_raw", "indel_call_shifted", "indel_call_merged", "indel_call_skipped"]
SET2 = dict(err=100, min_alt=3, min_depth=6, min_qual=30, shift=3)
SET2_ARGS = ["-inderr", "100", "-indmin", "3", "-inddp", "6", "-indqual", "30", "-indshift", "3", "-puq", "10"]


@pytest.fixture(scope="module")
def craft():
    g = S.Craft(); raw, tags = S.directed(g)
    return g, raw, tags


def test_the_directed_set_reaches_what_it_is_for(craft):
    """Asserted on the ORACLE's result, before anything of the product is compared with it."""
    g, raw, tags = craft
    norm = lambda name, shift=256: ico.normalise(raw[tags[name]][0], g.ref, g.sq, shift)
    assert len(g.sq) >= 3
    # every run allele moves, by exactly what its run allows: the wave-step edges on both sides
    for n in S.HOMO:
        assert norm("homo%d_ins" % n)[1] == n and norm("homo%d_del" % n)[1] == n - 1
    assert {norm("homo%d_ins" % n)[1] for n in S.HOMO} | {norm("homo%d_del" % n)[1] for n in S.HOMO} >= {0, 1, 2, 62, 63, 64, 65, 126, 127, 128, 129}
    # repeats whose length is no multiple of the unit, rotations with s mod L zero and not
    assert norm("di7_ins")[1] == 7 and norm("tri10_ins")[1] == 10 and norm("tri11_ins")[1] == 11 and norm("di8_ins")[1] == 8 and norm("ins21x2")[1] == 42
    for L in (2, 21, 22, 41, 42):
        key, s = norm("ins%d" % L)
        assert s == 2 * L + L // 2 and s % L != 0 and key[3] != raw[tags["ins%d" % L]][0][3] and sorted(key[3]) == sorted(raw[tags["ins%d" % L]][0][3])
    assert norm("ins21x2")[0][3] == raw[tags["ins21x2"]][0][3] and norm("ins43") is None
    for L in (2, 64, 65):
        assert norm("del%d" % L)[1] == L + 5
    assert norm("del300")[1] == 256 and norm("del300", 1000)[1] == 305
    # boundaries: the anchor cap at a sequence's first base (the run goes on in the previous sequence), an N in the run, alleles without an anchor
    e0 = g.runs["edge"][0]
    assert g.ref[e0 - 4:e0 + 6] == "T" * 10 and norm("edge_ins")[0][0] == e0 + 1 and norm("edge_ins")[1] == 5 and norm("edge_del")[0][0] == e0 + 1
    assert norm("broken_ins")[1] == 4 and norm("broken_del")[1] == 3 and norm("n_in_ins")[1] == 1
    assert norm("first_slot_del") is None and norm("first_slot_ins") is None
    # caps: 0, run - 1, run, run + 1
    assert [norm("homo64_ins", s)[1] for s in (0, 63, 64, 65)] == [0, 63, 64, 64]
    # merging: three become one, two stay two by length, a count saturates
    merged, st = ico.merge(raw, g.ref, g.sq, 256)
    r0 = g.runs["homo129"][0]
    assert merged[(r0, S.DEL, 1, "")] == 6 + 2 + 3 and norm("merge_mid")[0] == norm("merge_left")[0] == norm("homo129_del")[0]
    assert norm("stay_two")[0][0] == norm("homo65_del")[0][0] and norm("stay_two")[0] != norm("homo65_del")[0]
    assert merged[norm("saturate")[0]] == 0xFFFFFFFF and st == dict(raw=len(raw), shifted=st["shifted"], merged=3, skipped=3) and st["shifted"] > 40
    # judging: a > d, a = d, d = 0, the three genotypes, each threshold one below and at its value
    rows = S.RowTable(S.rows_for(g, merged, tags, raw))
    by = {k: v for k, v in ico.judged(merged, rows, keep=lambda v: True)}
    j = [by[norm("judge%d" % i)[0]] for i in range(len(S.JUDGE))]
    assert [(v["a"], v["d"]) for v in j] == list(S.JUDGE)
    assert j[0]["d"] == 0 and j[0]["r"] == 0 and j[1]["r"] == 0 and j[1]["a"] > j[1]["d"] and j[2]["a"] == j[2]["d"] and j[11]["r"] == 0
    assert {v["gt"] for v in j} == {0, 1, 2} and j[3]["gt"] == 1 and j[4]["gt"] == 0 and j[2]["gt"] == 2
    # (with the default costs two carrying reads over a depth of four never reach QUAL 20: -indmin at its value and one below is a second parameter set)
    assert (j[5]["a"], j[5]["call"], j[6]["a"], j[6]["call"], j[6]["qual"]) == (1, False, 2, False, 14)
    by5 = {k: v for k, v in ico.judged(merged, rows, min_alt=5, keep=lambda v: True)}
    assert (j[10]["a"], by5[norm("judge10")[0]]["call"], j[3]["a"], by5[norm("judge3")[0]]["call"]) == (4, False, 5, True)
    assert (j[7]["d"], j[7]["call"], j[8]["d"], j[8]["call"]) == (3, False, 4, True) and j[7]["qual"] >= 20
    assert (j[9]["qual"], j[9]["call"], j[10]["qual"], j[10]["call"]) == (19, False, 20, True) and j[9]["gt"] == 1
    assert ico.costs(50) == (22, 1301, 301)


def _driver_input(g, raw, rows, shift, cst, thr):
    starts, at = [], 0
    image = []
    for _n, s in g.seqs:
        at += 3                                                                  # (sequences are padded in the image: a slot is no offset)
        image.append("N" * 3); starts.append((at, len(s))); image.append(s); at += len(s)
    lines = ["S %d" % len(starts)] + ["%d %d" % s for s in starts] + ["B " + "".join(image), "M %d" % shift, "P %d %d %d %d %d %d" % (cst + thr)]
    lines += ["A %d" % len(raw)] + ["%d %d %d %d" % (ico.words(k) + (n,)) for k, n in raw]
    lines += ["R %d" % len(rows)] + ["%d %s" % (s, " ".join(str(x) for x in r)) for s, r in sorted(rows.items())]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("icdrv") / "indelcall_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "fixtures", "indelcall_driver.cpp")])
    return exe


@pytest.mark.parametrize("shift,params", [(256, None), (0, None), (63, None), (64, None), (65, None), (1000, (100, 3, 6, 30)), (65535, (10, 1, 1, 0)), (256, (50, 5, 4, 20))])
def test_the_shared_core_equals_the_oracle_on_the_directed_set(craft, driver, tmp_path, shift, params):
    """Normalisation, merging and every field of every verdict, for the caps around a run of 64, no cap to speak of and the largest one."""
    g, raw, tags = craft
    err, thr = (params[0], params[1:]) if params else (50, (2, 4, 20))
    merged, st = ico.merge(raw, g.ref, g.sq, shift)
    rows = S.rows_for(g, ico.merge(raw, g.ref, g.sq, 256)[0], tags, raw)          # (the rows of the default shift: other caps meet other anchors, many of them bare)
    path = str(tmp_path / "in.txt"); open(path, "w").write(_driver_input(g, raw, rows, shift, ico.costs(err), thr))
    p = subprocess.run([driver, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    got = p.stdout.decode().split("\n")
    assert got[0] == "stats %d %d %d %d" % (st["raw"], st["shifted"], st["merged"], st["skipped"])
    want = ico.judged(merged, S.RowTable(rows), err, *thr, keep=lambda v: True)
    recs = ico.records(want, g.ref)
    assert len(got) == len(want) + 2 and got[-1] == "" and len(want) == len(merged) > 40
    for line, (k, v), r in zip(got[1:], want, recs):
        assert line == "%d %d %d %d %d %s" % (r[0], r[1], r[2], v["a"], v["call"], " ".join(str(x) for x in r[3:12])), (k, line)
    assert any(v["call"] for _k, v in want) and not all(v["call"] for _k, v in want)


# ---- the command line with the test double for the device ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("icexe") / "yaha_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-pthread", "-o", out] + SRCS)
    return out


def _run(exe, args, env=None):
    e = dict(os.environ, YAHA_KEEP_TEARDOWN="1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1", YAHA_STATS="1")
    e.update(env or {})
    p = subprocess.run([exe] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = p.stderr.decode()
    assert "AddressSanitizer" not in err and "runtime error:" not in err, err[-4000:]
    return p


def _stats(p):
    return json.loads([l for l in p.stderr.decode().split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])


@pytest.fixture(scope="module")
def reads(work, tmp_path_factory):
    fasta = po.read_fasta(os.path.join(work, "genome_small.fa"))
    text, planted = S.indel_reads(fasta)
    path = str(tmp_path_factory.mktemp("icreads") / "indels.fa")
    open(path, "w").write(text)
    return path, planted, fasta


@pytest.fixture(scope="module")
def base_run(exe, index11, reads, tmp_path_factory):
    """The default run: its SAM text, its file, its stats -- and the oracle's alleles and pileups of that SAM text (Q = 0 and 10), made once."""
    out = str(tmp_path_factory.mktemp("icbase") / "calls.vcf")
    p = _run(exe, ["-x", index11, "-q", reads[0], "-osh", "stdout", "-oindel", out])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().split("\n"); sq = po.sq_table(lines); ref = po.ref_letters(sq, reads[2]).tobytes().decode()
    pus = {Q: po.pileup(lines, sq, Q) for Q in (0, 10)}; als = {Q: io.alleles(lines, sq, Q, 1) for Q in (0, 10)}
    for a in pus.values():
        a.setflags(write=False)
    return dict(p=p, lines=lines, sq=sq, ref=ref, pu=pus, al=als, got=open(out).read())


def test_command_line_file_equals_the_oracle(exe, index11, reads, base_run, tmp_path):
    sq, ref = base_run["sq"], base_run["ref"]
    want = ico.text(base_run["al"][0], base_run["pu"][0], sq, ref)
    merged, st = ico.merge(base_run["al"][0], ref, sq, 256)
    cl = ico.judged(merged, base_run["pu"][0])
    # what the reads reach, on the oracle's result: calls of both types and both genotypes, alleles that moved and alleles that merged
    assert {(k[1], v["gt"]) for k, v in cl} == {(S.DEL, 1), (S.DEL, 2), (S.INS, 1), (S.INS, 2)} and len(cl) > 40
    assert st["shifted"] > 20 and st["merged"] > 0
    print("planted %d, calls %d, raw alleles %d, shifted %d, merged away %d, skipped %d" % (len(reads[1]), len(cl), st["raw"], st["shifted"], st["merged"], st["skipped"]))
    assert base_run["got"] == want
    got = _stats(base_run["p"])
    assert [k for k in got if k.startswith("indel")] == KEYS and not [k for k in got if "pileup" in k or "snv" in k]
    assert (got["indel_calls"], got["indel_call_het"], got["indel_call_hom"], got["indel_call_on_device"]) == (
        len(cl), sum(v["gt"] == 1 for _k, v in cl), sum(v["gt"] == 2 for _k, v in cl), 0)
    assert (got["indel_call_raw"], got["indel_call_shifted"], got["indel_call_merged"], got["indel_call_skipped"]) == (st["raw"], st["shifted"], st["merged"], st["skipped"])
    # the SAM text is what a run without the option prints
    plain = _run(exe, ["-x", index11, "-q", reads[0], "-osh", "stdout"])
    assert plain.returncode == 0 and strip_pg(plain.stdout.decode()) == strip_pg(base_run["p"].stdout.decode())
    assert not [k for k in _stats(plain) if k.startswith("indel")]
    # another option set with the gate, and without normalisation
    out = str(tmp_path / "calls.vcf")
    p = _run(exe, ["-x", index11, "-q", reads[0], "-osh", "stdout", "-oindel", out, "-batch", "97"] + SET2_ARGS)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    want2 = ico.text(base_run["al"][10], base_run["pu"][10], sq, ref, Q=10, **SET2)
    assert open(out).read() == want2 and want2 != want and want2.count("0/1") >= 1 and want2.count("1/1") >= 1
    p = _run(exe, ["-x", index11, "-q", reads[0], "-osh", "stdout", "-oindel", out, "-indshift", "0", "-t", "3"], env={"YAHA_CPUS": "6"})
    assert p.returncode == 0 and open(out).read() == ico.text(base_run["al"][0], base_run["pu"][0], sq, ref, shift=0) != want
    assert _stats(p)["indel_call_shifted"] == 0


def test_beside_the_other_outputs_and_the_refused_combination(exe, index11, reads, base_run, tmp_path):
    t = lambda n: str(tmp_path / n)
    v = ["-x", index11, "-q", reads[0], "-osh", "stdout"]
    three = ["-oid", t("id.tsv"), "-opu", t("pu.tsv"), "-osnv", t("snv.vcf")]
    alone = _run(exe, v + three)
    assert alone.returncode == 0, alone.stderr.decode()[-2000:]
    files = [open(t(n)).read() for n in ("id.tsv", "pu.tsv", "snv.vcf")]
    for n in ("id.tsv", "pu.tsv", "snv.vcf"):
        os.remove(t(n))
    both = _run(exe, v + three + ["-oindel", t("calls.vcf")])
    assert both.returncode == 0, both.stderr.decode()[-2000:]
    assert [open(t(n)).read() for n in ("id.tsv", "pu.tsv", "snv.vcf")] == files and files[0].count("\n") > 40 and files[1].count("\n") > 40
    assert open(t("calls.vcf")).read() == base_run["got"]
    a, b = _stats(alone), _stats(both)
    assert [k for k in b if k not in a] == KEYS and all(a[k] == b[k] for k in a if k.startswith(("indel_", "pileup_", "snv_")))
    pg = lambda p: [l for l in p.stdout.decode().split("\n") if l.startswith("@PG")][0]
    assert pg(both) == pg(alone) + " -oindel " + t("calls.vcf") + " -inderr 50 -indmin 2 -inddp 4 -indqual 20 -indshift 256"
    # beside -osnv alone (its array is shared), and beside -oid alone
    for extra in (["-osnv", t("snv.vcf")], ["-oid", t("id.tsv")]):
        p = _run(exe, v + extra + ["-oindel", t("calls.vcf")])
        assert p.returncode == 0 and open(t("calls.vcf")).read() == base_run["got"] and open(extra[1]).read() == files[2 if extra[0] == "-osnv" else 0]
    # refused: another -oid setting beside -oindel, the options without the output, values out of range, two outputs on standard output
    os.remove(t("calls.vcf"))
    for bad in (v + ["-oid", t("x.tsv"), "-idlen", "2", "-oindel", t("calls.vcf")], v + ["-oid", t("x.tsv"), "-idq", "5", "-oindel", t("calls.vcf")],
                v + ["-oid", t("x.tsv"), "-oindel", t("calls.vcf"), "-puq", "5"], v + ["-inderr", "50"], v + ["-indshift", "3"], v + ["-indmin", "2"],
                v + ["-oindel", t("calls.vcf"), "-indshift", "65536"], v + ["-oindel", t("calls.vcf"), "-inderr", "0"], v + ["-oindel", t("calls.vcf"), "-indmin", "0"],
                v + ["-oindel", t("calls.vcf"), "-inddp", "0"], v + ["-oindel", "stdout"], ["-g", t("g.fa"), "-oindel", t("calls.vcf")]):
        p = _run(exe, bad)
        assert p.returncode == 3, (bad, p.returncode, p.stderr.decode()[-300:])
        assert not os.path.exists(t("calls.vcf")) and not os.path.exists(t("x.tsv"))
    assert "-idlen 1 and -idq equal to -puq" in _run(exe, v + ["-oid", t("x.tsv"), "-idlen", "2", "-oindel", t("calls.vcf")]).stderr.decode()
    # -oid with -idq equal to -puq is shared
    p = _run(exe, v + ["-oid", t("id.tsv"), "-idq", "10", "-oindel", t("calls.vcf")] + SET2_ARGS)
    assert p.returncode == 0 and open(t("calls.vcf")).read() == ico.text(base_run["al"][10], base_run["pu"][10], base_run["sq"], base_run["ref"], Q=10, **SET2)


def test_default_costs_and_sizes(work, index11):
    import yaha_amd as ya
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout", "-oindel", "unused.vcf"]) as s:
        p = ya.IndelCallParams()
        assert ya.lib().yaha_session_indelcall_params(s._h, C.byref(p)) == 0
        assert (p.cost_match, p.cost_error, p.cost_het, p.min_alt, p.min_depth, p.min_qual) == (22, 1301, 301, 2, 4, 20)
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout", "-oindel", "unused.vcf"] + SET2_ARGS) as s:
        p = ya.IndelCallParams()
        assert ya.lib().yaha_session_indelcall_params(s._h, C.byref(p)) == 0
        assert (p.cost_match, p.cost_error, p.cost_het, p.min_alt, p.min_depth, p.min_qual) == ico.costs(100) + (3, 6, 30)
    assert C.sizeof(ya.IndelCallParams) == 32
