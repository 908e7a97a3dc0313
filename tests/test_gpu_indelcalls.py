"""GPU tier: indel calls with genotypes (-oindel) on the device (device/indelcall_stage.h: k_indel_norm left-normalises a raw allele per wave against the
image's reference and merges into a table, k_select_count / k_select_emit over IndelCallSel (device/select.h) judge every merged allele at its anchor
against the image's pileup array).  The direct cases run the directed set of tests/indelcall_sets.py on an index of the crafted genome, built here; the command-line cases run the variant read
set with planted indels on the golden genome.  Every comparison is with tests/indelcall_oracle.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import indel_oracle as io
import indelcall_oracle as ico
import indelcall_sets as S
import pileup_oracle as po
import yaha_amd as ya
from conftest import strip_pg

pytestmark = pytest.mark.gpu

KEYS = ["indel_calls", "indel_call_het", "indel_call_hom", "indel_call_on_device", "indel_call_raw", "indel_call_shifted", "indel_call_merged", "indel_call_skipped"]


# ---- direct: the directed set on the crafted index ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("craft"))
    g = S.Craft(); raw, tags = S.directed(g)
    open(os.path.join(d, "craft.fa"), "w").write(g.fasta())
    ya.build_index(["-g", os.path.join(d, "craft.fa"), "-L", "11"])
    reads = os.path.join(d, "one.fa"); open(reads, "w").write(">r0\n%s\n" % g.ref[200:500].replace("N", "A"))
    merged, st = ico.merge(raw, g.ref, g.sq, 256)
    return dict(g=g, raw=raw, tags=tags, index=os.path.join(d, "craft.X11_01_65525S"), reads=reads, merged=merged, st=st, rows=S.rows_for(g, merged, tags, raw))


def _entries(raw):
    return [ico.words(k) + (n,) for k, n in raw]


def _alleles(ctx):
    return [(io.entry_key(e.w0, e.w1, e.w2), e.count) for e in ctx.indelcall_alleles()]


def _params(err=50, min_alt=2, min_depth=4, min_qual=20):
    p = ya.IndelCallParams(); p.cost_match, p.cost_error, p.cost_het = ico.costs(err); p.min_alt, p.min_depth, p.min_qual = min_alt, min_depth, min_qual
    return p


def _rows(got):
    return [tuple(int(x) for x in r) for r in got.tolist()]


def _want(c, merged, **kw):
    return ico.records(ico.judged(merged, S.RowTable(c["rows"]), **kw), c["g"].ref)


def test_direct_normalise_merge_and_judge_on_the_directed_set(crafted):
    c = crafted; g, raw = c["g"], c["raw"]
    with ya.Session(["-x", c["index"], "-q", c["reads"], "-osh", "stdout", "-oindel", "unused.vcf"]) as s:
        sq = po.sq_table(s.header().split("\n")); assert sq == g.sq
        with ya.Context(s.index, s.params) as a:
            with pytest.raises(RuntimeError, match="ygpu_pileup_enable"):
                a.indelcall_normalize(_entries(raw))
            a.set_postfilter(s); a.pileup_enable(s)
            with pytest.raises(RuntimeError, match="ygpu_indelcall_normalize"):
                a.indel_calls(s)
            n, st = a.indelcall_normalize(_entries(raw))
            want = sorted(c["merged"].items(), key=lambda kv: io.order(kv[0]))
            assert st == c["st"] and n == len(want) and _alleles(a) == want
            assert len(a.indel_calls(s)) == 0                                     # an empty array: d = 0 everywhere, -inddp fails
            # the rows of the anchors folded into the empty array; then every record
            slots = sorted(c["rows"]); a.pileup_add(slots, [c["rows"][x] for x in slots])
            got = a.indel_calls(s)
            assert got.dtype.names == ya.INDEL_CALL_FIELDS and got.itemsize == 64
            w = _want(c, c["merged"])
            assert _rows(got) == w and 10 < len(w) < n
            # a second parameter set, one that keeps everything with a depth, then the first again; the alleles are still there
            for kw in (dict(err=100, min_alt=3, min_depth=6, min_qual=30), dict(min_alt=1, min_depth=1, min_qual=0), dict(min_alt=5), {}):
                assert _rows(a.indel_calls(_params(**kw))) == _want(c, c["merged"], **kw), kw
            assert len(_want(c, c["merged"], min_alt=1, min_depth=1, min_qual=0)) > len(w) > len(_want(c, c["merged"], min_alt=5))
            assert _alleles(a) == want
            with pytest.raises(RuntimeError, match="at least 1"):
                a.indel_calls(_params(min_depth=0))
            # every cap around the run of 64, none, and the largest: normalised again on the same context (the rows stay; other anchors are bare or shared)
            for shift in (0, 63, 64, 65, 1000, 65535):
                m2, st2 = ico.merge(raw, g.ref, g.sq, shift)
                n2, got_st = a.indelcall_normalize(_entries(raw), shift)
                assert got_st == st2 and _alleles(a) == sorted(m2.items(), key=lambda kv: io.order(kv[0])), shift
                assert _rows(a.indel_calls(_params(min_alt=1, min_depth=1, min_qual=0))) == _want(c, m2, min_alt=1, min_depth=1, min_qual=0), shift
            # inputs of 0, 1, 64 and 65 alleles (the list repeated to reach them: equal raw alleles merge)
            many = (raw * 2)[:65]
            for k in (0, 1, 64, 65):
                mk, stk = ico.merge(many[:k], g.ref, g.sq, 256)
                nk, got_st = a.indelcall_normalize(_entries(many[:k]))
                assert (nk, got_st) == (len(mk), stk) and _alleles(a) == sorted(mk.items(), key=lambda kv: io.order(kv[0])), k
                assert _rows(a.indel_calls(s)) == _want(c, mk), k
            # a sibling context of the image: the same array and reference, a table of its own; the first context's result stays
            a.indelcall_normalize(_entries(raw))
            with ya.Context(s.index, s.params, parent=a) as b:
                b.set_postfilter(s); b.pileup_enable(s)
                nb, stb = b.indelcall_normalize(_entries(raw[:30]))
                mb, wst = ico.merge(raw[:30], g.ref, g.sq, 256)
                assert stb == wst and _alleles(b) == sorted(mb.items(), key=lambda kv: io.order(kv[0]))
                assert _rows(b.indel_calls(s)) == _want(c, mb) and _rows(a.indel_calls(s)) == w


# ---- the command line ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reads(work, tmp_path_factory):
    fasta = po.read_fasta(os.path.join(work, "genome_small.fa"))
    text, planted = S.indel_reads(fasta)
    path = str(tmp_path_factory.mktemp("icreads") / "indels.fa")
    open(path, "w").write(text)
    return path, planted, fasta


def _cli(index11, reads, out, extra=(), env=None):
    p = subprocess.run([ya.CLI_PATH, "-x", index11, "-q", reads, "-osh", "stdout", "-oindel", out] + list(extra), env=dict(os.environ, YAHA_STATS="1", **(env or {})),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    assert "state check" not in err, err[-2000:]
    st = json.loads([l for l in err.split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])
    return p.stdout.decode(), open(out).read(), st


@pytest.fixture(scope="module")
def base_run(index11, reads, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("icbase") / "calls.vcf")
    sam, got, st = _cli(index11, reads[0], out)
    lines = sam.split("\n"); sq = po.sq_table(lines); ref = po.ref_letters(sq, reads[2]).tobytes().decode()
    pu = po.pileup(lines, sq, 0); pu.setflags(write=False); al = io.alleles(lines, sq, 0, 1)
    return dict(sam=sam, lines=lines, got=got, st=st, sq=sq, ref=ref, pu=pu, al=al, want=ico.text(al, pu, sq, ref))


def test_command_line_calls_are_made_on_the_device_and_equal_the_oracle(base_run):
    merged, mst = ico.merge(base_run["al"], base_run["ref"], base_run["sq"], 256)
    cl = ico.judged(merged, base_run["pu"])
    assert {(k[1], v["gt"]) for k, v in cl} == {(S.DEL, 1), (S.DEL, 2), (S.INS, 1), (S.INS, 2)} and len(cl) > 40 and mst["shifted"] > 20 and mst["merged"] > 0
    assert base_run["got"] == base_run["want"]
    st = base_run["st"]
    assert [k for k in st if k.startswith("indel")] == KEYS and st["indel_call_on_device"] == 1 and st["indel_calls"] == len(cl)
    assert (st["indel_call_raw"], st["indel_call_shifted"], st["indel_call_merged"], st["indel_call_skipped"]) == (mst["raw"], mst["shifted"], mst["merged"], mst["skipped"])


@pytest.mark.parametrize("extra", [["-ctx", "1", "-batch", "97"], ["-ctx", "2", "-batch", "211"], ["-ctx", "3", "-batch", "150"]], ids=["ctx1", "ctx2", "ctx3"])
def test_command_line_contexts_and_small_batches(index11, reads, base_run, tmp_path, extra):
    sam, got, st = _cli(index11, reads[0], str(tmp_path / "calls.vcf"), extra)
    assert strip_pg(sam) == strip_pg(base_run["sam"]) and got == base_run["want"] and st["indel_call_on_device"] == 1


def test_command_line_another_option_set_and_the_gate(index11, reads, base_run, tmp_path):
    sq, ref = base_run["sq"], base_run["ref"]
    sam, got, st = _cli(index11, reads[0], str(tmp_path / "calls.vcf"), ["-inderr", "100", "-indmin", "3", "-inddp", "6", "-indqual", "30", "-indshift", "3", "-puq", "10"])
    lines = sam.split("\n")
    want2 = ico.text(io.alleles(lines, sq, 10, 1), po.pileup(lines, sq, 10), sq, ref, err=100, min_alt=3, min_depth=6, min_qual=30, shift=3, Q=10)
    assert got == want2 and want2 != base_run["want"] and st["indel_call_on_device"] == 1


def test_command_line_folds_the_hosts_share_and_the_host_routine(index11, reads, base_run, tmp_path):
    out = str(tmp_path / "calls.vcf")
    # reads of more than three clumps come back unfiltered: the host counts them, and its rows are folded into the image's array before the selection
    sam, got, st = _cli(index11, reads[0], out, ["-batch", "300"], env={"YGPU_OQC_MAX": "3"})
    assert strip_pg(sam) == strip_pg(base_run["sam"]) and got == base_run["want"] and st["indel_call_on_device"] == 1
    sam, got, st = _cli(index11, reads[0], out, ["-batch", "300"], env={"YAHA_HOST_INDELCALL": "1"})
    assert got == base_run["want"] and st["indel_call_on_device"] == 0 and st["indel_calls"] == base_run["st"]["indel_calls"]


def test_command_line_folds_the_other_image_and_shares_with_the_snv_calls(index11, reads, base_run, tmp_path):
    out = str(tmp_path / "calls.vcf"); snv = str(tmp_path / "snv.vcf")
    # two index images (the same device twice): the second image's rows at the anchors are folded into the first
    sam, got, st = _cli(index11, reads[0], out, ["-gpus", "2", "-ctx", "2", "-batch", "150"], env={"YAHA_DEVICES": "0,0"})
    assert strip_pg(sam) == strip_pg(base_run["sam"]) and got == base_run["want"]
    assert st["indel_call_on_device"] == 1 and all(n > 0 for n in st["reads_per_device"]), st
    # beside -osnv: both files equal their own runs', nothing is folded twice (a row added twice would change depths and with them the lines)
    p = subprocess.run([ya.CLI_PATH, "-x", index11, "-q", reads[0], "-osh", "stdout", "-osnv", snv, "-gpus", "2", "-ctx", "2", "-batch", "150"],
                       env=dict(os.environ, YAHA_STATS="1", YAHA_DEVICES="0,0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    snv_alone = open(snv).read(); os.remove(snv)
    snv_st = json.loads([l for l in p.stderr.decode().split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])
    for extra, env in ((["-gpus", "2", "-ctx", "2", "-batch", "150"], {"YAHA_DEVICES": "0,0"}), (["-batch", "300"], {"YGPU_OQC_MAX": "3"})):
        sam, got, st = _cli(index11, reads[0], out, ["-osnv", snv] + extra, env=env)
        assert got == base_run["want"] and open(snv).read() == snv_alone and st["indel_call_on_device"] == 1 and st["snv_on_device"] == 1
        if "-gpus" in extra:
            assert st["snv_folded_slots"] == snv_st["snv_folded_slots"] > 0
