"""GPU tier: SNV calls with genotypes (-osnv) judged on the device from the pileup array (device/snv_stage.h: k_pileup_add folds the other sources into one
image's array, k_select_count / k_select_emit over SnvSel (device/select.h) select and judge -- a wave per tile of 2 048 slots, the records written by
ballot and population count).  Every comparison is with tests/snv_oracle.py over tests/pileup_oracle.py, which recompute the calls from SAM text and the reference FASTA alone, or -- the direct
cases -- from the very rows the test folds into an empty array.  The reads of the command-line cases are the variant set snv_oracle.variant_reads makes."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import pileup_oracle as po
import snv_oracle as so
import yaha_amd as ya
from conftest import strip_pg

pytestmark = pytest.mark.gpu

SNV_KEYS = ["snv_calls", "snv_het", "snv_hom", "snv_on_device", "snv_folded_slots"]


@pytest.fixture(scope="module")
def variants(work, tmp_path_factory):
    fasta = po.read_fasta(os.path.join(work, "genome_small.fa"))
    text, planted = so.variant_reads(fasta)
    path = str(tmp_path_factory.mktemp("snvreads") / "variants.fa")
    open(path, "w").write(text)
    return path, planted, fasta


def _cli(index11, reads, out, extra=(), env=None):
    p = subprocess.run([ya.CLI_PATH, "-x", index11, "-q", reads, "-osh", "stdout", "-osnv", out] + list(extra), env=dict(os.environ, YAHA_STATS="1", **(env or {})),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    assert "state check" not in err, err[-2000:]
    st = json.loads([l for l in err.split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])
    return p.stdout.decode(), open(out).read(), st


@pytest.fixture(scope="module")
def base_run(index11, variants, tmp_path_factory):
    """The default run, the oracle's pileup of its SAM text and the file that follows from it -- made once, shared, never written to."""
    out = str(tmp_path_factory.mktemp("snvbase") / "calls.vcf")
    sam, got, st = _cli(index11, variants[0], out)
    lines = sam.split("\n"); sq = po.sq_table(lines); ref = po.ref_letters(sq, variants[2])
    pu = po.pileup(lines, sq, 0); pu.setflags(write=False)
    return dict(sam=sam, got=got, st=st, sq=sq, ref=ref, pu=pu, want=so.text(pu, sq, ref))


def test_command_line_calls_are_judged_on_the_device_and_equal_the_oracle(index11, variants, base_run, tmp_path):
    pu, ref, sq = base_run["pu"], base_run["ref"], base_run["sq"]
    # what the comparison stands on, asserted on the oracle's result over the run's own SAM text
    cl = so.calls(pu, ref)
    assert sum(v["gt"] == 1 for _s, v in cl) >= 20 and sum(v["gt"] == 2 for _s, v in cl) >= 20 and {chr(ref[s]) for s, _v in cl} == set("ACGT")
    assert so.calls(pu, ref, keep=lambda v: v["gt"] != 0 and v["a"] >= 2 and v["depth"] >= 4 and v["qual"] < 20)
    assert base_run["got"] == base_run["want"]
    st = base_run["st"]
    assert st["snv_on_device"] == 1 and st["snv_calls"] == len(cl) and st["snv_het"] == sum(v["gt"] == 1 for _s, v in cl) and st["snv_folded_slots"] == 0
    assert [k for k in st if "snv" in k] == SNV_KEYS and not [k for k in st if "pileup" in k]


@pytest.mark.parametrize("extra", [["-ctx", "1", "-batch", "97"], ["-ctx", "2", "-batch", "211"], ["-ctx", "3", "-batch", "150"]], ids=["ctx1", "ctx2", "ctx3"])
def test_command_line_contexts_and_small_batches(index11, variants, base_run, tmp_path, extra):
    sam, got, st = _cli(index11, variants[0], str(tmp_path / "calls.vcf"), extra)
    assert strip_pg(sam) == strip_pg(base_run["sam"]) and got == base_run["want"]
    assert st["snv_on_device"] == 1 and st["snv_calls"] == base_run["st"]["snv_calls"] > 40, st


def test_command_line_another_option_set_and_the_gate(index11, variants, base_run, tmp_path):
    sq, ref = base_run["sq"], base_run["ref"]
    sam, got, st = _cli(index11, variants[0], str(tmp_path / "calls.vcf"), ["-snverr", "50", "-snvmin", "3", "-snvdp", "6", "-snvqual", "30", "-puq", "10"])
    want2 = so.text(po.pileup(sam.split("\n"), sq, 10), sq, ref, err=50, min_alt=3, min_depth=6, min_qual=30, Q=10)
    assert got == want2 and want2 != base_run["want"] and st["snv_on_device"] == 1


def test_command_line_folds_the_hosts_share(index11, variants, base_run, tmp_path):
    out = str(tmp_path / "calls.vcf"); n_calls = base_run["st"]["snv_calls"]
    # reads of more than three clumps come back unfiltered: the host counts them, and its slots are folded into the image's array before the selection
    sam, got, st = _cli(index11, variants[0], out, ["-batch", "300"], env={"YGPU_OQC_MAX": "3"})
    assert strip_pg(sam) == strip_pg(base_run["sam"]) and got == base_run["want"]
    assert st["snv_folded_slots"] > 0 and st["snv_on_device"] == 1 and st["snv_calls"] == n_calls, st
    # the host's routine by switch
    sam, got, st = _cli(index11, variants[0], out, ["-batch", "300"], env={"YAHA_HOST_SNV": "1"})
    assert got == base_run["want"] and st["snv_on_device"] == 0 and st["snv_calls"] == n_calls


def test_command_line_folds_the_other_image(index11, variants, base_run, tmp_path):
    out = str(tmp_path / "calls.vcf")
    # two index images (the same device twice): the second image's rows at the union of the candidates are folded into the first
    sam, got, st = _cli(index11, variants[0], out, ["-gpus", "2", "-ctx", "2", "-batch", "150"], env={"YAHA_DEVICES": "0,0"})
    assert strip_pg(sam) == strip_pg(base_run["sam"]) and got == base_run["want"]
    assert st["snv_folded_slots"] > 0 and st["snv_on_device"] == 1 and all(n > 0 for n in st["reads_per_device"]), st
    # beside -opu: one array, the pileup's table as from its own run, written before the fold
    pu_file = str(tmp_path / "pu.tsv")
    sam, got, st = _cli(index11, variants[0], out, ["-opu", pu_file, "-pumin", "3", "-gpus", "2", "-ctx", "1", "-batch", "300"], env={"YAHA_DEVICES": "0,0"})
    assert got == base_run["want"] and open(pu_file).read() == po.text(base_run["pu"], base_run["sq"], base_run["ref"], 3)
    assert st["snv_on_device"] == 1 and st["pileup_host_records"] == 0 and [k for k in st if "snv" in k or "pileup" in k][-5:] == SNV_KEYS


def _params(err=100, min_alt=2, min_depth=4, min_qual=20):
    p = ya.SnvParams(); p.cost_match, p.cost_error, p.cost_het = so.costs(err); p.min_alt, p.min_depth, p.min_qual = min_alt, min_depth, min_qual
    return p


def _want(model, ref, **kw):
    return so.records(so.calls(model, ref, **kw), ref)


def _rows(got):
    return [tuple(int(x) for x in r) for r in got.tolist()]


def test_direct_folds_into_an_empty_array_and_the_selection(work, index11):
    """Rows folded with pileup_add into an enabled, empty array; the result is the oracle's list, record for record."""
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa"), "-osh", "stdout", "-osnv", "unused.vcf"]) as s:
        sq = po.sq_table(s.header().split("\n")); ref = po.ref_letters(sq, po.read_fasta(os.path.join(work, "genome_small.fa")))
        n = po.n_slots(sq); assert n % 64 != 0 and n > 3 * 2048 and len(sq) >= 2
        L = "ACGT"; ch = lambda c: L.index(c)
        is_base = np.isin(ref, np.frombuffer(b"ACGT", dtype=np.uint8))
        model = np.zeros((n, 7), dtype=np.uint32)

        def hom(slot, depth=10):
            """A row that calls 1/1 at a slot whose reference is a base: `depth` reads of the next base."""
            assert is_base[slot], slot
            r = [0] * 7; r[(ch(chr(ref[slot])) + 1) % 4] = depth
            return r

        def fold(ctx, slots, rows):
            ctx.pileup_add(slots, rows)
            for sl, r in zip(slots, rows):
                if sl < n:
                    model[sl] += np.array(r, dtype=np.uint32)

        with ya.Context(s.index, s.params) as a:
            with pytest.raises(RuntimeError, match="ygpu_pileup_enable"):
                a.snv_calls(s)
            with pytest.raises(RuntimeError, match="ygpu_pileup_enable"):
                a.pileup_add([0], [[0] * 7])
            a.set_postfilter(s); a.pileup_enable(s)
            assert len(a.snv_calls(s)) == 0                                                        # an empty array has no calls
            with pytest.raises(RuntimeError, match="at least 1"):
                a.snv_calls(_params(min_alt=0))
            # the edges of waves, rows and tiles, the last slot; tile 2 (slots 4096 .. 6143) stays empty between tiles with calls
            edge = [0, 63, 64, 2047, 2048, 2049, 6144, n - 1]
            first2 = sq[0][1]                                                                      # the first slot of the second sequence; first2 - 1: the last of the first
            edge += [first2 - 1, first2]
            assert all(is_base[e] for e in edge)
            fold(a, edge, [hom(e) for e in edge])
            # a row of a tile where all 64 lanes call (tile 5, its third row)
            full = list(range(5 * 2048 + 128, 5 * 2048 + 192)); assert is_base[full].all()
            fold(a, full, [hom(e, 7 + e % 5) for e in full])
            # alt ties: two and three other channels with the same count -- the lowest channel is the alt
            tie = []
            for k, c in enumerate("ACGT"):
                at = np.nonzero(ref[20000 + 700 * k:] == ord(c))[0][:2] + 20000 + 700 * k; others = [x for x in range(4) if x != ch(c)]
                r1 = [0, 0, 0, 0, 1, 2, 3]; r1[ch(c)] = 1
                for x in others:
                    r1[x] = 6                                                                      # three ways: the lowest of the three
                r2 = [0] * 7; r2[others[0]] = 4; r2[others[1]] = r2[others[2]] = 5                  # two ways, the lowest other channel below them: the middle one
                tie += [(int(at[0]), r1), (int(at[1]), r2)]
            assert len({x for x, _ in tie}) == 8
            fold(a, [x for x, _ in tie], [r for _, r in tie])
            # a reference N: never a call, whatever the reads say
            nslot = int(np.nonzero(ref == ord("N"))[0][5])
            fold(a, [nslot, nslot + 1], [[9, 0, 0, 0, 0, 0, 0], [0, 9, 0, 0, 0, 0, 0]])
            # each threshold at its value and one below (defaults 2, 4, 20): alt reads 2 / 1, depth 4 / 3, QUAL 20 / 19 and thereabouts
            th = [s0 for s0 in range(40000, 40400) if is_base[s0]][:12]
            def ra(slot, r, a_, extra=0):
                row = [0] * 7; c = ch(chr(ref[slot])); row[c] = r; row[(c + 1) % 4] = a_; row[(c + 2) % 4] = extra
                return row
            thr_rows = [ra(th[0], 2, 2), ra(th[1], 3, 1), ra(th[2], 0, 2, 2), ra(th[3], 0, 2, 1), ra(th[4], 0, 3), ra(th[5], 0, 4), ra(th[6], 6, 3), ra(th[7], 5, 3),
                        ra(th[8], 122, 32), ra(th[9], 121, 32), ra(th[10], 1, 2, 1), ra(th[11], 0, 1, 3)]
            fold(a, th, thr_rows)
            # a list with a repeated slot (the rows add up to a call, neither is one alone) and slots past the array
            rep = 50001 + int(np.nonzero(is_base[50001:])[0][0])
            fold(a, [rep, n, rep, n + 5, 0xFFFFFFFF, rep], [ra(rep, 1, 1), hom(0), ra(rep, 1, 1), hom(0), hom(0), ra(rep, 0, 1)])
            want = _want(model, ref)
            got = a.snv_calls(s)
            assert got.dtype.names == ya.SNV_CALL_FIELDS and got.itemsize == 48
            assert _rows(got) == want
            slots = [w[0] for w in want]
            assert all(e in slots for e in edge + full + [rep]) and nslot not in slots and nslot + 1 not in slots
            assert not any(4096 <= x < 6144 for x in slots) and slots == sorted(slots)
            assert 0 < sum(x in slots for x in th) < len(th)
            # both sides of every threshold are in the model: every slot of `th` is a genotype other than 0/0 or fails exactly one test
            by = dict(so.calls(model, ref, keep=lambda v: True))
            assert {(by[x]["a"] >= 2, by[x]["depth"] >= 4, by[x]["qual"] >= 20) for x in th if by[x]["gt"] != 0} >= {(True, True, True), (True, False, True), (True, True, False)}
            assert by[th[7]]["qual"] == 20 and by[th[8]]["qual"] == 19 and by[th[0]]["depth"] == 4 and by[th[3]]["depth"] == 3 and by[th[2]]["a"] == 2
            # (with the default costs a slot with one alt read never reaches QUAL 20: -snvmin at its value and one below is the set of parameters below)
            w4 = [w[0] for w in _want(model, ref, min_alt=4, min_depth=1, min_qual=0)]
            assert th[5] in w4 and th[4] not in w4 and _rows(a.snv_calls(_params(min_alt=4, min_depth=1, min_qual=0))) == _want(model, ref, min_alt=4, min_depth=1, min_qual=0)
            # the array itself is what the model says
            arr, _st = a.pileup_collect()
            assert np.array_equal(arr, model)
            # a second selection with other parameters on the same array, then the first again
            for kw in (dict(err=50, min_alt=3, min_depth=6, min_qual=30), dict(min_alt=1, min_depth=1, min_qual=0), dict(err=300, min_alt=2, min_depth=4, min_qual=0), {}):
                got = a.snv_calls(_params(**kw)); w = _want(model, ref, **kw)
                assert _rows(got) == w and len(w) > 0, kw
            assert len(_want(model, ref, min_alt=1, min_depth=1, min_qual=0)) > len(want) > len(_want(model, ref, err=50, min_alt=3, min_depth=6, min_qual=30))
            # a sibling context of the image: the same array; parked, it still answers, and so does the first while the sibling is parked
            with ya.Context(s.index, s.params, parent=a) as b:
                b.set_postfilter(s); b.pileup_enable(s)
                assert _rows(b.snv_calls(s)) == want
                b.park()
                assert _rows(b.snv_calls(s)) == want and _rows(a.snv_calls(s)) == want
                extra = [th[0] + 1000 + int(np.nonzero(is_base[th[0] + 1000:])[0][0])]
                fold(b, extra, [hom(extra[0])])                                                    # a fold through the parked sibling
                want = _want(model, ref)
                assert extra[0] in [w[0] for w in want] and _rows(b.snv_calls(s)) == want and _rows(a.snv_calls(s)) == want
