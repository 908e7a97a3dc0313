"""GPU tier: the post-filter stage on the device (device/oqc_stage.h: k_oqc_classify, k_oqc_wave, k_oqc_raw, k_oqc_gather behind ygpu_postfilter) against the plain
model of tests/oqc_model.py, read by read and field by field, on the directed clump lists of tests/oqc_sets.py injected with ygpu_inject_results: every read class and
class edge, first partitions of 63 .. 129 scanned elements, all keys equal and no two equal, ties on both sides of a 64-chunk's end, the sort's stack running over into
HBM, duplicate scans that end at a block's last lane, at the next block's first and two blocks on, tables in both pools, survivors at and beyond what the LDS holds,
more than 64 primaries in LDS and in HBM -- under the filter's parameter sets.  Before anything is compared the model's Coverage must say that the batch reaches the
edges it was built for (tests/test_oqc_model.py shows each of them reachable, and model == oqc_core.h on these very lists, on the CPU tier).  Every batch runs twice on
one context (the work arrays are reused) and once on a clone.  Nothing here reads SAM text.

Not repeated here: ygpu_selftest_primitives (test_own_sums_and_orderings in test_gpu_parity.py) already runs waveSort alone through k_oqc_sort_test -- arrays of
2 .. 1 792 entries with ties, an LDS stack of only eight ints, so that the HBM part of the stack is used by ordinary inputs -- against oqc_core.h's sortRange."""
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import oqc_model as om
import oqc_sets as sets
import yaha_amd as ya
from conftest import ROOT

pytestmark = pytest.mark.gpu

OUT_CLUMP = np.dtype([("sro", "<u4"), ("sqo", "<u2"), ("eqo", "<u2"), ("refLen", "<u2"), ("totScore", "<u2"), ("totLength", "<u2"), ("matched", "<u2"), ("mismatched", "<u2"),
                      ("gap", "<u2"), ("cstatus", "u1"), ("reserved", "u1"), ("pad", "<u2"), ("op_start", "<u4"), ("n_ops", "<u4"),
                      ("status", "u1"), ("mapQuality", "u1"), ("numSecondaries", "<u2"), ("matchedPrimary", "<u2"), ("primaryCount", "<u2")])
assert OUT_CLUMP.itemsize == C.sizeof(ya.OutClump) == 40


def expected_reads(runs, dev_max=om.YQ_DEVICE_MAX):
    """per read, what the filtered batch must hold: (sro, sqo, eqo, strand, status, mapQuality, numSecondaries, matchedPrimary, primaryCount, ops) per printed clump"""
    out = []
    for _label, _codes, cl, m in runs:
        if len(cl) > dev_max:                                          # handed back unfiltered: marked, all clumps in the hot path's order
            out.append([(c.sro, c.sqo, c.eqo, c.status & 1, c.status, 255, 0, 0, 0xFFFF, c.ops) for c in cl])
        else:
            out.append([(cl[o.clump].sro, cl[o.clump].sqo, cl[o.clump].eqo, cl[o.clump].status & 1, o.status, o.mapQuality, o.numSecondaries, o.matchedPrimary, m.primary_count,
                         cl[o.clump].ops) for o in m.out])
    return out


def device_reads(ctx, n_reads):
    """the filtered batch ctx.postfilter() just collected, per read, in the shape of expected_reads"""
    cs = np.frombuffer(ctx._f_cs, dtype=np.uint32); cl = np.frombuffer(ctx._f_cl, dtype=OUT_CLUMP); ops = np.frombuffer(ctx._f_ops, dtype=np.uint32)
    out = []
    for i in range(n_reads):
        mine = []
        for k in range(int(cs[i]), int(cs[i + 1])):
            c = cl[k]; o = ops[int(c["op_start"]):int(c["op_start"]) + int(c["n_ops"])]
            mine.append((int(c["sro"]), int(c["sqo"]), int(c["eqo"]), int(c["cstatus"]) & 1, int(c["status"]), int(c["mapQuality"]), int(c["numSecondaries"]), int(c["matchedPrimary"]),
                         int(c["primaryCount"]), tuple((int(x) & 0xFFFF, chr((int(x) >> 16) & 0xFF)) for x in o)))
        out.append(mine)
    return out


def run_and_compare(s, b, runs, exp, what):
    """the batch twice on one context and once on a clone of it, in this process; every read equal to the model"""
    lists = [cl for _l, _c, cl, _m in runs]
    r, _keep = sets.as_result(lists)
    took = []

    def once(ctx, tag):
        ctx.upload(b); ctx.inject_results(r)
        t0 = time.perf_counter(); f = ctx.postfilter(); took.append(time.perf_counter() - t0)
        assert f.n_reads == len(runs)
        got = device_reads(ctx, len(runs))
        for i, (label, _codes, cl, m) in enumerate(runs):
            assert got[i] == exp[i], "%s, %s: read %d (%s, %d clumps) differs from the model\n device %s\n model  %s\n sorted order %s\n survivors %s\n best predecessors %s" % (
                what, tag, i, label, len(cl), got[i][:6], exp[i][:6], m.sorted_order[:48], m.survivors[:48], getattr(m, "best_prev", [])[:48])
    with ya.Context(s.index, s.params) as ctx:
        ctx.set_postfilter(s)
        once(ctx, "first run"); once(ctx, "second run on the same context")
        clone = ya.Context(s.index, s.params, parent=ctx)
        try:
            clone.set_postfilter(s)
            once(clone, "cloned context")
        finally:
            clone.close()
    print("%s: ygpu_postfilter %s ms" % (what, ", ".join("%.1f" % (1e3 * t) for t in took)))


def modelled(s, b, reads):
    P, seqs = sets.session_inputs(s)
    codes = sets.batch_codes(b)
    return [(label, codes[i], cl, om.run_read(P, seqs, codes[i], len(codes[i]), cl)) for i, (label, cl) in enumerate(reads)]


def check(ok, what):
    assert ok, "the batch does not reach what it was built for: " + what


def check_coverage_of_the_directed_batch(runs, pset, hbm):
    cov = {label: om.Coverage(m, cl, hbm=hbm) for label, _c, cl, m in runs}
    for n, cls in ((0, "settled_by_classify"), (1, "settled_by_classify"), (2, 0), (112, 0), (113, 1), (224, 1), (225, 2), (448, 2), (449, 3)):
        check(cov["class_edge_%d" % n].n == n and cov["class_edge_%d" % n].cls == cls, "%d clumps in class %s" % (n, cls))
    dev = [c for c in cov.values() if isinstance(c.cls, int)]
    check(all(c.sort_on_wave for c in dev), "every read sorts on the wave")
    first = {max(p["m"] for p in c.partitions) for c in dev if c.partitions}
    check({63, 64, 65, 127, 128, 129} <= first, "first partitions of 63, 64, 65, 127, 128 and 129 scanned elements")
    parts = [p for c in dev for p in c.partitions]
    check(any(p["m"] == 63 and p["ties"] == 63 for p in parts) and any(p["m"] == 64 and p["ties"] == 64 for p in parts), "all keys equal on either side of the register path's limit")
    check(any(p["m"] >= 64 and p["ties"] == 0 for p in parts), "a long partition without ties")
    big = max(cov["straddle_130"].partitions, key=lambda p: p["m"])
    check(big["ties"] == 9 and big["tie_chunks"] == 2, "ties on both sides of the first 64-chunk's end")
    for lo, hi in ((1, 63), (64, 10 ** 6)):
        check(any(lo <= p["m"] <= hi and p["nL"] == 0 for p in parts) and any(lo <= p["m"] <= hi and p["nL"] == p["m"] for p in parts), "nL == 0 and nL == m, partitions of %d .. %d" % (lo, hi))
    ends = sum((c.scan_ends for c in dev), om.Counter())
    for k in ("own_block", "next_block", "two_or_more_blocks_on", "list_end", "at_lane_63", "at_lane_0_of_the_next_block"):
        check(ends[k] > 0, "a duplicate scan that ends: " + k)
    ev = sum((c.events for c in cov.values()), om.Counter())
    for k in ("dup_kill_score8_in_block", "dup_kill_score8_out_of_block", "dup_kill_same_place_in_block", "dup_kill_same_place_out_of_block", "dup_dead_at_its_turn",
              "relax_better", "relax_lost_before_penalty", "overlap_right_best", "overlap_path_best", "overlap_walk_through_several_nodes", "bpp_near", "bpp_at_a_step",
              "bpp_one_below_a_step", "bpp_one_above_a_step", "bpp_other_sequence", "startj_first_far_in_later_chunk", "startj_none_far", "startj_at_cnt", "primaries_1", "primaries_2",
              "second_score_updated", "third_score_updated", "mq_no_second", "mq_both", "node_overlaps_no_primary", "reversed_clump"):
        check(ev[k] > 0, "event " + k)
    check(cov["duplicates_70"].events["dup_kill_same_place_in_block"] + cov["duplicates_70"].events["dup_kill_same_place_out_of_block"] == 69, "70 exact duplicates")
    t = cov["tables_overrun_112"]
    if hbm:
        check(not any(c.graph_in_lds for c in dev), "YGPU_OQC_HBM: every graph in HBM")
    else:
        check(t.cls == 0 and t.cnt == 112 and t.tables_lds > 0 and t.tables_hbm > 0, "class 0, 112 survivors, tables in both pools")
    if pset == "mno1":
        a, c = cov["primaries_70_in_hbm"], cov["primaries_70_in_lds"]
        check(a.events["primaries_more_than_64"] == 1 and not a.primaries_in_lds and a.graph_in_lds, "more than 64 primaries that do not fit behind the nodes")
        check(c.events["primaries_more_than_64"] == 1 and c.primaries_in_lds, "more than 64 primaries behind the nodes")
    if pset.startswith("fbs") or pset == "mno1":
        check(ev["secondary_pushed"] > 0 and ev["secondary_failed_with_FBS_on"] > 0, "secondaries pushed and not pushed with FBS on")
    else:
        check(ev["secondary_counted_not_pushed"] > 0, "secondaries counted but not printed")


@pytest.mark.parametrize("pset,hbm", [(p, False) for p in sorted(sets.PARAM_SETS)] + [("defaults", True)])
def test_directed_batch_equals_the_model(work, index11, pset, hbm, monkeypatch):
    """48 directed reads under one parameter set; (defaults, True): the same lists with every read's nodes and tables in HBM (YGPU_OQC_HBM=1) -- the same records."""
    if hbm:
        monkeypatch.setenv("YGPU_OQC_HBM", "1")
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa")] + sets.PARAM_SETS[pset]) as s:
        P, seqs = sets.session_inputs(s)
        b = s.next_batch(48)
        qlens = [len(c) for c in sets.batch_codes(b)]
        runs = modelled(s, b, sets.edges(qlens, seqs, P))
        check_coverage_of_the_directed_batch(runs, pset, hbm)
        run_and_compare(s, b, runs, expected_reads(runs), "directed batch, %s%s" % (pset, ", graph in HBM" if hbm else ""))


def test_large_reads_equal_the_model(work, index11):
    """The reads only size reaches, in a function of their own: 1 792 clumps in the anti-quicksort order, 1 793 (handed back), 1 349 and 1 400 survivors, 500 equal keys."""
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa")]) as s:
        _P, seqs = sets.session_inputs(s)
        b = s.next_batch(6)
        qlens = [len(c) for c in sets.batch_codes(b)]
        runs = modelled(s, b, sets.large(qlens, seqs))
        cov = {label: om.Coverage(m, cl) for label, _c, cl, m in runs}
        check(cov["adversarial_1792"].cls == 3 and cov["adversarial_1792"].max_waiting > om.YQ_STACK_LDS // 2 and cov["adversarial_1792"].stack_spills, "the sort's stack runs over its LDS")
        check(cov["handed_back_1793"].cls == "host", "1 793 clumps are handed back")
        check(cov["survivors_1349"].cnt == 1349 and cov["survivors_1349"].graph_at_lds_limit and cov["survivors_1349"].tables_lds == 0, "1 349 survivors: the last count in LDS")
        check(cov["survivors_1400"].cnt > 1349 and not cov["survivors_1400"].graph_in_lds, "more than 1 349 survivors: oqcGraph<false> without the hook")
        check(any(p["ties"] >= 400 and p["tie_chunks"] >= 7 for p in cov["family_500"].partitions), "hundreds of ties in one partition")
        check(cov["class_edge_1792"].n == 1792 and cov["class_edge_1792"].cls == 3, "1 792 clumps in class 3")
        run_and_compare(s, b, runs, expected_reads(runs), "large reads")


@pytest.mark.parametrize("dev_max", [None, 4])
def test_classes_of_many_small_reads(work, index11, dev_max, monkeypatch):
    """130 reads of 0 .. 5 clumps and three larger ones: k_oqc_classify settles the reads of no and of one clump itself and its ballots make lists of 1, 2 and more than 64
    reads across wave boundaries; with YGPU_OQC_MAX=4 reads of four clumps are filtered and reads of five handed back."""
    if dev_max:
        monkeypatch.setenv("YGPU_OQC_MAX", str(dev_max))
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa")]) as s:
        _P, seqs = sets.session_inputs(s)
        b = s.next_batch(130)
        assert b.n_reads == 130
        qlens = [len(c) for c in sets.batch_codes(b)]
        runs = modelled(s, b, sets.tiny_batch(qlens, seqs))
        cls = om.Counter(om.Coverage(m, cl, dev_max=dev_max or om.YQ_DEVICE_MAX).cls for _l, _c, cl, m in runs)
        if dev_max:
            check(cls[0] > 64 and cls["host"] >= 16 and cls["settled_by_classify"] > 16, "lists under YGPU_OQC_MAX=4: %s" % dict(cls))
        else:
            check(cls[0] > 64 and cls[1] == 1 and cls[2] == 2 and cls["settled_by_classify"] > 16, "lists of 1, 2 and more than 64 reads: %s" % dict(cls))
        run_and_compare(s, b, runs, expected_reads(runs, dev_max or om.YQ_DEVICE_MAX), "small reads%s" % (", YGPU_OQC_MAX=4" if dev_max else ""))


# What the records cannot show: WHICH class k_oqc_classify put a read in (a read in a larger class than its own is filtered all the same, in more LDS).  The stage says
# it itself, in the line it prints under YGPU_TRACE -- a switch the library reads once, when it is loaded, so the batches run in a fresh process.
CLASSES_CHILD = """
import os, sys
sys.path[:0] = sys.argv[1:3]
import oqc_sets as sets, yaha_amd as ya
work, index11 = sys.argv[3:5]
with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa")]) as s:
    P, seqs = sets.session_inputs(s)
    b = s.next_batch(130)
    qlens = [len(c) for c in sets.batch_codes(b)]
    batches = {"tiny": [cl for _l, cl in sets.tiny_batch(qlens, seqs)], "edges": [cl for _l, cl in sets.edges(qlens, seqs, P)] + [[]] * 82}
    with ya.Context(s.index, s.params) as ctx:
        ctx.set_postfilter(s)
        for name, dev_max in (("tiny", ""), ("tiny", "4"), ("edges", "")):
            os.environ["YGPU_OQC_MAX"] = dev_max or "1792"
            r, _keep = sets.as_result(batches[name])
            ctx.upload(b); ctx.inject_results(r)
            assert ctx.postfilter().n_reads == 130
"""
CLASS_LINE = re.compile(r"post-filter: (\d+) reads with two or more clumps in classes of <= 112 / 224 / 448 / 1792 clumps: (\d+) / (\d+) / (\d+) / (\d+), left to the host (\d+)")


def test_the_device_puts_every_read_in_its_class(work, index11):
    """The per-class counts the stage prints for the small-reads batch, the same under YGPU_OQC_MAX=4, and the directed batch (reads of exactly 2, 112, 113, 224, 225, 448
    and 449 clumps among its 48) == the counts of the model's device_class over the same lists: a capacity one off moves a read of 112, 224 or 448 clumps, or one of
    113, 225 or 449, to the neighbouring class and shows here, where every record would still be right."""
    env = dict(os.environ, YGPU_TRACE="1")
    p = subprocess.run([sys.executable, "-c", CLASSES_CHILD, ROOT, os.path.join(ROOT, "tests"), work, index11], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-3000:]
    got = [tuple(int(x) for x in m.groups()) for m in CLASS_LINE.finditer(err)]
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa")]) as s:
        P, seqs = sets.session_inputs(s)
        qlens = [len(c) for c in sets.batch_codes(s.next_batch(130))]
    tiny = [len(cl) for _l, cl in sets.tiny_batch(qlens, seqs)]; edges = [len(cl) for _l, cl in sets.edges(qlens, seqs, P)]
    for n in (2, 112, 113, 224, 225, 448, 449):
        check(n in edges, "a read of %d clumps in the directed batch" % n)
    exp = []
    for sizes, dev_max in ((tiny, om.YQ_DEVICE_MAX), (tiny, 4), (edges, om.YQ_DEVICE_MAX)):
        c = om.Counter(om.device_class(n, dev_max) for n in sizes)
        exp.append((c[0] + c[1] + c[2] + c[3] + c["host"], c[0], c[1], c[2], c[3], c["host"]))
    check(exp[1][5] >= 16 and exp[0][2] == 1 and exp[0][3] == 2 and exp[2][1] > 0 and exp[2][2] > 0 and exp[2][3] > 0 and exp[2][4] > 0, "reads in every class: %s" % exp)
    assert got == exp, "classes on the device %s, by the model %s" % (got, exp)
