"""CPU tier: the post-filter of one read, csrc/oqc_core.h (yoqc::run, the routine the host compiles and the device stage takes its steps from), against the plain
model of tests/oqc_model.py -- stated from the reference's GraphPath.cpp, not from the header -- on the directed inputs of tests/oqc_sets.py (the very lists
tests/test_gpu_oqc_edges.py injects on the device), on the random lists of test_postfilter_on_synthetic_clump_lists, and on real reads whose SAM the goldens pin
to the reference.  The header runs in tests/fixtures/oqc_driver.cpp under AddressSanitizer and UBSan with every scratch array at the size the header promises.
The last test is the condition of the GPU tier: every device edge the directed inputs are built for is shown reachable here, with the model alone."""
import functools
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import oqc_model as om
import oqc_sets as sets
from conftest import ROOT


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("oqc")), "oqc_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "fixtures", "oqc_driver.cpp")])
    return exe


def drive(exe, P, seqs, reads):
    """reads: (codes, clumps) each -> [(out records, primaryCount)] of oqc_core.h's run()"""
    t = ["%d %d %d %d %d %d %d %d %d %d" % (P.GOCost, P.GECost, P.RCost, P.MScore, P.minNonOverlap, P.BPCost, P.maxBPLog, P.FBS, int(np.float32(P.PSLength).view(np.uint32)),
                                            int(np.float32(P.PSScore).view(np.uint32))), str(len(seqs))]
    t += ["%d %d" % s for s in seqs] + [str(len(reads))]
    for codes, clumps in reads:
        t.append("%d %d %s" % (len(codes), len(clumps), "".join("%x" % (c & 15) for c in codes) or "-"))
        for c in clumps:
            t.append("%d %d %d %d %d %d %d %d %s" % (c.sro, c.sqo, c.eqo, c.refLen, c.totScore, c.totLength, c.status, len(c.ops), " ".join("%s %d" % (k, l) for l, k in c.ops)))
    p = subprocess.run([exe], input="\n".join(t).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines, out, k = p.stdout.decode().split("\n"), [], 0
    for _ in reads:
        tag, pc, m = lines[k].split(); assert tag == "read"
        recs = [om.Out(*map(int, lines[k + 1 + j].split())) for j in range(int(m))]
        out.append((recs, int(pc))); k += 1 + int(m)
    return out


@functools.lru_cache(maxsize=None)
def inputs(work, index11, pset, n_reads=48):
    """(P, seqs, codes of the first reads of r1k.fa) under a parameter set"""
    import yaha_amd as ya
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa")] + sets.PARAM_SETS[pset]) as s:
        P, seqs = sets.session_inputs(s)
        codes = sets.batch_codes(s.next_batch(n_reads))
    return P, seqs, codes


@functools.lru_cache(maxsize=None)
def modelled(work, index11, pset, which):
    """the directed reads of a set under a parameter set, each with the model's run: [(label, codes, clumps, Model)] -- computed once, shared"""
    P, seqs, codes = inputs(work, index11, pset, 130 if which == "tiny" else 48)
    qlens = [len(c) for c in codes]
    reads = sets.edges(qlens, seqs, P) if which == "edges" else sets.large(qlens, seqs) if which == "large" else sets.tiny_batch(qlens, seqs)
    return [(label, codes[i], cl, om.run_read(P, seqs, codes[i], len(codes[i]), cl)) for i, (label, cl) in enumerate(reads)]


def compare(exe, P, seqs, runs):
    got = drive(exe, P, seqs, [(codes, cl) for _l, codes, cl, _m in runs])
    for (label, _codes, cl, m), (recs, pc) in zip(runs, got):
        assert (m.out, m.primary_count) == (recs, pc), "model and oqc_core.h differ on %s (%d clumps): sorted order %s, survivors %s, best predecessors %s" % (
            label, len(cl), m.sorted_order[:40], m.survivors[:40], getattr(m, "best_prev", [])[:40])


@pytest.mark.parametrize("pset", sorted(sets.PARAM_SETS))
def test_model_equals_the_core_on_the_directed_batch(work, index11, driver, pset):
    P, seqs, _codes = inputs(work, index11, pset)
    compare(driver, P, seqs, modelled(work, index11, pset, "edges"))


@pytest.mark.parametrize("which", ["large", "tiny"])
def test_model_equals_the_core_on_the_large_and_the_tiny_reads(work, index11, driver, which):
    P, seqs, _codes = inputs(work, index11, "defaults", 130 if which == "tiny" else 48)
    compare(driver, P, seqs, modelled(work, index11, "defaults", which))


@pytest.mark.parametrize("seed,max_clumps,pset", [(1, 60, "defaults"), (3, 200, "fbs_loose"), (10, 112, "mno1"), (11, 30, "bp40")])
def test_model_equals_the_core_on_random_lists(work, index11, driver, seed, max_clumps, pset):
    """the distribution of test_postfilter_on_synthetic_clump_lists (its generator, imported)"""
    import yaha_amd as ya
    from test_gpu_parity import _synthetic_results
    with ya.Session(["-x", index11, "-q", os.path.join(work, "r1k.fa")] + sets.PARAM_SETS[pset]) as s:
        P, seqs = sets.session_inputs(s)
        b = s.next_batch(24)
        codes = sets.batch_codes(b)
        r, _keep = _synthetic_results(s, b, np.random.default_rng(seed), max_clumps)
        lists = sets.result_clumps(r)
    compare(driver, P, seqs, [("random_%d_%d" % (seed, i), codes[i], cl, om.run_read(P, seqs, codes[i], len(codes[i]), cl)) for i, cl in enumerate(lists)])


@pytest.mark.parametrize("reads,extra", [("r1k.fa", []), ("rchim.fa", []), ("r1k.fa", ["-FBS", "Y", "-PSS", "0.5", "-PRL", "0.5"]), ("rchim.fa", ["-FBS", "Y", "-PSS", "0.5", "-PRL", "0.5"])])
def test_model_equals_the_printed_text_on_real_reads(work, index11, reads, extra):
    """What Session.emit prints for real reads is pinned to the reference by the goldens (test_oracle_golden.py); the model must foretell it: which clumps, in which
    order, with which flag, position, MAPQ, AS and YF / YI / YP / YS tags."""
    import oracle
    import yaha_amd as ya
    with ya.Session(["-x", index11, "-q", os.path.join(work, reads), "-osh", "stdout"] + extra) as s:
        P, seqs = sets.session_inputs(s)
        b = s.next_batch(150)
        codes = sets.batch_codes(b)
        r, _own = oracle.run(s.index, s.params, b, threads=4)
        lists = sets.result_clumps(r)
        text = s.emit(r)
    got = []
    for line in text.split("\n"):
        if not line or line.startswith("@"):
            continue
        f = line.split("\t"); tags = dict((t[:2], t[5:]) for t in f[11:])
        got.append((int(f[1]), int(f[3]), int(f[4]), int(tags["AS"]), tags["YF"], int(tags["YI"]), int(tags["YP"]), int(tags["YS"]) if "YS" in tags else None))
    exp, several = [], 0
    for code, cl in zip(codes, lists):
        m = om.run_read(P, seqs, code, len(code), cl)
        several += m.primary_count > 1
        for o in m.out:
            c = cl[o.clump]; si = om.find_seq(seqs, c.sro)
            if si < 0 or c.sro + c.refLen - 1 >= seqs[si][0] + seqs[si][1]:
                continue                                               # spans two sequences: not printed (AlignOutput.c:129-136)
            exp.append((16 if o.status & 1 else 0, c.sro - seqs[si][0] + 1, o.mapQuality, c.totScore, "%02X" % o.status, o.matchedPrimary, m.primary_count,
                        o.numSecondaries if o.status & om.ST_PRIMARY else None))
    assert len(exp) >= 100 and (reads != "rchim.fa" or several > 20)
    assert got == exp


def test_tie_sets_depend_on_the_draws(work, index11):
    """A tie set proves something about the generator's stepping only if another draw sequence prints another record: every one of them, run again with all coins
    turned over, must print differently (another survivor -- its edit list differs --, another primary, or another order).  That shows dependence on the VALUES of
    the draws; for their COUNT, every tie set with eight or more ties is run once more with one draw too few for the ties of every 64 scanned elements (what a ballot
    counted one short does) and must print differently as well."""
    P, seqs, _c = inputs(work, index11, "fbs_loose")
    seen = counted = 0
    for pset, which in (("fbs_loose", "edges"), ("defaults", "large")):
        for label, codes, cl, m in modelled(work, index11, pset, which):
            if label.startswith(("all_equal", "family", "duplicates", "straddle")):
                Pm = inputs(work, index11, pset)[0]
                other = om.run_read(Pm, seqs, codes, len(codes), cl, rand=om.FlippedRand)
                ident = lambda mm: [(cl[o.clump].sro, cl[o.clump].status, cl[o.clump].ops, o.matchedPrimary) for o in mm.out]
                assert ident(other) != ident(m), label
                seen += 1
                if sum(p["ties"] for p in m.partitions) >= 8:
                    slipped = om.run_read(Pm, seqs, codes, len(codes), cl, rand=om.ShortDrawRand)
                    assert slipped.draws < m.draws and ident(slipped) != ident(m), label
                    counted += 1
    assert seen >= 10 and counted >= 8


def test_the_directed_inputs_reach_every_device_edge(work, index11):
    """om.Coverage over the union of the directed sets: statements about device/oqc_stage.h's layout and branches, shown reachable with the model alone.  The GPU tier
    asserts nothing about coverage that is not asserted here."""
    missing = []

    def need(ok, what):
        if not ok:
            missing.append(what)
    ev, covs = Counter(), {}
    for pset in sorted(sets.PARAM_SETS):
        for label, _codes, cl, m in modelled(work, index11, pset, "edges"):
            c = om.Coverage(m, cl); covs[(pset, label)] = c; ev.update(c.events)
    for which in ("large", "tiny"):
        for label, _codes, cl, m in modelled(work, index11, "defaults", which):
            c = om.Coverage(m, cl); covs[(which, label)] = c; ev.update(c.events)
    D = {label: c for (pset, label), c in covs.items() if pset in ("defaults", "large")}
    cov = list(covs.values()); dev = [c for c in cov if isinstance(c.cls, int)]
    # classes and placement
    for n, cls in ((0, "settled_by_classify"), (1, "settled_by_classify"), (2, 0), (112, 0), (113, 1), (224, 1), (225, 2), (448, 2), (449, 3), (1792, 3), (1793, "host")):
        need(any(c.n == n and c.cls == cls for c in cov), "a read of %d clumps in class %s" % (n, cls))
    by_n = {len(cl): (m, cl) for _label, _codes, cl, m in modelled(work, index11, "defaults", "tiny")}
    need(om.Coverage(*by_n[5], dev_max=4).cls == "host" and om.Coverage(*by_n[4], dev_max=4).cls == 0, "under YGPU_OQC_MAX=4 four clumps are filtered, five handed back")
    tiny = Counter(c.cls for (w, _l), c in covs.items() if w == "tiny")
    tiny4 = Counter(om.device_class(len(cl), 4) for _l, _c, cl, _m in modelled(work, index11, "defaults", "tiny"))
    need(tiny4[0] > 64 and tiny4["host"] >= 16 and tiny4["settled_by_classify"] > 16, "k_oqc_classify under YGPU_OQC_MAX=4: more than 64 reads filtered, 16 or more handed back (%s)" % dict(tiny4))
    need(tiny[0] > 64 and tiny[1] == 1 and tiny[2] == 2 and tiny["settled_by_classify"] > 16, "k_oqc_classify: lists of 1, 2 and more than 64 reads (%s)" % dict(tiny))
    need(all(c.keys_in_lds and c.sort_on_wave for c in dev), "every read the device takes sorts on the wave (the one-lane sort needs n > 1 799: beyond YQ_DEVICE_MAX)")
    need(D["tables_overrun_112"].cls == 0 and D["tables_overrun_112"].cnt == 112 and D["tables_overrun_112"].tables_lds > 0 and D["tables_overrun_112"].tables_hbm > 0,
         "class 0, 112 survivors, tables in both pools")
    need(D["survivors_1400"].cnt > 1349 and not D["survivors_1400"].graph_in_lds, "more than 1 349 survivors: the graph in HBM without the hook")
    need(D["survivors_1349"].cnt == 1349 and D["survivors_1349"].graph_at_lds_limit and D["survivors_1349"].tables_lds == 0, "1 349 survivors: the last count in LDS, every table in HBM")
    M1 = {label: c for (pset, label), c in covs.items() if pset == "mno1"}
    need(M1["primaries_70_in_hbm"].events["primaries_more_than_64"] == 1 and not M1["primaries_70_in_hbm"].primaries_in_lds and M1["primaries_70_in_hbm"].graph_in_lds,
         "more than 64 primaries that do not fit behind the nodes")
    need(M1["primaries_70_in_lds"].events["primaries_more_than_64"] == 1 and M1["primaries_70_in_lds"].primaries_in_lds, "more than 64 primaries behind the nodes")
    # the sort, in the device's formulation
    parts = [p for c in dev for p in c.partitions]
    first = {max(p["m"] for p in c.partitions) for c in dev if c.partitions}          # (the first partition scans n - 1 elements: the longest of a read)
    for m_ in (63, 64, 65, 127, 128, 129):
        need(m_ in first, "a first partition of %d scanned elements" % m_)
    need(any(p["m"] == 63 and p["ties"] == 63 for p in parts), "63 scanned elements, all ties (registers)")
    need(any(p["m"] == 64 and p["ties"] == 64 for p in parts), "64 scanned elements, all ties: 64 draws in one chunk")
    need(any(p["m"] >= 64 and p["ties"] == 0 for p in parts) and any(p["m"] < 64 and p["ties"] == 0 and p["m"] > 8 for p in parts), "partitions without ties, both paths")
    need(any(p["m"] >= 64 and p["tie_chunks"] >= 2 for p in parts), "ties in more than one 64-chunk of a long partition")
    need(any(p["ties"] >= 400 and p["tie_chunks"] >= 7 for p in D["family_500"].partitions), "hundreds of ties in one partition, in seven or more 64-chunks")
    s = D["straddle_130"].partitions
    need(max(s, key=lambda p: p["m"])["ties"] == 9 and max(s, key=lambda p: p["m"])["tie_chunks"] == 2, "nine ties around scan position 64 in the first partition")
    for lo, hi, name in ((1, 63, "registers"), (64, 10 ** 6, "LDS")):
        need(any(lo <= p["m"] <= hi and p["nL"] == 0 for p in parts), "nL == 0, " + name)
        need(any(lo <= p["m"] <= hi and p["nL"] == p["m"] for p in parts), "nL == m, " + name)
    need(D["adversarial_1792"].max_waiting > om.YQ_STACK_LDS // 2 and D["adversarial_1792"].stack_spills, "more than 64 right parts waiting: the stack runs over into HBM")
    need(not any(c.stack_spills for l, c in D.items() if l != "adversarial_1792"), "(no other read spills)")
    # the duplicate scan
    ends = Counter()
    for c in dev:
        ends.update(c.scan_ends)
    for k in ("own_block", "next_block", "two_or_more_blocks_on", "list_end", "at_lane_63", "at_lane_0_of_the_next_block"):
        need(ends[k] > 0, "a duplicate scan that ends: " + k)
    for k in ("dup_kill_score8_in_block", "dup_kill_score8_out_of_block", "dup_kill_same_place_in_block", "dup_kill_same_place_out_of_block", "dup_dead_at_its_turn"):
        need(ev[k] > 0, k)
    need(D["duplicates_70"].events["dup_kill_same_place_in_block"] + D["duplicates_70"].events["dup_kill_same_place_out_of_block"] == 69, "a family of 70 exact duplicates")
    # the graph and the finish
    for k in ("relax_eqo_too_close", "relax_lost_before_penalty", "relax_lost_after_penalty", "relax_lost_after_overlap", "relax_better", "relax_tie_shorter_path", "relax_tie_not_shorter", "relax_tie_no_prev",
              "best_lower", "best_higher", "best_tie_shorter_path", "best_tie_not_shorter",
              "bpp_near", "bpp_far", "bpp_at_a_step", "bpp_one_below_a_step", "bpp_one_above_a_step", "bpp_other_sequence",
              "overlap_right_best", "overlap_path_best", "overlap_walk_through_several_nodes",
              "startj_first_far_in_later_chunk", "startj_none_far", "startj_at_cnt",
              "primaries_1", "primaries_2", "primaries_more_than_64", "secondary_pushed", "secondary_counted_not_pushed", "secondary_failed_with_FBS_on",
              "second_score_updated", "third_score_updated", "second_and_third_kept",
              "mq_no_second", "mq_second_at_least_total", "mq_second_and_third_at_least_total", "mq_third_zero", "mq_both", "node_overlaps_no_primary", "reversed_clump"):
        need(ev[k] > 0, "event " + k)
    assert not missing, "not reached:\n  " + "\n  ".join(missing)
