"""The seed stage (A1 + A2) on the device, edge by edge, against the oracle and seed_model.py: the sets of test_seed_model.py, which proves there -- without a
GPU -- that they fill every shape of the workgroup sort exactly, one short and one past, reach every bucket count and several levels of the cuts, the wrapping
diagonals and the end of ROA, and put every link between two hits on a row, a wave and a tile boundary of k_frag_scan_build.

Every comparison is exact:
  ctx.seed_join()            every fragment                                  == oracle.seed_join
  ctx.seed_join(kept=True)   the array as ygpu_run builds it                 == the model's fragments without its dead ones (that dropping those changes no clump
                                                                                is test_seed_model.py's chain check)
  ctx.run()                  records; hits, fragments, regions, kmer_lookups == oracle.run
A difference names the set (so the edge), the entry point (so the kernel: the sort and the cuts for both arrays, the dead-single masks for `kept` alone) and the
first fragment that differs."""
import os
import re
import subprocess

import pytest

import oracle
import seed_model as sm
import yaha_amd as ya
from conftest import strip_pg
from test_seed_model import DEEP_LIMITS, LADDER_LOW_MAX, SETS, first_difference, make_batch, seedsets  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
COUNTERS = ("hits", "fragments", "regions", "kmer_lookups")


def frag_tuples(f, n):
    return [(f[i].startRefOff, f[i].startQueryOff, f[i].endQueryOff, f[i].refLen, f[i].read_strand) for i in range(n)]


def check_fragments(ctx, S, what=""):
    """the uploaded set's two fragment arrays"""
    got = frag_tuples(*ctx.seed_join())
    assert got == S.oracle_frags, first_difference(got, S.oracle_frags, "%s%s, every fragment, device against oracle" % (S.name, what))
    got = frag_tuples(*ctx.seed_join(kept=True))
    assert got == S.model.kept, first_difference(got, S.model.kept, "%s%s, kept fragments, device against model" % (S.name, what))


def check_run(ctx, S, what=""):
    ctx.run()
    r = ctx.collect()
    ro, _own = oracle.run(S.s.index, S.s.params, S.batch, threads=8)
    assert ya.result_records(r) == ya.result_records(ro), "%s%s: device clump records differ from the oracle" % (S.name, what)
    got, exp = r.counters.as_dict(), ro.counters.as_dict()
    for key in COUNTERS:
        assert got[key] == exp[key], (S.name + what, key, got[key], exp[key])
    return r


def check_set(S, what=""):
    with ya.Context(S.s.index, S.s.params) as ctx:
        ctx.upload(S.batch)
        check_fragments(ctx, S, what)
        check_run(ctx, S, what)


@pytest.mark.parametrize("name", list(SETS))
def test_each_set_against_the_oracle_and_the_model(seedsets, name):
    S = seedsets[name]
    check_set(S)
    if name == "link_M11":                                                   # one word is a whole match: nothing is dropped
        assert S.model.kept == S.oracle_frags


@pytest.mark.parametrize("switch,value", [("YGPU_SORT_RANK", "ballots"), ("YGPU_SORT_WIDE", "0"), ("YGPU_SEGSORT_MAX", str(LADDER_LOW_MAX))])
def test_the_ladder_set_under_the_other_rankings_shapes_and_limit(seedsets, monkeypatch, switch, value):
    """every shape full, one short and one past: ranked by ballots, in the 1 024-thread shapes of the four largest classes, and under a limit that sends 12 288
    and 12 289 hits through k_seg_split (two buckets against four)"""
    monkeypatch.setenv(switch, value)
    check_set(seedsets["ladder"], " under %s=%s" % (switch, value))


@pytest.mark.parametrize("rank", ["atomic", "ballots"])
@pytest.mark.parametrize("limit", DEEP_LIMITS)
def test_the_deep_cut_set_at_both_limits_and_rankings(seedsets, monkeypatch, limit, rank):
    monkeypatch.setenv("YGPU_SEGSORT_MAX", str(limit))
    monkeypatch.setenv("YGPU_SORT_RANK", rank)
    S = seedsets["deep"]
    with ya.Context(S.s.index, S.s.params) as ctx:
        ctx.upload(S.batch)
        check_fragments(ctx, S, " under a limit of %d, ranking %s" % (limit, rank))


@pytest.mark.parametrize("limit", DEEP_LIMITS)
def test_the_command_line_cuts_the_deep_set_as_deep_as_the_model_says(seedsets, tmp_path, limit):
    """the library's own `hit sort: cut N` lines (YGPU_TRACE, read once a process: a child) against seed_model.cut_plan, level by level; the SAM against the oracle's"""
    S = seedsets["deep"]
    reads, out = str(tmp_path / "deep.fa"), str(tmp_path / "o.sam")
    with open(reads, "w") as f:
        for k, r in enumerate(S.reads):
            f.write(">deep%d\n%s\n" % (k, r))
    with ya.Session(["-x", S.index, "-q", reads, "-osh", "stdout"]) as s:
        b = s.next_batch(len(S.reads) + 1)
        assert b.n_reads == len(S.reads)
        ro, _own = oracle.run(s.index, s.params, b, threads=8)
        exp = strip_pg(s.header() + s.emit(ro))
    p = subprocess.run([ya.CLI_PATH, "-x", S.index, "-q", reads, "-osh", out, "-ctx", "1", "-batch", "64"], stderr=subprocess.PIPE,
                       env=dict(os.environ, YGPU_TRACE="1", YGPU_SEGSORT_MAX=str(limit)))
    err = p.stderr.decode()
    assert p.returncode == 0, err[-1500:]
    cuts = [tuple(int(x) for x in m) for m in re.findall(r"hit sort: cut (\d+): (\d+) pieces cut again, (\d+) of their buckets still too long", err)]
    want = [(lv + 2, n, still) for lv, (n, still) in enumerate(S.coverage(limit).cut_levels)]
    print("limit %d: cuts %r" % (limit, cuts))
    assert len(want) >= 3 and cuts == want, (cuts, want)
    assert strip_pg(open(out).read()) == exp


def test_one_context_counts_first_runs_again_with_room_and_redoes(seedsets, monkeypatch):
    """a context's first batch is counted before it is written (the fragment array has no room yet); a batch with more fragments than the array holds -- the
    link set behind the one-hit batch, by seed_model.frag_room_after -- is written as far as the room goes and run again with room; the same batches again
    fit; a redo of the chain stage (YGPU_CLUMP_BOUND) rebuilds the array and finishes it with k_frag_finish.  Each gives what a fresh context gives.  Here
    the count pass and the second run are ygpu_seed_join's, with every fragment kept; the next test takes them with the drop on."""
    tiny, link = seedsets["hits1"], seedsets["link"]
    assert len(tiny.oracle_frags) == 1 and len(link.oracle_frags) > sm.frag_room_after(1)
    with ya.Context(link.s.index, link.s.params) as ctx:
        for k, S in enumerate((tiny, link, tiny, link)):
            ctx.upload(S.batch)
            check_fragments(ctx, S, ", batch %d of one context" % k)
            check_run(ctx, S, ", batch %d of one context" % k)
        monkeypatch.setenv("YGPU_CLUMP_BOUND", "4")
        ctx.upload(link.batch)
        r = check_run(ctx, link, ", redone")
        assert r.counters.as_dict()["clumps_formed"] > 4
        monkeypatch.delenv("YGPU_CLUMP_BOUND")
        check_fragments(ctx, link, ", after the redo")


@pytest.mark.parametrize("first", ["kept", "run"])
def test_the_count_pass_and_the_second_run_with_the_dead_singles_dropped(seedsets, first):
    """a fresh context whose every call drops the dead singles, as production does: two exact reads (the count pass; the array then holds
    frag_room_after(their kept fragments)), then the link set, whose KEPT fragments exceed that room (written as far as it goes, counted, run again).  Once
    through seed_join(kept=True), once through run(), which must still report every fragment in its counter."""
    two, link = seedsets["exact2"], seedsets["link"]
    assert 0 < len(two.model.kept) and len(link.model.kept) > sm.frag_room_after(len(two.model.kept))
    with ya.Context(link.s.index, link.s.params) as ctx:
        for S in (two, link):
            ctx.upload(S.batch)
            if first == "kept":
                got = frag_tuples(*ctx.seed_join(kept=True))
                assert got == S.model.kept, first_difference(got, S.model.kept, "%s, kept fragments as a context's first call, device against model" % S.name)
            check_run(ctx, S, ", run by a context that kept no dead single before")
        check_fragments(ctx, link, ", behind the runs")


def test_a_read_of_32001_bases_is_refused(seedsets):
    S = seedsets["lengths"]
    long_read = max(S.reads, key=len)
    b, _keep = make_batch([long_read[:100], long_read + "T"])
    with ya.Context(S.s.index, S.s.params) as ctx:
        with pytest.raises(RuntimeError, match="32000"):
            ctx.upload(b)
        ctx.upload(S.batch)                                                  # ... and the context goes on
        check_fragments(ctx, S, ", after a refused upload")
