"""CPU tier: the plain model of the index file (tests/index_model.py: the reference's sequential scan, its sampling pass and its generator) on the directed genomes
of tests/index_sets.py, under every option list they come with -- equal to the host builder's file (`yaha -g ... -cpuindex`), to the live reference binary's where
it is built, and to the recorded SHA-256 of the two genome_small goldens -- and the Coverage of every set: what tests/test_gpu_index_edges.py relies on the sets to
reach on the device (thread-span, workgroup and grid edges of the walk, N-run phases under -S, every list class and its boundaries, sampled-list shapes) is asserted
here, so that a set which stops reaching its edge fails on the CPU, before any GPU run."""
import hashlib
import os
import shutil
import subprocess

import pytest

import index_model as im
import index_sets as sets
import oracle
import yaha_amd as ya
from index_sets import index_name, modelled, nib2_of, the_sets

CASES = [(name, opt) for name, gs in sorted(the_sets().items()) for opt in gs.options]


@pytest.fixture(scope="module")
def genomes(work, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("index_sets"))
    return {name: nib2_of(gs, d) for name, gs in the_sets().items()}


@pytest.mark.parametrize("name,opt", CASES, ids=["%s-L%d-S%d-H%d" % ((n,) + o) for n, o in CASES])
def test_model_equals_the_host_builder_and_the_reference(genomes, name, opt, tmp_path):
    gs = the_sets()[name]
    image, _cov, ix = modelled(gs, opt, genomes[name])
    g = os.path.join(str(tmp_path), name + ".nib2")
    shutil.copy(genomes[name], g)
    args = ["-L", str(opt[0]), "-S", str(opt[1]), "-H", str(opt[2])]
    out = os.path.join(str(tmp_path), index_name(name, opt))
    r = subprocess.run([ya.CLI_PATH, "-g", g, "-cpuindex"] + args, stderr=subprocess.PIPE, check=True)
    assert b"Building the index on GPU" not in r.stderr
    diff = im.first_difference(image, open(out, "rb").read(), opt[0], ix.counts)
    assert diff is None, "the host builder's file differs from the model: " + diff
    # Left out of the comparison with the reference binary, by name: the sets of index_sets.SHORTER_THAN_K (walk_fa, walk_tight) hold sequences shorter than
    # wordLen, where the reference's unsigned endingOffset wraps and its scan runs on into the sequences behind.
    if oracle.have_reference() and name not in sets.SHORTER_THAN_K:
        os.remove(out)
        oracle.run_reference(["-g", g] + args)
        diff = im.first_difference(image, open(out, "rb").read(), opt[0], ix.counts)
        assert diff is None, "the MODEL is wrong: the reference binary's file differs from it: " + diff


def test_sets_left_out_of_the_reference_comparison_are_the_ones_with_a_short_sequence(genomes):
    for name, gs in the_sets().items():
        shortest = min(len(s) for s in gs.seqs)
        assert (name in sets.SHORTER_THAN_K) == any(shortest < o[0] for o in gs.options), name


@pytest.mark.parametrize("args,name", [(("-L", "11"), "genome_small.X11_01_65525S"), (("-L", "8", "-H", "20"), "genome_small.X08_01_00020S")])
def test_model_equals_the_recorded_goldens(work, meta, args, name):
    k = int(args[1]); h = int(args[3]) if len(args) > 2 else sets.DEFAULT_H
    image, _cov, _ix = im.model(open(os.path.join(work, "genome_small.nib2"), "rb").read(), k, 1, h)
    assert hashlib.sha256(image).hexdigest() == meta["index"][name]["sha256"], name


def test_generator_and_sample_are_the_references():
    """the first words of the default-seeded generator, by hand from Math.c:274-284, and the sample's two branches (mark the kept / mark the dropped)"""
    s = [123456789, 362436069, 521288629, 88675123, 886756453]
    t = s[0] ^ (s[0] >> 7)
    v = ((s[4] ^ (s[4] << 6)) ^ (t ^ (t << 13))) & 0xFFFFFFFF
    assert im.Rand().bits() == ((2 * s[2] + 1) * v) & 0xFFFFFFFF
    for n, m in ((10, 3), (10, 5), (10, 6), (10, 9), (3, 1), (2, 1)):
        out = im.rand_sample(im.Rand(), list(range(100, 100 + n)), m)
        assert len(out) == m and out == sorted(set(out)) and set(out) <= set(range(100, 100 + n))


# ---- what the sets reach -----------------------------------------------------------------------------------------------------------------------------------
def check(ok, what):
    assert ok, "the set does not reach what it was built for: " + what


def cov_of(genomes, name, opt):
    return modelled(the_sets()[name], opt, genomes[name])[1]


BAD_PLACES = ("first_base", "last_base", "span_offset_0", "span_offset_15", "crosses_a_span", "crosses_a_workgroup")


def test_coverage_of_the_walk_sets(genomes):
    for opt in the_sets()["walk_fa"].options:
        c = cov_of(genomes, "walk_fa", opt); k = opt[0]
        check({-1, 0, 1} <= c.len_minus_k, "sequences of k-1, k and k+1 bases, k = %d" % k)
        check(c.last_base_mod_16 == set(range(16)), "a sequence end at every residue mod 16")
        check(c.start_mod_16 == {0, 8}, "a sequence start at both residues mod 16 that a FASTA genome has")
        check(c.odd_lengths >= 10 and c.last_is_odd, "odd lengths, the last sequence too")
        for p in BAD_PLACES:
            check(c.bad_places.get(p) == {"N", "iupac"}, "N and another IUPAC code: " + p)
        check(c.all_n_seqs >= 1 and c.no_clean_window_seqs >= 2 and c.clean_seqs >= 1, "a sequence of N only, sequences without a clean window, a clean one")
        check(c.n_offsets > 2 * im.IX_WG, "more than two workgroups")
    c = cov_of(genomes, "walk_tight", (8, 1, sets.DEFAULT_H))
    check(c.start_mod_16 == set(range(0, 16, 2)), "a sequence start at every residue mod 16 that the format has (the header counts bytes)")
    check(c.last_base_mod_16 == set(range(16)), "a sequence end at every residue mod 16")
    check({2, 3} <= c.kept_seqs_in_a_span, "two and three sequences of the table inside one 16-offset span at -L 8")
    check(max(c.seqs_in_a_span) >= 4 and min(c.len_minus_k) < 0, "dropped sequences between kept ones inside a span")
    ends = {}
    for d in (-1, 0, 1):
        c = cov_of(genomes, "grid_edge_%s" % {-1: "short", 0: "exact", 1: "past"}[d], (8, 1, sets.DEFAULT_H))
        ends[d] = (c.end_of_bases, c.n_offsets)
    check(ends[0][0] % im.IX_WG == 0 and ends[-1][0] == ends[0][0] - 1 and ends[1][0] == ends[0][0] + 1, "the last base ends a multiple of 4 096, one short, one past: %s" % ends)
    check(ends[0][1] % im.IX_WG == 0 and ends[1][1] == ends[0][1] + 8, "an offset count that fills the last workgroup, and one that opens a new one with 8 offsets: %s" % ends)


def test_coverage_of_the_skip_set(genomes):
    assert {(o[1] if o[1] != o[0] else "k") for o in sets.SKIP_OPTIONS} == {2, 3, 7, "k"}
    for opt in sets.SKIP_OPTIONS:
        c = cov_of(genomes, "skip", opt); k, S = opt[0], opt[1]; what = " (-L %d -S %d)" % (k, S)
        check(c.start_mod_S == set(range(0, S, 2 if S % 2 == 0 else 1)), "sequence starts at every residue mod S that the format has" + what)
        check(c.fb_in_first_window >= 3, "a first bad code inside the very first window" + what)
        check(c.window_ends_at_first_bad >= 2, "a window that ends one base before the first bad code" + what)
        check({"multiple", "one_before", "one_after"} <= c.run_end_vs_S, "N runs that end at a multiple of S, one before it, one after it" + what)
        # (-S 2: every start is even, because the header counts bytes, and so is every re-phased offset -- no residue to change)
        check(c.rephase_changes_residue >= 10 if S != 2 else c.rephase_changes_residue == 0, "a re-phase that changes the residue" + what)
        check(c.max_runs_with_visits >= 3, "k-mers behind a second and a third N run" + what)
        check(c.fb_far == 1, "a first bad code more than 4 096 offsets into its sequence" + what)
        check(c.max_first_bads_in_a_span >= 2, "several sequences with their own first bad code inside one thread's span" + what)
        check(c.clean_seqs >= 1, "a sequence without any bad code" + what)
        check({"N", "iupac"} <= set().union(*c.bad_places.values()), "N and other IUPAC codes" + what)


def test_coverage_of_the_list_set(genomes):
    c = cov_of(genomes, "lists", (sets.LIST_K, 1, 8192))
    check(set(sets.LIST_LENGTHS) <= c.list_lengths, "lists of %s entries; has %s" % (sets.LIST_LENGTHS, sorted(c.list_lengths)))
    check(c.len_hash_0 == 16385 and c.len_hash_max == 16384, "hash 0 and hash 4^k - 1 above 8 192")
    check(c.network_sizes() == {16384, 32768}, "k_ix_bitonic_global for one and for two merge sizes")
    check(c.network_sizes(64) >= {128, 256, 8192, 16384, 32768} and c.network_sizes(32) >= {64, 128, 256}, "under the hook: m = 64 (cnt = m), 128, 256")
    cl = c.classes()
    check(all(cl[x] > 0 for x in (im.list_class(2), im.list_class(33), im.list_class(8193))), "all three sort classes: %s" % dict(cl))
    for n in (8191, 8192, 8193, 16384, 16385):
        check(c.workgroups_of_long_lists[n] >= 3, "the list of %d entries is filled from three or more workgroups of the walk" % n)
    for n in (33, 64, 65, 128, 129):
        check(c.workgroups_of_long_lists[n] >= 2, "the list of %d entries is filled from more than one workgroup" % n)
    # k_ix_compact under -H 8192: 8 193, 16 384, 16 385 sampled; copied by the wave: 8 191 and 8 192 and the planted ones
    check(c.sampled_lengths == {8193, 16384, 16385} and c.hash_0_sampled and c.hash_max_sampled, "sampled lists, hash 0 and hash 4^k - 1 among them")
    check(c.max_wave_copies_in_a_wave >= 3 and {33, 65, 129, 8191, 8192} <= c.unsampled_lengths, "several lanes of one wave own a list above 32")
    c = cov_of(genomes, "lists", (sets.LIST_K, 1, sets.DEFAULT_H))
    check(c.n_over == 0, "no list sampled under the default -H")


def test_coverage_of_the_sampling_sets(genomes):
    assert sets.SAMPLING_H == (1, 20, 32, 33, 64, 100)
    for H in sets.SAMPLING_H:
        c = cov_of(genomes, "sampling", (sets.LIST_K, 1, H)); what = " (-H %d)" % H
        check({H - 1, H, H + 1} <= c.list_lengths and H + 1 in c.sampled_lengths and {H - 1, H} <= c.unsampled_lengths, "lists of H-1, H and H+1 entries" + what)
        check(c.len_hash_0 == 40 and c.len_hash_max == 70, "hash 0 and hash 4^k - 1 above 32")
        check(c.hash_0_sampled == (H < 40) and c.hash_max_sampled == (H < 70), "sampled at hash 0 / at hash 4^k - 1" + what)
        if H == 33:
            check({32, 33} <= c.unsampled_lengths and 34 in c.sampled_lengths, "unsampled lists of 32 and 33 entries (the two copy paths of k_ix_compact) next to sampled ones")
        if H == 64:
            check(0 in c.wave_copy_lanes and c.max_wave_copies_in_a_wave >= 2, "-H 64: lane 0 and two lanes of one wave own an unsampled list above 32")
        if H == 100:
            check({0, 63} <= c.wave_copy_lanes and c.max_wave_copies_in_a_wave >= 3, "-H 100: lanes 0 and 63 and three lanes of one wave own an unsampled list above 32")
    c = cov_of(genomes, "sampling", (sets.LIST_K, 1, 32))
    check(c.hash_0_sampled and c.hash_max_sampled, "sampled lists at hash 0 and at hash 4^k - 1")
    check(c.network_sizes(32) >= {64, 128}, "YAHA_IX_HUGE_MIN=32: m = 64 < IX_BLOCK and m = 128")
    # the two hooks (tests/test_gpu_index_edges.py): both long-list arrays overflow a capacity of 4; groups of at most 100 entries
    check(c.n_long > 4 and c.n_over > 4, "more long lists and more over-represented lists than YAHA_IX_LIST_CAP=4")
    groups = c.transfer_groups(100)
    check(len(groups) >= 4 and any(len(g) == 1 and g[0] > 100 for g in groups) and any(len(g) > 1 for g in groups),
          "YAHA_IX_GROUP_CAP=100: several groups, a boundary between two lists, a single list larger than the cap: %s" % groups)
    c = cov_of(genomes, "many_over", (8, 1, 2))
    check(c.n_over >= 2000, "several thousand over-represented k-mers: %d" % c.n_over)
