"""GPU tier: the index build on the device (device/index_build.hip: k_ix_first_bad, k_ix_count, k_ix_fill, k_ix_order_small, k_ix_order_block, k_ix_pad_copy,
k_ix_bitonic_local, k_ix_bitonic_global, k_ix_clamp, k_ix_compact, k_ix_pack, k_ix_unpack, k_ix_gather and the two scans) through the command line, against the plain
model of tests/index_model.py, byte for byte, on the directed genomes of tests/index_sets.py.  What those genomes reach -- every thread-span, workgroup and grid edge
of the walk, the N-run phases of -S 2, 3, 7 and k, lists of 0 .. 16 385 entries on both sides of every class boundary, sampled lists of H-1, H and H+1 entries -- is
asserted by tests/test_index_model.py on the CPU tier, where model == host builder == reference binary on the same files.

Every run asserts that the command line says it builds on the GPU and does NOT say that the device build failed: runIndex falls back to the host builder without
another sign, and a fallback would compare the host builder with the model.  A difference names the first differing k-mer, its list length and the kernel that ordered it.

Process starts: 30 in all (each a device build of a genome of at most 75 kbp at -L 8, 10 or 11); each prints its wall time."""
import os
import shutil
import subprocess
import time

import pytest

import index_model as im
import index_sets as sets
import yaha_amd as ya
from index_sets import index_name, modelled, nib2_of, the_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def genomes(work, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("index_sets_gpu"))
    return {name: nib2_of(gs, d) for name, gs in the_sets().items()}


def device_build(genomes, name, opt, tmp_path, env=None, tag=""):
    """one device build by the command line; the file's bytes"""
    d = os.path.join(str(tmp_path), "run%d" % len(os.listdir(str(tmp_path))))
    os.makedirs(d)
    g = os.path.join(d, name + ".nib2")
    shutil.copy(genomes[name], g)
    t0 = time.perf_counter()
    r = subprocess.run([ya.CLI_PATH, "-g", g, "-L", str(opt[0]), "-S", str(opt[1]), "-H", str(opt[2])], stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=120)
    took = time.perf_counter() - t0
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-2000:]
    assert "Building the index on GPU" in err, err[-2000:]
    assert "Index build on the GPU failed" not in err, err[-2000:]
    print("%s -L %d -S %d -H %d %s: %.2f s" % ((name,) + tuple(opt) + (tag or " ".join("%s=%s" % kv for kv in sorted((env or {}).items())), took)))
    return open(os.path.join(d, index_name(name, opt)), "rb").read()


def compare(genomes, name, opt, tmp_path, env=None, times=1):
    image, _cov, ix = modelled(the_sets()[name], opt, genomes[name])
    huge_min = int((env or {}).get("YAHA_IX_HUGE_MIN", im.IX_BLOCK))
    for t in range(times):
        got = device_build(genomes, name, opt, tmp_path, env)
        diff = im.first_difference(image, got, opt[0], ix.counts, huge_min)
        assert diff is None, "%s, -L %d -S %d -H %d, %s, run %d: the device-built index differs from the model: %s" % ((name,) + tuple(opt) + (env or "no hook", t + 1, diff))


WALK_CASES = [(n, o) for n in ("walk_fa", "walk_tight", "grid_edge_short", "grid_edge_exact", "grid_edge_past") for o in the_sets()[n].options]


@pytest.mark.parametrize("name,opt", WALK_CASES, ids=["%s-L%d" % (n, o[0]) for n, o in WALK_CASES])
def test_walk_edges_equal_the_model(genomes, name, opt, tmp_path):
    """sequences of k-1, k and k+1 bases, two and three inside one thread's span, starts and ends at every residue, odd lengths, bad codes at every span and
    workgroup edge, and a last base that ends a multiple of 4 096 offsets, one short of it and one past it"""
    compare(genomes, name, opt, tmp_path)


@pytest.mark.parametrize("opt", sets.SKIP_OPTIONS, ids=["L%d-S%d" % (o[0], o[1]) for o in sets.SKIP_OPTIONS])
def test_skip_distances_equal_the_model(genomes, opt, tmp_path):
    """-S 2, 3, 7 and k: the closed form of walkKmers against the reference's loop -- first bad codes in the first window, one base behind a window, more than a
    workgroup into the sequence, several in one span; runs that end at, before and behind a multiple of S; second and third runs"""
    compare(genomes, "skip", opt, tmp_path)


@pytest.mark.parametrize("huge_min", [None, 64, 32])
def test_list_classes_equal_the_model_twice(genomes, huge_min, tmp_path):
    """lists of 0, 1, 2, 32, 33, 64, 65, 128, 129, 8 191, 8 192, 8 193, 16 384 and 16 385 entries (m = 16 384 and 32 768 for the network: one and two merge sizes
    of k_ix_bitonic_global), hash 0 and hash 4^k - 1 above 8 192; under -H 8192 the three longest are sampled and the others go through k_ix_compact's wave copy.
    With the hook every list above 64, then above 32, takes the network.  Each twice: the atomics' order differs between runs and the file must not."""
    env = {"YAHA_IX_HUGE_MIN": str(huge_min)} if huge_min else None
    compare(genomes, "lists", (sets.LIST_K, 1, 8192), tmp_path, env, times=2)
    if not huge_min:
        compare(genomes, "lists", (sets.LIST_K, 1, sets.DEFAULT_H), tmp_path)


@pytest.mark.parametrize("H", sets.SAMPLING_H)
def test_sampled_lists_equal_the_model(genomes, H, tmp_path):
    """-H 1, 20, 32, 33, 64, 100 with lists of H-1, H and H+1 entries; sampled and wave-copied lists at hash 0 and at hash 4^k - 1"""
    compare(genomes, "sampling", (sets.LIST_K, 1, H), tmp_path)


@pytest.mark.parametrize("H,huge_min,times", [(33, 32, 2), (100, 32, 1), (64, 64, 1)])
def test_sampled_lists_through_the_network(genomes, H, huge_min, times, tmp_path):
    """the sampling set with every list above 32 (m = 64 < IX_BLOCK: the cnt = m path of k_ix_bitonic_local) or above 64 in the multi-workgroup sort"""
    compare(genomes, "sampling", (sets.LIST_K, 1, H), tmp_path, {"YAHA_IX_HUGE_MIN": str(huge_min)}, times=times)


def test_thousands_of_sampled_kmers_equal_the_model(genomes, tmp_path):
    """-L 8 -H 2 on random sequence: the generator is consumed in k-mer order by several thousand lists (the std::sort of `over`)"""
    compare(genomes, "many_over", (8, 1, 2), tmp_path)


@pytest.mark.parametrize("env", [{"YAHA_IX_LIST_CAP": "4"}, {"YAHA_IX_GROUP_CAP": "100"}], ids=["regrow_and_redo", "transfer_groups"])
def test_hooks_reach_the_regrow_and_the_group_split(genomes, env, tmp_path):
    """YAHA_IX_LIST_CAP=4: both long-list arrays overflow and k_ix_order_small runs again on regrown ones.  YAHA_IX_GROUP_CAP=100: the over-represented lists of the
    sampling set under -H 32 go through several pack / sample / unpack groups, with a boundary between two lists and a single list larger than the cap
    (test_coverage_of_the_sampling_sets asserts both on the model's list lengths)."""
    compare(genomes, "sampling", (sets.LIST_K, 1, 32), tmp_path, env)
