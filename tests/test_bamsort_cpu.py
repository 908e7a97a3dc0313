"""CPU tier: -obsort through the whole command line -- host sources, main.cpp and the test double tests/fixtures/oracle_device.cpp, which has no ygpu_bamsort_*
and no ygpu_bgzf_*: store, order and blocks are the host's here (the device's: tests/test_gpu_bamsort.py) -- and the index routines with the host's ordering
as a program of their own (tests/fixtures/bai_driver.cpp), plainly and under AddressSanitizer + UBSan.  The files are judged by tests/bam_oracle.py (strict
BGZF reader, BAM -> SAM) and tests/bai_oracle.py (strict BAI parser, the index rebuilt from the file, the reader's region query against a scan)."""
import json
import os
import random
import subprocess

import pytest

import bai_oracle as ba
import bam_oracle as bo
from conftest import ROOT, golden_lines
from test_bam_cpu import SETS, SRCS, check_bam

FIX = os.path.join(ROOT, "tests", "fixtures")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bamsort") / "yaha_double")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-o", out] + SRCS)
    return out


def run(exe, args, env=None, ok=True):
    p = subprocess.run([exe] + args, env=dict(os.environ, YAHA_STATS="1", YAHA_CPUS="6", **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = p.stderr.decode()
    if not ok:
        return p.returncode, err
    assert p.returncode == 0, err[-2000:]
    return p.stdout, json.loads([l for l in err.split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])


def sorted_sam(lines):
    """A SAM's lines with the header of a sorted run and the record lines in coordinate order: (index of the sequence in @SQ order, position), stable."""
    lines = [l for l in lines if not l.startswith("@PG")]
    order = {l.split("\t")[1][3:]: i for i, l in enumerate(l for l in lines if l.startswith("@SQ"))}
    head = ["@HD\tVN:1.0\tSO:coordinate" if l.startswith("@HD") else l for l in lines if l.startswith("@")]
    assert head[0].startswith("@HD") and lines[0] == "@HD\tVN:1.0"
    recs = [l for l in lines if l and not l.startswith("@")]
    recs.sort(key=lambda l: (order[l.split("\t")[2]], int(l.split("\t")[3])))
    return head + recs + [""]


def check_sorted_run(out, want_lines, st, oflag, device):
    data, bai = open(out, "rb").read(), open(out + ".bai", "rb").read()
    raw = check_bam(data, sorted_sam(want_lines), st, oflag)
    pg = [l for l in bo.bam_to_sam(raw)[0].split("\n") if l.startswith("@PG")][0]
    assert " %s %s -obsort -t " % (oflag, out) in pg
    bam, refs = ba.check_contract(data, bai)
    assert st["bam_sorted_records"] == len(bam.records) == st["bam_records"] and st["bai_bytes"] == len(bai) and st["bam_sort_device"] == device
    assert st["bam_sort_windows"] >= 1
    return raw, bam, refs


@pytest.mark.parametrize("oflag", ["-obh", "-obs"])
@pytest.mark.parametrize("name,reads", SETS)
def test_golden_sets_sorted(exe, work, index11, tmp_path, name, reads, oflag):
    q = os.path.join(work, reads); out = str(tmp_path / "sorted.bam")
    if oflag == "-obh":
        want = golden_lines(name)
    else:
        want = run(exe, ["-x", index11, "-q", q, "-oss", "stdout"])[0].decode().split("\n")
    _o, st = run(exe, ["-x", index11, "-q", q, oflag, out, "-obsort"])
    _raw, bam, refs = check_sorted_run(out, want, st, oflag, 0)
    for seq in range(bam.n_ref):                                                      # every whole sequence through the index
        assert ba.query(bam, refs, seq, 0, 1 << 29) == ba.brute(bam, seq, 0, 1 << 29)


# ---- a genome made here: three sequences, the second without a read ---------------------------------------------------------------------------------------------------
L1, L2, L3 = 160000, 3000, 5000                                                       # the first passes 2^17 + 2^14 = 147 456
READ = 300


def make_genome(d):
    rnd = random.Random(41)
    seqs = [("big", L1), ("empty", L2), ("small", L3)]
    text = {n: "".join(rnd.choice("ACGT") for _ in range(l)) for n, l in seqs}
    fa = os.path.join(d, "three.fa")
    with open(fa, "w") as f:
        for n, _l in seqs:
            f.write(">%s\n" % n)
            for i in range(0, len(text[n]), 50):
                f.write(text[n][i:i + 50] + "\n")
    # reads: exact pieces (a random genome has no repeats: each maps where it was cut) -- inside 16 384-base windows, across 16 384 boundaries, across 2^17,
    # at the ends of the sequences, two of them twice (equal keys: only stability decides), and shuffled so that arrival order is not coordinate order
    starts = [("big", p) for p in (0, 1000, 16384 - READ, 16384 - 150, 16384, 20000, 32768 - 1, 32768 - READ + 1, 49152 - 7, 65536 - 100, 81920 - 299, 100000, 114688 - 150,
                                   131072 - 150, 131072 - 1, 131072 - READ + 1, 131072, 140000, 147456 - 20, 150000, L1 - READ)]
    starts += [("small", p) for p in (0, 777, 2000, L3 - READ)]
    starts += [("big", 20000), ("big", 131072 - 150), ("small", 777)]                # the identical copies
    rnd.shuffle(starts)
    fq = os.path.join(d, "three_reads.fa")
    with open(fq, "w") as f:
        for i, (n, p) in enumerate(starts):
            f.write(">r%d_%s_%d\n%s\n" % (i, n, p, text[n][p:p + READ]))
    return fa, fq, starts


@pytest.fixture(scope="module")
def three(exe, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("three"))
    fa, fq, starts = make_genome(d)
    subprocess.check_call([exe, "-g", fa, "-L", "11"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.join(d, "three.X11_01_65525S"), fq, starts


def regions_agree(bam, refs, lengths):
    """query == brute over the regions the index can get wrong; returns how many regions had records."""
    hits = 0
    def same(seq, beg, end):
        nonlocal hits
        got, want = ba.query(bam, refs, seq, beg, end), ba.brute(bam, seq, beg, end)
        assert got == want, (seq, beg, end, got, want)
        hits += bool(want)
    for seq, length in enumerate(lengths):
        same(seq, 0, length)
        for w in range(0, length, 16384):                                             # every 16 384-aligned window, and it with its two neighbours
            same(seq, w, min(w + 16384, length)); same(seq, max(0, w - 16384), min(w + 2 * 16384, length))
    for ref, pos, end, _bin, _s, _e in bam.records:                                   # the single bases at a record's edges and just outside
        for p in (pos - 1, pos, end - 1, end):
            if p >= 0:
                same(ref, p, p + 1)
        if pos > 0:
            same(ref, max(0, pos - 50), pos)                                          # a region that ends exactly where the record starts
    return hits


def test_three_sequences_regions(exe, three, tmp_path):
    index, fq, starts = three
    out = str(tmp_path / "three.bam")
    _o, st = run(exe, ["-x", index, "-q", fq, "-obh", out, "-obsort"])
    sam = run(exe, ["-x", index, "-q", fq, "-osh", "stdout"])[0].decode().split("\n")
    _raw, bam, refs = check_sorted_run(out, sam, st, "-obh", 0)
    assert len(bam.records) == len(starts)                                            # every read gave its one record
    assert sorted((("big", "empty", "small")[r[0]], r[1]) for r in bam.records) == sorted(starts)
    # the bin levels reached: 5 = inside a 16 384 window, 4 = across such a boundary inside 2^17, 3 = across 2^17
    levels = [ba.bin_level(r[3]) for r in bam.records]
    want_levels = [ba.bin_level(bo.reg2bin(p, p + READ)) for _n, p in starts]           # (from where the reads were cut, not from the file)
    assert (levels.count(5), levels.count(4), levels.count(3)) == (want_levels.count(5), want_levels.count(4), want_levels.count(3)) == (16, 8, 4), levels
    assert refs[1] == ([], []) and len(refs[0][1]) == ((L1 - 1) >> 14) + 1            # the empty sequence; the linear index reaches the last read's end
    assert regions_agree(bam, refs, (L1, L2, L3)) > 100
    assert ba.query(bam, refs, 1, 0, L2) == [] and ba.query(bam, refs, 1, 100, 200) == []
    # equal keys keep print order = read order: the copies' names in the order of the input
    text = bo.bam_to_sam(bam.raw)[0].split("\n")
    names = [l.split("\t")[0] for l in text if l and not l.startswith("@")]
    for n, p in (("big", 20000), ("big", 131072 - 150), ("small", 777)):
        twins = [int(x.split("_")[0][1:]) for x in names if x.endswith("_%s_%d" % (n, p))]
        assert len(twins) == 2 and twins == sorted(twins), twins


def test_stream_does_not_depend_on_batches_contexts_threads(exe, work, index11, three, tmp_path):
    for index, q in ((index11, os.path.join(work, "rchim.fa")), three[:2]):
        out = str(tmp_path / "b.bam"); streams = {}
        for extra in ([], ["-batch", "1"], ["-batch", "7"], ["-ctx", "1"], ["-ctx", "3", "-batch", "5"], ["-t", "1"], ["-t", "4", "-batch", "3"]):
            _o, st = run(exe, ["-x", index, "-q", q, "-obh", out, "-obsort"] + extra, env={"YTEST_DEVICES": "1"})
            data = open(out, "rb").read()
            raw = bo.read_file(data)[0]
            ba.check_contract(data, open(out + ".bai", "rb").read())
            # (-t is echoed in the header's @PG line; -batch and -ctx are not: the whole stream is the same)
            streams[" ".join(extra)] = bo.records_of(raw) if "-t" in extra else raw
        assert streams["-batch 1"] == streams["-batch 7"] == streams[""] == streams["-ctx 1"] == streams["-ctx 3 -batch 5"]
        assert streams["-t 1"] == streams["-t 4 -batch 3"] == bo.records_of(streams[""])


def test_argument_errors_and_untouched_unsorted_output(exe, work, index11, tmp_path):
    q = os.path.join(work, "r100.fa"); out = str(tmp_path / "e.bam")
    base = ["-x", index11, "-q", q]
    for args, word in ((base + ["-obsort"], "-obh or -obs"), (base + ["-obh", out, "-o8", out, "-obsort"], "-obh or -obs"), (base + ["-obsort", "-obh", out, "-osh", out], "-obh or -obs"),
                       (base + ["-obs", out, "-oss", out, "-obsort"], "-obh or -obs"), (base + ["-obh", "stdout", "-obsort"], "standard output"),
                       (base + ["-obh", "-stdout", "-obsort"], "standard output"), (base + ["-obh", out, "-sortmem", "4"], "-sortmem needs -obsort"),
                       (base + ["-obh", out, "-obsort", "-sortmem", "0"], "at least 1"), (["-g", os.path.join(work, "genome_small.fa"), "-obsort"], "index creation")):
        rc, err = run(exe, args, ok=False)
        assert rc == 2 and word in err, (args, rc, err[:300])
        assert not os.path.exists(out) and not os.path.exists(out + ".bai")
    assert "-obsort" in run(exe, [], ok=False)[1] and "spill" in run(exe, [], ok=False)[1]
    # the store is full: the run stops, names -sortmem and leaves nothing behind
    rc, err = run(exe, base + ["-obh", out, "-obsort", "-sortmem", "1"], env={"YAHA_SORTMEM_BYTES": "4096"}, ok=False)
    assert rc not in (0, 2) and "-sortmem" in err, (rc, err[-500:])
    assert not os.path.exists(out) and not os.path.exists(out + ".bai")
    # without the flag -obh is what it was: the golden SAM in arrival order, the old header, no index, no new keys in the stats line
    _o, st = run(exe, base + ["-obh", out])
    raw = check_bam(open(out, "rb").read(), golden_lines("r100_default"), st, "-obh")
    assert "SO:coordinate" not in bo.bam_to_sam(raw)[0] and "-obsort" not in bo.bam_to_sam(raw)[0]
    assert not os.path.exists(out + ".bai") and "bam_sorted_records" not in st and "bai_bytes" not in st
    # ... and with it the same records, reordered
    _o, st = run(exe, base + ["-obh", out, "-obsort", "-sortmem", "1"])
    raw2 = check_sorted_run(out, golden_lines("r100_default"), st, "-obh", 0)[0]
    assert len(bo.records_of(raw2)) == len(bo.records_of(raw))


# ---- the index routines and the host's ordering as a program of their own -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("bai"); src = os.path.join(FIX, "bai_driver.cpp")
    plain, san = str(d / "bai_driver"), str(d / "bai_driver_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", plain, src])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", san, src])
    return plain, san


def test_index_driver_plain_and_sanitized(drivers, tmp_path):
    rnd = random.Random(53)
    # a few thousand entries over five sequences (one of them without any): all bin levels, long records over many windows, many equal keys, more than a block
    many = []
    for _ in range(3000):
        ref = rnd.choice((0, 0, 0, 2, 3, 4)); kind = rnd.random()
        pos = rnd.randrange(0, 1 << 16) if kind < 0.5 else rnd.randrange(0, (1 << 29) - 70000000)
        span = rnd.choice((0, 1, 50, 300, 16384, 20000)) if kind < 0.9 else rnd.randrange(1, 70000000)
        many.append((ref, rnd.choice((pos, pos, 12345)), span))
    for name, entries, n_ref in (("many", many, 5), ("none", [], 2), ("one", [(1, 16383, 2)], 3)):
        src, dst = str(tmp_path / (name + ".txt")), str(tmp_path / (name + ".bam"))
        open(src, "w").write("".join("%d %d %d\n" % e for e in entries))
        outs = []
        for exe in drivers:
            p = subprocess.run([exe, src, str(n_ref), dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1"))
            assert p.returncode == 0, (name, p.stderr.decode()[-2000:])
            outs.append((open(dst, "rb").read(), open(dst + ".bai", "rb").read()))
            assert json.loads(p.stdout)["records"] == len(entries)
        assert outs[0] == outs[1]                                                     # the two builds write the same bytes
        bam, refs = ba.check_contract(*outs[0])
        assert len(refs) == n_ref and len(bam.records) == len(entries)
        # the ordering is stable: a record's name is its arrival number, and among equal keys the names ascend
        names = [int(bam.raw[r[4] + 36:bam.raw.index(b"\0", r[4] + 36)]) for r in bam.records]
        assert [(entries[i][0], entries[i][1]) for i in names] == [(r[0], r[1]) for r in bam.records]
        assert all(a < b for (a, ka), (b, kb) in zip(zip(names, bam.records), zip(names[1:], bam.records[1:])) if ka[:2] == kb[:2])
        if name == "many":
            assert {ba.bin_level(r[3]) for r in bam.records} == {0, 1, 2, 3, 4, 5} and len(bam.block_at) > 2
            assert refs[1] == ([], []) and len(set(r[:2] for r in bam.records)) < len(bam.records)
            rq = random.Random(59)
            for _ in range(300):
                r = bam.records[rq.randrange(len(bam.records))]
                for beg, end in ((r[1], r[1] + 1), (r[2] - 1, r[2]), (r[2], r[2] + 1), (max(0, r[1] - 1), r[1]), (r[1] & ~16383, (r[1] & ~16383) + 16384)):
                    assert ba.query(bam, refs, r[0], beg, end) == ba.brute(bam, r[0], beg, end), (r, beg, end)
        if name == "none":
            assert refs == [([], []), ([], [])]
        if name == "one":
            assert [b for b, _c in refs[1][0]] == [585, ba.PSEUDO_BIN] and len(refs[1][1]) == 2
