"""GPU tier: the coordinate order of BAM records on the device (device/bamsort_stage.h behind ygpu_bamsort_*, yaha_amd.BamSort) and -obsort of the command line
through it.  The order is compared with numpy's stable argsort on key sets built for the radix sort's edges (one tile and its neighbours, several tiles, equal
keys, one pass of every kind, none at all, all eight); the windows with the records themselves in that order, and every block with tests/bgzf_model.py's
device block of its payload -- the file does not depend on segments, windows or batches.  The command line's files go through tests/bai_oracle.py."""
import json
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

import bai_oracle as ba
import bam_oracle as bo
import yaha_amd as ya
from conftest import golden_lines
from test_bam_cpu import blocks_are_modelled
from test_bamsort_cpu import L1, L2, L3, check_sorted_run, make_genome, regions_agree

pytestmark = pytest.mark.gpu
P = bo.PAYLOAD_MAX
BIG = 1 << 30


def T():
    return ya.BamSort.tile_keys()


def key_sets(n, rnd):
    """name -> (keys, radix passes the sort must run, or None where that depends on the draw)."""
    base = np.uint64(0x1122334455667788)
    r8 = rnd.integers(0, 256, n, dtype=np.uint64)
    varied = n >= 200                                                                 # (256 values drawn 200 times: more than one, whatever the seed)
    sets = {
        "equal": (np.full(n, 0x0123456789ABCDEF, dtype=np.uint64), 0),
        "two_values": (np.where(rnd.integers(0, 2, n) == 1, np.uint64(5 << 32 | 9), np.uint64(5 << 32 | 7)).astype(np.uint64), 1 if varied else None),
        "random64": (rnd.integers(0, 1 << 64, n, dtype=np.uint64), 8 if varied else None),
        "byte0": ((base & ~np.uint64(0xFF)) | r8, 1 if varied else None),
        "byte3": ((base & ~np.uint64(0xFF << 24)) | (r8 << np.uint64(24)), 1 if varied else None),
        "byte4": ((base & ~np.uint64(0xFF << 32)) | (r8 << np.uint64(32)), 1 if varied else None),
        "ascending": (np.arange(n, dtype=np.uint64) * np.uint64(3), None),
        "descending": (np.arange(n, dtype=np.uint64)[::-1].copy() * np.uint64(3), None),
        "last_differs": (np.concatenate([np.full(n - 1, 1000, dtype=np.uint64), np.array([3], dtype=np.uint64)]), 2 if n > 1 else 0),
        "digits_0_255": (np.where(np.arange(n) % 2 == 1, np.uint64(0x00FF), np.uint64(0xFF00)).astype(np.uint64) | (rnd.integers(0, 2, n, dtype=np.uint64) << np.uint64(16)), None),
    }
    return sets


@pytest.mark.parametrize("which", range(7))
def test_order_is_numpys_stable_order(which):
    t = T(); n = [1, 2, t - 1, t, t + 1, 3 * t + 1, 200000][which]
    rnd = np.random.default_rng(100 + which)
    for name, (keys, passes) in key_sets(n, rnd).items():
        if name == "two_values" and n == 2:
            keys = np.array([7, 7], dtype=np.uint64); passes = 0                      # n = 2 with equal keys
        with ya.BamSort(BIG, segment_bytes=1 << 20) as s:
            cut = n // 3                                                              # two appends: the arrays grow, the record numbers go on
            for a, b in ((0, cut), (cut, n)):
                if b > a:
                    s.append(bytes(b - a), keys[a:b], np.ones(b - a, dtype=np.uint32))
            perm = s.sort()
            want = np.argsort(keys, kind="stable")
            assert np.array_equal(perm, want), (name, n, np.flatnonzero(perm != want)[:5])
            if passes is not None:
                assert s.passes == passes, (name, n, s.passes)


def _segment_offsets(batches, segment_bytes):
    """Where every record lies in its segment, by the rule of include/yaha_hip.h: a batch goes behind the last one where it fits whole, else into a new segment
    (its own size when it is larger than a segment).  Returns (the offsets, the number of segments)."""
    offs, used, cap, n_seg = [], 0, 0, 0
    for batch in batches:
        size = sum(len(r) for r in batch)
        if n_seg == 0 or cap - used < size:
            n_seg += 1; cap = max(size, segment_bytes); used = 0
        for r in batch:
            offs.append(used); used += len(r)
    return offs, n_seg


def _run_store(batches, keys, segment_bytes, window_bytes):
    """The file bytes (all windows' blocks), the permutation, the windows' raw sizes, the segments."""
    with ya.BamSort(BIG, segment_bytes=segment_bytes, window_bytes=window_bytes) as s:
        at = 0
        for batch in batches:
            s.append(b"".join(batch), keys[at:at + len(batch)], np.array([len(r) for r in batch], dtype=np.uint32)); at += len(batch)
        perm = s.sort()
        out, raws = [], []
        for blocks, n_raw in s.windows():
            out.append(blocks); raws.append(n_raw)
        assert s.next() == (b"", 0)                                                   # the end stays the end
        return b"".join(out), perm, raws, s.info(ya.BamSort.SEGMENTS)


def _check_store(batches, keys, segment_bytes, window_bytes):
    recs = [r for b in batches for r in b]
    data, perm, raws, n_seg = _run_store(batches, keys, segment_bytes, window_bytes)
    want_perm = np.argsort(keys, kind="stable")
    assert np.array_equal(perm, want_perm)
    stream = b"".join(recs[i] for i in want_perm)
    payload, bl = bo.read_stream(data)
    assert payload == stream and b"".join(zlib.decompress(data[a:a + size][18:-8], -15) for a, size in _block_spans(data)) == stream
    assert all(len(p) == P for p, _s, _st in bl[:-1]) and sum(raws) == len(stream)
    assert blocks_are_modelled(data, 0) == len(bl) == -(-len(stream) // P)           # every block: the device model's of its payload, bit for bit
    # the same records in one batch with the default segment and window sizes: the same file
    again = _run_store([recs], keys, 0, 0)
    assert again[0] == data and np.array_equal(again[1], perm) and again[3] == 1
    return stream, perm, raws, n_seg


def _block_spans(data):
    at, out = 0, []
    while at < len(data):
        size = int.from_bytes(data[at + 16:at + 18], "little") + 1
        out.append((at, size)); at += size
    return out


def test_gather_and_deflate_incompressible_records():
    rnd = random.Random(61)
    small = [1, 2, 3, 4, 5, 35, 36, 37]
    fill = lambda k: [rnd.randrange(1, 10) for _ in range(k)]
    b1 = small + fill(150) + [20000, 20001, 9000]
    b2 = [65279, 65280, 65281, 70000]                                                 # a batch larger than a segment
    b3 = fill(150) + [20002, 20003, 45000] + small
    batches = [[rnd.randbytes(l) for l in b] for b in (b1, b2, b3)]
    n = sum(len(b) for b in batches)
    keys = np.random.default_rng(67).integers(0, 1 << 40, n, dtype=np.uint64)
    keys[5] = keys[200] = keys[n - 3]                                                 # equal keys among them
    seg, win = 100000, 2 * P
    stream, perm, raws, n_seg = _check_store(batches, keys, seg, win)
    src, want_seg = _segment_offsets(batches, seg)
    assert n_seg == want_seg == 3 and sum(len(r) for r in batches[1]) > seg
    assert len(raws) >= 4 and all(r == win for r in raws[:-1])
    # every source alignment meets every destination alignment, and records cross window and block boundaries
    lens = [len(r) for b in batches for r in b]
    dst = np.concatenate([[0], np.cumsum([lens[i] for i in perm])])
    assert {(src[i] % 4, int(dst[j]) % 4) for j, i in enumerate(perm)} == {(a, b) for a in range(4) for b in range(4)}
    assert any(int(dst[j]) // win != (int(dst[j + 1]) - 1) // win for j in range(len(perm)))
    assert any(int(dst[j + 1]) - int(dst[j]) > P for j in range(len(perm)))


def test_gather_and_deflate_compressible_records():
    """Records cut from a few 200-byte motifs: the matches run across record boundaries, through the same checks."""
    rnd = random.Random(71)
    motifs = [bytes(rnd.choice(b"ACGTN!#5I") for _ in range(200)) for _ in range(6)]
    def rec():
        out = b""
        for _ in range(rnd.randrange(1, 5)):
            m = rnd.choice(motifs); a = rnd.randrange(0, 100); out += m[a:a + rnd.randrange(50, 200 - a + 1)]
        return out
    batches = [[rec() for _ in range(400)] for _ in range(3)]
    n = 1200
    keys = np.random.default_rng(73).integers(0, 3000, n, dtype=np.uint64) | (np.random.default_rng(74).integers(0, 3, n, dtype=np.uint64) << np.uint64(32))
    stream, _perm, raws, n_seg = _check_store(batches, keys, 150000, 2 * P)
    assert n_seg >= 2 and len(raws) >= 2
    data = _run_store(batches, keys, 150000, 2 * P)[0]
    assert len(data) < len(stream) // 2 and not any(st for _p, _s, st in bo.read_stream(data)[1])


def test_errors():
    k = np.arange(10, dtype=np.uint64); l = np.full(10, 6000, dtype=np.uint32); data = bytes(60000)
    with ya.BamSort(250000, segment_bytes=64000) as s:                                # two segments of 64 000 fit beside the arrays (80 KB), a third does not
        s.append(data, k, l); s.append(data, k, l)
        with pytest.raises(ya.BamSortError, match="max_store_bytes") as e:
            s.append(data, k, l)
        assert e.value.code == -3                                                     # YGPU_ENOMEM
        assert s.info(ya.BamSort.RECORDS) == 20
    with ya.BamSort(BIG) as s:
        with pytest.raises(ya.BamSortError, match="not been sorted") as e:
            s.next()
        assert e.value.code == -1                                                     # YGPU_EINVAL
        s.append(data, k, l)
        with pytest.raises(ya.BamSortError, match="add up") as e:
            s.append(data[:-1], k, l)
        assert e.value.code == -1
        assert list(s.sort()) == list(range(10))
        with pytest.raises(ya.BamSortError, match="sorted already") as e:
            s.append(data, k, l)
        assert e.value.code == -1
        assert sum(n_raw for _b, n_raw in s.windows()) == 60000
    with ya.BamSort(BIG) as s:                                                        # an empty store sorts, and has no window
        assert len(s.sort()) == 0 and s.next() == (b"", 0) and s.passes == 0
    with pytest.raises(ya.BamSortError, match="ygpu_bamsort_open"):
        ya.BamSort(BIG, device=9999)


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------------------------
def _cli(index, reads, out, extra=(), env=None):
    p = subprocess.run([ya.CLI_PATH, "-x", index, "-q", reads, "-obh", out, "-obsort"] + list(extra), env=dict(os.environ, YAHA_STATS="1", **(env or {})),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    return json.loads([l for l in err.split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])


@pytest.fixture(scope="module")
def three_gpu(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("three_gpu"))
    fa, fq, _starts = make_genome(d)
    ya.build_index(["-g", fa, "-L", "11"])
    sam = subprocess.run([ya.CLI_PATH, "-x", os.path.join(d, "three.X11_01_65525S"), "-q", fq, "-osh", "stdout"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, check=True)
    return os.path.join(d, "three.X11_01_65525S"), fq, sam.stdout.decode().split("\n")


@pytest.mark.parametrize("which", ["golden", "three"])
def test_command_line_sorted_on_the_device(work, index11, three_gpu, tmp_path, which):
    if which == "golden":
        index, q, want, lengths = index11, os.path.join(work, "r1k.fa"), golden_lines("r1k_default"), None
    else:
        index, q, want = three_gpu; lengths = (L1, L2, L3)
    host_out, out = str(tmp_path / "host.bam"), str(tmp_path / "dev.bam")
    st_host = _cli(index, q, host_out, env={"YAHA_HOST_BAMSORT": "1"})
    raw_host, _b, _r = check_sorted_run(host_out, want, st_host, "-obh", 0)
    for extra in ([], ["-ctx", "3", "-batch", "5"]):
        st = _cli(index, q, out, extra)
        raw, bam, refs = check_sorted_run(out, want, st, "-obh", 1)
        assert bo.records_of(raw) == bo.records_of(raw_host)                          # (the headers differ in the file name of their @PG line)
        assert st["bam_sort_segments"] >= 1 and st["bam_sort_passes"] >= 1 and st["bam_device_batches"] == st["bam_sort_windows"]
        if lengths is None:
            lengths = [length for _n, length in bo.bam_to_sam(raw)[1]]
        assert regions_agree(bam, refs, lengths) > 10
        # every block: the header's the host model's, every record block the device model's of its payload
        data = open(out, "rb").read(); n_header = -(-(len(raw) - len(bo.records_of(raw))) // P)
        assert 0 < n_header < blocks_are_modelled(data[:-28], n_header) == st["bam_blocks"]
