"""GPU tier: BGZF blocks deflated on the device (device/bgzf_stage.h behind ygpu_bgzf_*, yaha_amd.Bgzf) and BAM output of the command line through them.
Every output goes through the strict reader of tests/bam_oracle.py (framing, one final deflate block that zlib inflates exactly, ISIZE, CRC-32), through
gzip.decompress with the end-of-file block appended, and is made a second time: the same bytes.  The byte strings are the smallest at which the kernel can
still go wrong: every length around the four-byte hash, the 64-lane wave, the 256-position tile and the 65 280-byte payload, runs (distance 1, overlapping
copies of length 258), the distance limit and one past it, bytes that do not compress (the stored form), and real BAM records (matches across tiles).
And every output is compared byte for byte with tests/bgzf_model.py: the device's blocks are a pure function of the payload (tiles of 256, the table of
earlier tiles, the candidate and then distance 1, greedy), which the model restates from the written contract; tests/test_bam_cpu.py shows from the model
alone that the inputs reach every length, every distance code, the fullest and the empty tile."""
import gzip
import json
import os
import random
import subprocess

import pytest

import bam_oracle as bo
import bgzf_model as bm
import yaha_amd as ya
from conftest import golden_lines
from test_bam_cpu import DEVICE_BLOCKS, blocks_are_modelled, byte_sets, check_bam

pytestmark = pytest.mark.gpu
P = bo.PAYLOAD_MAX
CAP = 3 * P + 17 + 300000


def _cli(index11, reads, out, extra=(), env=None):
    p = subprocess.run([ya.CLI_PATH, "-x", index11, "-q", reads, "-obh", out] + list(extra), env=dict(os.environ, YAHA_STATS="1", **(env or {})),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    st = json.loads([l for l in err.split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])
    return open(out, "rb").read(), st


@pytest.fixture(scope="module")
def host_runs(work, index11, tmp_path_factory):
    """name -> (the BAM file, its decompressed stream, the stats) of a run whose blocks the HOST's encoder made (YAHA_HOST_BGZF=1)."""
    d = tmp_path_factory.mktemp("hostbam"); out = {}
    for name, reads in (("r1k_default", "r1k.fa"), ("rq_default", "rq.fq")):
        data, st = _cli(index11, os.path.join(work, reads), str(d / (name + ".bam")), env={"YAHA_HOST_BGZF": "1"})
        out[name] = (data, check_bam(data, golden_lines(name), st, "-obh"), st)
        assert blocks_are_modelled(data[:-28], st["bam_blocks"]) == st["bam_blocks"]  # every block: the host model's of its own payload
    return out


@pytest.fixture(scope="module")
def bgzf():
    with ya.Bgzf(CAP) as b:
        yield b


def _check(b, data, name):
    out = b.compress(data)
    payload, bl = bo.read_stream(out)
    assert payload == data, name
    assert gzip.decompress(out + ya.Bgzf.EOF) == data, name
    assert len(bl) == -(-len(data) // P) and len(out) <= ya.Bgzf.bound(len(data))
    assert all(size <= min(bo.BLOCK_MAX, 18 + 5 + len(pl) + 8) for pl, size, _st in bl), name      # never larger than the stored form
    assert b.compress(data) == out, name                                                            # the same input, the same bytes
    assert out == bm.stream(data, bm.device_tokens, DEVICE_BLOCKS), "%s: not the bytes the contract gives" % name
    return out, bl


def test_byte_strings(bgzf, host_runs):
    real = host_runs["rq_default"][1][:300000]                                        # real BAM records with qualities
    # the handle's whole capacity in random bytes first: every later, shorter input has these (and its predecessors') bytes behind its end in the device's
    # input buffer, as a batch has the previous batch's in BgzfPacker's handle -- the model never sees them, so equality shows they do not matter
    _check(bgzf, random.Random(29).randbytes(CAP), "the capacity in random bytes")
    outs = {}
    for name, data in sorted(byte_sets(real).items()):
        outs[name] = _check(bgzf, data, name)
    assert outs["acgt_0"][0] == b""                                                   # no input, no block (the end-of-file block is the writer's)
    # a literal, then 254 matches of length 258 (the last one shorter), 31 bits each at the very most, and the framing
    assert len(outs["zeros"][0]) < 254 * 31 // 8 + 64
    # what does not compress is stored: 18 + 5 + 65 280 + 8 bytes, inside the slot of 65 536
    assert [(size, st) for _p, size, st in outs["random"][1]] == [(P + 31, True)]
    assert [st for _p, _s, st in outs["period_32769"][1]] == [True]                  # one past the distance limit no match may be used: random bytes, stored
    print("period 32768: %d bytes, period 32769: %d bytes" % (len(outs["period_32768"][0]), len(outs["period_32769"][0])))
    assert len(outs["period_32768"][0]) <= len(outs["period_32769"][0])
    assert len(outs["bam"][0]) < len(real) and not any(st for _p, _s, st in outs["bam"][1])
    print("real BAM records: %d -> %d bytes on the device, zlib level 1: %d" % (len(real), len(outs["bam"][0]), len(__import__("zlib").compress(real, 1))))


def test_more_blocks_than_one_trip_of_the_offsets_kernel():
    """k_bgzf_offsets sums the sizes 256 blocks a trip and carries the total: streams of exactly 256, 257 and 513 payloads -- three full ones (zeros: about
    0.6 KB a block; random text: about 60 KB; random bytes: stored, 65 311) in a seeded order, a short one behind them for 257 and 513 -- against the
    concatenation of the modelled blocks, with exactly ygpu_bgzf_bound bytes of room."""
    sets = byte_sets(); kinds = [sets["zeros"], sets["text_%d" % P], sets["random"]]
    sizes = [len(bm.stream(k, bm.device_tokens, DEVICE_BLOCKS)) for k in kinds]
    assert sizes[0] < 1024 and 40000 < sizes[1] < P and sizes[2] == P + 31, sizes
    rnd = random.Random(31)
    with ya.Bgzf(512 * P + 1000) as b:
        for n_full, tail in ((512, 1000), (256, 777), (256, 0)):                      # the longest first: the shorter ones meet its bytes behind their end
            order = [rnd.randrange(3) for _ in range(n_full)]
            assert set(order) == {0, 1, 2}
            data = b"".join(kinds[k] for k in order) + sets["text_%d" % P][5000:5000 + tail]
            n_blocks = n_full + (tail > 0); cap = ya.Bgzf.bound(len(data))
            assert cap == n_blocks * bo.BLOCK_MAX and len(data) == n_full * P + tail
            out = b.compress(data, out_cap=cap)
            want = bm.stream(data, bm.device_tokens, DEVICE_BLOCKS)
            assert len(out) == len(want) and out == want, "%d blocks" % n_blocks
            assert len(bm.split_blocks(out)) == n_blocks and bo.read_stream(out)[0] == data


def test_errors_leave_the_handle_usable():
    data = bytes(random.Random(5).choice(b"ACGT") for _ in range(1000))
    with ya.Bgzf(1000) as b:
        with pytest.raises(RuntimeError, match="-1 .*opened for 1000"):
            b.compress(data + b"A")
        with pytest.raises(RuntimeError, match="-1 .*out_cap"):
            b.compress(data, out_cap=ya.Bgzf.bound(len(data)) - 1)
        _check(b, data, "after the errors")
        with ya.Bgzf(70000) as b2:                                                    # a second handle beside the first
            _check(b2, data * 70, "second handle")
            _check(b, data, "first handle again")
    with pytest.raises(RuntimeError, match="ygpu_bgzf_open failed"):
        ya.Bgzf(1000, device=9999)


@pytest.mark.parametrize("name,reads", [("r1k_default", "r1k.fa"), ("rq_default", "rq.fq")])
def test_command_line_bam_from_device_blocks(work, index11, tmp_path, host_runs, name, reads):
    q = os.path.join(work, reads); out = str(tmp_path / "out.bam")
    _file, raw_host, st_host = host_runs[name]
    assert st_host["bam_device_batches"] == 0 and st_host["bam_host_batches"] > 0
    for extra in ([], ["-ctx", "2", "-batch", "64"]):
        data, st = _cli(index11, q, out, extra)
        # the decompressed records: the host encoder's run byte for byte, whatever the batches (the headers differ in the file name of their @PG line)
        assert bo.records_of(check_bam(data, golden_lines(name), st, "-obh")) == bo.records_of(raw_host)
        assert st["bam_device_batches"] > 0 and st["bam_host_batches"] == 0, st
        # every block is the block one of the two models makes of its own payload: the header's blocks the host's, every later one the device's
        raw = bo.read_file(data)[0]; n_header = -(-(len(raw) - len(bo.records_of(raw))) // P)
        assert 0 < n_header < blocks_are_modelled(data[:-28], n_header) == st["bam_blocks"]
