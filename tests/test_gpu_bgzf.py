"""GPU tier: BGZF blocks deflated on the device (device/bgzf_stage.h behind ygpu_bgzf_*, yaha_amd.Bgzf) and BAM output of the command line through them.
Every output goes through the strict reader of tests/bam_oracle.py (framing, one final deflate block that zlib inflates exactly, ISIZE, CRC-32), through
gzip.decompress with the end-of-file block appended, and is made a second time: the same bytes.  The byte strings are the smallest at which the kernel can
still go wrong: every length around the four-byte hash, the 64-lane wave, the 256-position tile and the 65 280-byte payload, runs (distance 1, overlapping
copies of length 258), the distance limit and one past it, bytes that do not compress (the stored form), and real BAM records (matches across tiles)."""
import gzip
import json
import os
import random
import subprocess

import pytest

import bam_oracle as bo
import yaha_amd as ya
from conftest import golden_lines
from test_bam_cpu import byte_sets, check_bam

pytestmark = pytest.mark.gpu
P = bo.PAYLOAD_MAX


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
    return out


@pytest.fixture(scope="module")
def bgzf():
    with ya.Bgzf(3 * P + 17 + 300000) as b:
        yield b


def _check(b, data, name):
    out = b.compress(data)
    payload, bl = bo.read_stream(out)
    assert payload == data, name
    assert gzip.decompress(out + ya.Bgzf.EOF) == data, name
    assert len(bl) == -(-len(data) // P) and len(out) <= ya.Bgzf.bound(len(data))
    assert all(size <= min(bo.BLOCK_MAX, 18 + 5 + len(pl) + 8) for pl, size, _st in bl), name      # never larger than the stored form
    assert b.compress(data) == out, name                                                            # the same input, the same bytes
    return out, bl


def test_byte_strings(bgzf, host_runs):
    real = host_runs["rq_default"][1][:300000]                                        # real BAM records with qualities
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
