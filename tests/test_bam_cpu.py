"""CPU tier: BAM output (-obh / -obs) through the whole command line -- host sources, main.cpp and the test double tests/fixtures/oracle_device.cpp, which has no
ygpu_bgzf_*: every block here comes from the host's encoder (csrc/bgzf_core.h, the source the device kernel compiles as well) -- and that encoder alone as a
program of its own (tests/fixtures/bgzf_driver.cpp), plainly and under AddressSanitizer + UBSan.  Everything is judged by tests/bam_oracle.py: a strict BGZF
reader, and the SAM text a BAM stream stands for against the golden SAM of the same options."""
import glob
import gzip
import json
import os
import random
import subprocess

import pytest

import bam_oracle as bo
from conftest import GOLDEN, ROOT, golden_lines, strip_pg

HOST = os.path.join(ROOT, "yaha_amd", "csrc", "host")
SRCS = sorted(glob.glob(os.path.join(HOST, "*.cpp"))) + [os.path.join(ROOT, "yaha_amd", "csrc", "main.cpp"), os.path.join(ROOT, "tests", "fixtures", "oracle_device.cpp"),
                                                          os.path.join(ROOT, "oracle", "hotpath.cpp")]
SETS = [("r1k_default", "r1k.fa"), ("rchim_default", "rchim.fa"), ("rq_default", "rq.fq"), ("r100_default", "r100.fa")]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bam") / "yaha_double")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-o", out] + SRCS)
    return out


def _run(exe, args, env=None):
    p = subprocess.run([exe] + args, env=dict(os.environ, YAHA_STATS="1", YAHA_CPUS="6", **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    st = json.loads([l for l in p.stderr.decode().split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])
    return p.stdout, st


def check_bam(data, want_lines, st, oflag):
    """data: a whole BAM file; want_lines: the SAM of the same options (header lines and records, @PG included or not)."""
    raw, bl = bo.read_file(data)
    sam, refs, kinds = bo.bam_to_sam(raw)
    got = sam.split("\n")
    pg = [l for l in got if l.startswith("@PG")]
    assert len(pg) == 1 and " %s " % oflag in pg[0]                                   # the option actually used
    assert strip_pg(sam) == [bo.normalise_sam_seq(l) for l in want_lines if not l.startswith("@PG")]
    sq = [l.split("\t") for l in got if l.startswith("@SQ")]
    assert refs == [(f[1][3:], int(f[2][3:])) for f in sq] and refs                   # the reference list is the header's
    for k in kinds:                                                                   # integer tags: the smallest unsigned type that holds the value
        assert k and all(typ == bo.smallest_unsigned(v) for typ, v in k.values())
    n_rec = len([l for l in got if l and not l.startswith("@")])
    assert st["bam_records"] == n_rec > 0 and st["bam_bytes_raw"] == len(raw) and st["bam_bytes_written"] == len(data)
    assert st["bam_blocks"] == len(bl) and st["bam_blocks_stored"] == sum(1 for _p, _s, stored in bl if stored)
    return raw


@pytest.mark.parametrize("name,reads", SETS)
def test_command_line_bam_is_the_golden_sam(exe, work, index11, tmp_path, name, reads):
    q = os.path.join(work, reads); out = str(tmp_path / "out.bam")
    # hard clipping against the reference's golden output
    _o, st = _run(exe, ["-x", index11, "-q", q, "-obh", out])
    raw1 = check_bam(open(out, "rb").read(), golden_lines(name), st, "-obh")
    assert st["bam_device_batches"] == 0 and st["bam_host_batches"] > 0              # (the double has no device encoder)
    # the blocks follow -batch and -ctx, the decompressed stream does not
    _o, st = _run(exe, ["-x", index11, "-q", q, "-obh", out, "-ctx", "2", "-batch", "64"], env={"YTEST_DEVICES": "1"})
    data = open(out, "rb").read()
    assert check_bam(data, golden_lines(name), st, "-obh") == raw1
    _o, st1 = _run(exe, ["-x", index11, "-q", q, "-obh", out, "-ctx", "1"])
    assert bo.read_file(open(out, "rb").read())[0] == raw1
    # soft clipping against -oss of the same binary; to standard output
    sam, _st = _run(exe, ["-x", index11, "-q", q, "-oss", "stdout"])
    bam, st = _run(exe, ["-x", index11, "-q", q, "-obs", "-stdout", "-batch", "50"])
    check_bam(bam, sam.decode().split("\n"), st, "-obs")


def test_selectors_and_untouched_sam(exe, work, index11, tmp_path):
    q = os.path.join(work, "rchim.fa"); out = str(tmp_path / "o")
    # the last output selector wins, either way round
    sam, st = _run(exe, ["-x", index11, "-q", q, "-obh", out, "-osh", "stdout"])
    assert strip_pg(sam.decode()) == golden_lines("rchim_default") and "bam_records" not in st
    bam, st = _run(exe, ["-x", index11, "-q", q, "-osh", out, "-obh", "stdout"])
    check_bam(bam, golden_lines("rchim_default"), st, "-obh")
    # a track cannot share standard output with the BAM either
    p = subprocess.run([exe, "-x", index11, "-q", q, "-obh", "stdout", "-ocov", "stdout"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 2 and b"standard output" in p.stderr
    assert b"-obh" in subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE).stderr


# ---- the host's encoder as a program of its own ---------------------------------------------------------------------------------------------------------------------
def byte_sets(real_bam=None):
    """The inputs both encoders are tried on (tests/test_gpu_bgzf.py feeds the device the same ones): name -> bytes."""
    rnd = random.Random(7); P = bo.PAYLOAD_MAX
    sets = {}
    for n in list(range(0, 71)) + [255, 256, 257, 258, 259, 260, 511, 512, 513]:
        sets["acgt_%d" % n] = bytes(rnd.choice(b"ACGT") for _ in range(n))
    text = bytes(rnd.choice(b"ACGTN\t0123456789:") for _ in range(3 * P + 17))
    for n in (P - 1, P, P + 1, 3 * P + 17):
        sets["text_%d" % n] = text[:n]
    sets["zeros"] = bytes(P)
    base = random.Random(3).randbytes(32769)
    sets["period_32768"] = (base[:32768] * 2)[:P]
    sets["period_32769"] = (base * 2)[:P]
    sets["random"] = random.Random(1).randbytes(P)
    if real_bam is not None:
        sets["bam"] = real_bam
    return sets


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf"); src = os.path.join(ROOT, "tests", "fixtures", "bgzf_driver.cpp")
    plain, san = str(d / "bgzf_driver"), str(d / "bgzf_driver_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", plain, src])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", san, src])
    return plain, san


def test_host_encoder_on_byte_sets(drivers, tmp_path):
    with gzip.open(os.path.join(GOLDEN, "rq_default.out.gz"), "rb") as g:
        real = g.read()                                                               # (real alignment text: names, bases, qualities, tags)
    outs = {}
    for name, data in sorted(byte_sets(real).items()):
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bgzf")
        open(src, "wb").write(data)
        for exe in drivers:
            p = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1"))
            assert p.returncode == 0, (name, p.stderr.decode()[-2000:])
            got = open(dst, "rb").read()
            payload, bl = bo.read_file(got)
            assert payload == data, name
            assert gzip.decompress(got) == data
            info = json.loads(p.stdout)
            assert info["blocks"] == len(bl) == -(-len(data) // bo.PAYLOAD_MAX) and info["stored"] == sum(1 for _p, _s, st in bl if st)
            assert all(size <= min(bo.BLOCK_MAX, 18 + 5 + len(pl) + 8) for pl, size, _st in bl), name      # never larger than the stored form
            assert outs.setdefault(name, got) == got                                  # the two builds write the same bytes
    assert [st for _p, _s, st in bo.read_file(outs["random"])[1]] == [True]           # what does not compress is stored
    # a literal, then 254 matches of length 258 (the last one shorter), 31 bits each at the very most, and the framing of block and end-of-file block
    assert len(outs["zeros"]) < 254 * 31 // 8 + 64 + 28
    # at the distance limit some matches survive the table's collisions (a block is deflated only where that is smaller than stored) ...
    assert len(outs["period_32768"]) < len(outs["period_32769"])
    assert [st for _p, _s, st in bo.read_file(outs["period_32769"])[1]] == [True]     # ... one past it no match may be used: random bytes, stored
    assert len(outs["bam"]) < len(real)                                               # ASCII literals cost 8 bits, every repeated name or tag saves some
