"""GPU tier: every side output (-ocov -oev -opu -obp -oid) beside the main one in ONE run of the command line.  The run driver knows the outputs as a list
(host/yaha_host.h SideOutput, RecordSink): output k is bit k of a batch's mask and owns slot k of every batch object, and the device stages of all five sit
behind one post-filter.  Here each side file of the combined run equals, byte for byte, the file of a run with that option alone, the device did the work for
every output, and the stats line is the single-option runs' keys put together in the list's order -- with SAM text and with a sorted BAM as the main output,
with one context and with three contexts on small batches.  What each file must contain is the business of the option's own tests."""
import functools
import json
import os
import subprocess

import pytest

import yaha_amd as ya
from conftest import golden_lines, strip_pg

pytestmark = pytest.mark.gpu

SIDE = [("-ocov", "cov"), ("-oev", "ev"), ("-opu", "pu"), ("-obp", "bp"), ("-oid", "id")]
DEVICE_KEYS = ["depth_device_records", "events_device_records", "pileup_device_records", "bp_device_reads", "indel_device_records"]
SORTED = ["-obs", "-obsort"]


def _cli(index11, reads, d, main, opts, extra=()):
    """One run into directory d (made here); returns the stats of the run."""
    os.makedirs(d)
    out = os.path.join(d, "out.bam" if main == SORTED else "out.sam")
    args = [ya.CLI_PATH, "-x", index11, "-q", reads] + ([main[0], out] + main[1:] if main == SORTED else ["-osh", out]) + [x for o, n in opts for x in (o, os.path.join(d, n))]
    if ("-oid", "id") in list(opts):
        args += ["-idmin", "1"]                                               # (few alleles of these read sets are carried by two records: the default could leave the file empty)
    p = subprocess.run(args + list(extra), env=dict(os.environ, YAHA_STATS="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    assert "state check" not in err, err[-2000:]
    return json.loads([l for l in err.split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])


@functools.lru_cache(maxsize=None)
def _alone(index11, reads, root):
    """The runs with one option each, and the two without a side option: every side file's bytes, and the keys each run adds to those of the plain SAM run."""
    base = list(_cli(index11, reads, os.path.join(root, "plain"), "sam", []))
    files, keys = {}, {}
    for o, n in SIDE:
        d = os.path.join(root, "alone_" + n)
        st = list(_cli(index11, reads, d, "sam", [(o, n)]))
        assert st[:len(base)] == base
        files[n], keys[n] = open(os.path.join(d, n), "rb").read(), st[len(base):]
        assert files[n] and keys[n]
    st = list(_cli(index11, reads, os.path.join(root, "plain_sorted"), SORTED, []))
    assert st[:len(base)] == base
    return base, files, keys, st[len(base):]


@pytest.mark.parametrize("main", ["sam", SORTED], ids=["sam", "sorted_bam"])
@pytest.mark.parametrize("extra", [["-ctx", "1"], ["-ctx", "3", "-batch", "17"]], ids=["ctx1", "ctx3_batch17"])
@pytest.mark.parametrize("name,reads", [("rchim_default", "rchim.fa"), ("rsv_default", "rsv.fa")])
def test_all_side_outputs_in_one_run(work, index11, tmp_path_factory, tmp_path, name, reads, extra, main):
    q = os.path.join(work, reads)
    base, files, keys, bam_keys = _alone(index11, q, str(tmp_path_factory.getbasetemp() / ("all_outputs_" + name)))
    d = str(tmp_path / "all")
    st = _cli(index11, q, d, main, SIDE, extra)
    for _o, n in SIDE:
        assert open(os.path.join(d, n), "rb").read() == files[n], n
    assert all(st[k] > 0 for k in DEVICE_KEYS) and st["indel_lost"] == 0, st
    assert list(st) == base + [k for _o, n in SIDE for k in keys[n]] + (bam_keys if main == SORTED else [])
    if main == SORTED:
        assert st["bam_sorted_records"] == st["bam_records"] > 0 and os.path.getsize(os.path.join(d, "out.bam.bai")) == st["bai_bytes"] > 0
    else:
        assert strip_pg(open(os.path.join(d, "out.sam")).read()) == golden_lines(name)
