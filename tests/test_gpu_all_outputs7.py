"""GPU tier: all seven side outputs (-ocov -oev -opu -obp -oid -oep -osnv) beside the main one in ONE run of the command line.  Each side file of the combined
run equals, byte for byte, the file of a run with that option alone -- the SNV calls share the -opu track's device array in the combined run and have one of
their own alone, and the pileup's table is written before the calls' folds touch the array --, the device did the work for every output, and the stats line is
the single-option runs' keys put together in the list's order.  What each file must contain is the business of the option's own tests."""
import functools
import json
import os
import subprocess

import pytest

import yaha_amd as ya
from conftest import golden_lines, strip_pg

pytestmark = pytest.mark.gpu

SIDE = [("-ocov", "cov"), ("-oev", "ev"), ("-opu", "pu"), ("-obp", "bp"), ("-oid", "id"), ("-oep", "ep"), ("-osnv", "snv")]
DEVICE_KEYS = ["depth_device_records", "events_device_records", "pileup_device_records", "bp_device_reads", "indel_device_records", "eprofile_device_records", "snv_on_device"]
# (few alleles of this read set are carried by two records, and its reads are simulated from the reference itself: the defaults could leave the files empty)
OPTION_ARGS = {"-oid": ["-idmin", "1"], "-osnv": ["-snvmin", "1", "-snvdp", "1", "-snvqual", "0"]}


def _cli(index11, reads, d, opts, extra=()):
    """One run into directory d (made here); returns the stats of the run."""
    os.makedirs(d)
    args = [ya.CLI_PATH, "-x", index11, "-q", reads, "-osh", os.path.join(d, "out.sam")] + [x for o, n in opts for x in [o, os.path.join(d, n)] + OPTION_ARGS.get(o, [])]
    p = subprocess.run(args + list(extra), env=dict(os.environ, YAHA_STATS="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    assert "state check" not in err, err[-2000:]
    return json.loads([l for l in err.split("\n") if l.startswith("[yaha] stats ")][0][len("[yaha] stats "):])


@functools.lru_cache(maxsize=None)
def _alone(index11, reads, root):
    """The runs with one option each and the one without: every side file's bytes, and the keys each run adds to those of the plain run."""
    base = list(_cli(index11, reads, os.path.join(root, "plain"), []))
    files, keys = {}, {}
    for o, n in SIDE:
        d = os.path.join(root, "alone_" + n)
        st = list(_cli(index11, reads, d, [(o, n)]))
        assert st[:len(base)] == base
        files[n], keys[n] = open(os.path.join(d, n), "rb").read(), st[len(base):]
        assert files[n] and keys[n]
    return base, files, keys


@pytest.mark.parametrize("extra", [["-ctx", "1"], ["-ctx", "3", "-batch", "17"]], ids=["ctx1", "ctx3_batch17"])
def test_all_seven_side_outputs_in_one_run(work, index11, tmp_path_factory, tmp_path, extra):
    q = os.path.join(work, "rsv.fa")
    base, files, keys = _alone(index11, q, str(tmp_path_factory.getbasetemp() / "all_outputs7_rsv"))
    assert keys["snv"] == ["snv_calls", "snv_het", "snv_hom", "snv_on_device", "snv_folded_slots"]
    calls = [l for l in files["snv"].decode().split("\n") if l and not l.startswith("#")]
    assert any("\t0/1:" in l for l in calls) and any("\t1/1:" in l for l in calls)                 # an empty file proves nothing
    d = str(tmp_path / "all")
    st = _cli(index11, q, d, SIDE, extra)
    for _o, n in SIDE:
        assert open(os.path.join(d, n), "rb").read() == files[n], n
    assert all(st[k] > 0 for k in DEVICE_KEYS) and st["indel_lost"] == 0 and st["snv_calls"] == len(calls), st
    assert list(st) == base + [k for _o, n in SIDE for k in keys[n]]
    assert strip_pg(open(os.path.join(d, "out.sam")).read()) == golden_lines("rsv_default")
