"""BASECOUNT_BGZF=1 end to end: run() with the rows leaving as BGZF against the switch off.  The
exit status and the raised error are the same, the stream gunzips to the plain output byte for byte,
every block parses with at most 65,280 input bytes and the stream ends on the EOF block; regular
files at covered decimal places are compressed on the device (PLAN["bgzf"]), and the file is the same
bytes when the device formatter is made to decline everything, so that the kernels' host twin
compresses every reference.  The summary shapes stay plain text; the cohort command's --bgzf writes
DIR/X.tsv.gz."""
import gzip
import json
import os
import shutil
import subprocess
import sys

import pytest

from basecount_amd import bgzf

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")

# the CLI, then what main.PLAN recorded, on stderr; BGZF_TEST_DECLINE: no reference is covered by the
# device formatter, so every one takes the host formatter and the host twin; BGZF_TEST_SLICE: the
# formatter's slice (2^22 positions) made small, so that a golden's reference goes through in slices
DRIVER = """
import json, os, sys
from basecount_amd import main
if os.environ.get("BGZF_TEST_DECLINE"):
    main.D.fmt_supported = lambda dp, names: False
if os.environ.get("BGZF_TEST_SLICE"):
    main.FORMAT_SLICE = int(os.environ["BGZF_TEST_SLICE"])
try:
    main.run(sys.argv[1:])
finally:
    sys.stdout.flush()
    print("PLAN_JSON " + json.dumps({k: main.PLAN.get(k) for k in ("bgzf", "format")}), file=sys.stderr)
"""
CLEARED = ("BASECOUNT_BGZF", "BASECOUNT_DEVICE_FORMAT", "BASECOUNT_DEVICE_SELECT", "BASECOUNT_DEVICE_DECODE",
           "BASECOUNT_DEVICE_INFLATE", "BASECOUNT_BATCH_RECORDS", "BASECOUNT_LONG_READS", "BASECOUNT_GROUP_REFS",
           "BGZF_TEST_DECLINE", "BGZF_TEST_SLICE")


def run_cli(argv, **env):
    e = dict(os.environ, PYTHONPATH=REPO, PYTHONHASHSEED="0")
    for k in CLEARED:
        e.pop(k, None)
    e.update(env)
    p = subprocess.run([sys.executable, "-c", DRIVER] + argv, cwd=GOLDEN, env=e, capture_output=True, timeout=300)
    plan, rest = None, []
    for line in p.stderr.decode().replace("PLAN_JSON", "\nPLAN_JSON").splitlines():
        if line.startswith("PLAN_JSON "):
            plan = json.loads(line[len("PLAN_JSON "):])
        elif line:
            rest.append(line)
    return p, plan, rest


def assert_stream(data: bytes, plain: bytes):
    """A whole BGZF stream of ``plain``."""
    assert gzip.decompress(data) == plain
    bl = bgzf.blocks(data)
    assert all(isize <= 65280 and bsize <= 65536 for _, bsize, isize, _ in bl)
    assert data[-28:] == bgzf.EOF and bl[-1][2] == 0
    assert sum(isize for _, _, isize, _ in bl) == len(plain)


SHAPES = {"default": [], "long": ["--long-format"], "shown": ["--show-n-bases"], "dp5": ["--decimal-places", "5"],
          "chunk7": ["--chunk-size", "7"]}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("bam", ["c1.bam", "mixed.bam", "edge.bam", "ont/ont.bam"])
def test_the_stream_gunzips_to_the_plain_output(bam, shape):
    argv = [bam] + SHAPES[shape]
    off, plan_off, err_off = run_cli(argv)
    on, plan_on, err_on = run_cli(argv, BASECOUNT_BGZF="1")
    assert on.returncode == off.returncode == 0, (err_off[-1:], err_on[-1:])
    assert err_on[-1:] == err_off[-1:]
    assert plan_off["bgzf"] is None  # the switch off: nothing recorded
    assert len(off.stdout) > 100
    assert_stream(on.stdout, off.stdout)
    b = plan_on["bgzf"]
    if shape == "dp5":  # the formatter declines: every reference by the host twin
        assert b["device"] == 0 and b["host"] >= 1
    else:
        assert b["device"] >= 1, plan_on
    # the same file whichever side compressed a reference
    host, plan_host, _ = run_cli(argv, BASECOUNT_BGZF="1", BGZF_TEST_DECLINE="1")
    assert host.returncode == 0 and plan_host["bgzf"]["device"] == 0 and plan_host["bgzf"]["host"] >= 1
    assert host.stdout == on.stdout


@pytest.mark.parametrize("shape", ["default", "long"])
def test_a_reference_in_slices_is_cut_the_same_on_both_sides(shape):
    """A reference longer than the formatter's slice is one span per slice on the device; the twin
    cuts the host formatter's text at the same rows."""
    argv = ["c1.bam"] + SHAPES[shape]
    off, _, _ = run_cli(argv)
    env = dict(BASECOUNT_BGZF="1", BGZF_TEST_SLICE="1000", BASECOUNT_GROUP_REFS="0")  # (the per-reference path slices)
    on, plan_on, _ = run_cli(argv, **env)
    host, plan_host, _ = run_cli(argv, BGZF_TEST_DECLINE="1", **env)
    assert on.returncode == host.returncode == 0
    assert plan_on["bgzf"]["device"] >= 1 and plan_host["bgzf"]["device"] == 0
    assert_stream(on.stdout, off.stdout)
    rows = 1000 * (5 if shape == "long" else 1)
    first = bgzf.blocks(on.stdout)[1]  # (block 0 is the column line)
    assert gzip.decompress(on.stdout[first[0]:first[0] + first[1]]).count(b"\n") <= rows
    assert len(bgzf.blocks(on.stdout)) >= 2 + (off.stdout.count(b"\n") - 1) // rows
    assert host.stdout == on.stdout


@pytest.mark.parametrize("args", [["--summarise"], ["--summarise-with-bed", "scheme.bed"]])
def test_summaries_stay_plain_text(args):
    off, _, _ = run_cli(["mixed.bam"] + args)
    on, plan_on, _ = run_cli(["mixed.bam"] + args, BASECOUNT_BGZF="1")
    assert on.returncode == off.returncode == 0
    assert on.stdout == off.stdout and len(off.stdout) > 20
    assert plan_on["bgzf"] is None


def test_a_range_error_fails_the_same():
    off, _, err_off = run_cli(["err_range.bam"])
    on, _, err_on = run_cli(["err_range.bam"], BASECOUNT_BGZF="1")
    assert off.returncode == on.returncode == 1 and b"IndexError" in on.stderr
    assert err_on[-1:] == err_off[-1:]
    assert (gzip.decompress(on.stdout) if on.stdout else b"") == off.stdout


def test_cohort_bgzf_writes_tsv_gz(tmp_path):
    bams = []
    for i in range(3):
        bams.append(str(tmp_path / ("copy%d.bam" % i)))
        shutil.copy(os.path.join(GOLDEN, "c1.bam"), bams[-1])
    bams.append(str(tmp_path / "edge.bam"))
    shutil.copy(os.path.join(GOLDEN, "edge.bam"), bams[-1])
    e = dict(os.environ, PYTHONPATH=REPO, PYTHONHASHSEED="0")
    for k in CLEARED:
        e.pop(k, None)
    outs = {}
    for flag, d in (([], "plain"), (["--bgzf"], "gz")):
        p = subprocess.run([sys.executable, "-m", "basecount_amd.cohort", "--out-dir", str(tmp_path / d)] + flag + bams,
                           cwd=str(tmp_path), env=e, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        outs[d] = sorted(os.listdir(tmp_path / d))
    stems = ["copy0", "copy1", "copy2", "edge"]
    assert outs["plain"] == [s + ".tsv" for s in stems] and outs["gz"] == [s + ".tsv.gz" for s in stems]
    for s in stems:
        plain = (tmp_path / "plain" / (s + ".tsv")).read_bytes()
        assert len(plain) > 100
        assert_stream((tmp_path / "gz" / (s + ".tsv.gz")).read_bytes(), plain)
