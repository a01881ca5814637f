"""BASECOUNT_DEVICE_SELECT=1 end to end: run() with the batches selected on the device against the
default path, output and raised errors byte for byte.  Regular files must not pass by falling back
(PLAN["select"]: no batch on the host, none redone, at least one on the device, and the same
PLAN["groups"] / PLAN["ops"] routing); the two ungrouped goldens must report the decline; the files
with a faulty read are selected again on the host, the range files stay on the device (their bad
read's ordinal and record are read from there), and all of them fail exactly as ever."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from basecount_amd import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")

# the CLI, then what main.PLAN recorded, on stderr
DRIVER = """
import json, sys
from basecount_amd import main
try:
    main.run(sys.argv[1:])
finally:
    sys.stdout.flush()
    print("PLAN_JSON " + json.dumps({k: main.PLAN.get(k) for k in ("select", "decode", "groups", "ops")}),
          file=sys.stderr)
"""
SWITCHES = ("BASECOUNT_DEVICE_SELECT", "BASECOUNT_DEVICE_DECODE", "BASECOUNT_DEVICE_INFLATE")


def run_cli(cwd, argv, **env):
    e = dict(os.environ, PYTHONPATH=REPO, PYTHONHASHSEED="0")
    for k in SWITCHES + ("BASECOUNT_BATCH_RECORDS", "BASECOUNT_LONG_READS", "BASECOUNT_GROUP_REFS"):
        e.pop(k, None)
    e.update(env)
    p = subprocess.run([sys.executable, "-c", DRIVER] + argv, cwd=cwd, env=e, capture_output=True, timeout=300)
    plan, rest = None, []
    for line in p.stderr.decode().replace("PLAN_JSON", "\nPLAN_JSON").splitlines():
        if line.startswith("PLAN_JSON "):
            plan = json.loads(line[len("PLAN_JSON "):])
        elif line:
            rest.append(line)
    return p, plan, rest


def both(cwd, argv, **env):
    off, plan_off, err_off = run_cli(cwd, argv, **env)
    on, plan_on, err_on = run_cli(cwd, argv, BASECOUNT_DEVICE_SELECT="1", **env)
    assert on.returncode == off.returncode, (err_off[-1:], err_on[-1:])
    assert on.stdout == off.stdout
    assert err_on[-1:] == err_off[-1:]  # the raised error, if any
    assert plan_off["select"] is None  # the switch off: nothing recorded
    return off, plan_off, plan_on


def assert_on_the_device(plan_on):
    s = plan_on["select"]
    assert s["device"] >= 1 and s["host"] == 0 and s["redone"] == 0 and s["declined"] == [], s
    assert plan_on["decode"]["device"] >= 1 and plan_on["decode"]["host"] == 0


@pytest.mark.parametrize("bam,args,env", [
    ("c1.bam", [], {}),
    ("c1.bam", ["--summarise"], {}),
    ("mixed.bam", [], {}),
    ("mixed.bam", ["--min-mapping-quality", "30", "--min-base-quality", "20"], {}),
    ("mixed.bam", ["--min-mapping-quality", "30"], {}),
    ("mixed.bam", ["--min-base-quality", "20"], {}),
    ("mixed.bam", ["--summarise-with-bed", "scheme.bed"], {}),
    ("ont/ont.bam", [], {"BASECOUNT_BATCH_RECORDS": "3"}),
    ("ont/ont.bam", [], {}),
    ("ont/ont.bam", ["--summarise"], {}),
])
def test_regular_files_are_selected_on_the_device(bam, args, env):
    off, plan_off, plan_on = both(GOLDEN, [bam] + args, **env)
    assert off.returncode == 0 and len(off.stdout) > 100
    assert_on_the_device(plan_on)
    assert plan_on["groups"] == plan_off["groups"] and plan_on["ops"] == plan_off["ops"]
    if bam.startswith("ont"):
        assert plan_on["ops"], "the long reads take the ops shape"
    if env:
        assert plan_on["select"]["device"] > 3  # many tiny batches


@pytest.fixture(scope="module")
def many_refs(tmp_path_factory):
    rng = np.random.default_rng(300)
    contigs = [("ref%05d" % i, int(L)) for i, L in enumerate(rng.integers(400, 1200, 300))]
    path = str(tmp_path_factory.mktemp("select_cli") / "refs300.bam")
    synth.write_bam(synth.make_reads(contigs, 12, mixed=True, seed=301), path)
    return path


@pytest.mark.parametrize("args", [[], ["--summarise"]])
def test_three_hundred_references_take_the_grouped_path(many_refs, args):
    off, plan_off, plan_on = both(os.path.dirname(many_refs), [many_refs] + args)
    assert off.returncode == 0
    assert_on_the_device(plan_on)
    assert plan_on["groups"] == plan_off["groups"] and sum(len(g) for g in plan_on["groups"]) >= 250
    assert plan_on["ops"] == plan_off["ops"]


@pytest.mark.parametrize("bam,args", [("edge.bam", []), ("edge.bam", ["--show-n-bases"]),
                                      ("err_order.bam", []), ("err_order.bam", ["--chunk-size", "7"])])
def test_ungrouped_files_are_declined_to_the_host(bam, args):
    _, _, plan_on = both(GOLDEN, [bam] + args)
    s = plan_on["select"]
    assert "ungrouped" in s["declined"] and s["device"] == 0, s


@pytest.mark.parametrize("bam", ["err_nocigar.bam", "err_noqual.bam", "err_range.bam", "err_range_del.bam"])
def test_fault_and_range_files_fail_the_same(bam):
    off, _, plan_on = both(GOLDEN, [bam])
    assert off.returncode == 1
    s = plan_on["select"]
    assert s["device"] + s["redone"] + len(s["declined"]) + s["host"] >= 1, s
    if bam.startswith("err_no"):
        assert s["redone"] >= 1, s  # a faulty read: the batch is selected again on the host


def test_range_error_timeline_comes_from_the_device():
    """err_range's reads are well formed, so the batch stays on the device and the range timeline
    (the bad read's ordinal and record) is read from the device's ordinal / rec arrays."""
    off, _, plan_on = both(GOLDEN, ["err_range.bam"])
    assert off.returncode == 1 and b"IndexError" in off.stderr
    s = plan_on["select"]
    assert s["device"] >= 1 and s["redone"] == 0 and s["declined"] == [], s
