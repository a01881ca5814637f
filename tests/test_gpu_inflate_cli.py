"""BASECOUNT_DEVICE_INFLATE=1 end to end: the CLI's output with the streams' BGZF blocks inflated by
k_inflate is byte-identical to the reference-made goldens, every block after the header goes to the
device and none comes back to the host (the goldens are valid BGZF: the zero is a condition)."""
import contextlib
import gzip
import io
import json
import os
import subprocess
import sys

import pytest

from basecount_amd import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")

# the CLI, then what main.PLAN recorded about the inflate, on stderr
DRIVER = """
import json, sys
from basecount_amd import main
try:
    main.run(sys.argv[1:])
finally:
    sys.stdout.flush()
    print("PLAN_INFLATE " + json.dumps(main.PLAN.get("inflate")), file=sys.stderr)
"""


def run_cli(cwd, argv, hashseed="0", **env):
    e = dict(os.environ, PYTHONPATH=REPO, PYTHONHASHSEED=hashseed, **env)
    p = subprocess.run([sys.executable, "-c", DRIVER] + argv, cwd=cwd, env=e, capture_output=True, timeout=300)
    plan = None
    for line in p.stderr.decode().splitlines():
        if line.startswith("PLAN_INFLATE "):
            plan = json.loads(line[len("PLAN_INFLATE "):])
    return p, plan


def load_case(name):
    root = os.path.join(GOLDEN, "ont") if name.startswith("ont") else GOLDEN
    with open(os.path.join(root, "manifest.json")) as fh:
        c = json.load(fh)[name]
    if "stdout" not in c:  # an error case: no output to compare
        return root, c, None
    with open(os.path.join(root, c["stdout"]), "rb") as fh:
        return root, c, gzip.decompress(fh.read())


@pytest.mark.parametrize("name,batch", [("c1_default", None), ("edge_default_h1", None), ("edge_default_h1", "3"),
                                        ("mixed_bed", None), ("ont_default", None), ("c1_summary", None)])
def test_goldens_with_device_inflate(name, batch):
    root, c, want = load_case(name)
    env = {"BASECOUNT_DEVICE_INFLATE": "1"}
    if batch:
        env["BASECOUNT_BATCH_RECORDS"] = batch
    p, plan = run_cli(root, [c["bam"]] + c["args"], c.get("hashseed", "0"), **env)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert p.stdout == want
    assert plan["device"] > 0 and plan["host"] == 0, plan


def test_option_off_inflates_on_the_host():
    root, c, want = load_case("c1_default")
    p, plan = run_cli(root, [c["bam"]] + c["args"], BASECOUNT_DEVICE_INFLATE="0")
    assert p.returncode == 0 and p.stdout == want
    assert plan["device"] == 0 and plan["host"] > 0, plan


def test_error_file_fails_the_same():
    root, c, _ = load_case("err_range")
    argv = [c["bam"]] + c["args"]
    off, _ = run_cli(root, argv)
    on, plan = run_cli(root, argv, BASECOUNT_DEVICE_INFLATE="1")
    assert off.returncode == on.returncode == c["returncode"]
    last = [p.stderr.decode().replace("PLAN_INFLATE", "\nPLAN_INFLATE").splitlines() for p in (off, on)]
    last = [[ln for ln in lines if ln and not ln.startswith("PLAN_INFLATE")][-1] for lines in last]
    assert last[0] == last[1] and c["error"] in last[1]
    assert on.stdout == off.stdout
    assert plan["device"] > 0 and plan["host"] == 0, plan


def _in_process(argv):
    from basecount_amd import main

    buf = io.BytesIO()
    txt = io.TextIOWrapper(buf, encoding="utf-8", write_through=True)
    with contextlib.redirect_stdout(txt):
        main.run(argv)
        txt.flush()
    return buf.getvalue(), dict(main.PLAN["inflate"])


@pytest.mark.parametrize("level", [0, 9])
def test_synthetic_bam_same_output_with_and_without(tmp_path, monkeypatch, level):
    """About 20,000 reads, stored (level 0) and best-compression (level 9) blocks."""
    rs = synth.make_reads([("synthA", 30_000)], 20_000, mixed=True, seed=7)
    path = str(tmp_path / ("synth_l%d.bam" % level))
    synth.write_bam(rs, path, level=level)
    monkeypatch.delenv("BASECOUNT_DEVICE_INFLATE", raising=False)
    want, plan_off = _in_process([path])
    assert plan_off["device"] == 0 and plan_off["host"] >= 40, plan_off  # BGZF blocks after the header's
    monkeypatch.setenv("BASECOUNT_DEVICE_INFLATE", "1")
    got, plan_on = _in_process([path])
    assert got == want and len(got) > 100_000
    assert plan_on == {"device": plan_off["host"], "host": 0}, (plan_on, plan_off)
