"""BASECOUNT_DEVICE_DECODE=1 end to end: with the streams' records decoded on the device the CLI's
output is byte-identical to the reference-made goldens, every fill is decoded on the device and none
on the host (the goldens are valid: the zero is a condition); files the reference fails on fail the
same; fills the device declines are decoded on the host with the host's own error."""
import contextlib
import gzip
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_decode_inputs as B
from basecount_amd import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")

# the CLI, then what main.PLAN recorded about the decode, on stderr
DRIVER = """
import json, sys
from basecount_amd import main
try:
    main.run(sys.argv[1:])
finally:
    sys.stdout.flush()
    print("PLAN_DECODE " + json.dumps(main.PLAN.get("decode")), file=sys.stderr)
"""


def run_cli(cwd, argv, hashseed="0", **env):
    e = dict(os.environ, PYTHONPATH=REPO, PYTHONHASHSEED=hashseed, **env)
    for k in ("BASECOUNT_DEVICE_DECODE", "BASECOUNT_DEVICE_INFLATE"):
        if k not in env:
            e.pop(k, None)
    p = subprocess.run([sys.executable, "-c", DRIVER] + argv, cwd=cwd, env=e, capture_output=True, timeout=300)
    plan = None
    for line in p.stderr.decode().splitlines():
        if line.startswith("PLAN_DECODE "):
            plan = json.loads(line[len("PLAN_DECODE "):])
    return p, plan


def last_line(p):
    lines = p.stderr.decode().replace("PLAN_DECODE", "\nPLAN_DECODE").splitlines()
    return [ln for ln in lines if ln and not ln.startswith("PLAN_DECODE")][-1]


def load_case(name):
    root = os.path.join(GOLDEN, "ont") if name.startswith("ont") else GOLDEN
    with open(os.path.join(root, "manifest.json")) as fh:
        c = json.load(fh)[name]
    if "stdout" not in c:  # an error case: no output to compare
        return root, c, None
    with open(os.path.join(root, c["stdout"]), "rb") as fh:
        return root, c, gzip.decompress(fh.read())


@pytest.mark.parametrize("name,batch", [("c1_default", None), ("edge_default_h1", None), ("edge_default_h1", "3"),
                                        ("edge_q20_m30", None), ("mixed_bed", None), ("ont_default", None),
                                        ("c1_summary", None)])
def test_goldens_with_device_decode(name, batch):
    root, c, want = load_case(name)
    env = {"BASECOUNT_DEVICE_DECODE": "1"}
    if batch:
        env["BASECOUNT_BATCH_RECORDS"] = batch
    p, plan = run_cli(root, [c["bam"]] + c["args"], c.get("hashseed", "0"), **env)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert p.stdout == want
    assert plan["device"] > 0 and plan["host"] == 0, plan


def test_option_off_decodes_on_the_host():
    root, c, want = load_case("c1_default")
    p, plan = run_cli(root, [c["bam"]] + c["args"], BASECOUNT_DEVICE_DECODE="0")
    assert p.returncode == 0 and p.stdout == want
    assert plan == {"device": 0, "host": 0, "repaired": 0}, plan  # no decoder: nothing is counted


@pytest.mark.parametrize("name", ["err_range", "err_nocigar", "err_noqual"])
def test_error_files_fail_the_same(name):
    root, c, _ = load_case(name)
    argv = [c["bam"]] + c["args"]
    off, _ = run_cli(root, argv)
    on, plan = run_cli(root, argv, BASECOUNT_DEVICE_DECODE="1")
    assert off.returncode == on.returncode == c["returncode"]
    assert last_line(off) == last_line(on) and c["error"] in on.stderr.decode()
    assert on.stdout == off.stdout
    assert plan["device"] > 0 and plan["host"] == 0, plan


def _in_process(argv):
    from basecount_amd import main

    buf = io.BytesIO()
    txt = io.TextIOWrapper(buf, encoding="utf-8", write_through=True)
    with contextlib.redirect_stdout(txt):
        main.run(argv)
        txt.flush()
    return buf.getvalue(), dict(main.PLAN["decode"])


@pytest.mark.parametrize("level", [0, 9])
def test_synthetic_bam_same_output_with_and_without(tmp_path, monkeypatch, level):
    """About 20,000 reads, stored (level 0) and best-compression (level 9) blocks."""
    rs = synth.make_reads([("synthA", 30_000)], 20_000, mixed=True, seed=7)
    path = str(tmp_path / ("synth_l%d.bam" % level))
    synth.write_bam(rs, path, level=level)
    monkeypatch.delenv("BASECOUNT_DEVICE_DECODE", raising=False)
    monkeypatch.delenv("BASECOUNT_DEVICE_INFLATE", raising=False)
    want, plan_off = _in_process([path])
    assert plan_off == {"device": 0, "host": 0, "repaired": 0}
    monkeypatch.setenv("BASECOUNT_DEVICE_DECODE", "1")
    got, plan_on = _in_process([path])
    assert got == want and len(got) > 100_000
    assert plan_on["device"] > 0 and plan_on["host"] == 0, plan_on


# ---- fills the device declines: the host's own error, the fill counted under "host" ----
def _both(tmp_path, name, data):
    path = str(tmp_path / (name + ".bam"))
    with open(path, "wb") as f:
        f.write(data)
    off, _ = run_cli(str(tmp_path), [path])
    on, plan = run_cli(str(tmp_path), [path], BASECOUNT_DEVICE_DECODE="1")
    return off, on, plan


@pytest.mark.parametrize("name", sorted(B.refusals()))
def test_rule_violations_are_the_hosts_errors(tmp_path, name):
    raw, msg = B.refusals()[name]
    # the builder's header names chrA / chrB; the records lie on them
    off, on, plan = _both(tmp_path, name, B.bgzf(raw))
    assert off.returncode != 0 and on.returncode == off.returncode
    assert last_line(on) == last_line(off) and msg in last_line(on)
    assert on.stdout == off.stdout
    assert plan["host"] >= 1, plan


def test_a_block_the_device_inflater_refuses_goes_to_the_host(tmp_path):
    """A BGZF block whose deflate stream is damaged (a reserved block type): k_inflate refuses it,
    the fill is declined, and the host's inflate failure is the error, as with the option off."""
    b = B.Builder()
    B._small_records(b, 21, 400)
    data = bytearray(B.bgzf(b.raw(), chunk=16384))
    # second block: BFINAL=1, BTYPE=3 in its first deflate byte
    first_len = int.from_bytes(data[16:18], "little") + 1
    data[first_len + 18] = 0x07
    off, on, plan = _both(tmp_path, "badblock", bytes(data))
    assert off.returncode != 0 and on.returncode == off.returncode
    assert last_line(on) == last_line(off) and "inflate failed" in last_line(on)
    assert on.stdout == off.stdout
    assert plan["host"] >= 1, plan


def test_stream_batches_equal_the_host_streams(tmp_path):
    """BamStream(device_decode=ctx): every batch's arrays (the device-resident ones downloaded on
    first access) equal the host stream's, bcio_select gives the same selection, at several batch
    sizes; the trap file is repaired, not declined."""
    from basecount_amd import device as D
    from basecount_amd.bam import BamStream

    ctx = D.Context(0)
    trap, _ = B.trap_builder()
    tpath = str(tmp_path / "trap.bam")
    B.write_bam(tpath, trap)
    files = [(os.path.join(GOLDEN, "edge.bam"), (3, 50, 1 << 20), 0), (os.path.join(GOLDEN, "mixed.bam"), (1000, 1 << 20), 0),
             (tpath, (7, 1 << 20), 1024)]
    for path, sizes, seg in files:
        for bsz in sizes:
            with BamStream(path) as hs, BamStream(path, device_decode=ctx, seg_bytes=seg) as ds:
                assert ds.references == hs.references
                n = 0
                for hb, db in zip(hs.batches(bsz), ds.batches(bsz)):
                    assert db.device_arrays is not None and hb.device_arrays is None
                    assert db.n_records == hb.n_records and db.first_record == hb.first_record
                    for k in B.ARRAYS:
                        assert np.array_equal(getattr(db, k), getattr(hb, k)), (path, bsz, n, k)
                    sel = [1] * len(hs.references)
                    a, b = hb.select(0, sel), db.select(0, sel)
                    for k in ("ref_beg", "pos", "cig_beg", "cig_n", "seq_nib", "qlen", "ordinal", "rec", "span"):
                        assert np.array_equal(getattr(a, k), getattr(b, k)), k
                    assert db.cigartuples(0) == hb.cigartuples(0)
                    n += 1
                assert hs.next_batch(bsz) is None and ds.next_batch(bsz) is None
                st = ds.decode_stats()
                assert st["device"] >= 1 and st["host"] == 0, (path, bsz, st)
                if path == tpath:
                    assert st["repaired"] >= 1, st
    ctx.close()
