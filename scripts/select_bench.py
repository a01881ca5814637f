"""Device read selection against the host's, on the BAMs synth writes ("Device read selection"):
    python scripts/select_bench.py [--configs c2,c3,refs2000] [--passes 3] [--out DIR] [--parent TREE]

Per file, in ONE process, one untimed pass each way and then `passes` alternating passes of run()
(the CLI's own entry, its output kept in memory and compared) with
  off      the host inflates, decodes and selects (the default path)
  decode   BASECOUNT_DEVICE_DECODE=1: inflate and record decode on the device, bcio_select on the host
  select   BASECOUNT_DEVICE_SELECT=1: the same, and bc_bam_select on the device
and per pass: run()'s wall time, the host phases main.PHASES accumulates (select, upload, ...), the
select kernels' device time (event pairs around bc_bam_select), the host's wall time inside the
decoder's batch calls, and PLAN["select"].  The minimum over the passes is reported.
`refs2000` is scripts/many_refs.py's file of 2,000 references.

--parent TREE: a built checkout of the commit this change is measured against.  Its `decode` column
is taken in the same invocation, by a child process that imports the package from TREE and runs this
script's passes with the modes it has (--modes off,decode): the baseline is that library, never this
code against itself.
One JSON line per file."""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
TREE = os.environ.get("SELECT_BENCH_TREE") or os.path.dirname(HERE)
sys.path.insert(0, TREE)
sys.path.insert(1, HERE)

from basecount_amd import main as M  # noqa: E402
from basecount_amd import synth  # noqa: E402

MODES = {"off": {}, "decode": {"BASECOUNT_DEVICE_DECODE": "1"}, "select": {"BASECOUNT_DEVICE_SELECT": "1"}}
SWITCHES = ("BASECOUNT_DEVICE_INFLATE", "BASECOUNT_DEVICE_DECODE", "BASECOUNT_DEVICE_SELECT")


def one_pass(path, mode):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(MODES[mode])
    M.PHASES.clear()
    sel_ms = getattr(M, "_SELECT_MS", {"calls": 0, "device_ms": 0.0})
    before, before_sel = dict(M._DECODE_MS), dict(sel_ms)
    buf = io.BytesIO()
    txt = io.TextIOWrapper(buf, encoding="utf-8", write_through=True)
    t = time.perf_counter()
    with contextlib.redirect_stdout(txt):
        M.run([path])
        txt.flush()
    wall = (time.perf_counter() - t) * 1e3
    r = {"wall_ms": round(wall, 2), "phases_ms": {k: round(v * 1e3, 2) for k, v in M.PHASES.items()}}
    if mode != "off":
        r["batch_calls_wall_ms"] = round(M._DECODE_MS["next_wall_ms"] - before["next_wall_ms"], 3)
    if mode == "select":
        r["select_device_ms"] = round(sel_ms["device_ms"] - before_sel["device_ms"], 4)
        r["plan"] = dict(M.PLAN["select"])
    return buf.getvalue(), r


def bench_file(path, passes, modes):
    want = None
    for mode in modes:  # untimed
        out, _ = one_pass(path, mode)
        want = out if want is None else want
        assert out == want, "output differs with mode " + mode
    res = {m: [] for m in modes}
    for _ in range(passes):
        for mode in modes:
            out, r = one_pass(path, mode)
            assert out == want, "output differs with mode " + mode
            res[mode].append(r)

    def least(key, sub=None):
        return {m: min((x[key].get(sub, 0.0) if sub else x.get(key, 0.0)) for x in v) for m, v in res.items()}

    return {"file": os.path.basename(path), "output_bytes": len(want), "wall_ms_min": least("wall_ms"),
            "select_phase_ms_min": least("phases_ms", "select"), "upload_phase_ms_min": least("phases_ms", "upload"),
            "batch_calls_wall_ms_min": least("batch_calls_wall_ms"), "select_device_ms_min": least("select_device_ms"),
            "passes": res}


def write_input(name, tmp):
    p = os.path.join(tmp, name + ".bam")
    if name.startswith("refs"):
        import many_refs

        many_refs.make_bam(p, int(name[4:]), 50)
    else:
        synth.write_bam(synth.make_config(name), p)  # as bench.py writes it
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3,refs2000")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for the JSON lines (select_bench.jsonl)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its decode column")
    ap.add_argument("--modes", default="off,decode,select")
    ap.add_argument("--files", default=None, help="(child) BAM files already written, comma separated")
    a = ap.parse_args()
    modes = a.modes.split(",")
    M.SELECT_TIMING = True
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        paths = a.files.split(",") if a.files else [write_input(n, tmp) for n in a.configs.split(",")]
        for p in paths:
            rec = bench_file(p, a.passes, modes)
            if a.parent:
                env = dict(os.environ, SELECT_BENCH_TREE=os.path.abspath(a.parent))
                for k in SWITCHES:
                    env.pop(k, None)
                child = subprocess.run([sys.executable, os.path.abspath(__file__), "--files", p, "--passes", str(a.passes),
                                        "--modes", "off,decode"], env=env, capture_output=True, text=True, timeout=900)
                if child.returncode != 0:
                    raise RuntimeError("the parent tree's passes failed:\n" + child.stderr[-2000:])
                base = json.loads(child.stdout.strip().splitlines()[-1])
                assert base["output_bytes"] == rec["output_bytes"]
                rec["parent"] = {k: base[k] for k in ("wall_ms_min", "select_phase_ms_min", "upload_phase_ms_min",
                                                      "batch_calls_wall_ms_min")}
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            if a.out:
                os.makedirs(a.out, exist_ok=True)
                with open(os.path.join(a.out, "select_bench.jsonl"), "w") as fh:
                    fh.write("\n".join(lines) + "\n")
    M.release_device_memory()


if __name__ == "__main__":
    main()
