"""Device row formatting against the host's, on the BAMs synth writes ("Device row formatting"):
    python scripts/format_bench.py [--configs c2,c3,refs2000,big5m] [--passes 3] [--out DIR] [--parent TREE]

Per file, in ONE process, one untimed pass each way and then `passes` alternating passes of run()
(the CLI's own entry, its output kept in memory and compared byte for byte) with
  off   the five arrays of every reference downloaded, bcio_fmt_rows on the host threads (the default)
  on    BASECOUNT_DEVICE_FORMAT=1: bc_fmt_rows on the device, the header, seg_off and the text downloaded
and per pass: run()'s wall time, the host phases main.PHASES accumulates (`kernels + download`, which
holds the formatter's kernels and the text download with the switch on, and `format + write`, the
whole output phase of the off mode), the device time of k_fmt_measure + k_fmt_scan + k_fmt_write
(event pairs around bc_fmt_rows), the text download, and PLAN["format"].  The minimum over the
passes is reported, with the text bytes and the bytes of the arrays they replace (80 a position at
k = 5).  `refs2000` is scripts/many_refs.py's file of 2,000 references; `big5m` one reference of
5,000,000 positions under 200,000 reads of 150 bases.

--parent TREE: a built checkout of the commit this change is measured against.  Its column is taken
in the same invocation, by a child process that imports the package from TREE and runs this script's
passes with the mode it has (--modes off): the baseline is that library, never this code against itself.
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
TREE = os.environ.get("FORMAT_BENCH_TREE") or os.path.dirname(HERE)
sys.path.insert(0, TREE)
sys.path.insert(1, HERE)

from basecount_amd import main as M  # noqa: E402
from basecount_amd import synth  # noqa: E402

MODES = {"off": {}, "on": {"BASECOUNT_DEVICE_FORMAT": "1"}}
SWITCHES = ("BASECOUNT_DEVICE_INFLATE", "BASECOUNT_DEVICE_DECODE", "BASECOUNT_DEVICE_SELECT", "BASECOUNT_DEVICE_FORMAT")


def one_pass(path, mode):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(MODES[mode])
    M.PHASES.clear()
    ms = getattr(M, "_FORMAT_MS", {})
    before = dict(ms)
    buf = io.BytesIO()
    txt = io.TextIOWrapper(buf, encoding="utf-8", write_through=True)
    t = time.perf_counter()
    with contextlib.redirect_stdout(txt):
        M.run([path])
        txt.flush()
    wall = (time.perf_counter() - t) * 1e3
    r = {"wall_ms": round(wall, 2), "phases_ms": {k: round(v * 1e3, 2) for k, v in M.PHASES.items()}}
    if mode == "on":
        r["format_device_ms"] = round(ms["device_ms"] - before["device_ms"], 4)
        r["text_download_ms"] = round(ms["download_ms"] - before["download_ms"], 3)
        r["calls"] = ms["calls"] - before["calls"]
        r["retries"] = ms["retries"] - before["retries"]
        r["plan"] = {k: (v if not isinstance(v, list) else len(v)) for k, v in M.PLAN["format"].items()}
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

    header = want.index(b"\n") + 1
    positions = want.count(b"\n") - 1
    return {"file": os.path.basename(path), "positions": positions, "text_bytes": len(want) - header,
            "array_bytes": positions * 80, "wall_ms_min": least("wall_ms"),
            "kernels_download_phase_ms_min": least("phases_ms", "kernels + download"),
            "format_write_phase_ms_min": least("phases_ms", "format + write"),
            "format_device_ms_min": least("format_device_ms"), "text_download_ms_min": least("text_download_ms"),
            "passes": res}


def write_input(name, tmp):
    p = os.path.join(tmp, name + ".bam")
    if name.startswith("refs"):
        import many_refs

        many_refs.make_bam(p, int(name[4:]), 50)
    elif name == "big5m":
        synth.write_bam(synth.make_reads([("big5m", 5_000_000)], 200_000, mixed=True, seed=5), p)
    else:
        synth.write_bam(synth.make_config(name), p)  # as bench.py writes it
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3,refs2000,big5m")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for the JSON lines (format_bench.jsonl)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its off column")
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--files", default=None, help="(child) BAM files already written, comma separated")
    a = ap.parse_args()
    modes = a.modes.split(",")
    M.FORMAT_TIMING = True
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        paths = a.files.split(",") if a.files else [write_input(n, tmp) for n in a.configs.split(",")]
        for p in paths:
            rec = bench_file(p, a.passes, modes)
            if a.parent:
                env = dict(os.environ, FORMAT_BENCH_TREE=os.path.abspath(a.parent))
                for k in SWITCHES:
                    env.pop(k, None)
                child = subprocess.run([sys.executable, os.path.abspath(__file__), "--files", p, "--passes", str(a.passes),
                                        "--modes", "off"], env=env, capture_output=True, text=True, timeout=900)
                if child.returncode != 0:
                    raise RuntimeError("the parent tree's passes failed:\n" + child.stderr[-2000:])
                base = json.loads(child.stdout.strip().splitlines()[-1])
                assert base["text_bytes"] == rec["text_bytes"]
                rec["parent"] = {k: base[k]["off"] for k in ("wall_ms_min", "kernels_download_phase_ms_min",
                                                             "format_write_phase_ms_min")}
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            if a.out:
                os.makedirs(a.out, exist_ok=True)
                with open(os.path.join(a.out, "format_bench.jsonl"), "w") as fh:
                    fh.write("\n".join(lines) + "\n")
    M.release_device_memory()


if __name__ == "__main__":
    main()
