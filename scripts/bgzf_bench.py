"""Compressed row output: the device deflate against the routes to a compressed file there are without
it ("Device deflate"):
    python scripts/bgzf_bench.py [--configs c2,c3,refs2000,big5m] [--passes 3] [--out DIR] [--parent TREE]

Per file, in ONE process, one untimed pass of each mode and then `passes` alternating passes of run()
(the CLI's own entry, its output kept in memory) with
  off          the default: arrays downloaded, bcio_fmt_rows on the host threads, plain text
  format       BASECOUNT_DEVICE_FORMAT=1: bc_fmt_rows on the device, the text downloaded
  format+bgzf  BASECOUNT_BGZF=1: bc_bgzf_deflate behind bc_fmt_rows, whole BGZF blocks downloaded
and, timed on `off`'s text after the passes, the route users take today:
  host16       bc_bgzf_deflate_host (the kernels' twin) at 16 threads
  zlib1        Python's zlib at level 1, one thread (what `| gzip -1` costs)
Per pass: run()'s wall time, the host phases `kernels + download` and `format + write`, the device time
of the four deflate kernels (an event pair around bc_bgzf_deflate) and GB/s of text, compressed against
text bytes, the download, the blocks the stored fallback wrote.  The minimum over the passes is
reported.  The BGZF output is gunzipped and compared with `off`'s text byte for byte.

--parent TREE: a built checkout of the commit this change is measured against; its `off` column is
taken in the same invocation by a child process that imports the package from TREE (--modes off).
One JSON line per file."""
import argparse
import contextlib
import gzip
import io
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
TREE = os.environ.get("BGZF_BENCH_TREE") or os.path.dirname(HERE)
sys.path.insert(0, TREE)
sys.path.insert(1, HERE)

from basecount_amd import main as M  # noqa: E402
from format_bench import write_input  # noqa: E402

MODES = {"off": {}, "format": {"BASECOUNT_DEVICE_FORMAT": "1"}, "format+bgzf": {"BASECOUNT_BGZF": "1"}}
SWITCHES = ("BASECOUNT_DEVICE_INFLATE", "BASECOUNT_DEVICE_DECODE", "BASECOUNT_DEVICE_SELECT", "BASECOUNT_DEVICE_FORMAT",
            "BASECOUNT_BGZF")


def one_pass(path, mode):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(MODES[mode])
    M.PHASES.clear()
    fm, dm = getattr(M, "_FORMAT_MS", {}), getattr(M, "_BGZF_MS", {})
    f0, d0 = dict(fm), dict(dm)
    buf = io.BytesIO()
    txt = io.TextIOWrapper(buf, encoding="utf-8", write_through=True)
    t = time.perf_counter()
    with contextlib.redirect_stdout(txt):
        M.run([path])
        txt.flush()
    wall = (time.perf_counter() - t) * 1e3
    r = {"wall_ms": round(wall, 2), "phases_ms": {k: round(v * 1e3, 2) for k, v in M.PHASES.items()},
         "out_bytes": len(buf.getvalue())}
    if mode != "off":
        r["format_device_ms"] = round(fm["device_ms"] - f0["device_ms"], 4)
        r["text_download_ms"] = round(fm["download_ms"] - f0["download_ms"], 3)
    if mode == "format+bgzf":
        d = {k: dm[k] - d0[k] for k in dm}
        r.update(deflate_device_ms=round(d["device_ms"], 4), comp_download_ms=round(d["download_ms"], 3),
                 comp_bytes=d["comp_bytes"], deflate_text_bytes=d["text_bytes"], blocks=d["blocks"], stored=d["stored"],
                 retries=d["retries"], plan=dict(M.PLAN["bgzf"]))
        if d["device_ms"] > 0:
            r["deflate_gb_s"] = round(d["text_bytes"] / d["device_ms"] / 1e6, 2)
    return buf.getvalue(), r


def bench_file(path, passes, modes):
    text = None
    for mode in modes:  # untimed
        out, _ = one_pass(path, mode)
        plain = gzip.decompress(out) if mode == "format+bgzf" else out
        text = plain if text is None else text
        assert plain == text, "output differs with mode " + mode
    res = {m: [] for m in modes}
    for _ in range(passes):
        for mode in modes:
            out, r = one_pass(path, mode)
            assert (gzip.decompress(out) if mode == "format+bgzf" else out) == text, "output differs with mode " + mode
            res[mode].append(r)

    def least(key, sub=None):
        return {m: min((x[key].get(sub, 0.0) if sub else x.get(key, 0.0)) for x in v) for m, v in res.items()}

    rec = {"file": os.path.basename(path), "text_bytes": len(text), "wall_ms_min": least("wall_ms"),
           "kernels_download_phase_ms_min": least("phases_ms", "kernels + download"),
           "format_write_phase_ms_min": least("phases_ms", "format + write"), "out_bytes": least("out_bytes")}
    if "format+bgzf" in modes:
        b = res["format+bgzf"]
        rec.update(deflate_device_ms_min=min(x["deflate_device_ms"] for x in b),
                   deflate_gb_s_max=max(x.get("deflate_gb_s", 0.0) for x in b),
                   comp_download_ms_min=min(x["comp_download_ms"] for x in b), comp_bytes=b[0]["comp_bytes"],
                   blocks=b[0]["blocks"], stored=b[0]["stored"], plan=b[0]["plan"])
        # the route without the switch: off's text compressed on the host afterwards
        from basecount_amd import bgzf

        host16, z1, zsize = [], [], 0
        for _ in range(passes):
            t = time.perf_counter()
            comp = bgzf.compress(text, 16)
            host16.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            zsize = len(zlib.compress(text, 1))
            z1.append((time.perf_counter() - t) * 1e3)
        rec.update(host16_ms_min=round(min(host16), 2), host16_bytes=len(comp), zlib1_ms_min=round(min(z1), 2),
                   zlib1_bytes=zsize)
    rec["passes"] = res
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3,refs2000,big5m")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for the JSON lines (bgzf_bench.jsonl)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its off column")
    ap.add_argument("--modes", default="off,format,format+bgzf")
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
                env = dict(os.environ, BGZF_BENCH_TREE=os.path.abspath(a.parent), FORMAT_BENCH_TREE=os.path.abspath(a.parent))
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
            slim = {k: v for k, v in rec.items() if k != "passes"}
            print(json.dumps(slim), flush=True)
            lines.append(json.dumps(rec))
            if a.out:
                os.makedirs(a.out, exist_ok=True)
                with open(os.path.join(a.out, "bgzf_bench.jsonl"), "w") as fh:
                    fh.write("\n".join(lines) + "\n")
    M.release_device_memory()


if __name__ == "__main__":
    main()
