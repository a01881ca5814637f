"""Device record decode against the host's, on the BAMs synth writes ("Device record decode"):
    python scripts/decode_bench.py [--configs c2,c3] [--passes 3] [--out DIR]

Per file, in ONE process, one untimed pass each way and then `passes` alternating passes of run()
(the CLI's own entry, its output kept in memory and compared) with
  off      the host inflates and decodes (the default path)
  inflate  BASECOUNT_DEVICE_INFLATE=1: k_inflate, the host decodes
  decode   BASECOUNT_DEVICE_DECODE=1: k_inflate and the record decode on the device
and per pass: run()'s wall time, the host phases main.PHASES accumulates (decode, select, upload, ...)
and, for `decode`, the decoder's device times (uploads, k_inflate, k_bam_speculate + k_bam_stitch,
k_bam_fill, downloads), the host's wall time inside its fill and batch calls, and the fills decoded
on the device / declined / segments repaired.
One JSON line per file."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from basecount_amd import main as M  # noqa: E402
from basecount_amd import synth  # noqa: E402

MODES = {"off": {}, "inflate": {"BASECOUNT_DEVICE_INFLATE": "1"}, "decode": {"BASECOUNT_DEVICE_DECODE": "1"}}
DEVICE_KEYS = ("upload_ms", "inflate_ms", "index_ms", "fill_ms", "download_ms", "fill_wall_ms", "next_wall_ms")


def one_pass(path, mode):
    for k in ("BASECOUNT_DEVICE_INFLATE", "BASECOUNT_DEVICE_DECODE"):
        os.environ.pop(k, None)
    os.environ.update(MODES[mode])
    M.PHASES.clear()
    before = dict(M._DECODE_MS)
    buf = io.BytesIO()
    txt = io.TextIOWrapper(buf, encoding="utf-8", write_through=True)
    t = time.perf_counter()
    with contextlib.redirect_stdout(txt):
        M.run([path])
        txt.flush()
    wall = (time.perf_counter() - t) * 1e3
    r = {"wall_ms": round(wall, 2), "phases_ms": {k: round(v * 1e3, 2) for k, v in M.PHASES.items()}}
    if mode == "decode":
        r["device_ms"] = {k: round(M._DECODE_MS[k] - before[k], 3) for k in DEVICE_KEYS}
        r["plan"] = dict(M.PLAN["decode"])
    return buf.getvalue(), r


def bench_file(path, passes):
    want = None
    for mode in MODES:  # untimed
        out, _ = one_pass(path, mode)
        want = out if want is None else want
        assert out == want, "output differs with mode " + mode
    res = {m: [] for m in MODES}
    for _ in range(passes):
        for mode in MODES:
            out, r = one_pass(path, mode)
            assert out == want, "output differs with mode " + mode
            res[mode].append(r)
    return {"file": os.path.basename(path), "output_bytes": len(want),
            "wall_ms_min": {m: min(x["wall_ms"] for x in v) for m, v in res.items()},
            "decode_phase_ms_min": {m: min(x["phases_ms"].get("decode", 0.0) for x in v) for m, v in res.items()},
            "upload_phase_ms_min": {m: min(x["phases_ms"].get("upload", 0.0) for x in v) for m, v in res.items()},
            "passes": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for the JSON lines (decode_bench.jsonl)")
    a = ap.parse_args()
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.configs.split(","):
            rs = synth.make_config(name)
            p = os.path.join(tmp, name + ".bam")
            synth.write_bam(rs, p)  # as bench.py writes it
            line = json.dumps(bench_file(p, a.passes))
            print(line, flush=True)
            lines.append(line)
            if a.out:
                os.makedirs(a.out, exist_ok=True)
                with open(os.path.join(a.out, "decode_bench.jsonl"), "w") as fh:
                    fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
