"""Cohort runs against one run per file (DESIGN.md §4 "Cohort runs"), in one process, on seeded
synthetic BAMs (synth.make_reads + write_bam): 32 C2-like files (30 kb, 100,000 x 150 bp) and 256
amplicon-sized files (30 kb, 4,000 reads).  Rows and --summarise-with-bed over each set, three ways:

  (a) loop     a sequential in-process loop of run() per file, the output kept in memory
               (the baseline: the code of the single-file command, untouched by the cohort);
  (b) cohort   python -m basecount_amd.cohort's run() over all files, outputs written to a directory;
  (c) procs    for 8 files only, one `python -m basecount_amd` process per file.

One untimed pass each, then three alternating passes; the minimum and the spread (max - min) of
each are reported, and every output of (b) and (c) is compared with (a)'s byte for byte.  Prints one
JSON line.

    python scripts/cohort_bench.py [--c2 32] [--amp 256] [--repeats 3] [--procs 8]"""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from basecount_amd import cohort as Co  # noqa: E402
from basecount_amd import main as M  # noqa: E402
from basecount_amd import synth  # noqa: E402

CONTIG = [("MN908947.3", 29_903)]
SETS = {"c2": dict(reads=100_000, mixed=False, seed=20_000), "amp": dict(reads=4_000, mixed=True, seed=30_000)}
MODES = {"rows": [], "bed": None}  # bed: --summarise-with-bed <the ARTIC-style scheme written below>


def make_set(root, name, count):
    spec, out = SETS[name], []
    for i in range(count):
        path = os.path.join(root, f"{name}_{i:04d}.bam")
        synth.write_bam(synth.make_reads(CONTIG, spec["reads"], spec["mixed"], spec["seed"] + i), path)
        out.append(path)
    return out


def loop(bams, flags):
    """(a): run() per file in this process, stdout kept in memory."""
    outs = {}
    t0 = time.perf_counter()
    for b in bams:
        buf = io.BytesIO()
        txt = io.TextIOWrapper(buf, encoding="utf-8", write_through=True)
        with contextlib.redirect_stdout(txt):
            M.run([b] + flags)
            txt.flush()
        outs[b] = buf.getvalue()
        txt.detach()
    return time.perf_counter() - t0, outs


def cohort(bams, flags, out_dir):
    """(b): the cohort command's run(); the outputs are read back outside the timed part."""
    t0 = time.perf_counter()
    rc = Co.run(flags + ["--out-dir", out_dir] + bams)
    wall = time.perf_counter() - t0
    assert rc == 0
    outs = {}
    for b, path in zip(bams, Co.output_names(bams, out_dir)):
        with open(path, "rb") as fh:
            outs[b] = fh.read()
    plan = {"groups": len(Co.PLAN["groups"]), "singles": len(Co.PLAN["single"])}
    return wall, outs, plan


def procs(bams, flags):
    """(c): one process per file."""
    env = dict(os.environ, PYTHONPATH=REPO)
    outs = {}
    t0 = time.perf_counter()
    for b in bams:
        p = subprocess.run([sys.executable, "-m", "basecount_amd", b] + flags, env=env, capture_output=True, check=True)
        outs[b] = p.stdout
    return time.perf_counter() - t0, outs


def stats(walls):
    return {"min_ms": round(1e3 * min(walls), 2), "spread_ms": round(1e3 * (max(walls) - min(walls)), 2),
            "all_ms": [round(1e3 * w, 2) for w in walls]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--c2", type=int, default=32)
    ap.add_argument("--amp", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--procs", type=int, default=8)
    a = ap.parse_args()
    result = {"files": {"c2": a.c2, "amp": a.amp}, "repeats": a.repeats}
    with tempfile.TemporaryDirectory() as root:
        bed = os.path.join(root, "scheme.bed")
        with open(bed, "w") as fh:
            fh.write(synth.artic_bed())
        out_dir = os.path.join(root, "out")
        try:
            for name, count in (("c2", a.c2), ("amp", a.amp)):
                if count <= 0:
                    continue
                bams = make_set(root, name, count)
                for mode in MODES:
                    flags = ["--summarise-with-bed", bed] if mode == "bed" else []
                    _, base = loop(bams, flags)  # untimed: allocations, first-use scratch
                    _, got, plan = cohort(bams, flags, out_dir)
                    same = all(got[b] == base[b] for b in bams)
                    walls = {"loop": [], "cohort": []}
                    for _ in range(a.repeats):
                        walls["loop"].append(loop(bams, flags)[0])
                        walls["cohort"].append(cohort(bams, flags, out_dir)[0])
                    few = bams[:a.procs]
                    pw, pouts = procs(few, flags) if few else (0.0, {})
                    same_p = all(pouts[b] == base[b] for b in few)
                    lo, co = stats(walls["loop"]), stats(walls["cohort"])
                    r = {"loop": lo, "cohort": co, "plan": plan, "identical": same, "procs_identical": same_p,
                         "procs": {"files": len(few), "wall_ms": round(1e3 * pw, 2),
                                   "per_file_ms": round(1e3 * pw / max(1, len(few)), 2)},
                         "loop_per_file_ms": round(lo["min_ms"] / count, 3),
                         "cohort_per_file_ms": round(co["min_ms"] / count, 3),
                         "ratio": round(lo["min_ms"] / co["min_ms"], 3),
                         # ahead only by more than the baseline's own pass-to-pass spread
                         "cohort_ahead": co["min_ms"] < lo["min_ms"] - lo["spread_ms"]}
                    result[f"{name}_{mode}"] = r
                    print(f"{name} {mode}: loop {lo}, cohort {co}, ratio {r['ratio']}, ahead {r['cohort_ahead']}, "
                          f"identical {same}/{same_p}, procs {r['procs']}", file=sys.stderr)
                for b in bams:
                    os.remove(b)
        finally:
            M.release_device_memory()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
