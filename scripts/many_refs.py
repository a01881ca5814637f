"""Many small references: get_basecounts with the references of a batch grouped into one launch
(bc_pileup_segments) against the per-reference path (BASECOUNT_GROUP_REFS=0, the
code a file of one or a few large references runs), on a seeded synthetic BAM of 2,000 references
of 1-3 kb with 50 reads each.  Rows and --summarise shape, grouping on and off alternating in one
process, three times each after one untimed pass; prints the wall times and the kernel launches
(timing_report) of one further pass per variant.

    python scripts/many_refs.py [--refs 2000] [--reads 50] [--keep FILE.bam]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from basecount_amd import main as M  # noqa: E402
from basecount_amd import synth  # noqa: E402

KERNEL1 = ("pileup", "solo", "rc", "count")


def make_bam(path: str, refs: int, reads: int, seed: int = 2000) -> None:
    rng = np.random.default_rng(seed)
    contigs = [(f"ref{i:05d}", int(L)) for i, L in enumerate(rng.integers(1000, 3001, refs))]
    synth.write_bam(synth.make_reads(contigs, reads, mixed=True, seed=seed + 1), path)


def one_pass(bam: str, mode: str, grouped: bool, timed: bool = False):
    os.environ["BASECOUNT_GROUP_REFS"] = "1" if grouped else "0"
    ctx = M.context()
    if timed:
        ctx.timing(True)
    t0 = time.perf_counter()
    out = M.get_basecounts(bam, _mode=mode, _keep_scratch=True)
    wall = time.perf_counter() - t0
    rep = None
    if timed:
        rep = ctx.timing_report()
        ctx.timing(False)
    return wall, rep, out


def same(a, b, mode: str) -> bool:
    if set(a) != set(b):
        return False
    for ref in a:
        if mode == "rows":
            x, y = a[ref]["rows"].d, b[ref]["rows"].d
            if not all(np.array_equal(getattr(x, f), getattr(y, f)) for f in ("counts", "pc", "ent", "sec", "cov")):
                return False
        elif a[ref] != b[ref]:
            return False
    return True


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=2000)
    ap.add_argument("--reads", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--keep", default=None, help="write the BAM here and keep it")
    a = ap.parse_args()
    tmp = None
    bam = a.keep
    if bam is None:
        tmp = tempfile.TemporaryDirectory()
        bam = os.path.join(tmp.name, "many_refs.bam")
    make_bam(bam, a.refs, a.reads)
    result = {"refs": a.refs, "reads_per_ref": a.reads}
    try:
        for mode in ("rows", "summary"):
            _, _, on = one_pass(bam, mode, True)  # untimed: allocations, first-use scratch
            groups = len(M.PLAN["groups"])
            _, _, off = one_pass(bam, mode, False)
            walls = {True: [], False: []}
            for _ in range(a.repeats):
                for grouped in (True, False):
                    walls[grouped].append(one_pass(bam, mode, grouped)[0])
            launches = {}
            for grouped in (True, False):
                rep = one_pass(bam, mode, grouped, timed=True)[1]
                launches[grouped] = {"kernel1": sum(rep.get(n, (0, 0.0))[0] for n in KERNEL1),
                                     "all": sum(v[0] for v in rep.values())}
            result[mode] = {
                "identical": same(on, off, mode), "groups": groups,
                "grouped_wall_ms": [round(1e3 * w, 2) for w in walls[True]],
                "per_reference_wall_ms": [round(1e3 * w, 2) for w in walls[False]],
                "grouped_launches": launches[True], "per_reference_launches": launches[False],
            }
            print(f"{mode}: grouped {result[mode]['grouped_wall_ms']} ms, per reference "
                  f"{result[mode]['per_reference_wall_ms']} ms; kernel-1 launches {launches[True]['kernel1']} vs "
                  f"{launches[False]['kernel1']}; identical {result[mode]['identical']}", file=sys.stderr)
    finally:
        M.release_device_memory()
        if tmp is not None:
            tmp.cleanup()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
