"""k_pileup's three instances by read length, at C2's contig (29,903 bp) and depth in bases
(15,000,000: 100,000 x 150 bp): all-M reads of 100, 150 and 250 bp, general / lean / slice forced
with bc_ctx_set_instance.  At 250 bp a chunk's 64 x 125 B of
sequence exceed the whole-read lean stage (6,016 B): every chunk of the lean instance falls to
walk_complex.

    python scripts/slice_lengths.py [--steps 200] [--reps 3] [--lengths 100,150,250] [--out FILE.json]

Per length and instance, `steps` bc_pileup calls captured into one graph, with four contexts in
flight (fork / join on the first) and serialized on one, wall clock around launch + sync, `reps`
times alternating the instances.  Prints us per step, run by run.  An instance is ahead of another
by the project's rule when every run of it beats every run of the other and the median gain is at
least twice the other's spread."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))
from basecount_amd import device as D  # noqa: E402
from lean_fraction import timed  # noqa: E402

INSTANCES = ("general", "lean", "slice")
L, BASES = 29_903, 15_000_000


def all_m_batch(n_bases, seed=0):
    """BASES / n_bases all-M reads of n_bases bases, uniform starts, sequence in start order."""
    rng = np.random.default_rng(seed)
    n = BASES // n_bases
    pos = np.sort(rng.integers(0, L - n_bases + 1, n)).astype(np.int32)
    per = n_bases + (n_bases & 1)
    codes = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, n * per)]
    return dict(pos=pos, cig_beg=np.arange(n, dtype=np.uint32), cig_n=np.ones(n, np.uint32),
                seq_nib=(np.arange(n, dtype=np.int64) * per).astype(np.uint32),
                cigar=np.full(n, (n_bases << 4) | 0, np.uint32), seq=((codes[0::2] << 4) | codes[1::2]).astype(np.uint8),
                qual=np.full(n * per, 40, np.uint8))


def ahead(a, b):
    """a over b: (median gain, b's spread, ahead by the rule)."""
    gain = (statistics.median(b) - statistics.median(a)) / statistics.median(b)
    spread = (max(b) - min(b)) / min(b)
    return round(gain, 4), round(spread, 4), bool(max(a) < min(b) and gain >= 2 * spread)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lengths", default="100,150,250")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    k = 5
    ctxs = [D.Context(0) for _ in range(4)]
    rows = []
    for n_bases in [int(x) for x in a.lengths.split(",")]:
        b = all_m_batch(n_bases)
        reads = [D.DeviceReads(c, b) for c in ctxs]
        bufs = [[c.alloc(n) for n in (4 * k * L, 4 * L, 8 * k * L, 8 * L, 8 * L)] for c in ctxs]
        outs = [[x.ptr for x in bb] for bb in bufs]
        for c in ctxs:
            c.set_shape("tile", 4)
        auto = D.pileup_launch_info(reads[0], L, "tile", 4)
        row = {"read_length": n_bases, "reads": int(b["pos"].size),
               "auto": "slice" if auto["slice"] else "lean" if auto["lean"] else "general",
               "in_flight": {i: [] for i in INSTANCES}, "serial": {i: [] for i in INSTANCES}}
        for _ in range(a.reps):
            for inst in INSTANCES:
                for c in ctxs:
                    c.set_instance(inst)
                info = D.pileup_launch_info(reads[0], L, "tile", 4, inst)
                assert (info["slice"], info["lean"]) == (inst == "slice", inst != "general"), info
                row["in_flight"][inst].append(round(timed(ctxs, reads, outs, L, k, a.steps), 3))
                row["serial"][inst].append(round(timed(ctxs[:1], reads[:1], outs[:1], L, k, a.steps), 3))
        for mode in ("in_flight", "serial"):
            m = row[mode]
            m["slice_over_lean"] = ahead(m["slice"], m["lean"])
            m["slice_over_general"] = ahead(m["slice"], m["general"])
            m["lean_over_general"] = ahead(m["lean"], m["general"])
        assert all(c.range_error() == -1 for c in ctxs)
        print(json.dumps(row), flush=True)
        rows.append(row)
        for c in ctxs:
            c.set_instance("auto")
        for r in reads:
            r.free()
        for bb in bufs:
            for x in bb:
                x.free()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
