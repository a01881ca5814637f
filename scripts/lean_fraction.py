"""k_pileup's lean instance against the general one at C2's shape (29,903 bp, 100,000 x 150 bp
reads) with a share of the reads carrying one 1-base insertion or deletion: the figure behind
kLeanMaxSlowShare (bc_internal.h).

    python scripts/lean_fraction.py [--steps 200] [--reps 3] [--out FILE.json]

Per share (0, 1/64, 1/16, 1/8, 1/4) and instance (forced with bc_ctx_set_instance), `steps`
bc_pileup calls captured into one graph, serialized on one context and with four contexts in
flight (fork / join on the first), wall clock around launch + sync, `reps` times alternating the
two instances.  Prints us per step, run by run; lean is ahead at a share by the project's rule when
every lean run beats every general run and the median gain is at least twice the general runs'
spread."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from basecount_amd import device as D  # noqa: E402
from basecount_amd import synth  # noqa: E402
from basecount_amd.main import norm_factors  # noqa: E402

M, I, DEL = 0, 1, 2


def with_indels(b, share):
    """The batch with every (1 / share)-th read's 150M turned into 75M 1I 74M or 75M 1D 74M."""
    if share == 0:
        return b
    n = b["pos"].size
    every = int(round(1 / share))
    pick = np.arange(every // 2, n, every)
    cig_n = b["cig_n"].copy()
    assert np.all(cig_n == 1)
    cig_n[pick] = 3
    cig_beg = np.zeros(n, np.uint32)
    cig_beg[1:] = np.cumsum(cig_n)[:-1]
    cigar = np.zeros(int(cig_n.sum()), np.uint32)
    cigar[cig_beg] = b["cigar"][b["cig_beg"]]
    qlen = (b["cigar"][b["cig_beg"][pick]] >> 4).astype(np.int64)
    ins = (np.arange(pick.size) & 1) == 0
    # (the last run one base shorter in both kinds: no read's span grows past the reference end)
    left = qlen // 2
    cigar[cig_beg[pick]] = (left << 4) | M
    cigar[cig_beg[pick] + 1] = (1 << 4) | np.where(ins, I, DEL)
    cigar[cig_beg[pick] + 2] = ((qlen - left - 1) << 4) | M
    return dict(b, cig_n=cig_n, cig_beg=cig_beg, cigar=cigar)


def timed(ctxs, reads, outs, L, k, steps):
    nf, nf2 = norm_factors(k)
    main = ctxs[0]

    def body():
        for c in ctxs[1:]:
            c.wait(main)
        for c, r, o in zip(ctxs, reads, outs):
            for _ in range(steps // len(ctxs)):
                c.pileup(r, L, 0, k, nf, nf2, *o)
        for c in ctxs[1:]:
            main.wait(c)

    body()
    for c in ctxs:
        c.sync()
    g = main.capture(body)
    g.launch()
    main.sync()
    t0 = time.perf_counter()
    g.launch()
    main.sync()
    us = (time.perf_counter() - t0) * 1e6 / (steps // len(ctxs) * len(ctxs))
    del g
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rs = synth.make_config("c2")
    base = synth.batch_arrays(rs, 0, 0)
    L, k = rs.lengths[0], 5
    ctxs = [D.Context(0) for _ in range(4)]
    rows = []
    for share in (0.0, 1 / 64, 1 / 16, 1 / 8, 1 / 4):
        b = with_indels(base, share)
        reads = [D.DeviceReads(c, b) for c in ctxs]
        bufs = [[c.alloc(n) for n in (4 * k * L, 4 * L, 8 * k * L, 8 * L, 8 * L)] for c in ctxs]
        outs = [[x.ptr for x in bb] for bb in bufs]
        row = {"share": share, "auto_is_lean": D.pileup_launch_info(reads[0], L)["lean"],
               "in_flight": {"lean": [], "general": []}, "serial": {"lean": [], "general": []}}
        for _ in range(a.reps):
            for inst in ("general", "lean"):
                for c in ctxs:
                    c.set_instance(inst)
                assert D.pileup_launch_info(reads[0], L, instance=inst)["lean"] == (inst == "lean")
                row["in_flight"][inst].append(round(timed(ctxs, reads, outs, L, k, a.steps), 3))
                row["serial"][inst].append(round(timed(ctxs[:1], reads[:1], outs[:1], L, k, a.steps), 3))
        for mode in ("in_flight", "serial"):
            g, l = row[mode]["general"], row[mode]["lean"]
            gain = (statistics.median(g) - statistics.median(l)) / statistics.median(g)
            spread = (max(g) - min(g)) / min(g)
            row[mode]["median_gain"] = round(gain, 4)
            row[mode]["general_spread"] = round(spread, 4)
            row[mode]["lean_ahead"] = bool(max(l) < min(g) and gain >= 2 * spread)
        assert all(c.range_error() == -1 for c in ctxs)
        print(json.dumps(row), flush=True)
        rows.append(row)
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
