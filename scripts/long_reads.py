"""Many-op (nanopore-like) batches: bc_pileup under the kernel shapes auto / rc / tile / ops on the
same HBM-resident batch in one process (DESIGN.md §3 "k_ops").  Seeded synth.make_long_reads:

  artic   100,000 reads x ~500 bp on a 30 kb reference, an indel every ~12 bases
  long     20,000 reads x ~8 kb on a 5 Mb reference, an indel every ~15 bases
  opsN     50,000 reads x ~500 bp on 30 kb with ~N CIGAR ops per read, N = 3 .. 129

Per batch every shape runs once untimed; then the shapes alternate, each call timed by the
library's event pairs (bc_timing_report: kernel 1 and the whole call) and, separately, as a
captured graph of K calls replayed between two events.  Outputs are compared array by array with
the first shape's and must be equal.  "tile" runs only where the spans allow it (<= 4096).

    python scripts/long_reads.py [--rounds 5] [--steps 20] [--only artic,long]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from basecount_amd import device as D  # noqa: E402
from basecount_amd import synth  # noqa: E402
from basecount_amd.main import norm_factors  # noqa: E402

KERNEL1 = ("pileup", "solo", "rc", "count")
BATCHES = {
    "artic": dict(L=30_000, n=100_000, mean_len=500, indel_every=12.0),
    "long": dict(L=5_000_000, n=20_000, mean_len=8000, indel_every=15.0),
}
for _ops in (3, 9, 17, 33, 65, 129):
    BATCHES[f"ops{_ops}"] = dict(L=30_000, n=50_000, mean_len=500, indel_every=1000.0 / (_ops - 1), clip_frac=0.0)


def measure(ctx, name, spec, rounds, steps, k=5, mbq=0):
    spec = dict(spec)
    L, n = spec.pop("L"), spec.pop("n")
    rs = synth.make_long_reads([("ref", L)], n, seed=100 + len(name), **spec)
    b = synth.batch_arrays(rs, 0)
    b["qual"] = None  # mbq 0
    n_ops = b["cig_n"].astype(np.int64)
    nf, nf2 = norm_factors(k)
    bufs = [ctx.alloc(x) for x in (4 * k * L, 4 * L, 8 * k * L, 8 * L, 8 * L)]
    ptrs = [x.ptr for x in bufs]
    shapes, reads, ref_out = ["auto", "rc", "tile", "ops"], {}, None
    row = {"batch": name, "reads": n, "L": L, "mean_ops": round(float(n_ops.mean()), 1),
           "share_over_8": round(float(np.mean(n_ops > 8)), 3), "events": synth.ref_events(rs), "identical": True}
    for shape in list(shapes):
        ctx.set_shape(shape)
        r = D.DeviceReads(ctx, b)  # (the upload builds the index of the shape in force)
        if shape == "tile" and r.r.max_span > 4096:
            r.free()
            shapes.remove(shape)
            continue
        reads[shape] = r
        for x in bufs:
            x.zero()
        ctx.pileup(r, L, mbq, k, nf, nf2, *ptrs)  # untimed pass: scratch, first use
        assert ctx.range_error() == -1
        out = [bufs[0].download(np.int32, k * L), bufs[1].download(np.int32, L), bufs[2].download(np.float64, k * L),
               bufs[3].download(np.float64, L), bufs[4].download(np.float64, L)]
        if ref_out is None:
            ref_out = out
        elif not all(np.array_equal(a, c) for a, c in zip(out, ref_out)):
            row["identical"] = False
    k1 = {s: [] for s in shapes}
    call = {s: [] for s in shapes}
    ctx.timing(True)
    ctx.timing_report()
    for _ in range(rounds):
        for shape in shapes:
            ctx.set_shape(shape)
            ctx.pileup(reads[shape], L, mbq, k, nf, nf2, *ptrs)
            rep = ctx.timing_report()
            k1[shape].append(sum(c * us for nm, (c, us) in rep.items() if nm in KERNEL1))
            call[shape].append(sum(c * us for c, us in rep.values()))
            row.setdefault("kernels", {})[shape] = sorted(rep)
    ctx.timing(False)
    graph = {}
    for shape in shapes:
        ctx.set_shape(shape)
        g = ctx.capture(lambda: [ctx.pileup(reads[shape], L, mbq, k, nf, nf2, *ptrs) for _ in range(steps)])
        g.launch()
        ts = []
        for _ in range(3):
            ctx.event_record(0)
            g.launch()
            ctx.event_record(1)
            ts.append(1e3 * ctx.event_elapsed_ms(0, 1) / steps)
        graph[shape] = ts
    ctx.set_shape("auto")
    for shape in shapes:
        row[shape] = {"kernel1_us": round(float(np.median(k1[shape])), 1), "call_us": round(float(np.median(call[shape])), 1),
                      "graph_us": round(float(np.median(graph[shape])), 1),
                      "graph_us_all": [round(t, 1) for t in graph[shape]]}
        reads[shape].free()
    for x in bufs:
        x.free()
    return row


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", default=None, help="comma-separated batch names")
    a = ap.parse_args()
    ctx = D.Context(0)
    names = a.only.split(",") if a.only else list(BATCHES)
    for name in names:
        row = measure(ctx, name, BATCHES[name], a.rounds, a.steps)
        print(json.dumps(row), flush=True)
        print(f"{name}: ops/read {row['mean_ops']}, identical {row['identical']}; graph us per call: "
              + ", ".join(f"{s} {row[s]['graph_us']}" for s in ("auto", "rc", "tile", "ops") if s in row),
              file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
