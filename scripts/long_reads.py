"""Many-op (nanopore-like) batches: bc_pileup under the kernel shapes auto / rc / tile / ops on the
same HBM-resident batch in one process (DESIGN.md §3 "k_ops").  Seeded synth.make_long_reads:

  artic   100,000 reads x ~500 bp on a 30 kb reference, an indel every ~12 bases
  mid1200  50,000 reads x ~1,200 bp on 30 kb: below half a window, the single-window launch
  long     20,000 reads x ~8 kb on a 5 Mb reference, an indel every ~15 bases
  long30k   5,000 reads x ~30 kb on 5 Mb
  opsN     50,000 reads x ~500 bp on 30 kb with ~N CIGAR ops per read, N = 3 .. 129

Per batch every variant runs once untimed; then the variants alternate, each call timed by the
library's event pairs (bc_timing_report: kernel 1 and the whole call) and, separately, as a
captured graph of K calls replayed between two events.  Outputs are compared array by array with
the first variant's and must be equal.  "tile" runs only where the spans allow it (<= 4096).
Per variant the minimum over the rounds, the spread (max - min) and the median are reported.

Variants: the shapes of --shapes; with "ops" among them also ``ops_p1`` (this library with
set_ops_passes(1): what the pass loop costs, never the baseline) and, for every N of --rpb,
``ops_rpbN`` (N reads per workgroup forced, the passes from the plan).  --parent LIBDIR adds
``parent``: the library of the commit this tree is measured against (LIBDIR/libbasecount_hip.so, built
from that commit), loaded into this process and run under "ops" on the very same resident batch,
alternating with the others: the baseline of every comparison.

    python scripts/long_reads.py [--rounds 5] [--steps 20] [--only artic,long] [--shapes ops]
                                 [--mbq 20] [--k 6] [--rpb 8,32] [--parent LIBDIR]"""
import argparse
import ctypes as C
import importlib.util
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
    "mid1200": dict(L=30_000, n=50_000, mean_len=1200, indel_every=12.0),
    "long": dict(L=5_000_000, n=20_000, mean_len=8000, indel_every=15.0),
    "long30k": dict(L=5_000_000, n=5000, mean_len=30_000, indel_every=15.0),
}
for _ops in (3, 9, 17, 33, 65, 129):
    BATCHES[f"ops{_ops}"] = dict(L=30_000, n=50_000, mean_len=500, indel_every=1000.0 / (_ops - 1), clip_frac=0.0)


class _Absent:
    """Stands in for a function the other library does not export (its signature is set, never called)."""


class _Lib:
    def __init__(self, cdll):
        self._cdll = cdll

    def __getattr__(self, name):
        try:
            return getattr(self._cdll, name)
        except AttributeError:
            return _Absent()


def other_device(libdir):
    """A second copy of basecount_amd.device bound to LIBDIR/libbasecount_hip.so: its own Context and
    structure classes over the same process's device memory."""
    spec = importlib.util.spec_from_file_location("basecount_amd._other_device", D.__file__)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    mod._libs = {}

    def load(name):
        if name not in mod._libs:
            mod._libs[name] = _Lib(C.CDLL(os.path.join(os.path.abspath(libdir), name)))
        return mod._libs[name]

    mod._load = load
    return mod


def stat(xs):
    return {"min": round(float(min(xs)), 1), "spread": round(float(max(xs) - min(xs)), 1),
            "median": round(float(np.median(xs)), 1)}


def measure(ctx, name, spec, rounds, steps, k=5, mbq=0, shapes=("auto", "rc", "tile", "ops"), rpbs=(), parent=None):
    spec = dict(spec)
    L, n = spec.pop("L"), spec.pop("n")
    rs = synth.make_long_reads([("ref", L)], n, seed=100 + len(name), **spec)
    b = synth.batch_arrays(rs, 0)
    if mbq == 0:
        b["qual"] = None
    n_ops = b["cig_n"].astype(np.int64)
    nf, nf2 = norm_factors(k)
    bufs = [ctx.alloc(x) for x in (4 * k * L, 4 * L, 8 * k * L, 8 * L, 8 * L)]
    ptrs = [x.ptr for x in bufs]
    row = {"batch": name, "reads": n, "L": L, "mbq": mbq, "k": k, "mean_ops": round(float(n_ops.mean()), 1),
           "share_over_8": round(float(np.mean(n_ops > 8)), 3), "events": synth.ref_events(rs), "identical": True}
    # variant -> (context, shape, reads per block, passes, the batch as that library's bc_reads)
    uploads, variants, ref_out = {}, {}, None
    for shape in shapes:
        ctx.set_shape(shape)
        r = D.DeviceReads(ctx, b)  # (the upload builds the index of the shape in force)
        if shape == "tile" and r.r.max_span > 4096:
            r.free()
            continue
        uploads[shape] = r
        variants[shape] = (ctx, shape, 0, 0, r.r)
    if "ops" in uploads:
        r = uploads["ops"].r
        row["plan"] = D.ops_plan(r, L)
        row["passes"] = row["plan"]["passes_max"]
        variants["ops_p1"] = (ctx, "ops", 0, 1, r)
        for rpb in rpbs:
            variants[f"ops_rpb{rpb}"] = (ctx, "ops", rpb, 0, r)
            row.setdefault("plans", {})[f"ops_rpb{rpb}"] = D.ops_plan(r, L, rpb)
        if parent is not None:
            pmod, pctx = parent
            variants["parent"] = (pctx, "ops", 0, None, pmod.BcReads.from_buffer_copy(bytes(r)))

    def call(v):
        c, shape, rpb, passes, r = variants[v]
        c.set_shape(shape, 0, rpb)
        if passes is not None:
            c.set_ops_passes(passes)
        c.pileup(r, L, mbq, k, nf, nf2, *ptrs)

    for v in variants:
        for x in bufs:
            x.zero()
        call(v)  # untimed: scratch, first use
        c = variants[v][0]
        assert c.range_error() == -1
        c.sync()
        out = [bufs[0].download(np.int32, k * L), bufs[1].download(np.int32, L), bufs[2].download(np.float64, k * L),
               bufs[3].download(np.float64, L), bufs[4].download(np.float64, L)]
        if ref_out is None:
            ref_out = out
        elif not all(np.array_equal(x, y) for x, y in zip(out, ref_out)):
            row["identical"] = False
            row.setdefault("differs", []).append(v)
    k1 = {v: [] for v in variants}
    whole = {v: [] for v in variants}
    for c in {id(x[0]): x[0] for x in variants.values()}.values():
        c.timing(True)
        c.timing_report()
    for _ in range(rounds):
        for v in variants:
            c = variants[v][0]
            call(v)
            rep = c.timing_report()  # (synchronises: the next variant starts on an idle device)
            k1[v].append(sum(cnt * us for nm, (cnt, us) in rep.items() if nm in KERNEL1))
            whole[v].append(sum(cnt * us for cnt, us in rep.values()))
            row.setdefault("kernels", {})[v] = sorted(rep)
    for c in {id(x[0]): x[0] for x in variants.values()}.values():
        c.timing(False)
    graphs = {}
    for v in variants:
        c = variants[v][0]
        graphs[v] = (c, c.capture(lambda: [call(v) for _ in range(steps)]))
        graphs[v][1].launch()
        c.sync()
    graph = {v: [] for v in variants}
    for _ in range(rounds):
        for v, (c, g) in graphs.items():
            c.event_record(0)
            g.launch()
            c.event_record(1)
            graph[v].append(1e3 * c.event_elapsed_ms(0, 1) / steps)
            c.sync()
    for c in {id(x[0]): x[0] for x in variants.values()}.values():
        c.set_shape("auto")
        if c is ctx:
            c.set_ops_passes(0)
    for v in variants:
        row[v] = {"kernel1_us": stat(k1[v]), "call_us": stat(whole[v]), "graph_us": stat(graph[v])}
    if "parent" in variants:
        # ahead / behind: this tree's minimum against the parent's, by more than the parent's spread
        for v in variants:
            if v.startswith("ops"):
                for what in ("kernel1_us", "graph_us"):
                    mine, base = row[v][what], row["parent"][what]
                    d = mine["min"] - base["min"]
                    row[v][what]["vs_parent"] = "ahead" if d < -base["spread"] else "behind" if d > base["spread"] else "level"
    for r in uploads.values():
        r.free()
    for x in bufs:
        x.free()
    return row


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", default=None, help="comma-separated batch names")
    ap.add_argument("--shapes", default="auto,rc,tile,ops", help="comma-separated kernel shapes")
    ap.add_argument("--mbq", type=int, default=0, help="min_base_quality (> 0: the batches keep their qualities)")
    ap.add_argument("--k", type=int, default=5, choices=(5, 6), help="columns: 6 counts N")
    ap.add_argument("--rpb", default="", help="comma-separated forced reads per workgroup, a variant each")
    ap.add_argument("--parent", default=None, help="directory of the parent commit's libbasecount_hip.so")
    a = ap.parse_args()
    ctx = D.Context(0)
    parent = None
    if a.parent:
        pmod = other_device(a.parent)
        parent = (pmod, pmod.Context(0))
    names = a.only.split(",") if a.only else list(BATCHES)
    rpbs = [int(x) for x in a.rpb.split(",") if x]
    for name in names:
        row = measure(ctx, name, BATCHES[name], a.rounds, a.steps, a.k, a.mbq, a.shapes.split(","), rpbs, parent)
        print(json.dumps(row), flush=True)
        shown = [v for v in row if isinstance(row[v], dict) and "graph_us" in row[v]]
        print(f"{name}: ops/read {row['mean_ops']}, passes {row.get('passes')}, identical {row['identical']}; "
              "kernel 1 / graph us per call (min): "
              + ", ".join(f"{v} {row[v]['kernel1_us']['min']} / {row[v]['graph_us']['min']}" for v in shown),
              file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
