"""Batches for k_ops' window passes (basecount_amd/csrc/bc_ops.hip, DESIGN.md §3 "k_ops") and a CPU
restatement of which pass owns which event.

The definition (include/basecount_hip.h, bc_ops_plan): a workgroup takes ``rpb`` consecutive reads of
a sorted batch; with P passes, pass p owns the positions [wbase + p·W, wbase + (p + 1)·W), wbase the
start of the workgroup's first read, W = 4096, and the last pass everything from its start on.  A
read's reference events are walked per batch of 64 CIGAR ops, 64 consecutive reference offsets per
step from the batch's first offset; a step that holds a window end is split per lane.  The passes end
when no read of the workgroup reaches further.

``case(name)`` builds the batch a test in tests/test_gpu_ops_passes.py runs, ``case(name, True)`` a
perturbed one without the piece the case is named for; tests/test_ops_passes_host.py proves both
with the functions below.  Nothing here loads the device library."""
import functools

import numpy as np

import saturation_batches as SB
from saturation_batches import DEL, EQOP, H, I, M, P, S, SKIP, X

W = SB.K_WIN_MAX  # positions per window
CAP = 16          # BC_OPS_PASSES_MAX
BASE = 100        # where every case's first read starts: the first workgroup's wbase
RPBS = (1, 3, 64)
FORCED = (2, 3, CAP)


# ------------------------------------------------------------------------------------ the model
def cigars(b):
    """[(op, len)] per read."""
    out = []
    for beg, n in zip(b["cig_beg"].astype(np.int64), b["cig_n"].astype(np.int64)):
        wd = b["cigar"][beg: beg + n].astype(np.int64)
        out.append([(int(x & 15), int(x >> 4)) for x in wd])
    return out


def ref_ops(ops):
    """(op index, op, first reference offset, length) of the non-empty reference-consuming ops."""
    out, at = [], 0
    for j, (op, ln) in enumerate(ops):
        if op in SB.REF_OPS:
            if ln:
                out.append((j, op, at, ln))
            at += ln
    return out


def steps(ops):
    """The walk's steps as (first offset, end offset): per batch of 64 ops, 64 offsets per step from
    the batch's first reference offset to its last."""
    out, at = [], 0
    for k0 in range(0, len(ops), 64):
        r0 = at
        at += SB.ref_span(ops[k0: k0 + 64])
        out += [(e0, min(e0 + 64, at)) for e0 in range(r0, at, 64)]
    return out


def owner(p, wbase, passes):
    """The pass that owns position p."""
    return min(max((p - wbase) // W, 0), passes - 1)


def blocks(b, rpb):
    n = b["pos"].size
    return [(r0, min(r0 + rpb, n)) for r0 in range(0, n, rpb)]


def block_of(b, rpb, i):
    r0 = i // rpb * rpb
    return r0, int(b["pos"][r0])


def passes_run(b, rpb, passes):
    """Per workgroup, the passes it runs: one more while a read reaches (or starts) beyond the
    pass's end, at most ``passes``."""
    pos, sp = b["pos"].astype(np.int64), SB.spans(b)
    out = []
    for r0, r1 in blocks(b, rpb):
        far = max(int(max(pos[i], pos[i] + sp[i] - 1)) for i in range(r0, r1))
        out.append(owner(far, int(pos[r0]), passes) + 1)
    return out


def read_passes(b, rpb, passes, i):
    """The set of passes that own a reference event of read i."""
    _, wbase = block_of(b, rpb, i)
    p0, out = int(b["pos"][i]), set()
    for _, _, at, ln in ref_ops(cigars(b)[i]):
        out |= set(range(owner(p0 + at, wbase, passes), owner(p0 + at + ln - 1, wbase, passes) + 1))
    return out


def split_lanes(b, rpb, passes, i):
    """The lanes (1..63) at which a step of read i is split between two passes."""
    _, wbase = block_of(b, rpb, i)
    p0, out = int(b["pos"][i]), set()
    for e0, e1 in steps(cigars(b)[i]):
        own = [owner(p0 + e, wbase, passes) for e in range(e0, e1)]
        out |= {l for l in range(1, len(own)) if own[l] != own[l - 1]}
    return out


def ops_across(b, rpb, passes, i):
    """The ops of read i whose events lie in two passes, as a set of op codes."""
    _, wbase = block_of(b, rpb, i)
    p0 = int(b["pos"][i])
    return {op for _, op, at, ln in ref_ops(cigars(b)[i])
            if owner(p0 + at, wbase, passes) != owner(p0 + at + ln - 1, wbase, passes)}


def ops_at_window_end(b, rpb, i):
    """The op indices of read i that consume no reference and sit exactly at a window end: the event
    before them is a window's last, the event after them the next window's first."""
    _, wbase = block_of(b, rpb, i)
    p0, at, out = int(b["pos"][i]), 0, []
    ops = cigars(b)[i]
    total = SB.ref_span(ops)
    for j, (op, ln) in enumerate(ops):
        quiet = op not in SB.REF_OPS or ln == 0
        if quiet and 0 < at < total and (p0 + at - wbase) % W == 0:
            out.append(j)
        if op in SB.REF_OPS:
            at += ln
    return out


def op_batch_starts(b, rpb, i):
    """(position - wbase) of the first reference offset of read i's op batches 1, 2, ..."""
    _, wbase = block_of(b, rpb, i)
    ops = cigars(b)[i]
    return [int(b["pos"][i]) + SB.ref_span(ops[:k0]) - wbase for k0 in range(64, len(ops), 64)]


def header(b):
    """The batch's bc_reads header as ops_plan reads it."""
    return dict(n_reads=int(b["pos"].size), sorted=1, max_span=int(SB.spans(b).max()), max_end=SB.max_end(b),
                seq_bytes=int(b["seq"].size))


# ------------------------------------------------------------------------------------- batches
def alternating(span, seed=0):
    """Nanopore-like ops over ``span`` reference positions: M / = / X runs of 5-14 with 1-2 I or D
    between them."""
    rng = np.random.default_rng(1000 + seed)
    ops, at = [], 0
    while at < span:
        ln = min(int(rng.integers(5, 15)), span - at)
        ops.append(((M, EQOP, X)[len(ops) % 3], ln))
        at += ln
        if at < span:
            if rng.random() < 0.5:
                ops.append((I, int(rng.integers(1, 3))))
            else:
                ln = min(int(rng.integers(1, 3)), span - at)
                ops.append((DEL, ln))
                at += ln
    return ops


def _read(rng, pos, ops):
    return SB.random_read(rng, int(pos), ops)


SPANS = (W - 1, W, W + 1, 2 * W, 2 * W + 1, 3 * W - 1, 3 * W, 3 * W + 1)


def _span(span, perturbed, rng):
    # (perturbed: the read ends half a window earlier or later than the edge it is named for)
    return [_read(rng, BASE, [(M, span + (W // 2 if perturbed else 0))])], None


def _straddle(perturbed, rng):
    # an anchor at the window's start, then a read 63 .. 1 positions before the window's end (its
    # first step is split at that lane) and one exactly at it; perturbed: all a window's half earlier
    reads = [_read(rng, BASE, [(M, 3 * W + 7)])]
    for s in range(63, -1, -1):
        reads.append(_read(rng, BASE + W - s - (W // 2 if perturbed else 0), [(M, 70 + s), (I, 2), (DEL, 3), (M, 9)]))
    return reads, None


def _across(perturbed, rng):
    d = 300 if perturbed else 0  # (perturbed: every op named here lies 300 positions before the end)
    tail = alternating(40, 3)
    return [
        _read(rng, BASE, [(M, W - 5 - d), (DEL, 10), (M, 20)] + tail),
        _read(rng, BASE, [(EQOP, W - 5 - d), (SKIP, 10), (M, 20)] + tail),
        _read(rng, BASE, [(M, 2 * W - 7 - d), (X, 15), (DEL, 1)] + tail),
        _read(rng, BASE, [(M, W - d), (I, 4), (M, 20)] + tail),
        _read(rng, BASE, [(S, 3), (M, W - d), (DEL, 0), (I, 0), (P, 2), (SKIP, 0), (H, 1), (M, 0), (M, 20), (S, 2)]),
        _read(rng, BASE, [(M, W - 1 - d), (I, 1), (M, 1), (I, 1), (M, 1), (DEL, W - 1), (I, 2), (M, 5)]),
    ], None


def _batch64(perturbed, rng):
    # 64 ops over exactly one window (two windows for the second read), then more ops: the second op
    # batch starts at a window's first position; perturbed: 3 positions later
    first = [(M, 127 + (3 if perturbed else 0)), (DEL, 1)] + [(M, 127), (DEL, 1)] * 31
    second = [(M, 256 + (3 if perturbed else 0)), (I, 1)] + [(M, 255), (DEL, 1)] * 31 + [(M, 31)]
    assert len(first) == 64 and len(second) == 65
    return [_read(rng, BASE, first + alternating(200, 5)), _read(rng, BASE, second + alternating(700, 6))], None


def _late(perturbed, rng):
    # reads that start late in pass 0 and end in pass 3 (perturbed: in pass 1)
    reads = [_read(rng, BASE, alternating(60, 7))]
    for j in range(24):
        reads.append(_read(rng, BASE + 3000 + 40 * j, alternating((W // 2 if perturbed else 3 * W) + 17 * j, 8 + j)))
    return reads, None


def _gap(perturbed, rng):
    # the first read ends in pass 0, the last starts in pass 2 (perturbed: in pass 0), nothing between
    far = 200 if perturbed else 2 * W + 100
    return [_read(rng, BASE, alternating(50, 40)), _read(rng, BASE + 10, alternating(90, 41)),
            _read(rng, BASE + far, alternating(300, 42)), _read(rng, BASE + far + 9, alternating(5000, 43))], None


def _early(perturbed, rng):
    # every read ends in pass 1 (perturbed: in pass 3)
    span = 3 * W if perturbed else 5000
    return [_read(rng, BASE + 25 * j, alternating(span + 13 * j, 50 + j)) for j in range(40)], None


def _outlier(perturbed, rng):
    # one read with a 70,000 N among normal reads: its far events lie beyond CAP windows
    skip = 700 if perturbed else 70_000
    reads = [_read(rng, BASE + 31 * j, alternating(5000 + 11 * j, 70 + j)) for j in range(20)]
    reads.insert(7, _read(rng, BASE + 200, alternating(300, 95) + [(SKIP, skip)] + alternating(400, 96)))
    return reads, None


def _cut(perturbed, rng):
    # L inside pass 2 of the first workgroup.  Bad reads: index 6 (from pass 1 over L and over the
    # next window's end, so a split step holds bad events), index 12 (starts just below L) and
    # index 13 (all of it in pass 3); perturbed: L beyond every read
    reads = [_read(rng, BASE + 20 * j, alternating(900 + j, 110 + j)) for j in range(6)]
    reads.append(_read(rng, BASE + W + 100, alternating(2 * W + 300, 120)))
    reads += [_read(rng, BASE + W + 200 + 30 * j, alternating(600, 121 + j)) for j in range(5)]
    reads.append(_read(rng, BASE + 2 * W + 480, alternating(100, 130)))
    reads.append(_read(rng, BASE + 3 * W + 50, alternating(100, 131)))
    return reads, (BASE + 4 * W + 1000 if perturbed else BASE + 2 * W + 500)


def _nbases(perturbed, rng):
    # N bases (and '=' bases, which count nowhere) on both sides of two window ends
    out = []
    for j, letter in enumerate((SB.N, SB.EQ, SB.N)):
        p, ops, codes, q = _read(rng, BASE, [(M, 3 * W)])
        for edge in (W, 2 * W):
            if not perturbed:
                codes[edge - 2 - j: edge + 2 + j] = letter
        q[:] = np.where(np.arange(q.size) % 3 == j, 19, 20)  # on either side of min_base_quality 20
        out.append((p, ops, codes, q))
    return out, None


BUILDERS = {f"span{s}": functools.partial(_span, s) for s in SPANS}
BUILDERS.update(straddle=_straddle, across=_across, batch64=_batch64, late=_late, gap=_gap, early=_early,
                outlier=_outlier, cut=_cut, nbases=_nbases)


def cases():
    return list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name, perturbed=False):
    """(batch, L) of the named case; the batch is sorted (stable) and shared: leave it unchanged."""
    rng = np.random.default_rng(4000 + sorted(BUILDERS).index(name))
    reads, L = BUILDERS[name](perturbed, rng)
    b = SB.pack_batch(reads)
    return b, (SB.max_end(b) + 3 if L is None else L)


# ---- depth: d identical long reads at one start (they share their CIGAR and their bases)
DEEP_SPAN = 9000


@functools.lru_cache(maxsize=2)
def deep_batch(d):
    """(batch of d identical 9 kb many-op reads at BASE, the one read's batch, L)."""
    one = SB.pack_batch([_read(np.random.default_rng(4100), BASE, alternating(DEEP_SPAN, 99))])
    rep = {f: np.repeat(one[f], d) for f in ("pos", "cig_beg", "cig_n", "seq_nib")}
    return dict(one, **rep), one, BASE + DEEP_SPAN + 2
