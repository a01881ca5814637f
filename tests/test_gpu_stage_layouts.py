"""Every sequence-layout branch of the tile walk (process_chunk, basecount_amd/csrc/bc_tile.h) against
the oracle: the speculative copy kept, missed and staged again, not issued, chunks walked from HBM,
complex chunks, the stage bound to the byte, the buffer's first and last bytes, an unaligned quality
pointer, and sequence above nibble 2^31.

The inputs are tests/stage_layouts.py's cases; tests/test_stage_layouts_host.py proves from a CPU
model of the decisions that each holds the chunk kinds it is named for.  Every kernel that runs
process_chunk takes every case, for min_base_quality 0 and 20 and k = 5 and 6:

  * k_pileup, general and lean instance forced (shape "tile_no_solo"; bc_pileup_launch_info must
    name the instance asked for), and bc_count's accumulate launch of it into zeroed counts;
  * k_pileup_solo, the one-wave sweep (shape "tile"), and k_sum_exact, the read-parallel summary
    (bc_pileup_summary with no per-position output).  A case's own reference (640-2,048 positions)
    is too deep for the sweep and too short for the summary's whole buffers, so both run on
    stage_layouts.sparse_length: the same reads on a reference of whole 8,192-position buffers,
    where bc_pileup_plan must say "solo".

All five outputs are prefilled with 0xFF bytes and compared bit for bit with O.bcount / O.stats;
bc_range_error must be the oracle's (on cut_short only that is compared, as the reference raises
there)."""
import functools

import numpy as np
import pytest

import oracle as O
import stage_layouts as SL
from basecount_amd import device as D
from basecount_amd.main import norm_factors

pytestmark = pytest.mark.gpu

NAMES = ("counts", "cov", "pc", "ent", "sec")
COMBOS = [(0, 5), (0, 6), (20, 5), (20, 6)]  # (min_base_quality, k)
ids = lambda c: f"q{c[0]}-k{c[1]}"


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    try:
        yield c
    finally:
        c.set_shape("auto")
        c.set_instance("auto")


def stats_of(cnt, k):
    return (cnt[:, :k].T.astype(np.int32),) + tuple(O.stats(cnt, k == 6))


@functools.lru_cache(maxsize=None)
def want(name, L, mbq, k):
    """The oracle's five arrays and first offending read of a case on L positions (computed once)."""
    cnt, (bad, _) = SL.expected(name, L, mbq)
    return stats_of(cnt, k), bad


def run(ctx, reads, L, mbq, k, stats=True):
    """bc_pileup over 0xFF-prefilled outputs (or bc_count into zeroed counts) -> (arrays, bad)."""
    sizes = (4 * k * L, 4 * L, 8 * k * L, 8 * L, 8 * L) if stats else (4 * k * L,)
    bufs = [ctx.alloc(max(8, n)) for n in sizes]
    for x in bufs:
        D.check(D.lib().bc_memset(ctx.h, x.ptr, 0xFF if stats else 0, x.nbytes))
    try:
        if stats:
            ctx.pileup(reads, L, mbq, k, *norm_factors(k), *[x.ptr for x in bufs])
        else:
            ctx.count(reads, L, mbq, k, bufs[0].ptr)
    except D.BcError as e:
        assert e.code == D.BC_E_RANGE, e
    bad = ctx.range_error()
    shapes = ((k, L), (L,), (k, L), (L,), (L,))
    types = (np.int32, np.int32, np.float64, np.float64, np.float64)
    out = tuple(x.download(t, int(np.prod(s))).reshape(s) for x, t, s in zip(bufs, types, shapes))
    for x in bufs:
        x.free()
    return out, bad


def same(got, exp, what):
    (arrays, bad), (earrays, ebad) = got, exp
    assert bad == ebad, (what, "range error", bad, ebad)
    if ebad >= 0:
        return
    for name, a, e in zip(NAMES, arrays, earrays):
        if not np.array_equal(a, e):
            at = np.flatnonzero((a != e).reshape(-1, a.shape[-1]).any(0))
            raise AssertionError(f"{what}: {name} differs at {at.size} positions, first {at[:4].tolist()}")


def tiled(ctx, reads, L, mbq, k, instance, stats=True):
    """k_pileup's forced instance under "tile_no_solo"; the launch must really be that instance."""
    ctx.set_shape("tile_no_solo")
    ctx.set_instance(instance)
    info = D.pileup_launch_info(reads, L, "tile_no_solo", 0, instance, mbq, k)
    assert info["kernel"] == "tiles" and info["lean"] == (instance == "lean"), info
    try:
        return run(ctx, reads, L, mbq, k, stats)
    finally:
        ctx.set_instance("auto")


def sweep(ctx, reads, L, mbq, k):
    """k_pileup_solo under "tile": the plan must say so (else this is one more k_pileup run)."""
    ctx.set_shape("tile")
    assert D.pileup_plan(reads, L, "tile")["kernel"] == "solo"
    return run(ctx, reads, L, mbq, k)


def summary_only(ctx, reads, L, mbq, k):
    """bc_pileup_summary with no per-position output -> its four doubles, and the range error."""
    ctx.set_shape("auto")
    assert D.pileup_plan(reads, L)["kernel"] == "solo" and L >= SL.NP_BUF  # the read-parallel summary's rule
    work, dout = ctx.alloc(D.summary_work_bytes(L)), ctx.alloc(32)
    work.zero()
    ctx.pileup_summary(reads, L, mbq, k, *norm_factors(k), None, None, None, None, None, work.ptr, dout.ptr)
    bad = ctx.range_error()
    out = dout.download(np.float64, 4)
    work.free()
    dout.free()
    return out, bad


def summary_want(arrays):
    cov, ent = arrays[1], arrays[3]
    return np.array([np.mean(cov.astype(np.int64)), np.mean(ent), np.count_nonzero(cov), cov.astype(np.int64).sum()],
                    np.float64)


@pytest.mark.parametrize("combo", COMBOS, ids=ids)
@pytest.mark.parametrize("name", SL.cases())
def test_tiled_instances(ctx, name, combo):
    """k_pileup, general and lean, and bc_count's launch of each into zeroed counts."""
    mbq, k = combo
    b, L = SL.case(name)
    reads = D.DeviceReads(ctx, b)
    try:
        exp = want(name, L, mbq, k)
        for inst in ("general", "lean"):
            same(tiled(ctx, reads, L, mbq, k, inst), exp, (name, inst, mbq, k))
            got, bad = tiled(ctx, reads, L, mbq, k, inst, stats=False)
            same((got, bad), (exp[0][:1], exp[1]), (name, inst, "bc_count", mbq, k))
    finally:
        reads.free()


@pytest.mark.parametrize("combo", COMBOS, ids=ids)
@pytest.mark.parametrize("name", SL.cases())
def test_sweep_and_summary(ctx, name, combo):
    """k_pileup_solo's per-position outputs and the read-parallel summary's four numbers (numpy's over
    the oracle's arrays, as test_summary_only_read_parallel compares them) on the sparse reference."""
    mbq, k = combo
    b, L = SL.case(name)
    big = SL.sparse_length(b, L)
    reads = D.DeviceReads(ctx, b)
    try:
        exp = want(name, big, mbq, k)
        assert exp[1] == -1
        same(sweep(ctx, reads, big, mbq, k), exp, (name, "sweep", mbq, k))
        got, bad = summary_only(ctx, reads, big, mbq, k)
        assert bad == -1 and np.array_equal(got, summary_want(exp[0])), (name, "summary", mbq, k, got)
    finally:
        reads.free()


@pytest.mark.parametrize("shift", [1, 8])
@pytest.mark.parametrize("name", SL.EDGE_CASES)
def test_buffer_edges_unaligned_qual(ctx, name, shift):
    """The same batches with the quality array 1 and 8 bytes off a 16-byte boundary (qual_bytes the
    same): the register staging and the read-parallel summary read it byte by byte."""
    b, L = SL.case(name)
    big = SL.sparse_length(b, L)
    reads = D.DeviceReads(ctx, b)
    moved = ctx.alloc(b["qual"].size + 16)
    try:
        q = np.ascontiguousarray(b["qual"])
        D.check(D.lib().bc_memcpy_h2d(ctx.h, moved.ptr + shift, q.ctypes.data, q.nbytes))
        ctx.sync()
        r = D.BcReads.from_buffer_copy(reads.r)
        r.qual = moved.ptr + shift
        assert r.qual % 16 == shift and r.qual_bytes == q.size
        for k in (5, 6):
            for inst in ("general", "lean"):
                same(tiled(ctx, r, L, 20, k, inst), want(name, L, 20, k), (name, shift, inst, k))
            exp = want(name, big, 20, k)
            same(sweep(ctx, r, big, 20, k), exp, (name, shift, "sweep", k))
            got, bad = summary_only(ctx, r, big, 20, k)
            assert bad == -1 and np.array_equal(got, summary_want(exp[0])), (name, shift, "summary", k, got)
    finally:
        moved.free()
        reads.free()


@pytest.mark.parametrize("mbq", [0, 20])
@pytest.mark.parametrize("layout", ["in_order", "reversed"])
def test_high_nibbles(ctx, layout, mbq):
    """Sequence above nibble 2^31 (stage_layouts.high_nibbles: a seq array of 2^30 + 65,536 bytes, and
    with min_base_quality 20 a quality array of 2^31 + 131,072 bytes, built here and dropped again),
    k = 5, one upload for every kernel shape: both instances of k_pileup, the sweep and the summary
    on the sparse reference, "rc" and "ops".  The time is the upload's: 1 GiB, or 3 GiB with
    qualities (a few seconds)."""
    k = 5
    b, L = SL.high_nibbles(layout, with_qual=mbq > 0)
    big = SL.sparse_length(b, L)
    exp = {}
    for n in (L, big):
        cnt, (bad, _) = O.bcount(n, mbq, b)
        exp[n] = (stats_of(cnt, k), bad)
        assert bad == -1
    reads = D.DeviceReads(ctx, b)
    failed = []

    def check(what, fn):
        try:
            fn()
        except AssertionError as e:
            failed.append(str(e).splitlines()[0][:160])

    try:
        for inst in ("general", "lean"):
            check(inst, lambda: same(tiled(ctx, reads, L, mbq, k, inst), exp[L], (layout, inst, mbq)))
        check("sweep", lambda: same(sweep(ctx, reads, big, mbq, k), exp[big], (layout, "sweep", mbq)))

        def summ():
            got, bad = summary_only(ctx, reads, big, mbq, k)
            assert bad == -1 and np.array_equal(got, summary_want(exp[big][0])), (layout, "summary", mbq, got)
        check("summary", summ)
        for shape in ("rc", "ops"):
            def shaped():
                ctx.set_shape(shape)
                same(run(ctx, reads, L, mbq, k), exp[L], (layout, shape, mbq))
            check(shape, shaped)
    finally:
        ctx.set_shape("auto")
        reads.free()
        del b
    assert not failed, "\n".join(failed)
