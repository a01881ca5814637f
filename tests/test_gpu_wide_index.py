"""The 64-bit-index instances of the tiled kernels against the oracle.

k_pileup and k_pileup_solo are compiled twice over their index type and take int64_t once
tiles_fit_i32 (bc_pileup.hip) fails: at 2^31 - 256 positions of reach, give or take the longest
span.  The wide instances are not the narrow ones with wider integers: without a quality threshold
k_pileup keeps the read-relative records and the SWAR walk (no bit planes) over a stage filled by
LDS-DMA, a combination no 32-bit k_pileup has (the sweep walks so at either width); the range
hand-off, the narrowed search results,
advance_cursor<int64_t> and the routing fall-backs (no slice instance, no lean one with a
threshold) exist on this side only.

Two routes reach them with a few thousand reads and a few thousand positions of output:

  raised bound   bc_reads.max_end is an upper bound of pos + span, which the kernels use to size the
                 tile loop: an ordinary batch inside [0, L) is launched on a copy of its struct with
                 max_end = 2^31 - 1 (wide_index.widen).  Nothing is out of range: every output must
                 be the oracle's, bit for bit.
  far read       the batch's own last reads end at 2^31 - 1: the upload derives that max_end, and the
                 call reports the first of them as the range error, with exact counts below L.

Every tiled launch asserts wide_index.is_wide (the 64 B of LDS the wider range hand-off takes; for
the sweep the predicate itself), every launch the BC_K_* kernel it was written for; outputs are
prefilled with 0xFF bytes; comparisons are np.array_equal against oracle.bcount / oracle.stats.
A widened launch walks 2^25 mostly empty tiles (tens of milliseconds: DESIGN.md section 5), so the
cases are cut into one shape or instance pair per test id."""
import numpy as np
import pytest

import oracle as O
import saturation_batches as SB
import stage_layouts as SL
import test_gpu_stage_layouts as GS
import wide_index as WI
from basecount_amd import device as D
from basecount_amd.main import norm_factors
from test_gpu_parity import random_batch
from test_gpu_saturation import closed_form_holds

pytestmark = pytest.mark.gpu

SHAPE_IDS = [f"{s}{w}" for s, w, _ in SB.TILED_SHAPES]


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    c.timing(True)
    try:
        yield c
    finally:
        c.set_shape("auto")
        c.set_instance("auto")


@pytest.fixture(autouse=True)
def _auto(ctx):
    yield
    ctx.set_shape("auto")
    ctx.set_instance("auto")


# ------------------------------------------------------- 1. every sequence-layout branch, wide
def tiled_wide(ctx, wide, L, mbq, k, inst, stats=True):
    """GS.tiled on the widened batch: the forced instance, 64-bit, and k_pileup is what ran.  With a
    threshold no lean instance is built at 64 bits: the forced one falls back to the general."""
    ctx.set_shape("tile_no_solo")
    ctx.set_instance(inst)
    info = D.pileup_launch_info(wide, L, "tile_no_solo", 0, inst, mbq, k)
    assert info["kernel"] == "tiles" and info["lean"] == (inst == "lean" and mbq == 0) and not info["slice"], info
    assert WI.is_wide(wide, L, "tile_no_solo", 0, inst, mbq, k)
    SB.launched(ctx)
    try:
        got = GS.run(ctx, wide, L, mbq, k, stats)
    finally:
        ctx.set_instance("auto")
    assert SB.launched(ctx) == {"pileup"}, (inst, mbq, k)
    return got


def sweep_wide(ctx, wide, L, mbq, k):
    assert WI.is_wide(wide, L, "tile")
    SB.launched(ctx)
    got = GS.sweep(ctx, wide, L, mbq, k)
    assert SB.launched(ctx) == {"solo"}, (mbq, k)
    return got


def summary_wide(ctx, wide, L, mbq, k):
    """bc_pileup_summary with every per-position output (the sweep that also computes the summary
    partials) -> (five arrays, range error, the four doubles)."""
    ctx.set_shape("tile")
    assert D.pileup_plan(wide, L, "tile")["kernel"] == "solo" and L >= SL.NP_BUF and WI.is_wide(wide, L, "tile")
    bufs = [ctx.alloc(n) for n in (4 * k * L, 4 * L, 8 * k * L, 8 * L, 8 * L)]
    work, dout = ctx.alloc(D.summary_work_bytes(L)), ctx.alloc(32)
    for x in bufs + [work, dout]:
        D.check(D.lib().bc_memset(ctx.h, x.ptr, 0xFF, x.nbytes))
    SB.launched(ctx)
    ctx.pileup_summary(wide, L, mbq, k, *norm_factors(k), *[x.ptr for x in bufs], work.ptr, dout.ptr)
    bad = ctx.range_error()
    assert SB.launched(ctx) == {"solo", "summary"}, (mbq, k)
    shapes = ((k, L), (L,), (k, L), (L,), (L,))
    types = (np.int32, np.int32, np.float64, np.float64, np.float64)
    out = tuple(x.download(t, int(np.prod(s))).reshape(s) for x, t, s in zip(bufs, types, shapes))
    four = dout.download(np.float64, 4)
    for x in bufs + [work, dout]:
        x.free()
    return out, bad, four


@pytest.mark.parametrize("combo", GS.COMBOS, ids=GS.ids)
@pytest.mark.parametrize("name", SL.cases())
def test_layouts_tiled_wide(ctx, name, combo):
    """k_pileup, general and lean forced, bc_pileup and bc_count into zeroed counts.  At mbq 0 the
    staging decisions are those stage_layouts.chunk_plan proves for the 32-bit run; the walk over
    the stage is the one only this side compiles."""
    mbq, k = combo
    b, L = SL.case(name)
    reads = D.DeviceReads(ctx, b)
    try:
        wide = WI.widen(reads)
        exp = GS.want(name, L, mbq, k)
        for inst in ("general", "lean"):
            GS.same(tiled_wide(ctx, wide, L, mbq, k, inst), exp, (name, inst, mbq, k))
            got, bad = tiled_wide(ctx, wide, L, mbq, k, inst, stats=False)
            GS.same((got, bad), (exp[0][:1], exp[1]), (name, inst, "bc_count", mbq, k))
    finally:
        reads.free()


@pytest.mark.parametrize("combo", GS.COMBOS, ids=GS.ids)
@pytest.mark.parametrize("name", SL.cases())
def test_layouts_sweep_and_summary_wide(ctx, name, combo):
    """k_pileup_solo from bc_pileup, and from bc_pileup_summary with every output (its runs of tiles
    are whole quarter buffers there), on the sparse reference."""
    mbq, k = combo
    b, L = SL.case(name)
    big = SL.sparse_length(b, L)
    reads = D.DeviceReads(ctx, b)
    try:
        wide = WI.widen(reads)
        exp = GS.want(name, big, mbq, k)
        assert exp[1] == -1
        GS.same(sweep_wide(ctx, wide, big, mbq, k), exp, (name, "sweep", mbq, k))
        out, bad, four = summary_wide(ctx, wide, big, mbq, k)
        GS.same((out, bad), exp, (name, "bc_pileup_summary", mbq, k))
        assert np.array_equal(four, GS.summary_want(exp[0])), (name, "summary", mbq, k, four)
    finally:
        reads.free()


# ------------------------------------------------------------------ 2. every CIGAR shape, wide
@pytest.mark.parametrize("shape", range(len(SB.TILED_SHAPES)), ids=SHAPE_IDS)
@pytest.mark.parametrize("variant", ["embedded", "deep"])
def test_catalogue_wide(ctx, variant, shape):
    """test_gpu_cigar_edges' catalogue (spans up to kTileMaxSpan) through the sweep and k_pileup at
    1, 2, 4 and 8 waves per tile: other waves read the range hand-off's 64-bit words at S > 1."""
    from test_gpu_cigar_edges import L_TILED

    b = SB.catalogue_batch("tiled", variant, L_TILED)
    assert int(SB.spans(b).max()) == SB.K_TILE_MAX_SPAN
    SB.check_sorted(ctx, b, L_TILED, (0, 20), SB.TILED_SHAPES[shape: shape + 1], max_end=WI.WIDE_END)


# ---------------------------------------------------------------- 3. counters at capacity, wide
WIDE_DEPTHS = (14, 17, 112, 113, 129, 257, 4096)


@pytest.mark.parametrize("shape", range(len(SB.TILED_SHAPES)), ids=SHAPE_IDS)
@pytest.mark.parametrize("runs3", [False, True], ids=["runs1", "runs3"])
@pytest.mark.parametrize("d", WIDE_DEPTHS)
def test_hot_columns_wide(ctx, d, runs3, shape):
    """The SWAR nibble and byte folds at their bounds (test_gpu_saturation.py's table): the walk that
    k_pileup reaches with min_base_quality 0 at 64 bits only."""
    closed_form_holds(d, runs3)
    SB.check_sorted(ctx, SB.hot_batch(d, runs3), SB.HOT_L, (0, 1), SB.TILED_SHAPES[shape: shape + 1],
                    max_end=WI.WIDE_END)


@pytest.mark.parametrize("shape", range(len(SB.TILED_SHAPES)), ids=SHAPE_IDS)
@pytest.mark.parametrize("d", [1022, 1025])
def test_hot_complex_wide(ctx, d, shape):
    """The six 10-bit fields of walk_complex up to and past their flush."""
    b = SB.hot_complex_batch(d)
    cnt, br = SB.expect(b, SB.COMPLEX_L, 0)
    assert br == -1 and np.array_equal(cnt, SB.complex_closed_form(d))
    SB.check_sorted(ctx, b, SB.COMPLEX_L, (0, 1), SB.TILED_SHAPES[shape: shape + 1], max_end=WI.WIDE_END)


# -------------------------------------------------------------------------------- 4. the far read
NEAR_L = 3000  # an edge tile of 56 positions


def near_batch():
    return random_batch(np.random.default_rng(31), NEAR_L, 4000)


@pytest.fixture(scope="module")
def near():
    b = near_batch()
    exp = {}
    for mbq in (0, 20):
        cnt, (br, _) = O.bcount(NEAR_L, mbq, b)
        assert br == -1
        exp[mbq] = cnt
    return b, exp


@pytest.mark.parametrize("shape", range(len(SB.TILED_SHAPES)), ids=SHAPE_IDS)
def test_far_read(ctx, near, shape):
    """Three reads that end at 2^31 - 1 behind 4,000 ordinary ones on 3,000 positions: the first of
    them is the range error (the oracle's, from a table of 3,000 rows), everything below the end
    is counted exactly, and the next call on the context is clean."""
    nb, nexp = near
    n_near = int(nb["pos"].size)
    b = WI.far_batch(nb, np.random.default_rng(32))
    shape, waves, _ = SB.TILED_SHAPES[shape]
    kern = SB.kernel_for(shape, waves, b)
    for mbq in (0, 20):
        _, (br, bp) = O.bcount(NEAR_L, mbq, b)  # (not SB.expect: it sizes its table by max_end)
        assert br == n_near and bp >= WI.WIDE_END - 400
    r = SB.upload(ctx, b, shape, waves)
    try:
        assert r.r.sorted == 1 and r.r.max_end == WI.WIDE_END and r.r.n_reads == n_near + 3
        assert r.r.tile_reads is None  # (no index at 2^25 tiles for 4,003 reads)
        for mbq in (0, 20):
            for k in (5, 6):
                what = (shape, waves, mbq, k)
                assert WI.is_wide(r, NEAR_L, shape, waves, "auto", mbq, k), what
                exp = SB.expect_stats(nexp[mbq], k)
                SB.launched(ctx)
                (got,), bad = GS.run(ctx, r, NEAR_L, mbq, k, stats=False)
                assert SB.launched(ctx) == {kern}, what
                assert bad == n_near, what
                assert np.array_equal(got, exp[0]), what
                got, bad = SB.pileup_on(ctx, r, NEAR_L, mbq, k, fill=0xFF)
                assert SB.launched(ctx) == {kern}, what
                assert bad == n_near, what
                SB.same(got, exp, what)
    finally:
        r.free()
    # the next call, with the near batch alone: 32-bit, exact, no error
    r = SB.upload(ctx, nb, shape, waves)
    try:
        assert not WI.is_wide(r, NEAR_L, shape, waves, "auto", 20, 6)
        got, bad = SB.pileup_on(ctx, r, NEAR_L, 20, 6, fill=0xFF)
        assert SB.launched(ctx) == {kern} and bad == -1
        SB.same(got, SB.expect_stats(nexp[20], 6), (shape, waves, "near alone"))
    finally:
        r.free()


# ------------------------------------------------------------------------------ 5. summaries, wide
@pytest.mark.parametrize("mbq,k", [(0, 5), (20, 6)])
def test_summaries_wide(ctx, mbq, k):
    """bc_pileup + bc_summary, bc_pileup_summary, partials + fold and summary only: four numbers,
    bit for bit, from the 64-bit sweep and the 64-bit k_pileup."""
    L = 2 * 8192 + 517
    b = random_batch(np.random.default_rng(33), L, 3000)
    SB.check_summaries(ctx, b, L, mbq, k, shapes=(("tile", 1), ("tile_no_solo", 1)), max_end=WI.WIDE_END)


# ------------------------------------------------------- 6. the two sides of the threshold agree
@pytest.mark.parametrize("mbq", [0, 20])
@pytest.mark.parametrize("shape,waves", [("tile_no_solo", 0), ("tile", 4)])
def test_threshold_sides_agree(ctx, near, shape, waves, mbq):
    """The same batch with max_end one position apart, the last that takes int32_t and the first
    that takes int64_t: byte-identical outputs, both the oracle's."""
    nb, nexp = near
    r = SB.upload(ctx, nb, shape, waves)
    try:
        span = int(r.r.max_span)
        sides = (WI.widen(r, WI.last_narrow_end(span, NEAR_L)), WI.widen(r, WI.first_wide_end(span, NEAR_L)))
        for k in (5, 6):
            exp = SB.expect_stats(nexp[mbq], k)
            for inst in ("general", "lean"):
                ctx.set_instance(inst)
                raw = []
                for wide, reads in enumerate(sides):
                    what = (shape, waves, inst, mbq, k, "wide" if wide else "narrow")
                    assert WI.is_wide(reads, NEAR_L, shape, waves, inst, mbq, k) == bool(wide), what
                    info = D.pileup_launch_info(reads, NEAR_L, shape, waves, inst, mbq, k)
                    assert info["lean"] == (inst == "lean" and (mbq == 0 or not wide)), what
                    SB.launched(ctx)
                    got, bad = SB.pileup_on(ctx, reads, NEAR_L, mbq, k, fill=0xFF)
                    assert SB.launched(ctx) == {"pileup"} and bad == -1, what
                    SB.same(got, exp, what)
                    raw.append(b"".join(a.tobytes() for a in got))
                assert raw[0] == raw[1], (shape, waves, inst, mbq, k)
    finally:
        ctx.set_instance("auto")
        r.free()
