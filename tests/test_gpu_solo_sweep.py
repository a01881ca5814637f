"""The sparse sweep (k_pileup_solo, bc_pileup.hip) where a wave takes MORE than one tile: the
fused-summary calls (runs of 32 tiles) and references above 2^21 positions (bc_pileup /
bc_count, 2 and 4 tiles per wave).  Only there do the read cursors move (advance_cursor: the
window reload, the whole-window continuation), is a run of read-free tiles stored as constants
(clipped at the next read's tile, at the end of the wave's run and at the last full tile), and
does the chain of numpy's leaves mix empty and non-empty tiles.

``sweep_layout`` builds the input: a dense target on an otherwise empty reference (amplicon /
panel data), every piece placed by what the SWEEP sees.  A tile is read-free for the sweep when no
read starts in [tile start - max_span + 1, tile end]: behind every read lies a shadow of
max_span / 64 tiles that are walked though nothing lands in them.  tests/test_solo_sweep_layout.py
(CPU) proves from pos, the spans and the tiles per wave alone that each piece is there.

Counts, coverage, percentages and both entropies are compared with the oracle bit for bit over
the whole reference, every output buffer pre-filled with 0xFF bytes so that a forgotten store
shows; the summary's four doubles with numpy over the oracle's arrays."""
import functools

import numpy as np
import pytest

import saturation_batches as SB
from basecount_amd import device as D
from basecount_amd.main import norm_factors

pytestmark = pytest.mark.gpu

TILE, BUF = 64, 8192
BUF_TILES = BUF // TILE
CLUSTER_SIZES = (64, 65, 128, 129, 300)  # one window of starts, one more, two, one more, several
LONG_SPAN = SB.K_TILE_MAX_SPAN           # the lone long read: 20M 4056N 20M
LONG_MIN_TILES = 4096                    # layouts of fewer tiles have no room for its shadows
ACGT = np.array([SB.A, SB.C_, SB.G, SB.T], np.uint8)
OTHER = np.array([SB.N, SB.EQ, 5, SB.IUPAC_M], np.uint8)  # N, =, R, M: 5 % of the letters

# (L, fused): the references of the tests below.  Fused: two buffers + a last tile of 37
# positions; three whole buffers; two buffers + four tiles + 37 (the reference ends read-free,
# inside the last partial buffer).  Rows mode: two and four tiles per wave.
L_FUSED = (2 * BUF + 37, 3 * BUF, 2 * BUF + 4 * TILE + 37)
L_ROWS = (2**21 + 101, 3 * 2**21 + 101)


def tiles_per_wave(L, fused):
    """The library's own figure (bc_pileup_plan) for a sparse batch on L positions; the
    fused-summary calls round it up to a multiple of 32 (include/basecount_hip.h)."""
    tpw = D.pileup_plan({"n_reads": 1, "max_span": 64, "max_end": L}, L)["tiles_per_wave"]
    return -(-tpw // 32) * 32 if fused else tpw


def header(b):
    """What bc_pileup_plan reads of a batch."""
    return {"n_reads": int(b["pos"].size), "max_span": int(SB.spans(b).max()), "max_end": SB.max_end(b)}


def letters(rng, q):
    codes = ACGT[rng.integers(0, 4, q)]
    other = rng.random(q) < 0.05
    codes[other] = OTHER[rng.integers(0, OTHER.size, int(other.sum()))]
    return codes


def read_at(rng, pos, ops):
    q = SB.stored_len(ops)
    return (int(pos), list(ops), letters(rng, q), rng.integers(0, 45, q).astype(np.uint8))


def cluster_ops(rng):
    """Soft clips, M / = / X stretches with insertions and deletions between them; span <= 64."""
    while True:
        ops = []
        if rng.random() < 0.4:
            ops.append((SB.S, int(rng.integers(1, 6))))
        ops.append((int(rng.choice([SB.M, SB.EQOP, SB.X])), int(rng.integers(2, 20))))
        for _ in range(int(rng.integers(0, 3))):
            ops.append((int(rng.choice([SB.I, SB.DEL])), int(rng.integers(1, 5))))
            ops.append((int(rng.choice([SB.M, SB.EQOP, SB.X])), int(rng.integers(2, 20))))
        if rng.random() < 0.4:
            ops.append((SB.S, int(rng.integers(1, 6))))
        if SB.ref_span(ops) <= TILE:
            return ops


def sweep_layout(L, tpw, rng):
    """A sorted batch on L positions for a sweep of ``tpw`` tiles per wave (tpw >= 2).  Pieces, in
    reference order (D = max_span / 64 + 1 tiles behind a start are not read-free):
      1. two read-free tiles at a run's first tile (tiles 0, 1), then a cluster of 64 starts
      2. one read-free tile alone (the skip needs two), then one read
      3. a cluster of 65 reads at ONE start, three read-free tiles ending at a run's last tile,
         a cluster of 128 in the next run's first tile
      4. 32 read-free tiles aligned at 32 (a whole quarter of a summary buffer); 33 across an
         8192-position buffer edge, then a cluster of 129 in a run's last tile; 31, then a
         cluster of 300 in the middle of a run (tpw > 2)
      5. two read-free tiles across a run boundary
      6. from 4,096 tiles on: a lone read of span 4,096 (20M 4056N 20M; the skipped bases count
         as deletions) in a read-free stretch: with it in the batch the lo cursor trails hi by 64
         tiles, and the 64 tiles behind EVERY start above are walked though nothing lands in
         them; then scattered further clusters up to about 5,500 reads
      7. the end: a read ending at L - 1 in the last, partial tile behind a read-free run; or,
         with L % 64 == 0 or a last partial buffer of three or more tiles, a read-free run to the
         end of the reference.
    max_span is 64 exactly without the long read, 4,096 with it."""
    assert tpw >= 2
    n_tiles, full = -(-L // TILE), L // TILE
    long_read = n_tiles >= LONG_MIN_TILES
    ms = LONG_SPAN if long_read else TILE
    shadow = ms // TILE + 1  # first read-free tile behind a start at offset >= 1 of tile c: c + shadow
    reads = []

    def one(tile, ops=None):
        reads.append(read_at(rng, tile * TILE + int(rng.integers(1, TILE)), ops or cluster_ops(rng)))

    def cluster(tile, size, same=False):
        offs = np.full(size, int(rng.integers(1, TILE))) if same else rng.integers(0, TILE, size)
        if not same:
            offs[:2] = (0, TILE - 1)  # both ends of the tile
        reads.extend(read_at(rng, tile * TILE + int(o), cluster_ops(rng)) for o in offs)

    def align(t, a, m=None):  # the first tile >= t that is a (mod m)
        m = m or tpw
        return t + (a - t) % m

    cluster(2, 64)                                   # 1
    t = 2 + shadow
    one(t + 1, None if long_read else [(SB.M, TILE)])  # 2 (the read of span 64 exactly)
    t = t + 1 + shadow
    c = align(t + shadow + 3, 0) - shadow - 3        # 3
    cluster(c, 65, same=True)
    cluster(c + shadow + 3, 128)
    t = c + shadow + 3 + shadow
    s = align(t + shadow, 0, 32)                     # 4: the whole quarter
    one(s - shadow)
    one(s + 32)
    t = s + 32 + shadow
    k = -(-(t + shadow + 2) // BUF_TILES)            # 33 tiles from two before a buffer edge
    while (BUF_TILES * k + 31) % tpw != tpw - 1:
        k += 1
    s = BUF_TILES * k - 2
    one(s - shadow)
    cluster(s + 33, 129)
    t = s + 33 + shadow
    c = t                                            # 31 tiles, the cluster mid-run
    while tpw > 2 and (c + shadow + 31) % tpw in (0, tpw - 1):
        c += 1
    one(c)
    cluster(c + shadow + 31, 300)
    t = c + shadow + 31 + shadow
    s = align(t + shadow, tpw - 1)                   # 5
    one(s - shadow)
    one(s + 2)
    t = s + 2 + shadow
    if long_read:                                    # 6
        c = t + 5
        reads.append(read_at(rng, c * TILE + 17, [(SB.M, 20), (SB.SKIP, LONG_SPAN - 40), (SB.M, 20)]))
        t = c + shadow
        more = 40
        sizes = rng.multinomial(5_500 - len(reads), np.full(more, 1.0 / more))
        for tile, size in zip(rng.integers(t + 3, full - 2 * shadow, more), sizes):
            if size >= 2:
                cluster(int(tile), int(size))
    assert t + 2 <= full, "the reference has no room for the layout"
    part = n_tiles - BUF_TILES * (L // BUF)          # 7: tiles of the last partial buffer
    if L % TILE and part < 3:
        span = min(20, L % TILE)
        reads.append(read_at(rng, L - span, [(SB.M, span)]))
    return SB.pack_batch(reads)


def tile_view(b, L):
    """(starts per tile, read-free as the sweep sees it, [(first tile, length)] of the maximal
    read-free stretches), from pos and the spans alone."""
    pos = b["pos"].astype(np.int64)
    ms = int(SB.spans(b).max())
    n_tiles = -(-max(L, SB.max_end(b)) // TILE)
    t0 = np.arange(n_tiles, dtype=np.int64) * TILE
    free = np.searchsorted(pos, t0 - ms + 1, "left") >= np.searchsorted(pos, t0 + TILE, "left")
    edge = np.flatnonzero(np.diff(np.concatenate([[0], free.astype(np.int8), [0]])))
    stretches = [(int(a), int(z - a)) for a, z in zip(edge[0::2], edge[1::2])]
    return np.bincount(pos >> 6, minlength=n_tiles), free, stretches


def cluster_tiles(b, L):
    """Tiles holding 64 or more starts."""
    return np.flatnonzero(tile_view(b, L)[0] >= 64)


@functools.lru_cache(maxsize=None)
def layout(L, fused):
    b = sweep_layout(L, tiles_per_wave(L, fused), np.random.default_rng(L % 100_003 + fused))
    return b


@functools.lru_cache(maxsize=2)
def expected(L, fused, mbq, k):
    """The oracle's five arrays of layout(L, fused): computed once per case, left unchanged."""
    cnt6, bad = SB.expect(layout(L, fused), L, mbq)
    assert bad == -1
    return SB.expect_stats(cnt6, k)


def summary_of(exp):
    cov, ent = exp[1], exp[3]
    c64 = cov.astype(np.int64)
    return [float(np.mean(c64)), float(np.mean(ent)), float(np.count_nonzero(cov)), float(c64.sum())]


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    c.timing(True)
    return c


@pytest.fixture(autouse=True)
def _auto_shape(ctx):
    yield
    ctx.set_shape("auto")


def sentinel(ctx, bufs):
    for x in bufs:
        D.check(D.lib().bc_memset(ctx.h, x.ptr, 0xFF, x.nbytes))


def run(ctx, r, L, mbq, k, call):
    """One of bc_pileup / bc_pileup_summary / bc_pileup_partials + bc_summary_fold with every
    output, percentages included, into buffers of 0xFF bytes: (the five arrays, the summary's four
    doubles or None, the range error)."""
    nf, nf2 = norm_factors(k)
    bufs = [ctx.alloc(n) for n in (4 * k * L, 4 * L, 8 * k * L, 8 * L, 8 * L)]
    extra = [] if call == "pileup" else [ctx.alloc(D.summary_work_bytes(L)), ctx.alloc(32)]
    try:
        sentinel(ctx, bufs + extra)
        ptrs = [x.ptr for x in bufs]
        if call == "pileup":
            ctx.pileup(r, L, mbq, k, nf, nf2, *ptrs)
        elif call == "summary":
            ctx.pileup_summary(r, L, mbq, k, nf, nf2, *ptrs, extra[0].ptr, extra[1].ptr)
        else:
            ctx.pileup_partials(r, L, mbq, k, nf, nf2, *ptrs, extra[0].ptr)
            ctx.summary_fold([L], [extra[0].ptr], [extra[1].ptr])
        bad = ctx.range_error()
        got = (bufs[0].download(np.int32, k * L).reshape(k, L), bufs[1].download(np.int32, L),
               bufs[2].download(np.float64, k * L).reshape(k, L), bufs[3].download(np.float64, L),
               bufs[4].download(np.float64, L))
        s = extra[1].download(np.float64, 4).tolist() if extra else None
    finally:
        for x in bufs + extra:
            x.free()
    return got, s, bad


@pytest.mark.parametrize("L", L_FUSED)
@pytest.mark.parametrize("mbq", [0, 20])
@pytest.mark.parametrize("k", [5, 6])
def test_sweep_fused_summary_clusters(ctx, k, mbq, L):
    """bc_pileup_summary and bc_pileup_partials + bc_summary_fold, percentages included, runs of
    32 tiles per wave: under "auto" and under ("tile", 1) the five arrays are the oracle's and the
    four summary doubles numpy's; the sweep ran, not the tiled or the read-chunked kernel."""
    b = layout(L, True)
    exp = expected(L, True, mbq, k)
    want = summary_of(exp)
    assert D.pileup_plan(header(b), L)["kernel"] == "solo"
    for shape in (("auto", 0), ("tile", 1)):
        r = SB.upload(ctx, b, *shape)
        try:
            for call in ("summary", "partials"):
                SB.launched(ctx)
                got, s, bad = run(ctx, r, L, mbq, k, call)
                ran = SB.launched(ctx)
                assert "solo" in ran and not ran & {"pileup", "rc"}, (shape, call, ran)
                assert bad == -1
                SB.same(got, exp, (shape, call))
                assert s == want, (shape, call)
        finally:
            r.free()


def test_sweep_fused_summary_long_read(ctx):
    """The fused-summary sweep with the span-4,096 read in the batch (the layout for runs of 32
    tiles on 2^21 + 101 positions): the 64 tiles behind every start are walked with nothing landing
    in them, so numpy's leaves mix tiles that are empty for the cursors, tiles that only count as
    not empty, and covered ones."""
    L, k, mbq = L_ROWS[0], 5, 0
    b = layout(L, True)
    exp = expected(L, True, mbq, k)
    r = SB.upload(ctx, b)
    try:
        assert D.pileup_plan(r, L)["kernel"] == "solo" and r.r.max_span == LONG_SPAN
        for call in ("summary", "partials"):
            SB.launched(ctx)
            got, s, bad = run(ctx, r, L, mbq, k, call)
            ran = SB.launched(ctx)
            assert "solo" in ran and not ran & {"pileup", "rc"}, (call, ran)
            assert bad == -1
            SB.same(got, exp, call)
            assert s == summary_of(exp), call
    finally:
        r.free()


@pytest.mark.parametrize("L", L_ROWS)
def test_sweep_rows_mode_above_2_21(ctx, L):
    """bc_pileup with percentages (the CLI's rows call) above 2^21 positions: two and four tiles
    per wave, the lone span-4,096 read, all five arrays the oracle's."""
    k, mbq = 6, 20
    b = layout(L, False)
    r = SB.upload(ctx, b)
    try:
        p = D.pileup_plan(r, L)
        assert (p["kernel"], p["tiles_per_wave"]) == ("solo", 2 if L == L_ROWS[0] else 4)
        assert 5_000 <= r.n <= 6_000
        SB.launched(ctx)
        got, _, bad = run(ctx, r, L, mbq, k, "pileup")
        assert SB.launched(ctx) == {"solo"}
        assert bad == -1
        SB.same(got, expected(L, False, mbq, k), L)
    finally:
        r.free()


@pytest.mark.parametrize("k", [5, 6])
def test_sweep_count_accumulates_above_2_21(ctx, k):
    """bc_count twice into one zeroed histogram through the sweep at two tiles per wave (no
    skip: every tile is read, added to and written back): twice the oracle's counts everywhere,
    and bc_stats over it gives twice the oracle's coverage."""
    L, mbq = L_ROWS[0], 20
    b = layout(L, False)
    exp = expected(L, False, mbq, k)
    r = SB.upload(ctx, b)
    hist = ctx.alloc(4 * k * L)
    outs = [ctx.alloc(n) for n in (4 * L, 8 * k * L, 8 * L, 8 * L)]
    try:
        assert D.pileup_plan(r, L)["tiles_per_wave"] == 2
        hist.zero()
        SB.launched(ctx)
        ctx.count(r, L, mbq, k, hist.ptr)
        ctx.count(r, L, mbq, k, hist.ptr)
        assert ctx.range_error() == -1
        assert SB.launched(ctx) == {"solo"}
        assert np.array_equal(hist.download(np.int32, k * L).reshape(k, L), 2 * exp[0])
        sentinel(ctx, outs)
        nf, nf2 = norm_factors(k)
        ctx.stats(hist.ptr, L, k, nf, nf2, *[x.ptr for x in outs])
        assert np.array_equal(outs[0].download(np.int32, L), 2 * exp[1])
    finally:
        for x in [hist] + outs:
            x.free()
        r.free()


def cut_in_last_cluster(b, L):
    """A reference length inside the last cluster of 64 or more starts: some of its reads end
    before it, some run across it, some start behind it."""
    return int(cluster_tiles(b, L)[-1]) * TILE + 30


def test_sweep_range_error_in_a_cluster(ctx):
    """The reference cut inside the last cluster: the first offending read is the oracle's, the
    in-range positions are exact (saturation_batches.check_sorted's convention), and the next
    call with the whole reference is clean."""
    L0 = L_FUSED[0]
    b = layout(L0, True)
    L = cut_in_last_cluster(b, L0)
    assert L >= BUF and D.pileup_plan(header(b), L)["kernel"] == "solo"
    for mbq, k in ((0, 5), (20, 6)):
        cnt6, br = SB.expect(b, L, mbq)
        assert br >= 0
        exp = SB.expect_stats(cnt6, k)
        for shape, call in ((("tile", 1), "summary"), (("auto", 0), "pileup")):
            r = SB.upload(ctx, b, *shape)
            try:
                SB.launched(ctx)
                got, _, bad = run(ctx, r, L, mbq, k, call)
                assert "solo" in SB.launched(ctx)
                assert bad == br, (shape, call)
                SB.same(got, exp, (shape, call, "cut"))
                got, s, bad = run(ctx, r, L0, mbq, k, call)
                assert bad == -1
                whole = expected(L0, True, mbq, k)
                SB.same(got, whole, (shape, call, "whole"))
                assert s is None or s == summary_of(whole)
            finally:
                r.free()
