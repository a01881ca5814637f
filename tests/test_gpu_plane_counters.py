"""The tiled walk's bit-plane counters and tile-relative records at their bounds (bc_planes.h,
bc_walk.h: Planes, counters_reserve, tile_events), against the oracle, np.array_equal throughout.

k_pileup without a quality threshold counts with bit planes; with a threshold, and in the sparse
sweep (k_pileup_solo), the walk keeps the SWAR counters (bc_walk.h: WalkCounters), so mbq 0 and one
threshold, and the shapes `tile` at 4 / 8 / 1 (solo) waves, `tile_no_solo` and `auto`, go through
both.  ``hot_batch(d)`` puts the whole depth d into one (position, column); a chunk of 64 reads adds
8 reads to each of a window's 8 read slots (lanes), and the wave w of S walks chunks w, w + S, ...

  bound (where)                                              depths that meet it
  carry into plane k, a slot's sum reaches 2^k               8 * 2^k - 1, 8 * 2^k, 8 * 2^k + 1 for k = 0..4
    (planes_add2)                                            (7..129) at one wave per tile; x 4, x 8
                                                             waves are covered by 255..1537
  five planes hold 31; the walk folds after a chunk when     191, 192, 193 (three whole chunks: 24 per
    na + 8 > 31, i.e. at 24 reads per slot                    slot, then a fourth chunk) at one wave
    (counters_reserve / planes_fold)                         per tile (tile_no_solo); 767, 768, 769 at
                                                             four waves; 1535, 1536, 1537 at eight
  a position's sum over 8 slots <= 8 x 31 in a byte          192 / 768 / 1536: 8 x 24 = 192 in the byte;
    (planes_join, planes_counts)                             247, 248, 249: 8 x kPlaneAdds itself as a
                                                             depth (the walk has folded at 192 by then)
  chunks that skip counters_reserve (walk_complex)           test_planes_between_complex_chunks
  fix-up nibbles hold 15; folded after a chunk when          63, 64, 65 (blocks N and del: 8 per slot;
    nf + 8 > 15, i.e. after every whole chunk (fix_fold)      A|N and T|del: every other slot) and
                                                             127, 128, 129 (A|N, T|del: half the depth)
  fix-up sum over 8 slots <= 8 x 15 in a byte                64 and up: 8 x 8 = 64
  planes - fix-up without borrow (A = plane0 - N, ...)       blocks N and del (equal), A|N and T|del
  everything again far past every field                      4096
  SWAR nibble <= 14 (the solo / quality instances)           112, 113 and test_gpu_saturation.py

The same depths run with three-run reads (``runs3``: four run slots, the GAP walk, packed
tile-relative records), and with ref_len = HOT_L - 3 (the first out-of-range read, the edge mask).
Every launch asserts the kernel it was meant for (bc_timing_report; bc_pileup_plan for `auto`)."""
import numpy as np
import pytest

import saturation_batches as SB
from basecount_amd import device as D

pytestmark = pytest.mark.gpu

DEPTHS = (7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 112, 113, 127, 128, 129, 191, 192, 193, 247, 248, 249,
          255, 256, 257, 767, 768, 769, 1535, 1536, 1537, 4096)
SHAPES = (("tile", 4, None), ("tile", 8, None), ("tile", 1, None), ("tile_no_solo", 1, None))
MBQS = (0, 20)  # every quality of hot_batch is 40: the threshold passes all, through the QUAL kernels


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    c.timing(True)
    return c


@pytest.fixture(autouse=True)
def _auto_shape(ctx):
    yield
    ctx.set_shape("auto")


def check_auto(ctx, b, L, mbqs, ks):
    """Shape `auto`: the kernel bc_pileup_plan names ran, and its results are the oracle's."""
    r = SB.upload(ctx, b, "auto", 0)
    try:
        kern = {"tiles": "pileup", "solo": "solo", "rc": "rc"}[D.pileup_plan(r, L)["kernel"]]
        for mbq in mbqs:
            cnt6, br = SB.expect(b, L, mbq)
            for k in ks:
                SB.launched(ctx)
                got, bad = SB.pileup_on(ctx, r, L, mbq, k)
                assert SB.launched(ctx) == ({"rc", "stats"} if kern == "rc" else {kern}), ("auto", mbq, k)
                assert bad == br, ("auto", mbq, k)
                SB.same(got, SB.expect_stats(cnt6, k), ("auto", mbq, k))
    finally:
        r.free()


@pytest.mark.parametrize("d", DEPTHS)
def test_plane_counters_hot_columns(ctx, d):
    b = SB.hot_batch(d)
    cnt, br = SB.expect(b, SB.HOT_L, 0)
    assert br == -1 and np.array_equal(cnt, SB.hot_closed_form(d))
    SB.check_sorted(ctx, b, SB.HOT_L, MBQS, SHAPES)
    check_auto(ctx, b, SB.HOT_L, MBQS, (5, 6))
    # three positions past the end: the first out-of-range read, counts below the end exact
    SB.check_sorted(ctx, b, SB.HOT_L - 3, MBQS, SHAPES, ks=(6,))


@pytest.mark.parametrize("d", DEPTHS)
def test_plane_counters_three_run_reads(ctx, d):
    b = SB.hot_batch(d, True)
    cnt, br = SB.expect(b, SB.HOT_L, 0)
    assert br == -1 and np.array_equal(cnt, SB.hot_closed_form(d, True))
    SB.check_sorted(ctx, b, SB.HOT_L, MBQS, SHAPES)
    check_auto(ctx, b, SB.HOT_L, MBQS, (5, 6))
    SB.check_sorted(ctx, b, SB.HOT_L - 3, MBQS, SHAPES)


def test_planes_between_complex_chunks(ctx):
    """Whole chunks of plain `16M` reads and of nine-op reads (walk_complex: the 10-bit fields, no
    counters_reserve) alternate at one start, seven chunks in all: at one wave per tile the planes
    reach 24 per slot with complex chunks in between, fold, and take a fourth plain chunk; at four
    and eight waves each wave sees one kind or both."""
    st = SB.stored_len(SB.COMPLEX_OPS)
    q16, qc = np.full(16, 40, np.uint8), np.full(st, 40, np.uint8)
    reads = []
    for grp in range(7):
        for i in range(64):
            if grp % 2 == 0:
                reads.append((60, [(SB.M, 16)], np.full(16, (SB.A, SB.N, SB.T, SB.C_)[grp // 2], np.uint8), q16))
            else:
                reads.append((60, list(SB.COMPLEX_OPS), np.full(st, (SB.A, SB.N)[i & 1], np.uint8), qc))
    b = SB.pack_batch(reads)
    L = SB.max_end(b)
    SB.check_sorted(ctx, b, L, MBQS, SHAPES)
    SB.check_sorted(ctx, b, L - 3, (0,), SHAPES, ks=(6,))


# ------------------------------------------------------------------- tile-relative records
TILE = 64
SWEEP_OPS = {
    "150M": [(SB.M, 150)],
    "70M5D75M": [(SB.M, 70), (SB.DEL, 5), (SB.M, 75)],
    "10S60M2I78M": [(SB.S, 10), (SB.M, 60), (SB.I, 2), (SB.M, 78)],
    "1M148N1M": [(SB.M, 1), (SB.SKIP, 148), (SB.M, 1)],
    # 64 reads x 125 bytes do not fit the 6144-byte stage: the unstaged walk (nibble index against
    # the whole buffer, widened to 64 bits by the fetch)
    "250M": [(SB.M, 250)],
    "120M10D130M": [(SB.M, 120), (SB.DEL, 10), (SB.M, 130)],
}
SWEEP_L = 200


def sweep_batch(name, per_start=40):
    """One contig of 200 positions; reads of one CIGAR at every start from 149 before tile 1 to 64
    after its first position (read start and end on every offset mod 8 around each window edge and
    both tile edges), ``per_start`` reads per start: several chunks per tile.  Starts below 0 are
    left out (a BAM position is not negative), so the sweep begins at 0, which is -64 from tile 1:
    the clamps of a read's END against every window and the first position of a tile are driven
    in tiles 2 and 3, which the same reads end in at every offset (ends 150 .. 278)."""
    rng = np.random.default_rng(len(name))
    reads = []
    for start in range(max(0, TILE - 149), TILE + 64 + 1):
        for _ in range(per_start):
            reads.append(SB.random_read(rng, start, SWEEP_OPS[name]))
    return SB.pack_batch(reads)


@pytest.mark.parametrize("name", sorted(SWEEP_OPS))
def test_tile_relative_records(ctx, name):
    """Clamps at 0 and 32, negative tile-relative bases and the stage-relative index: every read
    start and end against every window and tile edge, compared with the oracle (the reads run past
    position 200: the first out-of-range read is the oracle's too)."""
    b = sweep_batch(name)
    shapes = (("tile", 4, None), ("tile", 1, None))
    SB.check_sorted(ctx, b, SWEEP_L, MBQS, shapes)
    SB.check_sorted(ctx, b, SB.max_end(b), (0,), shapes, ks=(6,))
