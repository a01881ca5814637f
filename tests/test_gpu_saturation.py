"""Packed counters at capacity: one-letter columns of depth d through every launch shape.

Uniform random bases put about a quarter of the depth into one column, so the narrow fields of
the hot path never come near the bound their "flush before it overflows" rule assumes.  Here
every block of ``hot_batch(d)`` puts the WHOLE depth d into one (position, column): all A / C / G /
T / N, all deletion, A|N and T|deletion interleaved read by read.  Each depth sits next to a bound:

  bound (where)                                               depths that meet it
  4-bit nibble <= 14, fold at it4 >= 14 (walk_swar/swar_fold) 112, 113, 120, 128, 129: a nibble belongs to
    and byte sums <= 112 (sum8)                               one of a window's 8 read slots, so all
                                                              eight hold 14 (and sum8 112) at depth
                                                              8 x 14; 14..17 fill one slot pair only
  k_rc run-table walk, ++it4 >= 13 / rc_fold                  hot_batch(d, runs3=True) 255, 256, 257 (a
                                                              whole chunk in one window: 4 steps of 64
                                                              reads, so the fold at 13 is out of reach
                                                              of a 256-read chunk)
  k_rc LDS hist: 16-bit half <= 256 per chunk                 runs3 255, 256, 257, 511, 512, 513
  event image: 32 reads agree (xd[5] set), group byte <= 32   31, 32, 33
  event image: four groups <= 128 in a byte                   120, 128, 129
  event image: two halves <= 256 in 16 bits                   255, 256, 257
  event image: xd - nn / xd - ds without borrow, equality     blocks N and del (equality), A/N and
                                                              T/del (plane full, N / DS plane half)
  event image: yd[4], weight-16 carry of the N / DS planes    32 and up (16 N of 32 in A/N; 32 in N)
  six 10-bit fields, flush at pending + nr >= 1023            hot_complex_batch 1022..1025, 2047
    (walk_complex / count_event / flush_acc)
  k_count LDS window: 16-bit half, chunk <= 32768 reads       test_count_window_* (32767 + 1, 32768)
  everything again far past every field                       4096, 65535, 65536, 65537

Blocks start at 60 (mod 64): over an 8-position window edge and a 64-position tile edge.  The
last block ends exactly at the reference end (HOT_L); counted with ref_len = HOT_L - 3 it runs 3
positions past it: the oracle's first offending read, counts below the end still exact.

Everything is compared with oracle.bcount / oracle.stats by np.array_equal, and the oracle's
result is first checked against the closed form (depth d, 100.0 %, entropy 0.0, secondary entropy
1.0 for a one-letter column).  Every launch asserts the BC_K_* kernel it was written for
(bc_timing_report)."""
import numpy as np
import pytest

import saturation_batches as SB
from basecount_amd import device as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    c.timing(True)
    return c


@pytest.fixture(autouse=True)
def _auto_shape(ctx):
    yield
    ctx.set_shape("auto")


def closed_form_holds(d, runs3=False):
    """The oracle's counts of hot_batch(d) are the closed form, and a one-letter column's
    statistics are (100.0, 0.0, 1.0)."""
    b = SB.hot_batch(d, runs3)
    cnt, br = SB.expect(b, SB.HOT_L, 0)
    assert br == -1 and np.array_equal(cnt, SB.hot_closed_form(d, runs3))
    if runs3:
        return
    for k in (5, 6):
        _, cov, pc, ent, sec = SB.expect_stats(cnt, k)
        for j, s in enumerate(SB.hot_starts()[:4]):
            body = slice(s, s + SB.HOT_LEN)
            assert np.all(cov[body] == d) and np.all(pc[j, body] == 100.0)
            assert np.all(ent[body] == 0.0) and np.all(sec[body] == 1.0)
        n_blk = slice(SB.hot_starts()[4], SB.hot_starts()[4] + SB.HOT_LEN)
        assert np.all(cov[n_blk] == (d if k == 6 else 0))


def past_then_exact(ctx, b, L, shapes, repeat_last=False):
    # 3 positions past the end first (both QUAL instances), then the whole reference
    SB.check_sorted(ctx, b, L - 3, (0, 1), shapes, ks=(6,))
    SB.check_sorted(ctx, b, L, (0, 1), shapes, repeat_last=repeat_last)


@pytest.mark.parametrize("d", SB.DEPTHS)
def test_hot_columns_tiled(ctx, d):
    """The sparse sweep (k_pileup_solo) and k_pileup at 1 / 2 / 4 / 8 waves per tile: bc_count with
    5 and 6 columns, bc_pileup with k 5 and 6, at mbq 0 and at mbq 1 with every quality 40."""
    closed_form_holds(d)
    past_then_exact(ctx, SB.hot_batch(d), SB.HOT_L, SB.TILED_SHAPES)
    closed_form_holds(d, True)  # three-run reads: the walk with four run slots
    SB.check_sorted(ctx, SB.hot_batch(d, True), SB.HOT_L, (0, 1), SB.TILED_SHAPES, ks=(6,))


@pytest.mark.parametrize("d", SB.DEPTHS)
def test_hot_columns_read_chunked(ctx, d):
    """k_rc from the upload's run records and chunk summaries, from the records alone and from
    its own CIGAR decode; the call after a range error and a repeated bc_pileup call are exact
    (the accumulation scratch is left zeroed at these depths)."""
    past_then_exact(ctx, SB.hot_batch(d), SB.HOT_L, SB.RC_SHAPES, repeat_last=True)
    # three-run reads: chunks the event image does not take (the run-table walk, rc_fold, the LDS
    # histogram's 16-bit halves)
    past_then_exact(ctx, SB.hot_batch(d, True), SB.HOT_L, SB.RC_SHAPES, repeat_last=True)


@pytest.mark.parametrize("d", SB.DEPTHS)
def test_hot_columns_unsorted_and_device_sort(ctx, d):
    """The same reads permuted: k_count on global atomics at automatic reads_per_block, 1 and
    32768; then bc_reads_sort (every start in eight positions) and a count of the sorted copy."""
    b = SB.hot_batch(d)
    SB.check_unsorted(ctx, b, SB.HOT_L, (0, 1))
    SB.check_unsorted(ctx, b, SB.HOT_L - 3, (0,), rpbs=(0,), ks=(6,))


@pytest.mark.parametrize("d", SB.COMPLEX_DEPTHS)
def test_hot_complex_reads(ctx, d):
    """d identical nine-op reads of one letter: the complex path's six 10-bit fields up to and
    past their flush, in the tiled kernels and in k_rc."""
    b = SB.hot_complex_batch(d)
    cnt, br = SB.expect(b, SB.COMPLEX_L, 0)
    assert br == -1 and np.array_equal(cnt, SB.complex_closed_form(d))
    SB.check_sorted(ctx, b, SB.COMPLEX_L, (0, 1), SB.TILED_SHAPES + SB.RC_SHAPES)
    SB.check_sorted(ctx, b, SB.COMPLEX_L - 3, (0,), SB.TILED_SHAPES + SB.RC_SHAPES[:1], ks=(5,))


# ------------------------------------------------------------------- the LDS window of k_count
def device_bam_batch(ctx, b):
    """A sorted BC_SEQ_BAM batch assembled in device memory by the caller (basecount_hip.h: sorted,
    max_span and max_end set truthfully, no index).  bc_reads_upload always produces BC_SEQ_EVENT,
    which the tiled kernels and k_rc take; this layout is the one that reaches k_count's sorted
    path (the per-chunk LDS window)."""
    r, keep = D.BcReads(), []
    for f, dt in (("pos", np.int32), ("cig_beg", np.uint32), ("cig_n", np.uint32), ("seq_nib", np.uint32),
                  ("cigar", np.uint32), ("seq", np.uint8), ("qual", np.uint8)):
        a = np.ascontiguousarray(b[f], dt)
        keep.append(ctx.alloc(max(16, a.nbytes)).upload(a))
        setattr(r, f, keep[-1].ptr)
    r.n_reads, r.n_cigar_words = b["pos"].size, b["cigar"].size
    r.seq_bytes, r.qual_bytes = b["seq"].size, b["qual"].size
    assert r.qual_bytes >= 2 * r.seq_bytes and np.all(np.diff(b["pos"]) >= 0)
    r.sorted, r.seq_layout = 1, D.BC_SEQ_BAM
    r.max_span, r.max_end = int(SB.spans(b).max()), SB.max_end(b)
    ctx.sync()
    return r, keep


def check_window(ctx, b, L, rpb, mbqs=(0, 20)):
    r, keep = device_bam_batch(ctx, b)
    ctx.set_shape("auto", 0, rpb)
    try:
        for mbq in mbqs:
            cnt6, br = SB.expect(b, L, mbq)
            for k in (5, 6):
                SB.launched(ctx)
                got, bad = SB.count_on(ctx, r, L, mbq, k)
                assert SB.launched(ctx) == {"count"}, (mbq, k)
                assert bad == br, (mbq, k)
                assert np.array_equal(got, cnt6[:, :k].T.astype(np.int32)), (mbq, k)
    finally:
        ctx.set_shape("auto")
        for x in keep:
            x.free()


def test_count_window_full_halves(ctx):
    """Chunks of exactly 32768 reads (reads_per_block = 32768) in one window.  Chunk 0: every read
    `16M` of the letters C A T G N ..., so at each position one 16-bit half holds exactly 0x8000
    (for C, T and N the HIGH half: the word's top bit).  Chunk 1: 32767 reads all C and one all A,
    so both halves of one word are populated, 0x7FFF and 1.  (Both halves of a word cannot be at
    0x8000 together: a chunk has at most 32768 reads and a read adds one event per position.)"""
    b = SB.full_halves_batch()
    L = 188 + 16
    cnt, _ = SB.expect(b, L, 0)
    assert cnt[60, 1] == 0x8000 and cnt[64, 5] == 0x8000 and tuple(cnt[190, :2]) == (1, 0x7FFF)
    check_window(ctx, b, L, 32768)


def test_count_window_hot_batch_32768(ctx):
    """hot_batch(32768) as a BC_SEQ_BAM batch: each block is one 32768-read chunk, the deletion and
    N columns (plane DS|N) included."""
    check_window(ctx, SB.hot_batch(32768), SB.HOT_L, 32768, mbqs=(0, 20))


@pytest.mark.parametrize("wlen", [4095, 4096, 4097])
def test_count_window_switch(ctx, wlen):
    """Around use_lds = wlen <= kWinMax: chunk 0's window is 4095, 4096 or 4097 positions (the
    last falls back to global atomics), chunk 1's a few hundred; then the same batch with the
    reference cut 3 positions before the last read's end: chunk 1's window reaches past L."""
    b = SB.window_batch(wlen)
    assert SB.chunk_window(b, 64, 0) == wlen and SB.chunk_window(b, 64, 1) <= 600
    end = SB.max_end(b)
    check_window(ctx, b, end + 10, 64)
    _, br = SB.expect(b, end - 3, 0)
    assert br >= 64  # a read of chunk 1
    check_window(ctx, b, end - 3, 64)
