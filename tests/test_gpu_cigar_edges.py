"""CIGAR decode thresholds, both sides of each, through the kernels.

decode_runs / decode_fast2 / pack_runs (bc_runs.h) send a read to the "complex" path on any of the
conditions below; tests/test_runs_decode.py checks the decoders against each other on the host,
this module checks what the kernels count from the result.  The reads of
saturation_batches.catalogue_ops(), by threshold (below | at or above):

  cig_n > kPre (8)            ops8_runs3, ops8_runs4 | ops9_runs3, ops9_runs2 (9 ops, 2 runs), ops9_runs5
  runs > kMaxRuns (4)         ops7_runs4, ops8_runs4 | ops9_runs5   (five runs need four breaking ops
                              between them: no read of eight ops can have five)
  query delta outside int16   ins32767 | ins32768, ins32772          (span 8: stays on the tiled kernels)
  query length > 0xFFFF       qlen65535 | qlen65536 (every delta inside int16); m65535@long | m65536@long
  span <= kTileMaxSpan (4096) span4096 (4M 4088D 4M) | every @long read (k_rc whatever the shape)
  span >= 0x1FFF              span8190@long | span8191@long, span8192@long
  an op length >= 2^13        op8191@long | op8192@long; the 32760+ insertions above
  zero-length ops             zero_len (4M 0D 4M 0I 0M 4M)
  leading D / trailing N      lead_del, trail_skip
  reads that count no base    del_only, ins_only, clip_only, no_cigar (cig_n == 0: bc_reads_upload's
                              host checks accept it)
  no-op ops between two M     mid_H, mid_P, mid_B; mid_S (the reference does not advance the query)
  run boundary on / next to   EDGE_TWO_RUN: 7M|8M|9M + 1D|8D|2I|7N + 8M at every start mod 8
  an 8-position row edge

Bases are random letters from A C G T N M =, qualities random bytes, so a wrong query offset shows
in the counts.  ``embedded``: the catalogue once among 300 random reads; ``deep``: 8 or 12 copies
(more than 300 reads) and one plain read at the end, so every 256-read k_rc chunk holds catalogue
reads only.  Shapes, entry points and the bit-exact standard are those of test_gpu_saturation.py;
mbq 0 and 20."""
import numpy as np
import pytest

import saturation_batches as SB
from basecount_amd import device as D

pytestmark = pytest.mark.gpu

L_TILED, L_LONG, L_SUMMARY = 6_000, 70_000, 2 * 8192 + 37


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    c.timing(True)
    return c


@pytest.fixture(autouse=True)
def _auto_shape(ctx):
    yield
    ctx.set_shape("auto")


@pytest.mark.parametrize("variant", ["embedded", "deep"])
@pytest.mark.parametrize("shapes", ["tiled", "rc"])
def test_catalogue_on_tiled_spans(ctx, variant, shapes):
    """The reads of span <= 4096 through the sparse sweep, k_pileup at every waves-per-tile and
    k_rc (records + summaries, records, CIGARs: same counts, same first bad read as the oracle)."""
    b = SB.catalogue_batch("tiled", variant, L_TILED)
    assert int(SB.spans(b).max()) == SB.K_TILE_MAX_SPAN
    SB.check_sorted(ctx, b, L_TILED, (0, 20), SB.TILED_SHAPES if shapes == "tiled" else SB.RC_SHAPES,
                    repeat_last=shapes == "rc")


@pytest.mark.parametrize("variant", ["embedded", "deep"])
def test_catalogue_with_long_spans(ctx, variant):
    """With the reads of span > 4096 (up to 65,536): k_rc under every shape name."""
    b = SB.catalogue_batch("long", variant, L_LONG)
    assert int(SB.spans(b).max()) == 65_536
    SB.check_sorted(ctx, b, L_LONG, (0, 20), SB.RC_SHAPES + SB.TILED_SHAPES[:2], ks=(6,))


@pytest.mark.parametrize("which,L,cut", [("tiled", L_TILED, 4_500), ("long", L_LONG, 30_000)])
def test_catalogue_past_the_reference_end(ctx, which, L, cut):
    """The reference cut short: the oracle's first out-of-range read from every k_rc input mode
    (so the run with read_runs dropped agrees with the run on the upload's records) and from the
    tiled kernels, and every in-range event still counted."""
    b = SB.catalogue_batch(which, "embedded", L)
    assert SB.expect(b, cut, 0)[1] >= 0
    SB.check_sorted(ctx, b, cut, (0, 20), SB.RC_SHAPES + SB.TILED_SHAPES[:3], ks=(5,))


@pytest.mark.parametrize("which,L", [("tiled", L_TILED), ("long", L_LONG)])
def test_catalogue_unsorted_and_device_sort(ctx, which, L):
    """k_count on the permuted catalogue (its scalar CIGAR cursor), and the device sort of it (reads
    of 65,536 bases: a length past the bucketed record's 16 bits)."""
    b = SB.catalogue_batch(which, "embedded", L)
    SB.check_unsorted(ctx, b, L, (0, 20), rpbs=(0, 1, 32768), ks=(6,))


@pytest.mark.parametrize("mbq,k", [(0, 5), (20, 6)])
def test_catalogue_summaries(ctx, mbq, k):
    """bc_pileup_summary and the summary-only forms on a reference of 2 x 8192 + 37 positions
    holding the catalogue (bc_sum.hip's own read walk on the sparse shape) equal bc_pileup
    followed by bc_summary."""
    b = SB.catalogue_batch("tiled", "embedded", L_SUMMARY)
    SB.check_summaries(ctx, b, L_SUMMARY, mbq, k)


def test_upload_accepts_a_read_without_cigar(ctx):
    """cig_n == 0 passes bc_reads_upload's host checks and counts nothing, alone in its batch."""
    rng = np.random.default_rng(1)
    reads = [SB.random_read(rng, 5, []), SB.random_read(rng, 9, [(SB.M, 8)])]
    b = SB.pack_batch(reads)
    assert b["cig_n"][0] == 0
    SB.check_sorted(ctx, b, 40, (0,), SB.TILED_SHAPES[:2] + SB.RC_SHAPES[:2], ks=(6,))
