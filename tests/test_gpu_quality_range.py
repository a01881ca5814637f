"""The quality comparison over the whole byte range.

The kernels hold four scalar versions of ``qual >= min_base_quality`` (count_event, rc_complex,
walk_read, qual_mask_at) and three SWAR ones (stage_regs, k_rc staging, bc_sum.hip's
count_counted), with separate branches for a threshold with bit 7 set (ge_bytes: m & 0x80) and
for one above 255 (qual_nibmask: m > 255).  The other tests use thresholds 0 / 20 / 30 / 40 on
quality bytes 0..44.  Here the bytes are uniform over 0..255, one read in ten is entirely 0xFF,
0x80 or 0x7F, and the thresholds are 1, 2, 127, 128, 129, 200, 254, 255, 256 and 1000, through
every launch shape, the unsorted k_count, and the summary-only path."""
import numpy as np
import pytest

import saturation_batches as SB
from basecount_amd import device as D

pytestmark = pytest.mark.gpu

L = 3_000


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    c.timing(True)
    return c


@pytest.fixture(autouse=True)
def _auto_shape(ctx):
    yield
    ctx.set_shape("auto")


@pytest.mark.parametrize("mbq", SB.QUAL_THRESHOLDS)
def test_threshold_every_shape(ctx, mbq):
    b = SB.quality_batch(L)
    SB.check_sorted(ctx, b, L, (mbq,), SB.TILED_SHAPES + SB.RC_SHAPES)
    SB.check_unsorted(ctx, b, L, (mbq,), rpbs=(0,), ks=(6,))


@pytest.mark.parametrize("mbq", SB.QUAL_THRESHOLDS)
def test_threshold_summary_paths(ctx, mbq):
    """bc_sum.hip's count_counted (the summary-only walk of a sparse batch) and the fused tails."""
    Ls = 8192 + 3_000
    SB.check_summaries(ctx, SB.quality_batch(Ls, 2_000), Ls, mbq, 6 if mbq & 1 else 5)


@pytest.mark.parametrize("mbq", [1, 128, 255])
def test_qual_array_ends_with_the_last_read(ctx, mbq):
    """No padding after the last read: qual_bytes == 2 * seq_bytes and the last base is the last
    or the last but one byte, so the vectorised quality loads (q0 + 32 <= qual_bytes) end in
    their byte-wise tail."""
    b = SB.quality_batch(L, 600, tight=True)
    assert b["qual"].size == 2 * b["seq"].size
    SB.check_sorted(ctx, b, L, (mbq,), SB.TILED_SHAPES[:3] + SB.RC_SHAPES, ks=(6,))
    SB.check_unsorted(ctx, b, L, (mbq,), rpbs=(0,), ks=(6,))


def test_qualities_from_an_odd_host_address(ctx):
    """bc_reads_upload from a qualities array at an odd byte offset."""
    b = SB.quality_batch(L, 600)
    buf = np.zeros(b["qual"].size + 1, np.uint8)
    buf[1:] = b["qual"]
    q = buf[1:]
    assert q.ctypes.data & 1 and q.flags["C_CONTIGUOUS"]
    SB.check_sorted(ctx, dict(b, qual=q), L, (129,), SB.TILED_SHAPES[:2] + SB.RC_SHAPES[:1], ks=(6,))
