"""Where the tiled kernels switch from 32-bit to 64-bit indices, and what the launcher routes on the
wide side (bc_pileup_plan / bc_pileup_launch_info: host arithmetic over a batch header, no GPU
needed).  tiles_fit_i32 (bc_pileup.hip) keeps int32_t while

    n_reads < 0x7FFFFF00  and  ceil(reach / 64) * 64 + max_span + 128 < 0x7FFFFF00,

reach = max(max_end, ref_len).  The library says which side a launch is on through k_pileup's LDS:
the static range hand-off is ``IT rng[8][2]``, 64 B at 32 bits and 128 B at 64.  No slice instance
is built at 64 bits and, with a quality threshold, no lean one: a forced instance falls back there
(tile_instance).  tests/wide_index.py restates the predicate; tests/test_gpu_wide_index.py runs the
wide instances."""
import numpy as np
import pytest

import wide_index as WI
from basecount_amd import device as D

L = 10_000
TILE_SHAPES = [("tile_no_solo", 0), ("tile", 2), ("tile", 4), ("tile", 8)]


def hdr(n=1000, span=150, end=L, words=None):
    return {"n_reads": n, "max_span": span, "max_end": end, "n_cigar_words": n if words is None else words}


def kind(info):
    return "slice" if info["slice"] else "lean" if info["lean"] else "general"


def same_launch_but_rng(narrow, wide):
    assert wide["lds_bytes"] - narrow["lds_bytes"] == 64, (narrow, wide)
    for f in ("kernel", "waves_per_tile", "block_threads"):
        assert narrow[f] == wide[f], (f, narrow, wide)
    assert narrow["kernel"] == "tiles"
    for i in (narrow, wide):
        assert i["blocks"] % 8 == 0 and 0 < i["blocks"] <= 16_384, i


def test_constants():
    assert WI.WIDE_END == 2**31 - 1 and WI.I32_LIMIT == 0x7FFFFF00
    for span in (1, 150, 4096):
        lo, hi = WI.last_narrow_end(span, L), WI.first_wide_end(span, L)
        assert hi == lo + 1 and lo % 64 == 0 and hi <= WI.WIDE_END
        assert WI.fits_i32(1000, lo, span) and not WI.fits_i32(1000, hi, span)
        assert not WI.fits_i32(1000, WI.WIDE_END, span)
    assert WI.fits_i32(WI.I32_LIMIT - 1, L, 150) and not WI.fits_i32(WI.I32_LIMIT, L, 150)


@pytest.mark.parametrize("shape,waves", TILE_SHAPES)
@pytest.mark.parametrize("span", [1, 150, 4096])
def test_threshold_in_tiles(span, shape, waves):
    """One position of max_end apart: 64 B of LDS more, the same kernel, group size and block; the
    grid a multiple of the XCD count below its cap on both sides.  Both calls: the plan (which
    describes the general instance) and the launch of each instance."""
    lo, hi = WI.last_narrow_end(span, L), WI.first_wide_end(span, L)
    same_launch_but_rng(D.pileup_plan(hdr(span=span, end=lo), L, shape, waves),
                        D.pileup_plan(hdr(span=span, end=hi), L, shape, waves))
    for inst, mbq in (("general", 0), ("general", 20), ("lean", 0)):
        a = D.pileup_launch_info(hdr(span=span, end=lo), L, shape, waves, inst, mbq, 5)
        b = D.pileup_launch_info(hdr(span=span, end=hi), L, shape, waves, inst, mbq, 6)
        assert kind(a) == kind(b) == inst
        same_launch_but_rng(a, b)
    assert not WI.is_wide(hdr(span=span, end=lo), L, shape, waves)
    assert WI.is_wide(hdr(span=span, end=hi), L, shape, waves)
    # the reference's own length counts as the batch's end does
    same_launch_but_rng(D.pileup_plan(hdr(span=span, end=100), lo, shape, waves),
                        D.pileup_plan(hdr(span=span, end=100), hi, shape, waves))
    if waves:
        assert D.pileup_plan(hdr(span=span, end=hi), L, shape, waves)["waves_per_tile"] == waves


def test_threshold_in_reads():
    a = D.pileup_launch_info(hdr(n=WI.I32_LIMIT - 1), L, "tile", 4, "general")
    b = D.pileup_launch_info(hdr(n=WI.I32_LIMIT), L, "tile", 4, "general")
    same_launch_but_rng(a, b)
    same_launch_but_rng(D.pileup_plan(hdr(n=WI.I32_LIMIT - 1), L, "tile", 4), D.pileup_plan(hdr(n=WI.I32_LIMIT), L, "tile", 4))
    assert WI.is_wide(hdr(n=WI.I32_LIMIT), L, "tile", 4) and not WI.is_wide(hdr(n=WI.I32_LIMIT - 1), L, "tile", 4)


def test_sweep_plan_has_no_width_term():
    """k_pileup_solo has no static LDS: its plan is the same on both sides, and is_wide evaluates
    the predicate for it."""
    lo, hi = WI.last_narrow_end(150, L), WI.first_wide_end(150, L)
    a, b = D.pileup_plan(hdr(end=lo), L, "tile", 1), D.pileup_plan(hdr(end=hi), L, "tile", 1)
    assert a["kernel"] == b["kernel"] == "solo" and a["lds_bytes"] == b["lds_bytes"]
    assert not WI.is_wide(hdr(end=lo), L, "tile", 1) and WI.is_wide(hdr(end=hi), L, "tile", 1)
    assert WI.is_wide(hdr(end=WI.WIDE_END), L, "auto")  # (so few reads per tile: "auto" sweeps)


# (instance asked for, mbq, one op per read) -> the instance launched at 32 bits, at 64 bits
ROUTING = [
    ("lean", 0, False, "lean", "lean"),
    ("slice", 0, False, "slice", "lean"),     # no slice instance is built at 64 bits
    ("auto", 0, True, "slice", "lean"),       # max_span 150 > 64: slices where they exist
    ("lean", 20, False, "lean", "general"),   # with a threshold no lean instance either
]


@pytest.mark.parametrize("inst,mbq,one_op,narrow,wide", ROUTING)
def test_routing_at_64_bits(inst, mbq, one_op, narrow, wide):
    n = 1000
    words = n if one_op else 3 * n
    for shape, waves in (("tile", 4), ("tile_no_solo", 0)):
        for k in (5, 6):
            a = D.pileup_launch_info(hdr(n, 150, WI.last_narrow_end(150, L), words), L, shape, waves, inst, mbq, k)
            b = D.pileup_launch_info(hdr(n, 150, WI.WIDE_END, words), L, shape, waves, inst, mbq, k)
            assert (kind(a), kind(b)) == (narrow, wide), (shape, k, a, b)
            assert b["lean"] == (wide == "lean") and not b["slice"]
            # the width shows whatever the instance (is_wide asks both sides for the general one
            # where the instance itself differs)
            assert WI.is_wide(hdr(n, 150, WI.WIDE_END, words), L, shape, waves, inst, mbq, k)
            assert not WI.is_wide(hdr(n, 150, WI.last_narrow_end(150, L), words), L, shape, waves, inst, mbq, k)
    # multi-op reads under "auto": general on both sides
    a = D.pileup_launch_info(hdr(n, 150, WI.WIDE_END, 3 * n), L, "tile", 4, "auto", 0, 5)
    assert kind(a) == "general"


def test_fits_i32_restates_the_library():
    """2,000 random headers around both thresholds, judged by the 64 bytes under ("tile", 4)."""
    rng = np.random.default_rng(64)
    base = D.pileup_launch_info(hdr(), L, "tile", 4, "general")["lds_bytes"]
    sides = [0, 0]
    for i in range(2000):
        span = int(rng.choice([1, 30, 150, 151, 1000, 4095, 4096]))
        n, end, ref = 1000, int(rng.integers(1, 100_000)), int(rng.integers(1, 100_000))
        edge = WI.I32_LIMIT - span - 128
        which = i % 4
        if which == 0:    # the batch's end around the tile threshold
            end = edge + int(rng.integers(-200, 200))
        elif which == 1:  # the reference's length around it
            ref = edge + int(rng.integers(-200, 200))
        elif which == 2:  # the read count around its own
            n = WI.I32_LIMIT + int(rng.integers(-3, 3))
        else:             # anywhere: ends up to 2^31 - 1, reads up to 2^32
            end = int(rng.integers(1, 2**31))
            n = int(rng.integers(1, 2**32)) if rng.random() < 0.3 else n
        wide = D.pileup_launch_info(hdr(n, span, end), ref, "tile", 4, "general")["lds_bytes"] - base
        assert wide in (0, 64), (n, span, end, ref)
        assert (wide == 0) == WI.fits_i32(n, max(end, ref), span), (n, span, end, ref)
        sides[wide == 64] += 1
    assert min(sides) >= 500, sides
