"""bc_pileup_plan (host arithmetic, no GPU needed): the waves per tile the tiled pileup takes from
a batch's depth, the workgroup it launches and the LDS it asks for.

The rule (bc_pileup.hip, pileup_waves): with reads_per_tile = n_reads x
(max_span + 63) / reach, one wave per tile (the sparse sweep) up to 48, else the smallest S in
{4, 8} with reads_per_tile <= 512 x S; BC_SHAPE_AUTO hands batches of 2,048 and more reads per
tile to the read-chunked kernel.  A forced tile_waves is taken as given."""
import pytest

from basecount_amd import device as D

SPAN = 129   # max_span + 63 = 192
L = 1_920    # reads_per_tile = n_reads x 192 / 1,920 = n_reads / 10, exact in binary up to rounding
LDS_GRANULE = 1_280
LDS_PER_CU = 160 * 1024


def ceil_div(a, b):
    return -(-a // b)


def plan(n, shape="auto", tile_waves=0, length=L, span=SPAN):
    return D.pileup_plan({"n_reads": n, "max_span": span, "max_end": length}, length, shape, tile_waves)


def test_reads_per_tile_is_the_documented_figure():
    for n in (0, 1, 480, 481, 20_480, 100_000):
        assert plan(n)["reads_per_tile"] == n * (SPAN + 63) / L
    # the reach is the furthest read end when that lies past the reference
    p = D.pileup_plan({"n_reads": 1_000, "max_span": SPAN, "max_end": 2 * L}, L)
    assert p["reads_per_tile"] == 1_000 * 192 / (2 * L)


def test_solo_exactly_up_to_48_reads_per_tile():
    """S = 1 (k_pileup_solo) where reads_per_tile <= 48, as before this rule."""
    for n in (0, 1, 100, 479, 480):
        p = plan(n)
        assert (p["kernel"], p["waves_per_tile"]) == ("solo", 1), n
    for n in (481, 482, 1_000):
        p = plan(n)
        assert p["kernel"] == "tiles" and p["waves_per_tile"] > 1, n
    # tile_no_solo keeps one wave per tile there but runs the tiled kernel
    p = plan(480, "tile_no_solo")
    assert (p["kernel"], p["waves_per_tile"], p["block_threads"]) == ("tiles", 1, 256)


def test_wave_boundaries_sit_where_the_rule_says():
    """Four waves per tile from just above 48 up to 2,048 reads per tile, eight beyond; never two
    (the sweep in DESIGN.md: two waves per tile were behind four at every depth)."""
    for n in (481, 960, 1_920, 1_921, 3_840, 7_120, 20_470, 20_480):
        p = plan(n, "tile")
        assert (p["kernel"], p["waves_per_tile"]) == ("tiles", 4), n
    for n in (20_481, 30_000, 100_000):
        p = plan(n, "tile")
        assert (p["kernel"], p["waves_per_tile"]) == ("tiles", 8), n
    # BC_SHAPE_AUTO: the read-chunked kernel from 2,048 reads per tile on (the switch stays)
    assert plan(20_479)["kernel"] == "tiles" and plan(20_479)["waves_per_tile"] == 4
    for n in (20_480, 20_481, 100_000):
        p = plan(n)
        assert (p["kernel"], p["waves_per_tile"], p["block_threads"]) == ("rc", 0, 0), n
    # the headline shape: 100,000 reads of 150 bp on 29,903 positions
    p = D.pileup_plan({"n_reads": 100_000, "max_span": 150, "max_end": 29_903}, 29_903)
    assert (p["kernel"], p["waves_per_tile"], p["block_threads"], p["blocks"]) == ("tiles", 4, 256, 472)


def test_plan_is_monotone_in_depth():
    for shape in ("auto", "tile", "tile_no_solo"):
        last = 0
        for n in range(0, 20_480, 37):
            p = plan(n, shape)
            assert p["kernel"] != "rc"
            assert p["waves_per_tile"] >= last, (shape, n)
            last = p["waves_per_tile"]
        assert last == 4
    last = 0
    for n in range(0, 60_000, 113):
        w = plan(n, "tile")["waves_per_tile"]
        assert w >= last
        last = w
    assert last == 8


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_forced_tile_waves_are_respected(waves):
    for n in (1, 480, 481, 5_000, 50_000):
        for shape in ("tile", "tile_no_solo"):
            p = plan(n, shape, waves)
            if waves == 1 and shape == "tile":
                assert (p["kernel"], p["waves_per_tile"]) == ("solo", 1)
                continue
            assert (p["kernel"], p["waves_per_tile"]) == ("tiles", waves), (n, shape)
            assert p["block_threads"] == 64 * max(4, waves)
            groups = max(4, waves) // waves  # tiles per workgroup
            blocks = ceil_div(ceil_div(L, 64), groups)
            assert p["blocks"] == 8 * ceil_div(blocks, 8)  # a multiple of the 8 XCDs


def test_four_four_wave_blocks_fit_a_cu():
    """The LDS of a four-wave workgroup, rounded up to the 1,280 B the hardware allocates in, fits
    a CU's 160 KiB four times (16 waves: all the CU's wave slots at this kernel's registers), and
    an eight-wave workgroup twice."""
    def rounded(b):
        return ceil_div(b, LDS_GRANULE) * LDS_GRANULE

    four = plan(5_000, "tile", 4)["lds_bytes"]
    eight = plan(5_000, "tile", 8)["lds_bytes"]
    assert 4 * rounded(four) <= LDS_PER_CU
    assert 2 * rounded(eight) <= LDS_PER_CU
    assert four == 40_576 + 64 and eight == 77_568 + 64  # dynamic + the static range hand-off


def test_tiles_per_wave_of_the_sparse_sweep():
    """tiles_per_wave is bc_pileup's sweep run: one tile per wave up to 32,768 tiles (2^21
    positions), then ceil(tiles / 32,768); the furthest read end counts as in the reach; 0 for the
    tiled and the read-chunked plans."""
    for tiles, want in ((1, 1), (2, 1), (32_767, 1), (32_768, 1), (32_769, 2), (65_536, 2), (65_537, 3),
                        (98_304, 3), (98_305, 4), (98_306, 4), (131_072, 4), (131_073, 5)):
        for length in (64 * (tiles - 1) + 1, 64 * tiles):  # the first and the last length of that many tiles
            # (a reference of a tile or two is "deep" with any read on it: the sweep forced there)
            p = plan(100, length=length) if tiles > 2 else plan(1, "tile", 1, length=length)
            assert (p["kernel"], p["waves_per_tile"], p["tiles_per_wave"]) == ("solo", 1, want), (tiles, length)
            assert p["blocks"] == 8 * ceil_div(ceil_div(ceil_div(tiles, want), 4), 8)
    # the two rows-mode references of test_gpu_solo_sweep.py
    assert plan(5_500, length=2**21 + 101, span=4_096)["tiles_per_wave"] == 2
    assert plan(5_500, length=3 * 2**21 + 101, span=4_096)["tiles_per_wave"] == 4
    # edge tiles past the reference end are swept too
    p = D.pileup_plan({"n_reads": 100, "max_span": SPAN, "max_end": 2**21 + 1}, 2**21)
    assert (p["kernel"], p["tiles_per_wave"]) == ("solo", 2)
    p = plan(100, "tile", 1, length=2**22 + 1)
    assert (p["kernel"], p["tiles_per_wave"]) == ("solo", 3)
    for p in (plan(480, "tile_no_solo"), plan(481), plan(5_000, "tile", 4), plan(100, "tile_no_solo", 1, length=2**22),
              plan(20_480), plan(100, "rc"), plan(100, "rc", length=2**22)):
        assert p["kernel"] in ("tiles", "rc") and p["tiles_per_wave"] == 0, p


def test_bad_arguments():
    with pytest.raises(D.BcError):
        plan(100, "tile", 3)
    with pytest.raises(D.BcError):
        D.pileup_plan({"n_reads": -1, "max_span": 1, "max_end": 1}, 10)
    p = plan(100)
    assert p["blocks_per_cu"] == -1 or p["blocks_per_cu"] >= 1
