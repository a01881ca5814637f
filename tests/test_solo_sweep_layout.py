"""(CPU) The input of test_gpu_solo_sweep.py proves itself: from pos, the spans and the tiles per
wave alone, every piece sweep_layout promises is there, and bc_pileup_plan sends the batch to the
sparse sweep under BC_SHAPE_AUTO.  A change to the generator cannot silently empty a case."""
import numpy as np
import pytest

import oracle as O
import saturation_batches as SB
from basecount_amd import device as D
from test_gpu_solo_sweep import (BUF, BUF_TILES, CLUSTER_SIZES, L_FUSED, L_ROWS, LONG_MIN_TILES, LONG_SPAN, TILE,
                                 cluster_tiles, cut_in_last_cluster, header, layout, tile_view, tiles_per_wave)

CASES = [(L, True) for L in L_FUSED + L_ROWS[:1]] + [(L, False) for L in L_ROWS]


def test_tiles_per_wave_of_the_cases():
    assert [tiles_per_wave(L, True) for L in L_FUSED] == [32, 32, 32]
    assert [tiles_per_wave(L, False) for L in L_ROWS] == [2, 4]


@pytest.mark.parametrize("L,fused", CASES)
def test_layout_holds_every_kind(L, fused):
    b = layout(L, fused)
    tpw = tiles_per_wave(L, fused)
    pos, sp = b["pos"].astype(np.int64), SB.spans(b)
    n_tiles, full = -(-L // TILE), L // TILE
    starts, free, stretches = tile_view(b, L)
    assert np.all(np.diff(pos) >= 0) and pos[0] >= 0 and SB.max_end(b) <= L and starts.size == n_tiles
    first = lambda s: s[0] % tpw == 0                       # starts at a run's first tile
    last = lambda s: (s[0] + s[1] - 1) % tpw == tpw - 1     # ends at a run's last tile
    across = lambda s, m: s[0] // m != (s[0] + s[1] - 1) // m

    # ---- the rule: BC_SHAPE_AUTO takes the sparse sweep, with the tiles per wave laid out for
    h = header(b)
    p = D.pileup_plan(h, L)
    assert h["n_reads"] * (h["max_span"] + 63) / max(L, h["max_end"]) <= 48 and h["max_span"] <= LONG_SPAN
    assert (p["kernel"], p["waves_per_tile"]) == ("solo", 1)
    assert (-(-p["tiles_per_wave"] // 32) * 32 if fused else p["tiles_per_wave"]) == tpw

    # ---- start clusters: every size, one at a single start, first / middle / last tile of a run
    ct = cluster_tiles(b, L)
    assert set(CLUSTER_SIZES) <= set(starts[ct].tolist())
    same = [t for t in ct if np.unique(pos[(pos >> 6) == t]).size == 1]
    assert same and starts[same[0]] >= 65
    assert any(t % tpw == 0 and t > 0 for t in ct) and any(t % tpw == tpw - 1 for t in ct)
    assert tpw == 2 or any(0 < t % tpw < tpw - 1 for t in ct)
    in_cl = np.isin(pos >> 6, ct)
    ops_seen = set()
    for i in np.flatnonzero(in_cl):
        w = b["cigar"][int(b["cig_beg"][i]): int(b["cig_beg"][i]) + int(b["cig_n"][i])]
        ops_seen |= set((w & 15).tolist())
    assert {SB.M, SB.I, SB.DEL, SB.S, SB.EQOP, SB.X} <= ops_seen
    nib = np.stack([b["seq"] >> 4, b["seq"] & 15], 1).ravel()
    acgt = np.isin(nib, (SB.A, SB.C_, SB.G, SB.T))
    stored = sum(int(x) >> 4 for x in b["cigar"] if int(x) & 15 in SB.STORED_OPS)
    other = stored - int(acgt.sum())  # (padding nibbles are 0: neither stored nor A C G T)
    assert 0.03 <= other / stored <= 0.07
    assert b["qual"].max() == 44 and b["qual"].min() == 0

    # ---- read-free stretches as the sweep sees them
    lens = [s[1] for s in stretches]
    assert {1, 2, 3, 31, 32, 33} <= set(lens)
    short = [s for s in stretches if s[1] in (2, 3)]
    assert any(first(s) for s in short) and any(last(s) for s in short) and any(across(s, tpw) for s in short)
    assert any(s[1] == 32 and s[0] % 32 == 0 for s in stretches)                 # a whole quarter
    assert any(s[1] in (31, 32, 33) and across(s, BUF_TILES) for s in stretches)  # over a buffer edge
    # a cluster follows and precedes stretches directly: no stretch holds a start
    assert not starts[free].any()

    # ---- the lone long read: 64 tiles behind it are neither read-free nor started in
    if n_tiles >= LONG_MIN_TILES:
        assert sp.max() == LONG_SPAN and (sp == LONG_SPAN).sum() == 1
        c = int(pos[sp == LONG_SPAN][0]) >> 6
        assert free[c - 1] and starts[c] == 1 and not starts[c + 1: c + 65].any()
        assert not free[c: c + 65].any() and free[c + 65]
        at = int(pos[sp == LONG_SPAN][0])
        mid = SB.expect(b, L, 0)[0][at + 20: at + LONG_SPAN - 20]  # the skipped bases: deletions alone
        assert np.all(mid[:, 4] == 1) and not mid[:, [0, 1, 2, 3, 5]].any()
        assert 5_000 <= pos.size <= 6_000
    else:
        assert sp.max() == TILE
    # tiles the cursors do not see as read-free although nothing lands in them (the shadow of
    # max_span behind every start: 64 tiles behind each with the long read in the batch)
    cov = SB.expect(b, L, 0)[0].sum(1)
    landed = np.add.reduceat(cov, np.arange(0, L, TILE)) > 0
    assert (~free[:landed.size] & ~landed).sum() >= (10 * 64 if n_tiles >= LONG_MIN_TILES else 1)

    # ---- the end of the reference
    part = n_tiles - BUF_TILES * (L // BUF)
    s_end = stretches[-1]
    if L % TILE and part < 3:
        assert pos[-1] + sp[-1] == L and pos[-1] >> 6 == n_tiles - 1 and starts[-1] == 1
        assert s_end[0] + s_end[1] == full and s_end[1] >= 2    # the skip is clipped at L / 64
    else:
        assert s_end[0] + s_end[1] == n_tiles and s_end[1] >= 2  # read-free to the end
        if part:
            assert s_end[0] < BUF_TILES * (L // BUF) < full      # from a whole buffer into the partial one


def test_cut_reference_lies_in_a_cluster():
    """test_sweep_range_error_in_a_cluster's reference: cut inside the last cluster, the oracle
    reports a read there, and AUTO still takes the sweep."""
    L0 = L_FUSED[0]
    b = layout(L0, True)
    L = cut_in_last_cluster(b, L0)
    pos, sp = b["pos"].astype(np.int64), SB.spans(b)
    t = L // TILE
    in_tile = (pos >> 6) == t
    assert in_tile.sum() >= 64 and L >= BUF
    assert (pos[in_tile] + sp[in_tile] <= L).any() and ((pos[in_tile] < L) & (pos[in_tile] + sp[in_tile] > L)).any()
    assert (pos[in_tile] >= L).any()
    for mbq in (0, 20):
        _, (bad, _) = O.bcount(L, mbq, b)
        assert bad >= 0 and (pos[bad] >> 6) == t
    assert D.pileup_plan(header(b), L)["kernel"] == "solo"
