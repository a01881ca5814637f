"""(CPU) The inputs of test_gpu_saturation.py / test_gpu_cigar_edges.py / test_gpu_quality_range.py
prove themselves: worked out from the batches alone, with numpy, each bound of the packed counters
is met by some generated batch, each decode threshold has a read on either side, and the oracle
gives the closed form over the whole depth ladder."""
import numpy as np
import pytest

import oracle as O
import saturation_batches as SB

COLS = {SB.A: 0, SB.C_: 1, SB.G: 2, SB.T: 3, SB.N: 5}


def middle_class(b):
    """Per read of a hot batch: the column it counts at its second position (4 = deletion)."""
    first = b["cigar"][b["cig_beg"]]
    gap = (first >> 4) == 1  # 1M 14D 1M
    code = (b["seq"][b["seq_nib"] >> 1] >> 4).astype(np.int64)  # reads start on a byte
    return np.where(gap, 4, np.vectorize(COLS.get)(code))


def same_class_per_group(b, size):
    """For every aligned group of `size` consecutive reads: (reads sharing the commonest
    (start, class), reads of class N, reads of class deletion)."""
    cls, pos = middle_class(b), b["pos"].astype(np.int64)
    out = []
    for g0 in range(0, cls.size, size):
        key = pos[g0: g0 + size] * 8 + cls[g0: g0 + size]
        out.append((np.unique(key, return_counts=True)[1].max(), int((cls[g0: g0 + size] == 5).sum()),
                    int((cls[g0: g0 + size] == 4).sum())))
    return np.array(out)


@pytest.mark.parametrize("runs3", [False, True])
@pytest.mark.parametrize("d", SB.DEPTHS)
def test_depth_ladder_through_the_oracle(d, runs3):
    """One (position, column) holds the whole depth d, and oracle.bcount gives the closed form."""
    b = SB.hot_batch(d, runs3)
    assert np.all(np.diff(b["pos"]) >= 0) and b["pos"].size == 8 * d
    cnt, (bad, _) = O.bcount(SB.HOT_L, 0, b)
    assert bad == -1 and np.array_equal(cnt, SB.hot_closed_form(d, runs3))
    assert cnt.max() == d and all(cnt[:, c].max() == d for c in range(6))
    # ref_len = HOT_L - 3: the first read of the last block is the first past the end
    assert O.bcount(SB.HOT_L - 3, 0, b)[1] == (7 * d, SB.HOT_L - 3)
    assert SB.max_end(b) == SB.HOT_L and int(SB.spans(b).max()) == SB.HOT_LEN
    # block starts straddle an 8-position window edge and a 64-position tile edge
    assert all(s % 64 == 60 for s in SB.hot_starts())


def test_counter_bounds_are_met():
    """The bounds of the issue's table, from the batches alone."""
    # nibbles (fold at 14) and byte sums (112): columns of exactly these depths and one more
    for d in (14, 15, 16, 17, 112, 113, 128, 129):
        assert d in SB.DEPTHS and SB.hot_closed_form(d)[:, :4].max() == d
    # a 256-read k_rc chunk whose reads all share one class at one position (16-bit half = 256,
    # four 32-read groups of 32 = 128 in a byte twice), and chunks with 255 / 257 around it
    for d, full in ((256, 256), (512, 256), (4096, 256), (65536, 256)):
        per = same_class_per_group(SB.hot_batch(d), 256)
        assert np.all(per[: 6 * d // 256, 0] == full)  # blocks A C G T N del: homogeneous chunks
    assert same_class_per_group(SB.hot_batch(255), 256)[0, 0] == 255
    assert same_class_per_group(SB.hot_batch(257), 256)[0, 0] == 256
    # the event image's 32-read groups: all 32 agree (xd[5]) -- A, C, G, T, N (plane == N plane:
    # xd - nn is an equality) and deletion (xd - ds an equality); interleaved blocks: plane full
    # with the N / DS plane half, 16 of 32 (the weight-16 digit yd[4])
    g = same_class_per_group(SB.hot_batch(32), 32)
    assert g.shape[0] == 8 and np.all(g[:6, 0] == 32)
    assert g[4, 1] == 32 and g[5, 2] == 32          # all N, all deletion
    assert tuple(g[6]) == (16, 16, 0) and tuple(g[7]) == (16, 0, 16)
    assert same_class_per_group(SB.hot_batch(31), 32)[0, 0] == 31
    assert same_class_per_group(SB.hot_batch(33), 32)[:2, 0].tolist() == [32, 31]
    # the three-run variant: no read the event image takes but the `1M 14D 1M` ones
    r3 = SB.host_runs(SB.RUNS3_OPS)
    assert (r3["nrun"], r3["span"], r3["qlen"]) == (3, SB.HOT_LEN, 14) and not SB.is_complex(SB.RUNS3_OPS)
    assert set(SB.hot_batch(256, True)["cig_n"][: 5 * 256].tolist()) == {5}
    # the complex path's 10-bit fields: 9-op reads, depths on both sides of 1023
    assert len(SB.COMPLEX_OPS) == 9 and SB.is_complex(SB.COMPLEX_OPS)
    for d in SB.COMPLEX_DEPTHS:
        b = SB.hot_complex_batch(d)
        cnt, (bad, _) = O.bcount(SB.COMPLEX_L, 0, b)
        assert bad == -1 and np.array_equal(cnt, SB.complex_closed_form(d)) and cnt.max() == d
    assert min(SB.COMPLEX_DEPTHS) < 1023 < max(SB.COMPLEX_DEPTHS) and 1023 in SB.COMPLEX_DEPTHS
    # k_count's LDS window: chunks of exactly 32768 reads, a 16-bit half at 0x8000 and 0x7FFF | 1
    b = SB.full_halves_batch()
    assert b["pos"].size == 2 * 32768 and b["pos"][32767] == 60 and b["pos"][32768] == 188
    cnt, _ = O.bcount(204, 0, b)
    assert cnt[60, 1] == 0x8000 and cnt[61, 0] == 0x8000 and cnt[64, 5] == 0x8000
    assert tuple(cnt[190, :2]) == (1, 0x7FFF)
    # ... and the use_lds switch: chunk 0's window on both sides of kWinMax
    for wlen in (4095, 4096, 4097):
        wb = SB.window_batch(wlen)
        assert SB.chunk_window(wb, 64, 0) == wlen and SB.chunk_window(wb, 64, 1) <= 600
        assert np.all(np.diff(wb["pos"]) >= 0)
        assert O.bcount(SB.max_end(wb) - 3, 0, wb)[1][0] >= 64  # chunk 1 reaches past the cut
    assert SB.K_WIN_MAX == 4096


def test_catalogue_sits_on_both_sides_of_every_threshold():
    cat = {k: SB.host_runs(v) for k, v in SB.catalogue_ops().items()}
    cx = {k: SB.is_complex(v) for k, v in SB.catalogue_ops().items()}
    # cig_n against kPre = 8
    assert cat["ops8_runs3"]["cig_n"] == 8 and not cx["ops8_runs3"]
    assert cat["ops9_runs3"]["cig_n"] == 9 and cx["ops9_runs3"]
    assert cat["ops9_runs2"]["cig_n"] == 9 and cat["ops9_runs2"]["nrun"] == 2 and cx["ops9_runs2"]
    # runs against kMaxRuns = 4
    assert cat["ops7_runs4"]["nrun"] == 4 and cat["ops8_runs4"]["nrun"] == 4 and not cx["ops8_runs4"]
    assert cat["ops8_runs4"]["cig_n"] == 8 and cat["ops9_runs5"]["nrun"] == 5 and cx["ops9_runs5"]
    # zero lengths vanish
    assert cat["zero_len"] == dict(cat["zero_len"], nrun=1, span=12, qlen=12)
    # reads without an aligned base
    for name in ("del_only", "ins_only", "clip_only", "no_cigar"):
        assert cat[name]["nrun"] == 0
    assert cat["no_cigar"]["cig_n"] == 0
    # ops that neither break nor move a run; the mid-read S does not advance the query
    for name in ("mid_H", "mid_P", "mid_B", "mid_S"):
        assert cat[name]["nrun"] == 1 and cat[name]["qd"] == [0]
    # query delta around int16, span 8
    assert [cat[f"ins{n}"]["qd"][1] for n in (32767, 32768, 32772)] == [32767, 32768, 32772]
    assert [cx[f"ins{n}"] for n in (32767, 32768, 32772)] == [False, True, True]
    assert all(cat[f"ins{n}"]["span"] == 8 for n in (32767, 32768, 32772))
    # query length around 0xFFFF with deltas inside int16
    assert cat["qlen65535"]["qlen"] == 0xFFFF and not cx["qlen65535"]
    assert cat["qlen65536"]["qlen"] == 0x10000 and cx["qlen65536"] and max(cat["qlen65536"]["qd"]) <= 32767
    assert cat["m65535@long"]["qlen"] == 65535 and cat["m65536@long"]["qlen"] == 65536
    # spans: kTileMaxSpan, 0x1FFF; op lengths around 2^13
    assert cat["span4096"]["span"] == SB.K_TILE_MAX_SPAN and not cx["span4096"]
    assert [cat[f"span{s}@long"]["span"] for s in (8190, 8191, 8192)] == [8190, 8191, 8192]
    assert [cx[f"span{s}@long"] for s in (8190, 8191, 8192)] == [False, True, True]
    assert all(cat[f"span{s}@long"]["maxlen"] < 8192 for s in (8190, 8191, 8192))  # the span alone decides
    assert cat["op8191@long"]["maxlen"] == 8191 and cat["op8192@long"]["maxlen"] == 8192
    # two-run reads: run boundaries on and next to a row edge at every start mod 8
    edges = {(s + ops[0][1]) % 8 for s in range(8) for ops in SB.EDGE_TWO_RUN}
    assert edges == set(range(8)) and all(SB.host_runs(o)["nrun"] == 2 for o in SB.EDGE_TWO_RUN)


@pytest.mark.parametrize("which,variant,L", [("tiled", "embedded", 6_000), ("tiled", "deep", 6_000),
                                             ("long", "embedded", 70_000), ("long", "deep", 70_000)])
def test_catalogue_batches(which, variant, L):
    """The catalogue batches are sorted, stay inside the reference, hold every catalogue read (the
    deep ones at least 300 reads and nothing but the catalogue), and the oracle counts them."""
    b = SB.catalogue_batch(which, variant, L)
    assert np.all(np.diff(b["pos"]) >= 0) and SB.max_end(b) <= L
    n_cat = sum(1 for k in SB.catalogue_ops() if which == "long" or not k.endswith("@long"))
    copies = 1 if variant == "embedded" else (8 if which == "tiled" else 12)
    if which == "tiled":
        n_cat += 8 * len(SB.EDGE_TWO_RUN)
    assert b["pos"].size == copies * n_cat + 1 + (300 if variant == "embedded" else 0)
    assert variant == "embedded" or copies * n_cat >= 300
    assert (b["cig_n"] == 0).sum() == copies
    assert b["cig_beg"][b["cig_n"] == 0].max() < b["cigar"].size
    assert int(SB.spans(b).max()) == (65_536 if which == "long" else 4_096)
    for mbq in (0, 20):
        cnt, (bad, _) = O.bcount(L, mbq, b)
        assert bad == -1 and cnt.sum() > 0


def test_quality_batch_covers_the_byte_range():
    b = SB.quality_batch(3_000)
    q = b["qual"]
    assert np.all(np.bincount(q, minlength=256) > 0)
    counts = [int(O.bcount(3_000, m, b)[0][:, [0, 1, 2, 3, 5]].sum()) for m in (0,) + SB.QUAL_THRESHOLDS]
    assert all(x >= y for x, y in zip(counts, counts[1:]))
    # every threshold up to 255 changes what is counted; above it nothing but deletions is
    assert len(set(counts[:9])) == 9 and counts[9] == counts[10] == 0
    t = SB.quality_batch(3_000, 600, tight=True)
    assert t["qual"].size == 2 * t["seq"].size
