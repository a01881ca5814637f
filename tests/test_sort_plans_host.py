"""tests/sort_plans.py proved on the CPU: every catalogue case holds the decisions of the device sort
(basecount_amd/csrc/bc_sort.hip) it is named for, a perturbed case does not, the batches the suite
sorted before the catalogue all took one degenerate plan (the gap tests/test_gpu_sort_plans.py
closes), and the yardstick accepts a correct sorted view and rejects each corruption of it."""
import numpy as np
import pytest

import sort_plans as SP


def plan_of(name):
    b = SP.case(name)
    return b, SP.plan(b["pos"].size, SP.max_end_of(b))


def test_constants_are_the_kernels():
    """The restated constants against bc_sort.hip's own text."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "basecount_amd", "csrc",
                            "bc_sort.hip")).read()

    def const(name):
        return int(re.search(r"constexpr \w+ %s = (\w+);" % name, src).group(1).rstrip("u"), 0)

    assert const("kBktThreads") == SP.BKT_THREADS and const("kBktMax") == SP.BKT_MAX
    assert const("kBktTarget") == SP.BKT_TARGET and const("kBktChunk") == SP.BKT_CHUNK
    assert const("kRankThreads") * const("kRankRegs") == SP.RANK_REGS
    assert const("kScanTile") == SP.SCAN_TILE and const("kRelayReads") == SP.RELAY_READS
    assert const("kRelayWords") * 4 * 8 == SP.RELAY_BASES and const("kQlenMax") == SP.QLEN_MAX
    assert const("kSortCapMax") == SP.SORT_CAP_MAX
    assert "kSortRuns ? 1024 : %d" % SP.PERM_SLOTS in src and "65536 / H" in src


def test_tiny_cases():
    for name, n in (("one_read", 1), ("two_reads_same_start", 2)):
        b, P = plan_of(name)
        assert b["pos"].size == n and P["kind"] == "bucket" and P["chunk"] == n and P["nblk"] == 1
    assert np.unique(SP.case("two_reads_same_start")["pos"]).size == 1


def test_w0_tiny():
    b, P = plan_of("w0_tiny")
    assert SP.max_end_of(b) <= 254 and P["wbits"] == 0 and P["W"] == 1 and b["pos"].size == 700
    assert SP.plan(700, 255)["wbits"] == 1  # one more position: two starts per bucket


def test_all_one_start():
    b, P = plan_of("all_one_start")
    R = SP.rank_plan(b, P)
    assert R["counts"] == {"empty": P["nbkt"] - 1, "regs1": 0, "regs2": 0, "past_regs": 1}
    assert R["sizes"].max() == 9_000 > SP.RANK_REGS


def test_h_edges():
    (_, a), (_, b) = plan_of("h256_edge"), plan_of("h257_edge")
    assert (a["nbkt"], a["rows"], a["nblk"]) == (256, "4x16", 2)
    assert (b["nbkt"], b["rows"], b["nblk"]) == (257, "8x4", 2)
    _, c = plan_of("h_gt_512")
    assert (c["nbkt"], c["rows"], c["h0_iters"], c["nblk"]) == (733, "8x4", 2, 3)
    assert SP.plan(10_000, 1_500_000)["h0_iters"] == 1  # max_end halved: one bucket group


def test_row_loops():
    _, a = plan_of("rows_gt_64")
    assert (a["nbkt"], a["nblk"], a["rows"], a["row_iters"]) == (293, 66, "8x4", 2)
    assert SP.plan(a["n"] - 8_192, 1_200_000)["row_iters"] == 1  # two blocks fewer: 64 rows, one iteration
    b, p = plan_of("rows_gt_256")
    assert (p["nbkt"], p["nblk"], p["rows"], p["row_iters"]) == (200, 257, "4x16", 2)
    assert SP.plan(p["n"] // 2, 3_198)["row_iters"] == 1
    R = SP.rank_plan(b, p)
    assert R["counts"]["regs2"] >= 190 and R["counts"]["past_regs"] == 0  # ~5,250 reads: two perm passes
    assert np.all(SP.query_lengths(b) == 10)


def test_capped_rounds():
    _, P = plan_of("capped_rounds")
    assert (P["nbkt"], P["h0_iters"], P["nblk"], P["chunk"], P["W"]) == (4096, 8, 16, 8_750, 4096)
    assert (P["count_rounds"], P["scatter_rounds"]) == (2, 3)
    half = SP.plan(P["n"] // 2, (1 << 24) - 2)
    assert half["count_rounds"] == 1 and half["scatter_rounds"] == 2  # n halved: the cap no longer doubles a block
    assert SP.plan(P["n"], (1 << 23) - 2)["count_rounds"] == 1  # max_end halved: 32 blocks, no cap


def test_rank_edges():
    b, P = plan_of("rank_edges")
    assert P["wbits"] == 4 and abs(b["pos"].size - 30_000) < 100
    R = SP.rank_plan(b, P)
    for h, k in SP.RANK_EDGE_BUCKETS.items():
        assert R["sizes"][h] == k
    assert [R["path"][h] for h in SP.RANK_EDGE_BUCKETS] == ["regs1", "regs2", "regs2", "past_regs"]
    assert R["empty"] > 100 and np.any(np.diff(b["pos"]) < 0)  # empty buckets; the input is not in order


def test_alignments():
    b = SP.case("alignments")
    q, sn = SP.query_lengths(b), b["seq_nib"].astype(np.int64)
    assert {(int(o), int(x)) for o, x in zip(sn % 8, q)} == {(o, x) for o in range(8) for x in SP.ALIGN_QLENS}
    C = SP.copy_plan(b)
    assert C["past_unrolled"].size > 50 and q.max() > SP.RELAY_BASES
    assert b["qual"].size == int((sn + q).max())  # the read lying last: its last quality is the last byte
    assert 0 < C["bump"].size < q.size  # reads in their slots and reads from the bump allocator


def test_shrunk_and_big():
    b = SP.case("shrunk_many_long")
    C = SP.copy_plan(b)
    assert C["slots"] == "shrunk" and not C["overflows"]
    assert sorted(C["q"][C["bump"]].tolist()) == sorted(SP.SHRUNK_LONG) and b["pos"].size == 3_005
    b = SP.case("big_records")
    C = SP.copy_plan(b)
    assert C["slots"] == "shrunk" and sorted(C["q"][C["big"]].tolist()) == [SP.QLEN_MAX, 70_000]
    assert C["bump"].tolist() == C["big"].tolist() and not C["overflows"]
    small = SP.make_batch(np.random.default_rng(1), [5, 9], [SP.QLEN_MAX - 1, 30])
    assert SP.copy_plan(small)["big"].size == 0  # one base fewer: the 16-bit record
    for name in SP.cases():
        if name not in ("shrunk_many_long", "big_records", "alignments"):
            c = SP.copy_plan(SP.case(name))
            assert c["slots"] == "full" and c["bump"].size == 0 and c["big"].size == 0, name


def test_counting_cases():
    b, P = plan_of("counting_edge")
    assert P["kind"] == "counting" and P["nbins"] == (1 << 24) + 1 and P["relay_tail"] == 3 and P["n"] == 2_003
    assert SP.plan(2_003, (1 << 24) - 2)["kind"] == "bucket"  # one position fewer: the last bucketed size
    b, P = plan_of("counting_spread")
    assert P["kind"] == "counting" and P["n"] == 4_001 and P["relay_tail"] == 1 and P["scan_passes"] == 17
    tile = b["pos"].astype(np.int64) // SP.SCAN_TILE
    per_pass = np.bincount(tile // SP.SCAN_TILE, minlength=P["scan_passes"])
    assert np.all(np.cumsum(per_pass)[:-1] > 0)  # a non-zero carry into every pass of k_scan_sums after the first
    assert tile.min() == 0 and np.unique(tile).size > 3_000  # k_scan_add: a non-zero addend for every tile but the first
    for name, n in (("counting_tiny1", 1), ("counting_tiny3", 3)):
        b, P = plan_of(name)
        assert P["kind"] == "counting" and P["relay_groups"] == 1 and P["relay_tail"] == n
        assert SP.max_end_of(b) == SP.COUNTING_LONG


def test_overlap_case_overflows():
    b = SP.case("overlap")
    C = SP.copy_plan(b)
    assert C["slots"] == "shrunk" and C["bump"].size == 200 and C["overflows"]
    assert b["seq"].size == 4_000 and np.all(C["q"] == 6_000)


def test_bad_starts_are_outside():
    for name, base in SP.BAD_START_BASE.items():
        b = SP.case(base)
        me = SP.max_end_of(b)
        bad = SP.bad_starts(b)
        assert [p < 0 or p > me for _, p in bad] == [True, True]
        assert SP.plan(b["pos"].size, me)["kind"] == ("bucket" if name.endswith("bucket") else "counting")


def test_old_suite_took_one_plan():
    """Every batch the suite sorted before this catalogue: one count round, one scatter round, one
    bucket group, one row iteration, no more than one row for count_rows<8,4>, W > 1 -- for every
    max_end a batch on that reference can have."""
    for name, (n, L) in SP.OLD_SUITE.items():
        for me in range(max(300, L - 400), L + 1):
            P = SP.plan(n, me)
            assert P["kind"] == "bucket" and P["wbits"] > 0, name
            assert (P["count_rounds"], P["scatter_rounds"], P["h0_iters"], P["row_iters"]) == (1, 1, 1, 1), (name, P)
            assert P["rows"] == "4x16" or P["nblk"] == 1, (name, P)
            assert P["nblk"] < SP.MAT_WORDS // P["nbkt"], name  # never at the cap
    for name, (n, L) in SP.OLD_SUITE_COUNTING.items():
        assert SP.plan(n, L)["kind"] == "counting" and n % SP.RELAY_READS == 0


def test_catalogue_reaches_every_decision():
    plans = {name: plan_of(name)[1] for name in SP.cases()}
    bk = [p for p in plans.values() if p["kind"] == "bucket"]
    assert max(p["count_rounds"] for p in bk) >= 2 and max(p["scatter_rounds"] for p in bk) >= 3
    assert max(p["h0_iters"] for p in bk) >= 8
    assert {p["row_iters"] for p in bk if p["rows"] == "4x16"} >= {1, 2}
    assert {p["row_iters"] for p in bk if p["rows"] == "8x4"} >= {1, 2}
    assert any(p["rows"] == "8x4" and p["nblk"] >= 2 for p in bk) and any(p["wbits"] == 0 for p in bk)
    assert {p["relay_tail"] for p in plans.values() if p["kind"] == "counting"} == {1, 3}


def test_layout_bytes_pieces():
    """The restated total on two layouts worked out by hand (the GPU tests pin it to the library)."""
    # 5 reads, max_end 100, 64 sequence bytes, qualities: cap 105, room 160; 102 buckets, one block
    tail = 512 + 256 + 512  # mat (408 bytes), bstat (8), bbase (412)
    want = 256 + 256 + 4 * 256 + 256 + 512 + tail  # words, rec (160), four arrays, seq (176), qual (352)
    assert SP.seq_event_bytes(160) == 176 and SP.layout_bytes(5, 100, 64, True, False) == want
    assert SP.layout_bytes(5, 100, 64, False, True) == 256 + 256 + 4 * 256 + 256 + tail  # (run records: 80)
    assert SP.layout_bytes(0, 100, 64, True, False) == 0
    # the counting sort ignores a fields-only request
    assert SP.layout_bytes(7, 1 << 24, 64, False, True) == SP.layout_bytes(7, 1 << 24, 64, False, False)


# ------------------------------------------------------------------------------- the yardstick
@pytest.fixture(scope="module")
def pair():
    rng = np.random.default_rng(7)
    n = 300
    b = SP.make_batch(rng, rng.integers(0, 500, n), **SP.mixed_reads(rng, np.zeros(n), 5, 40))
    return b, SP.model_view(b)


def writable(v):
    return {k: (x.copy() if isinstance(x, np.ndarray) else x) for k, x in v.items()}


def test_yardstick_accepts_correct_views(pair):
    b, v = pair
    SP.sorted_view_matches(b, v)
    SP.sorted_view_matches(b, SP.model_view(b, fields=True))
    nq = dict(b, qual=None)
    SP.sorted_view_matches(nq, SP.model_view(nq))
    for name in ("alignments", "rank_edges", "big_records"):
        c = SP.case(name)
        SP.sorted_view_matches(c, SP.model_view(c))
        SP.sorted_view_matches(c, SP.model_view(c, fields=True))


def test_yardstick_rejects_swapped_sequences(pair):
    b, v = pair
    v = writable(v)
    q = SP.query_lengths(v)
    i = 0  # with a read of its length and parity at another start: only the bases differ
    cand = np.flatnonzero((q == q[i]) & ((v["seq_nib"] & 1) == (v["seq_nib"][i] & 1)) & (v["pos"] != v["pos"][i]))
    j = int(cand[0])
    v["seq_nib"][[i, j]] = v["seq_nib"][[j, i]]
    with pytest.raises(AssertionError, match="multiset"):
        SP.sorted_view_matches(b, v)


def test_yardstick_rejects_one_quality_byte(pair):
    b, v = pair
    v = writable(v)
    v["qual"][int(v["seq_nib"][40]) + 2] ^= 1
    with pytest.raises(AssertionError, match="multiset"):
        SP.sorted_view_matches(b, v)


def test_yardstick_rejects_moved_seq_nib(pair):
    b, v = pair
    v = writable(v)
    v["seq_nib"][123] += 1
    with pytest.raises(AssertionError, match="multiset|parity"):
        SP.sorted_view_matches(b, v)
    # a copy at the other parity with the right bases and qualities: only the parity check sees it
    v = writable(pair[1])
    q = int(SP.query_lengths(v)[5])
    old = int(v["seq_nib"][5])
    nib = np.zeros(2 * v["seq"].size, np.uint8)
    nib[0::2], nib[1::2] = v["seq"] & 15, v["seq"] >> 4
    nib[old + 1: old + 1 + q] = nib[old: old + q].copy()
    v["qual"][old + 1: old + 1 + q] = v["qual"][old: old + q].copy()
    v["seq"] = nib[0::2] | nib[1::2] << 4
    v["seq_nib"][5] = old + 1
    with pytest.raises(AssertionError, match="parity"):
        SP.sorted_view_matches(b, v)
    f = writable(SP.model_view(b, fields=True))
    f["seq_nib"][9] += 2
    with pytest.raises(AssertionError, match="multiset|seq_nib"):
        SP.sorted_view_matches(b, f)


def test_yardstick_rejects_dropped_and_duplicated(pair):
    b, v = pair
    v = writable(v)
    for k in ("cig_beg", "cig_n", "seq_nib"):  # read 11 in place of read 10 (same start order kept)
        v[k][10] = v[k][11]
    v["pos"][10] = v["pos"][11]
    with pytest.raises(AssertionError, match="multiset"):
        SP.sorted_view_matches(b, v)


def test_yardstick_rejects_unordered_starts(pair):
    b, v = pair
    v = writable(v)
    i = int(np.flatnonzero(np.diff(v["pos"]) > 0)[3])
    for k in ("pos", "cig_beg", "cig_n", "seq_nib"):
        v[k][[i, i + 1]] = v[k][[i + 1, i]]
    with pytest.raises(AssertionError, match="out of order"):
        SP.sorted_view_matches(b, v)


def test_yardstick_rejects_overlapping_slots(pair):
    """Two reads of the same bases sharing one slot pass the multiset; the byte ranges catch them."""
    rng = np.random.default_rng(8)
    b = SP.make_batch(rng, [4, 9, 9, 30], [12, 12, 12, 12])
    b["seq"][6:12] = b["seq"][12:18]  # reads 1 and 2: the same bases and qualities
    b["qual"][12:24] = b["qual"][24:36]
    v = writable(SP.model_view(b))
    SP.sorted_view_matches(b, v)
    v["seq_nib"][2] = v["seq_nib"][1]
    with pytest.raises(AssertionError, match="overlap"):
        SP.sorted_view_matches(b, v)
    v = writable(SP.model_view(b))
    v["room"] = int(v["seq_nib"][3] >> 1) + 2
    with pytest.raises(AssertionError, match="past room"):
        SP.sorted_view_matches(b, v)


def test_yardstick_rejects_changed_fields_only_sequence(pair):
    b, _ = pair
    f = writable(SP.model_view(b, fields=True))
    f["seq"][-1] ^= 0x10  # a byte no read uses
    with pytest.raises(AssertionError, match="sequence differs"):
        SP.sorted_view_matches(b, f)


def test_kept_reads_match():
    b = SP.case("overlap")
    v = writable(SP.model_view(b, fields=True))
    v["cig_n"][[3, 77]] = 0
    kept = SP.kept_reads_match(b, v)
    assert kept.size == 198 and SP.sub_batch(b, kept)["pos"].size == 198
    v["seq_nib"][5] += 2
    with pytest.raises(AssertionError, match="kept read"):
        SP.kept_reads_match(b, v)
