"""(CPU) The inputs of test_gpu_stage_layouts.py prove themselves: chunk_plan, the model of
process_chunk's staging decisions (tests/stage_layouts.py), finds in every case the chunk kinds the
case is named for, at the sizes and alignments that matter, and the oracle counts each case without
a range error (or, for cut_short, with the intended one).  A change to a generator cannot silently
turn a case into one more run of the usual staged path: a case that stops meeting these conditions
is rebuilt, never skipped."""
import collections

import numpy as np
import pytest

import oracle as O
import stage_layouts as SL
from basecount_amd import device as D

STAGED = ("spec_hit", "restaged", "staged_no_spec")


def plan(name, **kw):
    b, L = SL.case(name)
    return SL.chunk_plan(b, L, **kw)


def kinds(p, min_nr=1):
    return collections.Counter(c["kind"] for c in p if c["nr"] >= min_nr)


def first_byte(b, c):
    return int(b["seq_nib"][c["base"]]) >> 1


@pytest.mark.parametrize("name", SL.cases())
def test_case_counts_without_range_error(name):
    """Every case is a valid batch on its reference and on the longer one the sweeps run on, where
    bc_pileup_plan takes the one-wave sweep; on its own reference the tiled kernel's rule holds."""
    b, L = SL.case(name)
    assert np.all(np.diff(b["pos"]) >= 0) and b["qual"].max() == 44 and b["qual"].min() == 0
    nib = np.stack([b["seq"] >> 4, b["seq"] & 15], 1).ravel()
    stored = sum(SL.query_len(c) for c in SL.cigars(b))
    assert 0.03 <= 1 - np.isin(nib, SL.ACGT).sum() / stored <= 0.07
    big = SL.sparse_length(b, L)
    assert big >= SL.NP_BUF and D.pileup_plan(SL.header(b), big, "tile")["kernel"] == "solo"
    assert D.pileup_plan(SL.header(b), L, "tile_no_solo")["kernel"] == "tiles"
    for mbq in (0, 20):
        assert SL.expected(name, big, mbq)[1] == (-1, -1)
        if name not in SL.CUT_CASES:
            assert SL.expected(name, L, mbq)[1] == (-1, -1)


@pytest.mark.parametrize("lean", [False, True])
def test_in_order_150(lean):
    """The control: every chunk, and every window the sweeps could form, keeps its speculative copy;
    with a quality threshold every chunk is staged through registers."""
    p = plan("in_order_150", lean=lean)
    assert set(kinds(p)) == {"spec_hit"} and max(c["nr"] for c in p) == 64
    assert collections.Counter(c["tile"] for c in p).most_common(1)[0][1] >= 3  # several chunks per tile
    assert set(kinds(plan("in_order_150", lean=lean, qual=True))) == {"staged_no_spec"}
    if not lean:
        assert set(kinds(plan("in_order_150", windows=True))) == {"spec_hit"}


@pytest.mark.parametrize("lean", [False, True])
@pytest.mark.parametrize("windows", [False, True])
def test_reversed_stride256(lean, windows):
    """No chunk of two or more reads speculates; up to 24 reads the exact segment is staged, from
    25 on the chunk is walked from HBM: for the tiles' chunks and for every window of the sweeps."""
    for qual in (False, True):
        p = plan("reversed_stride256", lean=lean, qual=qual, windows=windows)
        for c in p:
            want = "unstaged" if c["nr"] >= 25 else "staged_no_spec" if c["nr"] >= 2 or qual else "spec_hit"
            assert c["kind"] == want and (c["nr"] == 1 or not c["spec"]), c
        sizes = {c["nr"] for c in p}
        assert 64 in sizes and any(25 <= s < 64 for s in sizes) and any(2 <= s <= 24 for s in sizes)
        assert not windows or {2, 24, 25} <= sizes


@pytest.mark.parametrize("name,kind", [("straggler_near", "restaged"), ("straggler_far", "unstaged")])
def test_stragglers(name, kind):
    """One read per chunk lies before (near) or 40,000 B behind (far) the others: the speculative
    copy is issued and misses in every chunk; near, the exact segment fits and is staged again."""
    for lean in (False, True):
        p = plan(name, lean=lean)
        assert all(c["kind"] == kind and c["spec"] for c in p), kinds(p)
        assert {5, 17, 30, 64} <= {c["nr"] for c in p}
        assert all(c["seg_len"] > 40_000 if kind == "unstaged" else c["seg_len"] <= SL.LEAN_STG for c in p)
        q = plan(name, lean=lean, qual=True)
        assert set(kinds(q)) == {"unstaged" if kind == "unstaged" else "staged_no_spec"}


def test_round_down():
    """The speculative copy starts at the first read's byte rounded down to 16: a small read in
    those bytes is covered (first cluster), one before them is not (second)."""
    b, L = SL.case("round_down")
    p = plan("round_down")
    hit = [c for c in p if c["kind"] == "spec_hit"]
    miss = [c for c in p if c["kind"] == "restaged"]
    assert hit and miss and len(hit) + len(miss) == len(p)
    for c in hit:
        assert first_byte(b, c) % 16 == 8 and c["seg_lo"] == c["spec_lo"] == first_byte(b, c) - 8
    for c in miss:
        assert first_byte(b, c) % 16 == 0 and c["spec_lo"] == first_byte(b, c) and c["seg_lo"] == c["spec_lo"] - 16


@pytest.mark.parametrize("lean", [False, True])
def test_long_tail_300(lean):
    """Chunks of 20 or fewer reads whose last read passes the 128-byte slack are staged again; a
    last read of exactly 256 bases ends at the slack's end and keeps the copy, one of 258 does not."""
    b, L = SL.case("long_tail_300")
    p = plan("long_tail_300", lean=lean)
    assert max(c["nr"] for c in p) == 20 and {1, 7, 13, 20} <= {c["nr"] for c in p}
    last_len = lambda c: SL.query_len(SL.cigars(b)[c["base"] + c["nr"] - 1])
    for c in p:
        assert c["spec"] and c["kind"] == ("spec_hit" if last_len(c) == 256 else "restaged"), c
        assert c["seg_hi"] - c["spec_hi"] == {300: 22, 256: 0, 258: 1}[last_len(c)]
        assert (c["spec_hi"] - c["spec_lo"]) % 16 == 0  # the copy's last 16-byte piece ends at spec_hi
    assert {last_len(c) for c in p} == {300, 256, 258}


@pytest.mark.parametrize("lean", [False, True])
@pytest.mark.parametrize("qual", [False, True])
def test_exact_fit(lean, qual):
    """Full chunks whose exact segment is the stage to the byte, and 1, 16, 8 and 15 bytes more, with
    the first byte at 0, 8 and 15 mod 16: staged up to the stage's size, walked from HBM beyond."""
    name = "exact_fit_lean" if lean else "exact_fit"
    b, L = SL.case(name)
    stg = SL.LEAN_STG if lean else SL.STG
    p = plan(name, lean=lean, qual=qual)
    chunks = SL.exact_fit_chunks(lean)
    assert all(c["nr"] == 64 for c in p) and len({c["base"] for c in p}) == len(chunks)
    want = [stg, stg + 1, stg + 16, stg + 8, stg + 15, stg, stg]
    for c in p:
        i = c["base"] // 64
        assert c["seg_len"] == want[i] and first_byte(b, c) % 16 == chunks[i][0], c
        assert c["kind"] == ("unstaged" if want[i] > stg else "staged_no_spec"), c
    lens = {SL.query_len(o) for o in SL.cigars(b)}
    assert {stg // 32 - 1, stg // 32, stg // 32 + 1} <= lens  # 191 / 192 / 193 (187 / 188 / 189)
    if lean and not qual:  # the general instance stages all of these, from the speculative copy
        assert set(kinds(plan(name))) == {"spec_hit"}


@pytest.mark.parametrize("name", SL.EDGE_CASES)
def test_buffer_edges(name):
    """The buffer's first read starts at its byte 0, 1 or 15; its last read's last base is the
    arrays' last nibble (odd and even totals): the speculative copy of the last chunk is cut at
    the buffer's end, and the last 16-byte piece staged with qualities reads them byte by byte."""
    b, L = SL.case(name)
    start, odd = next((s, o) for s, o in SL.EDGE_VARIANTS if name == f"buffer_edges_{s}_{'odd' if o else 'even'}")
    assert int(b["seq_nib"].min()) == 2 * start == int(b["seq_nib"][0])
    last = int(np.argmax(b["seq_nib"]))
    assert int(b["seq_nib"][last]) + SL.query_len(SL.cigars(b)[last]) == b["qual"].size
    assert b["qual"].size % 2 == odd and b["seq"].size == (b["qual"].size + 1) // 2
    for lean in (False, True):
        p = plan(name, lean=lean)
        assert set(kinds(p)) == {"spec_hit"}
        tail = [c for c in p if c["base"] + c["nr"] == b["pos"].size]
        assert tail and all(c["clamped"] and c["spec_hi"] == SL.seq_event_bytes(b["seq"].size) for c in tail)
        assert not any(c["clamped"] for c in p if c not in tail)
        assert any(c["spec_lo"] == 0 and c["base"] == 0 for c in p)
        q = plan(name, lean=lean, qual=True)
        assert set(kinds(q)) == {"staged_no_spec"}
        for c in q:
            if c["base"] + c["nr"] == b["pos"].size:  # stage_regs' last piece: q0 + 32 > qual_bytes
                piece = c["seg_lo"] + (c["seg_hi"] - c["seg_lo"] - 1) // 16 * 16
                assert 2 * piece + 32 > b["qual"].size > 2 * piece


def classes(p):
    """(staged | unstaged, gap, largest run count) of the chunks; a complex chunk's walk has neither."""
    walk = lambda c: "staged" if c["kind"] in STAGED else c["kind"]
    return {("complex",) if c["kind"] == "complex" else (walk(c), c["gap"], c["maxrun"]) for c in p}


@pytest.mark.parametrize("qual", [False, True])
def test_runs_matrix(qual):
    """Laid out in order and with a far straggler per chunk, the batch holds every (staged |
    unstaged) x gap x largest run count in {1, 2, 4} chunk and a complex one: 12 + 1 classes."""
    matrix = {(g, m) for g in (False, True) for m in (1, 2, 4)}
    a, f = plan("runs_matrix_in_order", qual=qual), plan("runs_matrix_far", qual=qual)
    assert classes(a) == {("staged", g, m) for g, m in matrix} | {("complex",)}
    # (a cluster's last tile walks only the few reads that start late: small chunks with no straggler)
    assert {("unstaged", g, m) for g, m in matrix} | {("complex",)} <= classes(f)
    assert all(c["kind"] in ("unstaged", "complex") for c in f if c["nr"] >= 20)
    assert set(kinds(a)) == {"staged_no_spec" if qual else "spec_hit", "complex"}
    assert all(c["spec"] for c in f if c["kind"] == "unstaged" and c["nr"] >= 20 and not qual)
    assert {64, SL.MATRIX_SIZE - 64} <= {c["nr"] for c in a}


@pytest.mark.parametrize("qual", [False, True])
def test_runs_matrix_lean(qual):
    """The lean instance on the same batches: chunks with no slow read, with some (also the complex
    ones, which it walks alone) and, far, whole chunks handed to walk_complex."""
    a, f = plan("runs_matrix_in_order", lean=True, qual=qual), plan("runs_matrix_far", lean=True, qual=qual)
    assert set(kinds(a)) == {"staged_no_spec" if qual else "spec_hit"}
    assert all(c["kind"] == "unstaged" for c in f if c["nr"] >= 20) and kinds(f)["unstaged"] >= 30
    assert {c["slow"] == 0 for c in a} == {False, True} and 3 in {c["slow"] for c in a}
    assert all(not c["gap"] and c["maxrun"] == 1 for c in a + f)


@pytest.mark.parametrize("name,kind", [("cut_short_near", "restaged"), ("cut_short_far", "unstaged")])
def test_cut_short(name, kind):
    """The reference ends inside the last cluster's reach: the oracle's first offending read is
    walked, in every tile that reaches past the end, in a chunk of the intended kind."""
    b, L = SL.case(name)
    for mbq in (0, 20):
        bad = SL.expected(name, L, mbq)[1][0]
        assert bad >= 0
        for lean in (False, True):
            p = [c for c in SL.chunk_plan(b, L, lean=lean) if c["base"] <= bad < c["base"] + c["nr"]]
            past = [c for c in p if 64 * c["tile"] + 64 > L]
            assert past and all(c["kind"] == kind and c["nr"] == 64 for c in p), (bad, p)


@pytest.mark.parametrize("layout", ["in_order", "reversed"])
def test_high_nibbles(layout):
    """Every base above nibble 2^31 + 4,096 of a 2^30 + 65,536 byte array: in order the chunks of up
    to about 55 reads keep their speculative copy (fuller ones do not fit a stage), reversed none of
    two or more reads does and those of 25 and more are walked from HBM."""
    b, L = SL.high_nibbles(layout, with_qual=False)
    assert b["seq"].size == (1 << 30) + 65_536 and int(b["seq_nib"].min()) > (1 << 31) + 4096 and L == 2048
    assert {SL.query_len(o) for o in SL.cigars(b)} == {150, 250}
    assert O.bcount(L, 0, b)[1] == (-1, -1)
    for lean in (False, True):
        k = kinds(SL.chunk_plan(b, L, lean=lean), min_nr=2)
        if layout == "in_order":
            assert k["spec_hit"] >= 20 and k["unstaged"] >= 1 and set(k) <= {"spec_hit", "unstaged"}
        else:
            assert k["unstaged"] >= 10 and k["staged_no_spec"] >= 1 and set(k) == {"unstaged", "staged_no_spec"}
    assert D.pileup_plan(SL.header(b), SL.sparse_length(b, L), "tile")["kernel"] == "solo"
