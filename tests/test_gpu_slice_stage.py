"""k_pileup's slice instance (the lean walk over per-read 64-B slices; process_chunk<.., SLICE> in
basecount_amd/csrc/bc_tile.h, the slot arithmetic in bc_slice.h) against the general instance and the
oracle.

Every case runs the slice and the general instance forced (bc_ctx_set_instance;
bc_pileup_launch_info must name the instance asked for) over outputs prefilled with 0xFF bytes:
the two must be equal array by array and equal to the oracle (O.bcount, O.stats) bit for bit, and
bc_range_error must be the oracle's first offending read.  bc_count's accumulate launch takes the
same kernels without the statistics tail.  With min_base_quality 20 no slice instance is built:
the launch must report the lean instance it falls back to and still be exact.

A read's slot is filled before its CIGAR is decoded, from the fields alone.  seq_nib names the
first base after a leading soft clip, so a soft clip moves nothing; a leading INSERTION does (the
run's query delta), and one longer than the slot's slack sends the read to walk_complex."""
import functools

import numpy as np
import pytest

import oracle as O
import stage_layouts as SL
import test_gpu_lean_instance as LI
import test_gpu_stage_layouts as GS
from basecount_amd import device as D

pytestmark = pytest.mark.gpu

M, I, DEL, S = 0, 1, 2, 4
SETTINGS = [("tile", 4), ("tile", 8), ("tile_no_solo", 1)]
sid = lambda s: f"{s[0]}-{s[1]}"
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 150, 151, 250, 300)
CLIPS = (0, 1, 23, 24, 25, 40, 100)


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    try:
        yield c
    finally:
        c.set_shape("auto")
        c.set_instance("auto")


def make_batch(reads, starts=None, residues=None, tail=2):
    """The batch dict of reads (pos, ops, codes, quals) in start order.  Read i's query begins at
    nibble starts[i] of the sequence (default: one after the other in the given order, each moved
    up to the next nibble congruent to residues[i] mod 32 when residues is given); seq_nib is
    that plus the leading soft clip.  The arrays end ``tail`` nibbles after the last base."""
    assert [r[0] for r in reads] == sorted(r[0] for r in reads)
    if starts is None:
        starts, at = [], 0
        for i, r in enumerate(reads):
            if residues is not None:
                at += (residues[i] - at) % 32
            starts.append(at)
            at += len(r[2])
    nibbles = max(s + len(r[2]) for s, r in zip(starts, reads)) + tail
    nibbles += nibbles & 1
    allc, qual = np.zeros(nibbles, np.uint8), np.zeros(nibbles, np.uint8)
    for s, (_, _, codes, q) in zip(starts, reads):
        assert not allc[s: s + len(codes)].any() or len(codes) == 0
        allc[s: s + len(codes)] = codes
        qual[s: s + len(q)] = q
    cig_n = np.array([len(r[1]) for r in reads], np.uint32)
    cig_beg = np.zeros(len(reads), np.uint32)
    cig_beg[1:] = np.cumsum(cig_n)[:-1]
    clip = [r[1][0][1] if r[1][0][0] == S else 0 for r in reads]
    return dict(pos=np.array([r[0] for r in reads], np.int32), cig_beg=cig_beg, cig_n=cig_n,
                seq_nib=np.array([s + c for s, c in zip(starts, clip)], np.uint32),
                cigar=np.array([(ln << 4) | op for r in reads for op, ln in r[1]], np.uint32),
                seq=((allc[0::2] << 4) | allc[1::2]).astype(np.uint8), qual=qual)


def read_of(rng, pos, ops):
    return SL.read_of(rng, pos, ops)


def expect(b, L, mbq, k):
    cnt, (bad, _) = O.bcount(L, mbq, b)
    return GS.stats_of(cnt, k), bad


def forced(ctx, reads, L, mbq, k, setting, inst, stats=True):
    """One forced instance; the launch must really be it (slice: the lean fallback under a threshold)."""
    ctx.set_shape(*setting)
    ctx.set_instance(inst)
    try:
        info = D.pileup_launch_info(reads, L, setting[0], setting[1], inst, mbq, k)
        assert info["kernel"] == "tiles", info
        if inst == "slice":
            assert info["lean"] and info["slice"] == (mbq == 0), info
            if mbq == 0:
                nw = max(4, setting[1])
                assert info["lds_bytes"] == D.slice_lds_bytes(nw, setting[1]), info
                # six waves per SIMD of registers; LDS in 1,280-B granules of a CU's 160 KiB
                by_lds = 160 * 1024 // (-(-info["lds_bytes"] // 1280) * 1280)
                assert info["blocks_per_cu"] == min(24 // nw, by_lds), info
                assert info["blocks_per_cu"] == {("tile", 4): 6, ("tile", 8): 3}.get(setting, info["blocks_per_cu"])
        else:
            assert not info["lean"] and not info["slice"], info
        return GS.run(ctx, reads, L, mbq, k, stats)
    finally:
        ctx.set_instance("auto")


def check(ctx, b, L, what, settings=SETTINGS, combos=((0, 5), (0, 6), (20, 5)), counts=True):
    """Slice == general == oracle for every setting and (min_base_quality, k)."""
    reads = D.DeviceReads(ctx, b)
    try:
        assert reads.r.sorted == 1
        for mbq, k in combos:
            exp = expect(b, L, mbq, k)
            for setting in settings:
                g = forced(ctx, reads, L, mbq, k, setting, "general")
                s = forced(ctx, reads, L, mbq, k, setting, "slice")
                GS.same(g, exp, (what, "general", setting, mbq, k))
                GS.same(s, exp, (what, "slice", setting, mbq, k))
                assert s[1] == g[1]
                if exp[1] < 0:
                    for name, a, b_ in zip(GS.NAMES, s[0], g[0]):
                        assert np.array_equal(a, b_), (what, name, "slice differs from general")
            if counts:  # bc_count's accumulate launch into zeroed counts
                got = forced(ctx, reads, L, mbq, k, settings[0], "slice", stats=False)
                GS.same(got, (exp[0][:1], exp[1]), (what, "bc_count", mbq, k))
    finally:
        reads.free()


# ---------------------------------------------------------------- the start sweep
@functools.lru_cache(maxsize=None)
def sweep_batch(order="file", tail=2):
    """64 all-M reads of every length of LENGTHS: every pos mod 64, every seq_nib mod 32 (both
    nibble parities) per length, the longest reads last (300 bases from 512-575, five or six tiles;
    250 from 576-639): they reach position 888.  order: the reads' order in the sequence buffer ("file": start order; "permuted":
    shuffled, as under a fields-only sorted view; "last_last": start order, read lengths arranged
    so that the last read ends the buffer)."""
    rng = np.random.default_rng(11)
    reads = []
    for j, n in enumerate(LENGTHS):
        for i in range(64):
            reads.append(read_of(rng, 64 * (9 - j % 10) + i, [(M, n)]))
    reads.sort(key=lambda r: r[0])
    res = [(7 * i + i // 32) % 32 for i in range(len(reads))]
    if order == "permuted":
        perm = rng.permutation(len(reads))
        starts, at = [0] * len(reads), 0
        for i in perm:
            at += (res[i] - at) % 32
            starts[i] = at
            at += len(reads[i][2])
        b = make_batch(reads, starts=starts, tail=tail)
    else:
        b = make_batch(reads, residues=res, tail=tail)
    assert set(b["pos"] % 64) == set(range(64)) and set(b["seq_nib"] % 32) == set(range(32))
    for n in LENGTHS:  # every length meets both nibble parities and at least 32 tile offsets
        sel = np.array([len(r[2]) == n for r in reads])
        assert set(b["seq_nib"][sel] & 1) == {0, 1} and len(set(b["pos"][sel] % 64)) == 64
    return b


@pytest.mark.parametrize("setting", SETTINGS, ids=sid)
def test_start_sweep(ctx, setting):
    """Every pos mod 64 x seq_nib residue x length, on L = 890 (the last tile is partial and the reads
    end on its last positions); reads of one, two and five tiles, tiles that begin before and after
    a read's start."""
    b = sweep_batch()
    assert b["seq_nib"][0] == 0  # the buffer's first read at nibble 0
    assert int((b["pos"] + (b["cigar"] >> 4)).max()) == 889 and expect(b, 890, 0, 5)[1] == -1
    check(ctx, b, 890, "sweep", settings=[setting], combos=((0, 5), (0, 6), (20, 5)))


@pytest.mark.parametrize("L", [700, 870, 640])
def test_reads_past_the_reference_end(ctx, L):
    """The same reads on shorter references: an edge tile (700 = 10 x 64 + 60; 870) and tiles wholly
    past L (640): the first offending read is the oracle's."""
    b = sweep_batch()
    assert expect(b, L, 0, 5)[1] >= 0
    check(ctx, b, L, ("past", L), combos=((0, 5), (20, 6)))


def test_buffer_ends(ctx):
    """The last read ends on the buffer's final nibble: its tiles' slots reach past the readable end
    and are cut there (pieces that begin beyond it are not copied)."""
    rng = np.random.default_rng(12)
    reads = [read_of(rng, p, [(M, 150)]) for p in np.sort(rng.integers(0, 700, 300))]
    reads.append(read_of(rng, 760, [(M, 150)]))  # alone on its tiles, last in the buffer
    for odd in (0, 1):
        b = make_batch(reads, residues=[(5 * i + odd) % 32 for i in range(len(reads))], tail=0)
        last = int(b["seq_nib"][-1]) + 150
        assert last in (2 * b["seq"].size, 2 * b["seq"].size - 1) and b["seq_nib"][0] == odd
        # the slot of the last read's last tile would end beyond bc_seq_event_bytes
        src = ((int(b["seq_nib"][-1]) + (896 - 760)) // 2) & ~15
        assert src + 64 > SL.seq_event_bytes(b["seq"].size) > src
        check(ctx, b, 960, ("buffer_ends", odd), combos=((0, 5), (0, 6)))


@pytest.mark.parametrize("setting", SETTINGS, ids=sid)
def test_scattered_sequence(ctx, setting):
    """Sequence not in file order (permuted seq_nib under sorted positions): no chunk-wide segment
    exists, every slot has its own source."""
    b = sweep_batch("permuted")
    assert np.any(np.diff(b["seq_nib"].astype(np.int64)) < 0)
    check(ctx, b, 890, "permuted", settings=[setting], combos=((0, 5), (0, 6)), counts=False)


# ---------------------------------------------------------------- clips and leading insertions
@functools.lru_cache(maxsize=None)
def clip_batch(kind):
    rng = np.random.default_rng(13 + len(kind))
    reads = []
    for i, p in enumerate(np.sort(rng.integers(0, 800, 1400))):
        c = CLIPS[i % len(CLIPS)]
        n = 150 + (i % 3)
        if kind == "soft":      # leading and trailing soft clips
            ops = ([(S, c)] if c else []) + [(M, n - c - (i % 4))] + ([(S, i % 4)] if i % 4 else [])
        elif kind == "insert":  # the run starts at query offset c
            ops = ([(I, c)] if c else []) + [(M, n - c)]
        else:                   # both, and a trailing insertion
            ops = [(S, 3)] + ([(I, c)] if c else []) + [(M, n - c - 5)] + [(I, 2)]
        reads.append(read_of(rng, p, ops))
    return make_batch(reads, residues=[(3 * i) % 32 for i in range(len(reads))])


@pytest.mark.parametrize("kind", ["soft", "insert", "both"])
def test_clips(ctx, kind):
    """Leading clips / insertions of 0, 1, 23, 24, 25, 40 and 100 bases (both sides of the slot's
    slack: a slot starts up to 31 nibbles below the assumed base and a tile reads 64 of its 128),
    trailing ones, at every alignment of the sequence."""
    check(ctx, clip_batch(kind), 1000, ("clips", kind), combos=((0, 5), (0, 6), (20, 6)))


# ---------------------------------------------------------------- slow reads
SLOW_OPS = {
    "ins": lambda n: [(M, n // 2), (I, 1), (M, n - n // 2 - 1)],
    "del": lambda n: [(M, n // 2), (DEL, 1), (M, n - n // 2)],
    "nine": lambda n: [(M, 20), (I, 1), (M, 20), (DEL, 1), (M, 20), (I, 1), (M, 20), (DEL, 2), (M, n - 82)],
}


@functools.lru_cache(maxsize=None)
def slow_batch(pattern):
    rng = np.random.default_rng(14 + len(pattern))
    n_reads = 64 * 5 + 17 if pattern == "one_per_chunk" else 1300
    hi = 40 if pattern == "one_per_chunk" else 800
    slow_at = {"one_per_chunk": lambda i: i % 64 == (i // 64) * 13 % 64, "sprinkled": lambda i: i % 64 == 9,
               "all": lambda i: True}[pattern]
    reads = []
    for i, p in enumerate(np.sort(rng.integers(0, hi, n_reads))):
        ops = SLOW_OPS[("ins", "del", "nine")[i % 3]](150) if slow_at(i) else [(M, 150)]
        reads.append(read_of(rng, p, ops))
    return make_batch(reads)


@pytest.mark.parametrize("pattern", ["one_per_chunk", "sprinkled", "all"])
def test_slow_reads(ctx, pattern):
    """An insertion, a deletion and a nine-op read among 150-base reads: one per chunk (reads that all
    start in tile 0, so the read index fixes chunk and slot), one in 64 everywhere, and every read."""
    check(ctx, slow_batch(pattern), 1000, ("slow", pattern), combos=((0, 5), (0, 6), (20, 5)))


# ---------------------------------------------------------------- the existing cases
@pytest.mark.parametrize("name", SL.cases())
def test_stage_layout_cases(ctx, name):
    """tests/stage_layouts.py's cases (stragglers, the stage bound to the byte, buffer edges, run
    matrices, references cut short)."""
    b, L = SL.case(name)
    reads = D.DeviceReads(ctx, b)
    try:
        for mbq, k in ((0, 5), (0, 6), (20, 5)):
            exp = GS.want(name, L, mbq, k)
            for setting in (("tile_no_solo", 1), ("tile", 4)):
                GS.same(forced(ctx, reads, L, mbq, k, setting, "slice"), exp, (name, setting, mbq, k))
            got = forced(ctx, reads, L, mbq, k, ("tile_no_solo", 1), "slice", stats=False)
            GS.same(got, (exp[0][:1], exp[1]), (name, "bc_count", mbq, k))
    finally:
        reads.free()


@pytest.mark.parametrize("name", sorted(LI.CASES))
def test_lean_instance_cases(ctx, name):
    """tests/test_gpu_lean_instance.py's CASES (30-base reads: slow reads per chunk, alternating
    chunks, flush_acc's bound, sequence out of file order)."""
    L = 640
    b, exp = LI.case(name)
    reads = D.DeviceReads(ctx, b)
    try:
        for k, mbq in ((5, 0), (6, 0), (5, 20)):
            for setting in SETTINGS:
                got = forced(ctx, reads, L, mbq, k, setting, "slice")
                GS.same(got, (exp[k, mbq], -1), (name, setting, k, mbq))
    finally:
        reads.free()


# ---------------------------------------------------------------- routing on the device
def test_c2_header_is_six_per_cu(ctx):
    """bench.py's C2 shape (100,000 x 150-base all-M reads on 29,903 positions) under BC_INSTANCE_AUTO:
    the slice instance, six workgroups resident per CU."""
    h = {"n_reads": 100_000, "max_span": 150, "max_end": 29_903, "n_cigar_words": 100_000}
    for k in (5, 6):
        i = D.pileup_launch_info(h, 29_903, k=k)
        assert (i["kernel"], i["lean"], i["slice"], i["lds_bytes"], i["blocks_per_cu"]) == ("tiles", True, True, 24_256, 6)
    i8 = D.pileup_launch_info(h, 29_903, "tile", 8)
    assert i8["slice"] and i8["blocks_per_cu"] == 3


def test_auto_takes_slice_on_long_all_m_reads(ctx):
    """BC_INSTANCE_AUTO on an all-M batch of 150-base reads: the slice instance launches (the reported
    instance is the one that runs: equal outputs) and bc_pileup_plan's answers are unchanged."""
    rng = np.random.default_rng(15)
    L = 1000
    b = make_batch([read_of(rng, p, [(M, 150)]) for p in np.sort(rng.integers(0, L - 150, 3000))])
    reads = D.DeviceReads(ctx, b)
    try:
        ctx.set_shape("tile", 4)
        ctx.set_instance("auto")
        info = D.pileup_launch_info(reads, L, "tile", 4)
        assert info["slice"] and info["blocks_per_cu"] == 6 and info["lds_bytes"] == 24_256
        p = D.pileup_plan(reads, L, "tile", 4)
        assert (p["kernel"], p["lds_bytes"], p["blocks_per_cu"], p["block_threads"]) == ("tiles", 40_640, 4, 256)
        for mbq, k in ((0, 5), (0, 6)):
            GS.same(GS.run(ctx, reads, L, mbq, k), expect(b, L, mbq, k), ("auto", mbq, k))
        assert not D.pileup_launch_info(reads, L, "tile", 4, "auto", 20, 5)["slice"]
    finally:
        ctx.set_shape("auto")
        reads.free()
