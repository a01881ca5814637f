"""One-op chunks of k_pileup's slice instance (process_chunk<.., SLICE> in basecount_amd/csrc/bc_tile.h
when every read of a chunk has ONE CIGAR op: three of a slot's four 16-B pieces issued, one CIGAR
word per read decoded directly, bc_slice::covered_one_op) against the forced general instance and
the oracle.

Every case runs the slice and the general instance forced over outputs prefilled with 0xFF bytes,
for k = 5 and 6, with the statistics tail (bc_pileup) and without it (bc_count's accumulate launch
into zeroed counts): the two instances must be equal array by array and equal to the oracle
(O.bcount, O.stats) bit for bit, and bc_range_error must be the oracle's first offending read.
References are 640-1,300 positions with at most 600 reads, but for `test_longest_tiled_reads`:
reads of 4,095 and 4,096 bases need a reference that long to be counted at all (on the short
references they only ever name the first offending read, which `test_read_beyond_the_reference`
checks).  4,096 is the longest span the tiled kernels are launched with (kTileMaxSpan,
bc_internal.h: a batch beyond it goes to the read-chunked kernel under any shape), so the lengths
0x1FFE and 0x1FFF, where a read turns complex, reach the one-op decode on the host alone
(tests/test_one_op_host.py).

The buffer's end: the readable bytes end 16-31 B after the last base's byte (bc_seq_event_bytes),
and a slot's first 16 B hold a needed base, so at least 32 B of a slot are readable: its last
16 B or its last 32 B can lie beyond the end, never its last 48.  `end_batch` builds the slots that
exist (64, 48 and 32 B of the last read's last slot below the readable end) and asserts that
arithmetic."""
import functools

import numpy as np
import pytest

import stage_layouts as SL
import test_gpu_slice_stage as SS
import test_gpu_stage_layouts as GS
from basecount_amd import device as D

pytestmark = pytest.mark.gpu

M, I, DEL, SKIP, S, H, P, EQ, X = 0, 1, 2, 3, 4, 5, 6, 7, 8
LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 129, 150, 250)  # and 0 (0M), 4,095, 4,096 below
SETTINGS = (("tile", 4), ("tile_no_solo", 1))


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    try:
        yield c
    finally:
        c.set_shape("auto")
        c.set_instance("auto")


@functools.lru_cache(maxsize=None)
def expected(key, L, k):
    """The oracle's arrays and first offending read of batch `key` (computed once per (L, k))."""
    return SS.expect(BATCHES[key](), L, 0, k)


def check(ctx, key, L, settings=SETTINGS):
    """Slice == general == oracle, k = 5 and 6, with and without the statistics tail."""
    b = BATCHES[key]()
    assert 640 <= L and b["pos"].size <= 600
    reads = D.DeviceReads(ctx, b)
    try:
        assert reads.r.sorted == 1
        for k in (5, 6):
            exp = expected(key, L, k)
            for setting in settings:
                for stats in (True, False):
                    e = exp if stats else (exp[0][:1], exp[1])
                    g = SS.forced(ctx, reads, L, 0, k, setting, "general", stats=stats)
                    s = SS.forced(ctx, reads, L, 0, k, setting, "slice", stats=stats)
                    GS.same(g, e, (key, "general", setting, k, stats))
                    GS.same(s, e, (key, "slice", setting, k, stats))
                    assert s[1] == g[1], (key, setting, k, stats)
                    if e[1] < 0:
                        for name, a, b_ in zip(GS.NAMES, s[0], g[0]):
                            assert np.array_equal(a, b_), (key, setting, k, stats, name, "slice differs from general")
    finally:
        reads.free()


def one_op_chunks(b):
    """Every read has one CIGAR op: every chunk of every tile is a one-op chunk."""
    return bool((b["cig_n"] == 1).all())


# ---------------------------------------------------------------- all-M reads
@functools.lru_cache(maxsize=None)
def lengths_batch():
    """32 all-M reads of every length of LENGTHS, each length at every seq_nib mod 32 (both nibble
    parities, every 16-B alignment), starts spread over [0, 740): they end below position 990."""
    rng = np.random.default_rng(21)
    reads = [SS.read_of(rng, (53 * i + 7 * j) % 740, [(M, n)]) for j, n in enumerate(LENGTHS) for i in range(32)]
    reads.sort(key=lambda r: r[0])
    seen, res = {}, []
    for r in reads:
        n = len(r[2])
        res.append((7 * seen.get(n, 0) + n) % 32)
        seen[n] = seen.get(n, 0) + 1
    b = SS.make_batch(reads, residues=res)
    for n in LENGTHS:
        sel = (b["cigar"] >> 4) == n
        assert sel.sum() == 32 and set(b["seq_nib"][sel] % 32) == set(range(32))
    assert one_op_chunks(b) and int((b["pos"] + (b["cigar"] >> 4)).max()) <= 990
    return b


def test_all_m_lengths(ctx):
    """Lengths 1-250 at every sequence alignment; L = 1000 holds every read."""
    assert expected("lengths", 1000, 5)[1] == -1
    check(ctx, "lengths", 1000)


def test_read_beyond_the_reference(ctx):
    """The same reads on 900 and 640 positions (an edge tile; tiles wholly past L), and the longest
    reads a tiled launch takes on 1,300: the first offending read is the oracle's."""
    for L in (900, 640):
        assert expected("lengths", L, 5)[1] >= 0
        check(ctx, "lengths", L, settings=SETTINGS[:1])
    assert expected("longest", 1300, 5)[1] >= 0
    check(ctx, "longest", 1300, settings=SETTINGS[:1])


@functools.lru_cache(maxsize=None)
def longest_batch():
    """Reads of 4,096 bases (kTileMaxSpan) and 4,095, at both nibble parities, among 150-base reads."""
    rng = np.random.default_rng(22)
    reads = [SS.read_of(rng, p, [(M, 150)]) for p in range(0, 1100, 11)]
    reads += [SS.read_of(rng, p, [(M, n)]) for p, n in ((3, 4096), (40, 4095), (77, 4096), (130, 4095))]
    reads.sort(key=lambda r: r[0])
    b = SS.make_batch(reads, residues=[(5 * i + 1) % 32 for i in range(len(reads))])
    long_ = (b["cigar"] >> 4) >= 4095
    assert one_op_chunks(b) and set(b["seq_nib"][long_] & 1) == {0, 1}
    return b


def test_longest_tiled_reads(ctx):
    """4,095 and 4,096 bases counted on a reference that holds them (4,352 positions)."""
    L = 4352
    b = BATCHES["longest"]()
    assert int((b["pos"] + (b["cigar"] >> 4)).max()) <= L and b["pos"].size <= 600
    reads = D.DeviceReads(ctx, b)
    try:
        for k in (5, 6):
            exp = expected("longest", L, k)
            assert exp[1] == -1
            g = SS.forced(ctx, reads, L, 0, k, ("tile", 4), "general")
            s = SS.forced(ctx, reads, L, 0, k, ("tile", 4), "slice")
            GS.same(g, exp, ("longest", "general", k))
            GS.same(s, exp, ("longest", "slice", k))
    finally:
        reads.free()


# ---------------------------------------------------------------- every op alone
@functools.lru_cache(maxsize=None)
def ops_batch():
    """Single-op reads of every op (I, S, D, N, =, X, H, P of 100, and 0M) among 150-base all-M
    reads: every chunk is a one-op chunk; D and N are gaps (walked alone), = and X count as M does,
    the others count nothing."""
    rng = np.random.default_rng(23)
    reads = [SS.read_of(rng, p, [(M, 150)]) for p in range(0, 1000, 5)]
    for j, op in enumerate((I, S, DEL, SKIP, EQ, X, H, P)):
        reads += [SS.read_of(rng, 29 * j + 97 * i + 3, [(op, 100)]) for i in range(10)]
    reads += [SS.read_of(rng, 61 * i + 9, [(M, 0)]) for i in range(10)]
    reads.sort(key=lambda r: r[0])
    b = SS.make_batch(reads, residues=[(11 * i) % 32 for i in range(len(reads))])
    assert one_op_chunks(b) and set(b["cigar"] & 15) == {M, I, DEL, SKIP, S, H, P, EQ, X}
    return b


def test_every_single_op(ctx):
    check(ctx, "ops", 1200)


# ---------------------------------------------------------------- both setups in one tile
@functools.lru_cache(maxsize=None)
def mixed_batch():
    """Reads that all start in tile 0 (the read index fixes chunk and slot there): reads 0-63 have
    one op, reads 64-127 hold one two-op read (5I145M) and one read without a CIGAR (cig_n == 0),
    reads 128-191 have one op again."""
    rng = np.random.default_rng(24)
    pos = np.sort(rng.integers(0, 40, 192))
    reads = [SS.read_of(rng, p, [(M, 150)]) for p in pos]
    reads[80] = SS.read_of(rng, pos[80], [(I, 5), (M, 145)])
    reads[101] = SS.read_of(rng, pos[101], [(H, 0)])  # its word is dropped below
    b = SS.make_batch(reads)
    w = int(b["cig_beg"][101])
    b["cigar"] = np.delete(b["cigar"], w)
    b["cig_n"][101] = 0
    b["cig_beg"][102:] -= 1
    n = b["cig_n"]
    assert (n[:64] == 1).all() and (n[128:] == 1).all() and n[80] == 2 and n[101] == 0 and (n[64:128] == 1).sum() == 62
    assert int(b["cig_beg"][-1]) + 1 == b["cigar"].size and int(b["cig_beg"][101]) < b["cigar"].size
    return b


def test_one_op_chunk_next_to_a_general_chunk(ctx):
    check(ctx, "mixed", 640)


# ---------------------------------------------------------------- the buffer's end
def end_cut(b):
    """Bytes of the last read's last tile's slot that lie below the buffer's readable end."""
    p, n, sn = int(b["pos"][-1]), int(b["cigar"][-1] >> 4), int(b["seq_nib"][-1])
    t0 = (p + n - 1) // 64 * 64
    src = ((sn + max(t0 - p, 0)) // 2) & ~15
    return SL.seq_event_bytes(b["seq"].size) - src


@functools.lru_cache(maxsize=None)
def end_batch(cut, odd):
    """300 reads of 150 bases and a last read, alone on its last tiles and last in the buffer (its
    last base is the buffer's last nibble or the one before), of the length that leaves `cut` bytes
    of its last slot below the readable end."""
    rng = np.random.default_rng(25)
    head = [SS.read_of(rng, p, [(M, 150)]) for p in np.sort(rng.integers(0, 700, 300))]
    for n in range(150, 280):
        reads = head + [SS.read_of(np.random.default_rng(26), 760, [(M, n)])]
        b = SS.make_batch(reads, residues=[(5 * i + odd) % 32 for i in range(len(reads))], tail=0)
        assert end_cut(b) >= 32  # a slot's first 16 B hold a needed base: never the last 16 alone
        if end_cut(b) == cut and one_op_chunks(b):
            assert int(b["seq_nib"][-1]) + n in (2 * b["seq"].size, 2 * b["seq"].size - 1)
            return b
    raise AssertionError(("no length leaves this cut", cut, odd))


@pytest.mark.parametrize("cut", [64, 48, 32])
def test_slices_at_the_buffer_end(ctx, cut):
    """The last slot ends at the buffer's readable end (64), its last 16 B (48) and its last 32 B
    (32) lie beyond it: the pieces that begin beyond it are not copied, and nothing of them is read."""
    for odd in (0, 1):
        check(ctx, ("end", cut, odd), 1100, settings=SETTINGS[:1])


# ---------------------------------------------------------------- N bases
@functools.lru_cache(maxsize=None)
def n_batch():
    """A third of all bases are N (BAM code 15): the fix-up counters run in every chunk."""
    rng = np.random.default_rng(27)
    reads = []
    for p in np.sort(rng.integers(0, 850, 500)):
        pos, ops, codes, q = SS.read_of(rng, p, [(M, 150)])
        codes[rng.random(codes.size) < 1 / 3] = 15
        reads.append((pos, ops, codes, q))
    b = SS.make_batch(reads, residues=[(3 * i + 2) % 32 for i in range(len(reads))])
    assert one_op_chunks(b)
    return b


def test_reads_with_n(ctx):
    exp = expected("n", 1000, 6)
    assert exp[1] == -1 and exp[0][0][5].sum() > 10_000  # the N column
    check(ctx, "n", 1000)


class _Batches(dict):
    def __missing__(self, key):  # ("end", cut, odd)
        return functools.partial(end_batch, key[1], key[2])


BATCHES = _Batches(lengths=lengths_batch, longest=longest_batch, ops=ops_batch, mixed=mixed_batch, n=n_batch)
