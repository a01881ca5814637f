"""k_pileup's lean instance (one-run, ungapped reads in the window walk; every other read walked
alone by walk_complex) against the general instance and the oracle.

Every case runs both instances forced (bc_ctx_set_instance) over output buffers prefilled with
0xFF bytes: the two must be equal array by array, and equal to the oracle (O.bcount, O.stats)
bit for bit; on references shorter than the reads' reach the first offending read index must be
the oracle's from both.  L = 640 with 30-base reads as in test_gpu_pileup_groups, and one case of
150-base reads on L = 1,000.

Chunks: a wave takes the reads [lo, hi) of its tile 64 at a time, wave w of S the chunks w, w + S,
...; tile 0's range starts at read 0, so for reads that all start inside tile 0 the read index
fixes the chunk and the slot."""
import functools

import numpy as np
import pytest

import oracle as O
import test_gpu_tile_tail as TT
from basecount_amd import device as D
from basecount_amd.main import norm_factors

pytestmark = pytest.mark.gpu

A, C_, G, T, N = TT.A, TT.C_, TT.G, TT.T, TT.N
M, I, DEL, S = TT.M, TT.I, TT.DEL, TT.S
SKIP, EQ, X = 3, 7, 8
NAMES = ("counts", "cov", "pc", "ent", "sec")
SETTINGS = [("tile", 4), ("tile", 8), ("tile_no_solo", 1), ("tile_no_solo", 2)]
FAST = ("plain", "clipped", "eqx")
SLOW = ("ins", "del", "skip", "many")


def ops_of(kind, n):
    """The CIGAR of an n-base read (n >= 24) of the given kind."""
    if kind == "plain":
        return [(M, n)]
    if kind == "clipped":  # three ops, one run
        return [(S, 3), (M, n - 5), (S, 2)]
    if kind == "eqx":      # M-like ops merge into one run
        return [(EQ, 10), (X, 4), (M, n - 14)]
    if kind == "ins":
        return [(M, n // 2), (I, 1), (M, n - n // 2 - 1)]
    if kind == "del":      # two runs
        return [(M, n // 2), (DEL, 1), (M, n - n // 2)]
    if kind == "skip":
        return [(M, 10), (SKIP, 7), (M, n - 10)]
    assert kind == "many"  # more than 8 ops
    return [(M, 3), (I, 1), (M, 3), (DEL, 1), (M, 3), (I, 1), (M, 3), (DEL, 2), (M, 3), (I, 1), (M, n - 18)]


def read_of(rng, pos, kind, n=30):
    ops = ops_of(kind, n)
    q = sum(ln for op, ln in ops if op in (M, I, S, EQ, X))
    assert q == n
    codes = np.array([A, C_, G, T], np.uint8)[rng.integers(0, 4, q)]
    codes[rng.random(q) < 0.05] = N
    return (int(pos), ops, codes, rng.integers(0, 45, q).astype(np.uint8))


def batch_of(n, lo, hi, slow_at, seed, nbases=30, scatter=False):
    """n reads with sorted starts in [lo, hi); read i (in start order) is slow where slow_at(i)."""
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(lo, hi, n))
    reads = [read_of(rng, p, SLOW[i % 4] if slow_at(i) else FAST[i % 3], nbases) for i, p in enumerate(pos)]
    b = TT.build_batch(reads)
    if scatter:  # every second read's bases far behind the others': a chunk's segment exceeds any stage
        b = scattered(b, reads)
    return b


def scattered(b, reads):
    reads = sorted(reads, key=lambda r: r[0])
    hole = 40_000  # nibbles
    total = int(sum(len(r[2]) + (len(r[2]) & 1) for r in reads))
    allc = np.zeros(total + hole + 2, np.uint8)
    qual = np.zeros(total + hole + 2, np.uint8)
    at = [0, total // 2 + hole]
    at[1] += at[1] & 1
    seq_nib = np.zeros(len(reads), np.uint32)
    for i, (_, ops, s, q) in enumerate(reads):
        h = i & 1 if at[0] + len(s) + 1 < total // 2 + hole else 1
        allc[at[h]: at[h] + len(s)] = s
        qual[at[h]: at[h] + len(q)] = q
        seq_nib[i] = at[h] + (ops[0][1] if ops[0][0] == S else 0)
        at[h] += len(s) + (len(s) & 1)
    assert at[1] <= allc.size - 2
    return dict(b, seq_nib=seq_nib, seq=((allc[0::2] << 4) | allc[1::2]).astype(np.uint8), qual=qual)


# name -> (n reads, start range, slow_at, extras)
CASES = {
    "all_one_run": dict(n=900, lo=0, hi=600, slow_at=lambda i: False),
    # one slow read per chunk of tile 0: slot 0, slot 63, and the last slot of the short final chunk
    "one_per_chunk": dict(n=64 * 5 + 17, lo=0, hi=40, slow_at=lambda i: i % 128 in (0, 127) or i == 64 * 5 + 16),
    # slow reads over the whole reference (straddling first and last windows of tiles), ~1 in 9
    "sprinkled": dict(n=1500, lo=0, hi=600, slow_at=lambda i: i % 9 == 4),
    "chunk_all_slow": dict(n=400, lo=0, hi=40, slow_at=lambda i: 64 <= i < 128),
    # S = 1 / 2 / 4 / 8: chunks alternate all-fast and all-slow for every wave of tile 0
    "alternate_1": dict(n=1500, lo=0, hi=34, slow_at=lambda i: (i // 64) % 2 == 1),
    "alternate_4": dict(n=1500, lo=0, hi=34, slow_at=lambda i: (i // 256) % 2 == 1),
    "alternate_8": dict(n=2100, lo=0, hi=34, slow_at=lambda i: (i // 512) % 2 == 1),
    # more slow reads in one wave's tile than flush_acc's 10-bit fields hold (one wave per tile: 1,200)
    "flush": dict(n=1200, lo=0, hi=34, slow_at=lambda i: True),
    # reads out of file order in seq: no chunk's segment fits the stage
    "scattered": dict(n=700, lo=0, hi=600, slow_at=lambda i: i % 50 == 7, scatter=True),
}


@functools.lru_cache(maxsize=None)
def case(name, L=640):
    kw = dict(CASES[name])
    b = batch_of(kw.pop("n"), kw.pop("lo"), kw.pop("hi"), kw.pop("slow_at"), sum(map(ord, name)), **kw)
    exp = {}
    for mbq in (0, 20):
        cnt, (bad, _) = O.bcount(L, mbq, b)
        assert bad == -1
        for k in (5, 6):
            exp[k, mbq] = (cnt[:, :k].T.astype(np.int32),) + tuple(O.stats(cnt, k == 6))
    return b, exp


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    yield c
    c.set_shape("auto")
    c.set_instance("auto")


def run(ctx, reads, L, mbq, k, stats=True):
    """bc_pileup (or bc_count into zeroed counts) over 0xFF-prefilled outputs -> (arrays, bad)."""
    sizes = (4 * k * L, 4 * L, 8 * k * L, 8 * L, 8 * L)
    bufs = [ctx.alloc(max(8, n)) for n in sizes]
    for x in bufs:
        D.check(D.lib().bc_memset(ctx.h, x.ptr, 0 if not stats else 0xFF, x.nbytes))
    if stats:
        nf, nf2 = norm_factors(k)
        try:
            ctx.pileup(reads, L, mbq, k, nf, nf2, *[x.ptr for x in bufs])
        except D.BcError:
            pass
    else:
        try:
            ctx.count(reads, L, mbq, k, bufs[0].ptr)
        except D.BcError:
            pass
    bad = ctx.range_error()
    out = (bufs[0].download(np.int32, k * L).reshape(k, L), bufs[1].download(np.int32, L),
           bufs[2].download(np.float64, k * L).reshape(k, L), bufs[3].download(np.float64, L),
           bufs[4].download(np.float64, L))
    for x in bufs:
        x.free()
    return (out if stats else out[:1]), bad


def both(ctx, reads, L, mbq, k, setting, stats=True):
    """Both instances forced: each must really be the one asked for; -> {instance: (arrays, bad)}."""
    ctx.set_shape(*setting)
    res = {}
    for inst in ("general", "lean"):
        ctx.set_instance(inst)
        info = D.pileup_launch_info(reads, L, setting[0], setting[1], inst, mbq, k)
        assert info["kernel"] == "tiles" and info["lean"] == (inst == "lean"), (inst, info)
        res[inst] = run(ctx, reads, L, mbq, k, stats)
    ctx.set_instance("auto")
    return res


def compare(res, exp, what):
    (g, gbad), (l, lbad) = res["general"], res["lean"]
    assert gbad == lbad == -1, what
    for name, a, b_, e in zip(NAMES, g, l, exp):
        assert np.array_equal(a, b_), (what, name, "lean differs from general")
        assert np.array_equal(b_, e), (what, name, "lean differs from the oracle")


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("name", sorted(CASES))
def test_lean_equals_general_and_oracle(ctx, name, setting):
    L = 640
    b, exp = case(name)
    reads = D.DeviceReads(ctx, b)
    assert reads.r.sorted == 1
    # k and the threshold vary with the case and the setting; every (k, mbq) is met by every
    # setting over the cases, and the two cases below by all four
    full = name in ("sprinkled", "one_per_chunk")
    combos = [(5, 0), (6, 0), (5, 20), (6, 20)]
    pick = combos if full else [combos[(sorted(CASES).index(name) + SETTINGS.index(setting)) % 4], (5, 0)]
    for k, mbq in dict.fromkeys(pick):
        compare(both(ctx, reads, L, mbq, k, setting), exp[k, mbq], (name, setting, k, mbq))
    reads.free()


@pytest.mark.parametrize("k", [5, 6])
def test_lean_counts_only(ctx, k):
    """bc_count's accumulate launch (no statistics) takes the same instances."""
    L = 640
    b, exp = case("sprinkled")
    reads = D.DeviceReads(ctx, b)
    for mbq in (0, 20):
        res = both(ctx, reads, L, mbq, k, ("tile", 4), stats=False)
        compare(res, exp[k, mbq][:1], ("counts", k, mbq))
    reads.free()


def test_long_reads(ctx):
    """150-base reads on L = 1,000: 64 x 75 B of sequence per chunk, inside the lean stage."""
    L = 1000
    b = batch_of(2000, 0, L - 160, lambda i: i % 16 == 3, 150, nbases=150)
    reads = D.DeviceReads(ctx, b)
    for mbq in (0, 20):
        cnt, (bad, _) = O.bcount(L, mbq, b)
        assert bad == -1
        exp = (cnt[:, :5].T.astype(np.int32),) + tuple(O.stats(cnt, False))
        for setting in (("tile", 4), ("tile", 8)):
            compare(both(ctx, reads, L, mbq, 5, setting), exp, ("long", setting, mbq))
    reads.free()


# (name, kinds of the reads that reach past L in start order): the first offender a fast read, a
# slow read, and one of each in the last tile in both orders
EDGE = [("fast", ("plain",)), ("slow", ("del",)), ("slow_then_fast", ("ins", "plain")),
        ("fast_then_slow", ("clipped", "many"))]


@pytest.mark.parametrize("name,kinds", EDGE)
def test_first_offending_read(ctx, name, kinds):
    """Reads that end past L, on an edge tile (L = 630: tile 9 is partial) and on tiles wholly
    past L (L = 576): both instances report the oracle's read index."""
    rng = np.random.default_rng(len(name))
    reads = [read_of(rng, p, (FAST + SLOW)[i % 7]) for i, p in enumerate(np.sort(rng.integers(0, 540, 600)))]
    reads += [read_of(rng, 612 + 2 * j, kind) for j, kind in enumerate(kinds)]  # ends at 642 and beyond
    b = TT.build_batch(reads)
    dr = D.DeviceReads(ctx, b)
    for L in (630, 576):
        for mbq in (0, 20):
            _, (br, _) = O.bcount(L, mbq, b)
            assert br >= 0
            for setting in (("tile", 4), ("tile_no_solo", 1)):
                res = both(ctx, dr, L, mbq, 5, setting)
                assert res["general"][1] == br and res["lean"][1] == br, (name, L, mbq, setting, br)
    _, (br, _) = O.bcount(630, 0, b)
    assert br == 600  # the first of the reads past L: the kind under test
    dr.free()


def test_auto_takes_lean_on_all_m_batch(ctx):
    """BC_SHAPE_AUTO with BC_INSTANCE_AUTO on an all-M batch above the sparse sweep's depth: the
    lean instance, five workgroups resident per CU, and bc_pileup_plan's answers unchanged."""
    import test_gpu_pileup_groups as PG
    L = 640
    b = PG.all_m_batch(2000, L, 30, 3)
    reads = D.DeviceReads(ctx, b)
    ctx.set_shape("auto")
    ctx.set_instance("auto")
    info = D.pileup_launch_info(reads, L)
    assert (info["kernel"], info["lean"], info["waves_per_tile"], info["block_threads"]) == ("tiles", True, 4, 256)
    assert info["lds_bytes"] == 31_936 and info["blocks_per_cu"] == 5
    p = D.pileup_plan(reads, L)
    assert (p["kernel"], p["lds_bytes"], p["blocks_per_cu"], p["block_threads"]) == ("tiles", 40_640, 4, 256)
    cnt, (bad, _) = O.bcount(L, 0, b)
    exp = (cnt[:, :5].T.astype(np.int32),) + tuple(O.stats(cnt, False))
    got, gbad = run(ctx, reads, L, 0, 5)
    assert gbad == -1
    for name, g, e in zip(NAMES, got, exp):
        assert np.array_equal(g, e), name
    reads.free()
