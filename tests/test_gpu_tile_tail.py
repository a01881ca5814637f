"""k_pileup's statistics tail (eight lanes per position, every wave of a tile's group finishing
its own positions after the reduce barrier): counts and coverage exact, percentages and both
entropies bit for bit the oracle's, at every waves-per-tile setting, at the tile edges, with the
deletion / N columns skipped (all-M batches), with more than one tile per block (the loop-end
barrier) and with two groups per block."""
import functools

import numpy as np
import pytest

import oracle as O
from basecount_amd import device as D
from basecount_amd.main import norm_factors

pytestmark = pytest.mark.gpu

A, C_, G, T, N = 1, 2, 4, 8, 15  # BAM 4-bit base codes
M, I, DEL, S = 0, 1, 2, 4         # CIGAR ops
BLOCK = 32                        # the hand-made reads cover [0, BLOCK)


@pytest.fixture(scope="module")
def ctx():
    return D.Context(0)


@pytest.fixture(autouse=True)
def _auto_shape(ctx):
    yield
    ctx.set_shape("auto")


def build_batch(reads):
    """The batch dict (bc_reads layout) of reads given as (pos, [(op, len)], codes, quals),
    coordinate-sorted; each read's SEQ starts on a byte boundary."""
    reads = sorted(reads, key=lambda r: r[0])
    nib = np.zeros(len(reads) + 1, np.int64)
    nib[1:] = np.cumsum([len(r[2]) + (len(r[2]) & 1) for r in reads])
    allc = np.zeros(int(nib[-1]) + 2, np.uint8)
    qual = np.zeros(int(nib[-1]) + 2, np.uint8)
    for i, (_, _, s, q) in enumerate(reads):
        allc[nib[i]: nib[i] + len(s)] = s
        qual[nib[i]: nib[i] + len(q)] = q
    cig_n = np.array([len(r[1]) for r in reads], np.uint32)
    cig_beg = np.zeros(len(reads), np.uint32)
    cig_beg[1:] = np.cumsum(cig_n)[:-1]
    qstart = np.array([r[1][0][1] if r[1][0][0] == S else 0 for r in reads], np.int64)
    return dict(pos=np.array([r[0] for r in reads], np.int32), cig_beg=cig_beg, cig_n=cig_n,
                seq_nib=(nib[:-1] + qstart).astype(np.uint32),
                cigar=np.array([(ln << 4) | op for r in reads for op, ln in r[1]], np.uint32),
                seq=((allc[0::2] << 4) | allc[1::2]).astype(np.uint8), qual=qual)


def plain(pos, codes):
    """An all-M read of the given base codes, every quality 40."""
    return (pos, [(M, len(codes))], np.array(codes, np.uint8), np.full(len(codes), 40, np.uint8))


def hand_reads():
    """Reads on [0, BLOCK) that make each kind of position the tail treats differently."""
    r = []
    # 0-3: no coverage.  4-7: one allele only (A x 3)
    r += [plain(4, [A] * 4)] * 3
    # 8-9: two-way tie A = C (first maximum: A).  10-11: two-way tie C = G with A below (first: C)
    r += [plain(8, [A, A]), plain(8, [C_, C_])]
    r += [plain(10, [C_, C_])] * 2 + [plain(10, [G, G])] * 2 + [plain(10, [A, A])]
    # 12-13: three-way tie C = G = T at 2 with A at 1 (first maximum: C)
    r += [plain(12, [b, b]) for b in (C_, C_, G, G, T, T, A)]
    # 16-23: 2M 4D 2M twice: positions 18-21 hold deletions only
    r += [(16, [(M, 2), (DEL, 4), (M, 2)], np.array([A, C_, G, T], np.uint8), np.full(4, 40, np.uint8))] * 2
    # 24-25: N only (a column with k = 6, no coverage with k = 5).  26-27: T against N
    r += [plain(24, [N, N]), plain(26, [T, T]), plain(26, [N, N])]
    return r


def random_reads(rng, n, lo, hi):
    """n short reads inside [lo, hi): soft clips, an insertion or a deletion, 5 % N, random quality."""
    out = []
    for _ in range(n):
        ops = []
        if rng.random() < 0.4:
            ops.append((S, int(rng.integers(1, 4))))
        ops.append((M, int(rng.integers(2, 9))))
        kind = rng.integers(0, 3)
        if kind == 1:
            ops += [(I, int(rng.integers(1, 3))), (M, int(rng.integers(2, 9)))]
        elif kind == 2:
            ops += [(DEL, int(rng.integers(1, 4))), (M, int(rng.integers(2, 9)))]
        if rng.random() < 0.4:
            ops.append((S, int(rng.integers(1, 4))))
        span = sum(ln for op, ln in ops if op in (M, DEL))
        if span > hi - lo:
            continue
        q = sum(ln for op, ln in ops if op in (M, I, S))
        codes = np.array([A, C_, G, T], np.uint8)[rng.integers(0, 4, q)]
        codes[rng.random(q) < 0.05] = N
        out.append((int(rng.integers(lo, hi - span + 1)), ops, codes, rng.integers(0, 45, q).astype(np.uint8)))
    return out


@functools.lru_cache(maxsize=None)
def edge_batch(L):
    """The batch of the tile-edge cases and, per (k, mbq), the oracle's results: computed once."""
    rng = np.random.default_rng(1000 + L)
    if L >= BLOCK:
        reads = hand_reads() + random_reads(rng, 300, BLOCK, L)
    else:  # L = 1: three one-base reads (the kinds below need BLOCK positions)
        reads = [plain(int(rng.integers(0, L)), [b]) for b in (A, A, C_)]
    b = build_batch(reads)
    exp = {}
    for mbq in (0, 20):
        cnt, (bad, _) = O.bcount(L, mbq, b)
        assert bad == -1
        for k in (5, 6):
            exp[k, mbq] = (cnt[:, :k].T.astype(np.int32),) + tuple(O.stats(cnt, k == 6))
    return b, exp


def run_pileup(ctx, b, L, mbq, k):
    r = D.DeviceReads(ctx, b)
    assert r.r.sorted == 1
    bufs = [ctx.alloc(max(8, n)) for n in (4 * k * L, 4 * L, 8 * k * L, 8 * L, 8 * L)]
    nf, nf2 = norm_factors(k)
    ctx.pileup(r, L, mbq, k, nf, nf2, *[x.ptr for x in bufs])
    bad = ctx.range_error()
    out = (bufs[0].download(np.int32, k * L).reshape(k, L), bufs[1].download(np.int32, L),
           bufs[2].download(np.float64, k * L).reshape(k, L), bufs[3].download(np.float64, L),
           bufs[4].download(np.float64, L))
    r.free()
    for x in bufs:
        x.free()
    return out, bad


def set_waves(ctx, waves):
    ctx.set_shape("tile_no_solo" if waves == 1 else "tile", waves)


def check(got, exp, what, sl=slice(None)):
    for name, g, e in zip(("counts", "cov", "pc", "ent", "sec"), got, exp):
        assert np.array_equal(g[..., sl], e[..., sl]), (what, name)


def test_edge_batch_holds_every_kind():
    """(CPU) the hand-made block really holds a stretch without coverage, one-allele positions,
    a two-way and a three-way tie for the maximum and deletion-only positions, for every L that
    has room for it; (pc -1, ent = sec = 1) and (sec = 1) follow in the oracle's results."""
    for L in (63, 64, 65, 129, 700):
        _, exp = edge_batch(L)
        for (k, mbq), (cnt, cov, pc, ent, sec) in exp.items():
            c = cnt[:, :BLOCK].astype(np.int64)
            cv, mx = c.sum(0), c.max(0)
            ties = (c == mx).sum(0) * (mx > 0)
            assert np.all(cv[0:4] == 0) and np.all(pc[:, 0:4] == -1.0)
            assert np.all(ent[0:4] == 1.0) and np.all(sec[0:4] == 1.0)
            one = (cv > 0) & (cv == mx)
            assert one[4:8].all() and np.all(sec[:BLOCK][one] == 1.0) and np.all(ent[:BLOCK][one] == 0.0)
            assert np.all(ties[8:12] == 2) and np.all(ties[12:14] == 3)
            assert np.all(c[0, 8:10] == mx[8:10]) and np.all(c[1, 10:14] == mx[10:14])  # first maximum
            assert np.all((c[4, 18:22] == 2) & (cv[18:22] == 2))  # deletions only
            assert np.all(cv[24:26] == (1 if k == 6 else 0))      # N only


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 129, 700])
def test_tail_at_tile_edges(ctx, L, waves):
    b, exp = edge_batch(L)
    set_waves(ctx, waves)
    for (k, mbq), e in exp.items():
        got, bad = run_pileup(ctx, b, L, mbq, k)
        assert bad == -1
        check(got, e, (L, waves, k, mbq))


@pytest.mark.parametrize("k", [5, 6])
def test_tail_all_m_batch(ctx, k):
    """No deletion and no N anywhere: the tail skips those columns' terms."""
    rng = np.random.default_rng(7)
    L = 300
    reads = [plain(int(rng.integers(0, L - 30)), np.array([A, C_, G, T])[rng.integers(0, 4, 30)]) for _ in range(400)]
    b = build_batch(reads)
    cnt, (bad, _) = O.bcount(L, 0, b)
    assert bad == -1 and not cnt[:, 4:].any()
    set_waves(ctx, 8)
    got, bad = run_pileup(ctx, b, L, 0, k)
    assert bad == -1
    check(got, (cnt[:, :k].T.astype(np.int32),) + tuple(O.stats(cnt, k == 6)), ("all-M", k))


@pytest.mark.parametrize("waves,rounds", [(8, 16_384), (4, 16_384), (2, 2 * 16_384), (1, 4 * 16_384)])
def test_tail_more_than_one_tile_per_block(ctx, waves, rounds):
    """More tiles than the grid has blocks (16,384 at the most, each of nw / S tiles), at every
    group size: the blocks of the first tiles go on to the last three tiles, so fin and rng are
    reused behind the loop-end barrier.  Reads at both ends."""
    L = 64 * rounds + 130
    rng = np.random.default_rng(8)
    reads = random_reads(rng, 1_500, 0, 192) + random_reads(rng, 1_000, 64 * rounds - 100, 64 * rounds + 64)
    reads += random_reads(rng, 500, L - 66, L)
    b = build_batch(reads)
    cnt, (bad, _) = O.bcount(L, 0, b)
    assert bad == -1
    exp = (cnt[:, :5].T.astype(np.int32),) + tuple(O.stats(cnt, False))
    set_waves(ctx, waves)
    r = D.DeviceReads(ctx, b)
    p = D.pileup_plan(r, L, *ctx.shape_args[:2])
    r.free()
    n_tiles, groups = -(-L // 64), p["block_threads"] // 64 // waves  # tiles; tiles per block
    assert p["kernel"] == "tiles" and p["waves_per_tile"] == waves and groups >= 1
    assert p["blocks"] < n_tiles / groups  # some block takes a second round of tiles
    got, bad = run_pileup(ctx, b, L, 0, 5)
    assert bad == -1
    empty = rng.integers(200, 64 * rounds - 200, 4_096)
    assert not exp[1][empty].any()
    for sl in (slice(0, 256), slice(64 * rounds - 128, L), empty):
        check(got, exp, "multi-tile", sl)
    assert np.array_equal(got[1], exp[1])  # coverage everywhere


def test_tail_two_groups_per_block(ctx):
    """Two waves per tile on a four-wave block, several hundred reads per tile: both groups run
    the multi-chunk walk and finish their tiles side by side."""
    L = 300
    rng = np.random.default_rng(9)
    b = build_batch(random_reads(rng, 2_500, 0, L))
    set_waves(ctx, 2)
    for k, mbq in ((5, 0), (6, 20)):
        cnt, (bad, _) = O.bcount(L, mbq, b)
        assert bad == -1
        got, bad = run_pileup(ctx, b, L, mbq, k)
        assert bad == -1
        check(got, (cnt[:, :k].T.astype(np.int32),) + tuple(O.stats(cnt, k == 6)), ("two groups", k, mbq))
