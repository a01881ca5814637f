"""k_pileup's tile groups and its statistics tail by 16-position groups: a group whose deletion
and N columns are zero takes one pass with four lanes per position, any other two passes with
eight, and the tiled kernel takes four waves per tile from the depth (bc_pileup_plan).

Every output is compared with the oracle (O.bcount, O.stats): counts and coverage exact,
percentages and both entropies bit for bit.  The output buffers are prefilled with a byte pattern
no result can equal and carry guard elements behind the last one: every element below L must have
been written, and nothing beyond."""
import functools

import numpy as np
import pytest

import oracle as O
import test_gpu_tile_tail as TT
from basecount_amd import device as D
from basecount_amd.main import norm_factors

pytestmark = pytest.mark.gpu

A, C_, G, T, N = TT.A, TT.C_, TT.G, TT.T, TT.N
M, DEL = TT.M, TT.DEL
plain = TT.plain
GUARD = 64                       # elements behind every output array
FILL = 0x5A                      # int32 0x5A5A5A5A, float64 ~2.9e130: no count, percentage or entropy
SETTINGS = [("tile", 1), ("tile", 2), ("tile", 4), ("tile", 8), ("tile_no_solo", 1)]
NAMES = ("counts", "cov", "pc", "ent", "sec")


@pytest.fixture(scope="module")
def ctx():
    return D.Context(0)


@pytest.fixture(autouse=True)
def _auto_shape(ctx):
    yield
    ctx.set_shape("auto")


def gapped(pos, left, gap, right):
    """left M, gap D, right M: deletions at [pos + left, pos + left + gap)."""
    n = left + right
    return (pos, [(M, left), (DEL, gap), (M, right)], np.array(([A, C_, G, T] * n)[:n], np.uint8),
            np.full(n, 40, np.uint8))


def hand_reads(L):
    """Reads inside [0, L) that make each kind of position the tail treats differently, laid out by
    16-position group so that one tile mixes both tail passes."""
    if L < 15:  # L = 1
        return [plain(0, [A]), plain(0, [A]), plain(0, [C_])]
    r = []
    if L < 54:
        # one group: 0-1 no coverage, 2-3 one allele, 4-5 a tie, 6-9 1M 2D 1M (7-8 deletions only:
        # the group takes the eight-lane passes), 10-11 N only, 12-13 T against N, 14 one A
        r += [plain(2, [A, A])] * 3 + [plain(4, [A, A]), plain(4, [C_, C_])]
        r += [gapped(6, 1, 2, 1)] * 2
        r += [plain(10, [N, N]), plain(12, [T, T]), plain(12, [N, N]), plain(14, [A])]
        # L = 16, 17: the positions behind; 16 opens a second group, without deletions or N
        r += [plain(p, [G]) for p in range(15, L)] + [plain(p, [C_]) for p in range(16, L)]
        return r
    # group 0, [0, 16): no deletion, no N.  0-3 no coverage, 4-7 one allele, 8-9 tie A = C (first
    # maximum A), 10-11 tie C = G above A (first maximum C), 12-13 three-way tie C = G = T above A
    r += [plain(4, [A] * 4)] * 3
    r += [plain(8, [A, A]), plain(8, [C_, C_])]
    r += [plain(10, [C_, C_])] * 2 + [plain(10, [G, G])] * 2 + [plain(10, [A, A])]
    r += [plain(12, [b, b]) for b in (C_, C_, G, G, T, T, A)]
    # group 1, [16, 32): the only group with deletions (20-23 deletions only; 18-19, 24-25 bases)
    r += [gapped(18, 2, 4, 2)] * 2 + [plain(28, [T, G, C_])]
    # group 2, [32, 48): all-M again
    r += [plain(32, [A, C_, G, T] * 4), plain(34, [C_] * 12), plain(40, [C_, A, A, T])]
    # group 3, [48, 64): N only at 50-51, T against N at 52-53: no column with k = 5 (a four-lane
    # group), column 5 with k = 6 (an eight-lane group)
    r += [plain(50, [N, N]), plain(52, [T, T]), plain(52, [N, N])]
    # the positions behind, up to the last one: all-M and mixed reads
    if L > 54:
        r += [plain(p, [G]) for p in range(54, min(L, 66))]
    if L > 70:
        r += TT.random_reads(np.random.default_rng(L), 200, 66, L)
        r += [plain(L - 4, [A, C_, G, T])]
    return r


@functools.lru_cache(maxsize=None)
def hand_batch(L):
    """The batch and, per (k, mbq), the oracle's results: computed once per L."""
    b = TT.build_batch(hand_reads(L))
    exp = {}
    for mbq in (0, 20):
        cnt, (bad, _) = O.bcount(L, mbq, b)
        assert bad == -1
        for k in (5, 6):
            exp[k, mbq] = (cnt[:, :k].T.astype(np.int32),) + tuple(O.stats(cnt, k == 6))
    return b, exp


class Outputs:
    """bc_pileup's five output arrays, prefilled, with GUARD elements behind each."""

    def __init__(self, ctx, L, k):
        self.sizes = (k * L, L, k * L, L, L)
        self.dtypes = (np.int32, np.int32, np.float64, np.float64, np.float64)
        self.shapes = ((k, L), (L,), (k, L), (L,), (L,))
        self.bufs = []
        for n, dt in zip(self.sizes, self.dtypes):
            buf = ctx.alloc((n + GUARD) * np.dtype(dt).itemsize)
            D.check(D.lib().bc_memset(ctx.h, buf.ptr, FILL, buf.nbytes))
            self.bufs.append(buf)

    def ptrs(self):
        return [x.ptr for x in self.bufs]

    def download(self):
        """The arrays; asserts that the guards still hold the fill pattern."""
        out = []
        for name, buf, n, dt, shape in zip(NAMES, self.bufs, self.sizes, self.dtypes, self.shapes):
            a = buf.download(dt, n + GUARD)
            assert np.all(a[n:].view(np.uint8) == FILL), ("written beyond the array", name)
            out.append(a[:n].reshape(shape))
        return out

    def free(self):
        for x in self.bufs:
            x.free()


def untouched(a):
    return np.all(a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,)) == FILL, axis=-1)


def run(ctx, reads, L, mbq, k):
    o = Outputs(ctx, L, k)
    nf, nf2 = norm_factors(k)
    ctx.pileup(reads, L, mbq, k, nf, nf2, *o.ptrs())
    assert ctx.range_error() == -1
    got = o.download()
    o.free()
    return got


def check(got, exp, what):
    for name, g, e in zip(NAMES, got, exp):
        assert not untouched(g).any(), (what, name, "an element below L was not written")
        assert np.array_equal(g, e), (what, name)


def test_hand_batches_hold_every_kind():
    """(CPU) the hand-made reads give a stretch without coverage, one-allele positions, ties,
    deletion-only positions in one group with none in its neighbours, and N-only positions."""
    for L in (63, 64, 65, 130):
        _, exp = hand_batch(L)
        for (k, mbq), (cnt, cov, pc, ent, sec) in exp.items():
            c = cnt.astype(np.int64)
            assert not cov[0:4].any() and np.all(pc[:, 0:4] == -1.0) and np.all(ent[0:4] == 1.0)
            assert np.all(c[0, 4:8] == cov[4:8]) and np.all(ent[4:8] == 0.0) and np.all(sec[4:8] == 1.0)
            assert np.all(c[0, 8:10] == c[1, 8:10]) and np.all(c[1, 10:14] == c[2, 10:14])
            assert np.all(c[2, 12:14] == c[3, 12:14])
            assert np.all(c[4, 20:24] == 2) and np.all(cov[20:24] == 2)       # deletions only
            assert not c[4, 0:16].any() and not c[4, 32:64].any()             # and none beside
            assert np.all(cov[50:52] == (1 if k == 6 else 0))                 # N only
            if k == 6:
                assert np.all(c[5, 50:54] == 1) and not c[5, 0:48].any()
    for L in (15, 16, 17):
        _, exp = hand_batch(L)
        cnt = exp[6, 0][0]
        assert np.all(cnt[4, 7:9] == 2) and np.all(cnt[5, 10:14] == 1) and not exp[5, 0][1][0:2].any()


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("L", [1, 15, 16, 17, 63, 64, 65, 130])
def test_groups_against_oracle(ctx, L, setting):
    b, exp = hand_batch(L)
    reads = D.DeviceReads(ctx, b)
    assert reads.r.sorted == 1
    ctx.set_shape(*setting)
    p = D.pileup_plan(reads, L, *setting)
    assert p["waves_per_tile"] == setting[1]
    assert p["kernel"] == ("solo" if setting == ("tile", 1) else "tiles")
    for (k, mbq), e in exp.items():
        check(run(ctx, reads, L, mbq, k), e, (L, setting, k, mbq))
    reads.free()


def all_m_batch(n, L, span, seed):
    """n all-M reads of `span` bases, sorted, inside [0, L): reads_per_tile = n (span + 63) / L."""
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, L - span + 1, n))
    pos[0], pos[-1] = 0, L - span  # the reach is L whatever the draw
    codes = np.array([A, C_, G, T], np.uint8)
    return TT.build_batch([plain(int(p), codes[rng.integers(0, 4, span)]) for p in pos])


# L = 640, 30-base reads: reads_per_tile = n x 93 / 640.  The rule's thresholds are 48 (one wave,
# the sparse sweep, up to it; four waves above) and 2,048 (the read-chunked kernel from there on)
THRESHOLDS = [(330, "solo", 1), (331, "tiles", 4), (14_093, "tiles", 4), (14_094, "rc", 0)]


@pytest.mark.parametrize("n,kernel,waves", THRESHOLDS)
def test_auto_at_the_rule_thresholds(ctx, n, kernel, waves):
    L, span = 640, 30
    b = all_m_batch(n, L, span, n)
    reads = D.DeviceReads(ctx, b)
    assert (reads.r.max_span, reads.r.max_end) == (span, L)
    p = D.pileup_plan(reads, L)
    assert p["reads_per_tile"] == n * 93 / 640
    assert (p["reads_per_tile"] <= 48) == (kernel == "solo") and (p["reads_per_tile"] >= 2048) == (kernel == "rc")
    assert (p["kernel"], p["waves_per_tile"]) == (kernel, waves)
    if kernel == "tiles":
        assert (p["block_threads"], p["blocks_per_cu"]) == (256, 4)  # four workgroups really resident
    cnt, (bad, _) = O.bcount(L, 0, b)
    assert bad == -1
    exp = (cnt[:, :5].T.astype(np.int32),) + tuple(O.stats(cnt, False))
    ctx.set_shape("auto")
    auto = run(ctx, reads, L, 0, 5)
    ctx.set_shape("tile", 8)
    assert D.pileup_plan(reads, L, "tile", 8)["blocks_per_cu"] == 2
    eight = run(ctx, reads, L, 0, 5)
    reads.free()
    for name, a, e in zip(NAMES, auto, eight):
        assert np.array_equal(a, e), (n, name, "auto differs from tile_waves = 8")
    check(auto, exp, (n, "auto"))


def test_two_contexts_in_one_graph(ctx):
    """Two contexts run the pileup side by side inside one captured graph (fork and join on the
    main context), on distinct batches and outputs: both equal the oracle, replay after replay."""
    L = 130
    side = D.Context(0)
    ctx.set_shape("auto")
    batches = [hand_batch(L)[0], all_m_batch(400, L, 30, 5)]
    exps = []
    for b in batches:
        cnt, (bad, _) = O.bcount(L, 0, b)
        assert bad == -1
        exps.append((cnt[:, :5].T.astype(np.int32),) + tuple(O.stats(cnt, False)))
    ctxs = (ctx, side)
    for c in ctxs:
        c.set_shape("tile", 4)
    reads = [D.DeviceReads(c, b) for c, b in zip(ctxs, batches)]
    outs = [Outputs(ctx, L, 5) for _ in ctxs]
    nf, nf2 = norm_factors(5)

    def both():
        side.wait(ctx)
        for c, r, o in zip(ctxs, reads, outs):
            for _ in range(3):
                c.pileup(r, L, 0, 5, nf, nf2, *o.ptrs())
        ctx.wait(side)

    both()  # (uncaptured first: the kernels' one-time launch setup stays out of the capture)
    ctx.sync()
    g = ctx.capture(both)
    for o in outs:  # the replays start from prefilled buffers again
        for buf in o.bufs:
            D.check(D.lib().bc_memset(ctx.h, buf.ptr, FILL, buf.nbytes))
    ctx.sync()
    for _ in range(2):
        g.launch()
        ctx.sync()
        side.sync()
        assert ctx.range_error() == -1 and side.range_error() == -1
        for o, e, tag in zip(outs, exps, ("main", "side")):
            check(o.download(), e, ("graph", tag))
    del g
    for r in reads:
        r.free()
    for o in outs:
        o.free()
    side.set_shape("auto")
    side.close()
