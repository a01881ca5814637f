"""k_ops' window passes (k_ops_passes, bc_ops.hip; DESIGN.md §3 "k_ops"): reads longer than the
4096-position LDS window are counted over consecutive windows, every event in exactly the pass that
owns its position.

Every case of tests/ops_passes.py (proved to hold the piece it is named for by
tests/test_ops_passes_host.py) runs with the passes forced to 2, 3 and the cap and chosen by the
plan, with 1, 3 and 64 reads per workgroup, and is compared bit for bit with the oracle, with the
single window (``set_ops_passes(1)``) and with the forced ``rc`` shape.  Then depth, qualities, the
sorted view of an unsorted batch, every tail that follows kernel 1, graph replay and the unsorted
batch."""
import numpy as np
import pytest

import ops_passes as OP
import oracle as O
import saturation_batches as SB
from basecount_amd import device as D
from basecount_amd import synth
from basecount_amd.main import norm_factors
from ops_passes import CAP, W

pytestmark = pytest.mark.gpu

PASSES = OP.FORCED + (0,)  # forced, and the plan's own choice


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    c.timing(True)
    return c


@pytest.fixture(autouse=True)
def _defaults(ctx):
    yield
    ctx.set_shape("auto")
    ctx.set_ops_passes(0)


def test_the_switch_is_checked(ctx):
    for p in (0, 1, 2, CAP):
        ctx.set_ops_passes(p)
    for p in (-1, CAP + 1):
        assert D.lib().bc_ctx_set_ops_passes(ctx.h, p) == D.BC_E_ARG


def counts_under(ctx, b, L, mbq, k, shape, rpb=0, passes=0):
    ctx.set_shape(shape, 0, rpb)
    ctx.set_ops_passes(passes)
    r = D.DeviceReads(ctx, b)
    try:
        SB.launched(ctx)
        got, bad = SB.count_on(ctx, r, L, mbq, k)
        assert ("rc" if shape == "rc" else "count") in SB.launched(ctx)
        assert ctx.range_error() == -1  # the error word was cleared by its read
        return got, bad
    finally:
        r.free()


def check_passes(ctx, b, L, mbq=0, k=6, rpbs=OP.RPBS, passes=PASSES, rc=True):
    """bc_count of the sorted batch under "ops" for every (reads per block, passes): the oracle's
    first out-of-range read, counts bit-equal to the oracle's below L, to the single window's and
    to k_rc's."""
    cnt6, br = SB.expect(b, L, mbq)
    want = cnt6[:, :k].T.astype(np.int32)
    ctx.set_shape("ops")
    r = D.DeviceReads(ctx, b)
    try:
        assert r.r.sorted == 1
        for rpb in rpbs:
            ctx.set_shape("ops", 0, rpb)
            ctx.set_ops_passes(1)
            single, bad = SB.count_on(ctx, r, L, mbq, k)
            assert bad == br and np.array_equal(single, want), ("single", rpb)
            for p in passes:
                ctx.set_ops_passes(p)
                SB.launched(ctx)
                got, bad = SB.count_on(ctx, r, L, mbq, k)
                assert SB.launched(ctx) == {"count"}
                assert bad == br, (rpb, p)
                assert np.array_equal(got, want), (rpb, p, np.flatnonzero((got != want).any(0))[:8])
                assert np.array_equal(got, single)
    finally:
        r.free()
    if rc:
        got, bad = counts_under(ctx, b, L, mbq, k, "rc")
        assert bad == br and np.array_equal(got, want)


@pytest.mark.parametrize("name", OP.cases())
def test_case(ctx, name):
    b, L = OP.case(name)
    check_passes(ctx, b, L)


def test_early_end_leaves_the_plan_alone(ctx):
    """A forced cap of 8 on a batch whose reads all end in pass 1: equal counts, the same launch."""
    b, L = OP.case("early")
    check_passes(ctx, b, L, mbq=20, k=5, passes=(8,), rc=False)
    h = OP.header(b)
    for rpb in (0,) + OP.RPBS:
        assert D.ops_plan(h, L, rpb, 8)["blocks"] == D.ops_plan(h, L, rpb, 0)["blocks"]
        assert D.ops_plan(h, L, rpb, 8)["reads_per_block"] == D.ops_plan(h, L, rpb, 0)["reads_per_block"]


def test_cut_reports_the_smallest_read_and_counts_nothing_past_L(ctx):
    b, L = OP.case("cut")
    cnt6, br = SB.expect(b, L, 0)
    assert br == 6
    check_passes(ctx, b, L, mbq=20, k=5, rc=False)
    # nothing of the bad reads' events at or beyond L lands anywhere: a guard band after the
    # histogram's last column stays zero
    ctx.set_shape("ops", 0, 3)
    ctx.set_ops_passes(CAP)
    r = D.DeviceReads(ctx, b)
    hist = ctx.alloc(4 * (6 * L + 4 * W))
    hist.zero()
    ctx.count(r, L, 0, 6, hist.ptr)
    assert ctx.range_error() == 6
    got = hist.download(np.int32, 6 * L + 4 * W)
    assert np.array_equal(got[: 6 * L].reshape(6, L), cnt6.T.astype(np.int32)) and not got[6 * L:].any()
    hist.free()
    r.free()


@pytest.mark.parametrize("mbq, k", [(20, 6), (20, 5), (0, 5)])
def test_qualities_and_n_bases_at_window_ends(ctx, mbq, k):
    b, L = OP.case("nbases")
    cnt6, _ = SB.expect(b, L, mbq)
    assert cnt6[:, 5].sum() > 0 and (mbq == 0 or cnt6.sum() < SB.expect(b, L, 0)[0].sum())  # N counted; bases dropped
    check_passes(ctx, b, L, mbq=mbq, k=k, rc=(k == 6))
    b, L = OP.case("late")
    check_passes(ctx, b, L, mbq=mbq, k=k, rpbs=(3,), rc=False)


# --------------------------------------------------------------------------------------- depth
def deep_counts(d):
    b, one, L = OP.deep_batch(d)
    cnt, (br, _) = O.bcount(L, 0, one)
    assert br == -1 and int(cnt.max()) == 1
    return b, L, (cnt.astype(np.int64) * d)[:, :6].T.astype(np.int32)


def test_depth_300_identical_reads_in_one_block(ctx):
    b, L, want = deep_counts(300)
    for rpb, passes in ((32768, 0), (32768, 2), (32768, CAP), (64, 3)):
        got, bad = counts_under(ctx, b, L, 0, 6, "ops", rpb, passes)
        assert bad == -1 and np.array_equal(got, want), (rpb, passes)


def test_depth_40000_identical_reads_over_block_cuts(ctx):
    """More reads at one start than a workgroup may take: the run is cut, and a 16-bit half of the
    window reaches 32768 in every pass."""
    b, L, want = deep_counts(40_000)
    assert int(want.max()) == 40_000
    for rpb, passes in ((32768, 0), (0, 0), (32768, 1)):
        got, bad = counts_under(ctx, b, L, 0, 6, "ops", rpb, passes)
        assert bad == -1 and np.array_equal(got, want), (rpb, passes)
    assert D.ops_plan(OP.header(b), L, 40_000)["reads_per_block"] == 32768


# ------------------------------------------------------------------- long reads, every tail
@pytest.fixture(scope="module")
def ont_long():
    """Nanopore-like reads of ~9 kb on 40,000 positions (sorted), with qualities."""
    rs = synth.make_long_reads([("x", 40_000)], 60, seed=31, mean_len=9000, indel_every=14)
    b = synth.batch_arrays(rs, 0)
    assert D.ops_plan(OP.header(b), 40_000)["passes_max"] > 1
    return b


def test_ont_like_long_reads(ctx, ont_long):
    assert ont_long["cig_n"].min() > 64
    check_passes(ctx, ont_long, 40_000, mbq=20, k=6)
    check_passes(ctx, ont_long, 40_000, mbq=0, k=5, rpbs=(3,), rc=False)


def test_sorted_view_of_an_unsorted_batch(ctx, ont_long):
    """bc_reads_sort's fields-only view: sorted fields over the sequence where it lies (seq_nib + q
    indexing), counted over passes; the unsorted batch itself has no window and takes no passes."""
    L, k = 40_000, 6
    cnt6, br = SB.expect(ont_long, L, 0)
    assert br == -1
    bu = dict(SB.permuted(ont_long), qual=None)
    ctx.set_shape("ops")
    r = D.DeviceReads(ctx, bu)
    try:
        assert r.r.sorted == 0 and D.ops_plan(r, L, 0, 4) == D.ops_plan(r, L, 0, 1) and D.ops_plan(r, L)["window"] == 0
        ctx.set_ops_passes(1)
        plain, bad = SB.count_on(ctx, r, L, 0, k)
        ctx.set_ops_passes(4)
        forced, bad4 = SB.count_on(ctx, r, L, 0, k)
        assert bad == bad4 == -1 and np.array_equal(plain, forced) and np.array_equal(plain, cnt6.T.astype(np.int32))
        nb = ctx.sort_bytes(r)
        mem = ctx.alloc(nb)
        s = ctx.sort(r, mem.ptr, nb)
        assert s.sorted == 1 and s.seq == r.r.seq  # fields only: the sequence stays in place
        assert D.ops_plan(s, L)["passes_max"] > 1
        for rpb, passes in ((0, 0), (3, CAP), (64, 2)):
            ctx.set_shape("ops", 0, rpb)
            ctx.set_ops_passes(passes)
            out, bad = SB.pileup_on(ctx, s, L, 0, k)
            assert bad == -1
            SB.same(out, SB.expect_stats(cnt6, k), (rpb, passes))
        mem.free()
    finally:
        r.free()


def _summaries(ctx, b, L, mbq, k, tiles, passes):
    """bc_pileup_summary and bc_pileup_summary_amplicons under "ops" with the passes given."""
    nf, nf2 = norm_factors(k)
    ctx.set_shape("ops", 0, 3)
    ctx.set_ops_passes(passes)
    r = D.DeviceReads(ctx, b)
    bufs = [ctx.alloc(n) for n in (4 * k * L, 4 * L, 8 * L, 8 * L)]
    counts, cov, ent, sec = [x.ptr for x in bufs]
    work, dout = ctx.alloc(D.summary_work_bytes(L)), ctx.alloc(32)
    lo, hi = np.array([t[0] for t in tiles], np.int64), np.array([t[1] for t in tiles], np.int64)
    dlo, dhi, damp = ctx.alloc(lo.nbytes).upload(lo), ctx.alloc(hi.nbytes).upload(hi), ctx.alloc(48 * len(tiles))

    def outs():
        return (bufs[0].download(np.int32, k * L).tobytes(), bufs[1].download(np.int32, L).tobytes(),
                bufs[2].download(np.float64, L).tobytes(), bufs[3].download(np.float64, L).tobytes())

    try:
        ctx.pileup_summary(r, L, mbq, k, nf, nf2, counts, cov, None, ent, sec, work.ptr, dout.ptr)
        res = {"summary": (dout.download(np.float64, 4).tolist(), outs())}
        dout.zero()
        for x in bufs:
            x.zero()
        ctx.pileup_summary_amplicons(r, L, mbq, k, nf, nf2, counts, cov, ent, sec, work.ptr, dout.ptr, dlo.ptr,
                                     dhi.ptr, len(tiles), damp.ptr)
        res["amplicons"] = (dout.download(np.float64, 4).tolist(),
                            damp.download(np.float64, 6 * len(tiles)).reshape(-1, 6).tolist(), outs())
        assert ctx.range_error() == -1
        return res
    finally:
        for x in bufs + [work, dout, dlo, dhi, damp]:
            x.free()
        r.free()


def test_summary_and_amplicons(ctx, ont_long):
    L, mbq, k = 40_000, 20, 6
    tiles = [(30 + 4500 * i, 30 + 4500 * i + 4200) for i in range(8)]
    cnt6, _ = SB.expect(ont_long, L, mbq)
    ocov, _, oent, osec = O.stats(cnt6, True)
    c64 = ocov.astype(np.int64)
    want = [float(np.mean(c64)), float(np.mean(oent)), float(np.count_nonzero(ocov)), float(c64.sum())]
    want_outs = (cnt6.T.astype(np.int32).tobytes(), ocov.astype(np.int32).tobytes(), oent.tobytes(), osec.tobytes())
    got = _summaries(ctx, ont_long, L, mbq, k, tiles, CAP)
    assert got == _summaries(ctx, ont_long, L, mbq, k, tiles, 1)
    assert got["summary"] == (want, want_outs) and got["amplicons"][0] == want and got["amplicons"][2] == want_outs
    for i, e in enumerate(O.amplicons(ocov, oent, osec, tiles)):
        assert got["amplicons"][1][i] == [float(x) for x in e], tiles[i]


def test_segments_of_three_long_read_references(ctx):
    contigs = [("s0", 14_000), ("s1", 13_000), ("s2", 17_000)]
    rs = synth.make_long_reads(contigs, 45, seed=33, mean_len=6000, indel_every=12, skip_frac=0.0)
    k, mbq, n = 6, 20, len(contigs)
    lens = np.asarray(rs.lengths, np.int64)
    per = [synth.batch_arrays(rs, t) for t in range(n)]
    allb = dict(per[0], **{f: np.concatenate([p[f] for p in per]) for f in ("pos", "cig_beg", "cig_n", "seq_nib")})
    read_beg = np.concatenate([[0], np.cumsum([p["pos"].size for p in per])]).astype(np.int64)
    voff = D.segments_layout(lens)
    Lv = int(voff[-1])
    nf, nf2 = norm_factors(k)
    results = []
    for passes in (CAP, 0, 1):
        ctx.set_shape("ops", 0, 3)
        ctx.set_ops_passes(passes)
        reads = D.DeviceReads(ctx, allb)
        tab = ctx.alloc(8 * (3 * n + 2)).upload(np.concatenate([lens, read_beg, voff]))
        vpos = ctx.alloc(4 * int(read_beg[-1]))
        bufs = [ctx.alloc(x) for x in (4 * k * Lv, 4 * Lv, 8 * k * Lv, 8 * Lv, 8 * Lv, 32 * n)]
        t = tab.ptr
        try:
            ctx.pileup_segments(reads, n, t, t + 8 * n, t + 8 * (2 * n + 1), Lv, vpos.ptr, mbq, k, nf, nf2,
                                *[x.ptr for x in bufs])
            assert ctx.range_error() == -1
            results.append((bufs[0].download(np.int32, k * Lv).reshape(k, Lv), bufs[1].download(np.int32, Lv),
                            bufs[3].download(np.float64, Lv), bufs[4].download(np.float64, Lv),
                            bufs[5].download(np.float64, 4 * n).reshape(n, 4)))
        finally:
            for x in bufs + [tab, vpos]:
                x.free()
            reads.free()
    for other in results[1:]:
        for a, c in zip(results[0], other):
            assert np.array_equal(a, c)
    cnt, cov, ent, sec, sums = results[0]
    for i, (_, L) in enumerate(contigs):
        sl = slice(int(voff[i]), int(voff[i]) + L)
        oc, (br, _) = O.bcount(L, mbq, per[i])
        assert br == -1 and SB.spans(per[i]).max() > W
        ocov, _, oent, osec = O.stats(oc, True)
        assert np.array_equal(cnt[:, sl], oc.T.astype(np.int32)), i
        assert np.array_equal(cov[sl], ocov) and np.array_equal(ent[sl], oent) and np.array_equal(sec[sl], osec), i
        assert sums[i, 2] == np.count_nonzero(ocov) and sums[i, 3] == int(ocov.astype(np.int64).sum()), i


def test_captured_once_replayed_twice(ctx, ont_long):
    """The window starts clean in every pass and every replay: the outputs are re-zeroed between the
    replays and each equals the oracle."""
    L, k, mbq = 40_000, 6, 20
    cnt6, _ = SB.expect(ont_long, L, mbq)
    exp = SB.expect_stats(cnt6, k)
    nf, nf2 = norm_factors(k)
    ctx.set_shape("ops", 0, 3)
    ctx.set_ops_passes(CAP)
    r = D.DeviceReads(ctx, ont_long)
    bufs = [ctx.alloc(n) for n in (4 * k * L, 4 * L, 8 * k * L, 8 * L, 8 * L)]

    def step():
        ctx.pileup(r, L, mbq, k, nf, nf2, *[x.ptr for x in bufs])

    step()  # (the accumulation scratch grows here, outside the capture)
    g = ctx.capture(step)  # a synchronisation or an allocation inside would fail the capture
    for _ in range(2):
        for x in bufs:
            x.zero()
        g.launch()
        got = (bufs[0].download(np.int32, k * L).reshape(k, L), bufs[1].download(np.int32, L),
               bufs[2].download(np.float64, k * L).reshape(k, L), bufs[3].download(np.float64, L),
               bufs[4].download(np.float64, L))
        SB.same(got, exp, "replay")
    assert ctx.range_error() == -1
    for x in bufs:
        x.free()
    r.free()
