"""The long-read kernel shape ``set_shape("ops")`` (k_ops, bc_ops.hip; DESIGN.md §3 "k_ops").

k_ops expands a read's CIGAR with wave scans, 64 ops and 64 reference positions at a time, into a
4096-position LDS window per block and global atomics past it.  Everything here runs under the
shape and is compared bit for bit with the oracle (saturation_batches.expect / expect_stats): the
scan's 64-op and 64-event boundaries, the window's edges, range errors on both sides of the
window, counter depth over block cuts, unsorted batches, every tail that follows kernel 1, graph
capture, and the CLI on the reference-made ``ont`` goldens."""
import contextlib
import gzip
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import saturation_batches as SB
from basecount_amd import device as D
from basecount_amd import main as M
from basecount_amd import synth
from basecount_amd.main import norm_factors
from saturation_batches import DEL, EQOP, H, I, M as MM, P, S, SKIP, X

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONT = os.path.join(REPO, "tests", "golden", "ont")
WIN = SB.K_WIN_MAX  # one block's LDS window


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    c.timing(True)
    return c


@pytest.fixture(autouse=True)
def _auto_shape(ctx):
    yield
    ctx.set_shape("auto")


def ont_batch(L=6000, n=300, seed=21, **kw):
    """One contig of make_long_reads as a bc_reads-layout batch (sorted)."""
    rs = synth.make_long_reads([("x", L)], n, seed=seed, **kw)
    return synth.batch_arrays(rs, 0)


@pytest.fixture(scope="module")
def ont():
    return ont_batch(mean_len=500, indel_every=12)


def check_ops(ctx, b, L, mbqs=(0, 20), ks=(5, 6), rpb=0, twice=False):
    """bc_count (accumulating) and bc_pileup of the sorted batch under "ops": the kernels that ran,
    the oracle's first out-of-range read, every output bit-equal to the oracle's below L."""
    ctx.set_shape("ops", 0, rpb)
    r = D.DeviceReads(ctx, b)
    try:
        assert r.r.sorted == 1
        assert not r.r.read_runs and not r.r.tile_reads  # BC_INDEX_AUTO builds nothing for the shape
        for mbq in mbqs:
            cnt6, br = SB.expect(b, L, mbq)
            for k in ks:
                what = (mbq, k, rpb)
                want = cnt6[:, :k].T.astype(np.int32)
                SB.launched(ctx)
                got, bad = SB.count_on(ctx, r, L, mbq, k)
                assert SB.launched(ctx) == {"count"}, what
                assert bad == br, what
                assert np.array_equal(got, want), what
                if twice:  # accumulates: two calls give twice the counts
                    hist = ctx.alloc(max(16, 4 * k * L))
                    hist.zero()
                    ctx.count(r, L, mbq, k, hist.ptr)
                    ctx.count(r, L, mbq, k, hist.ptr)
                    assert ctx.range_error() == br
                    assert np.array_equal(hist.download(np.int32, k * L).reshape(k, L), 2 * want), what
                    hist.free()
                    SB.launched(ctx)
                got, bad = SB.pileup_on(ctx, r, L, mbq, k)
                assert SB.launched(ctx) == {"count", "stats"}, what
                assert bad == br, what
                SB.same(got, SB.expect_stats(cnt6, k), what)
                assert ctx.range_error() == -1  # the error word was cleared by the read above
    finally:
        r.free()
        ctx.set_shape("auto")


# ------------------------------------------------------------------------------------ parity
def test_set_shape_ops_is_accepted(ctx):
    ctx.set_shape("ops")
    assert ctx.shape_args == ("ops", 0, 0)
    assert D.lib().bc_ctx_set_shape(ctx.h, 5, 0, 0) == D.BC_E_ARG
    ctx.set_shape("auto")


def test_parity_ont_like(ctx, ont):
    n_ops = ont["cig_n"]
    assert n_ops.min() > 8 and (n_ops > 64).any()
    check_ops(ctx, ont, 6000, twice=True)
    check_ops(ctx, ont, 6000, mbqs=(20,), ks=(6,), rpb=7)  # many small blocks


# --------------------------------------------------------------------------- scan boundaries
def alternating(n_ops, first=MM):
    """n_ops ops: M runs of 2-4 separated by 1I / 1D in turn."""
    ops = []
    for j in range(n_ops):
        if j % 2 == 0:
            ops.append((first if j == 0 else (MM, EQOP, X)[j // 2 % 3], 2 + j % 3))
        else:
            ops.append(((I, DEL)[j // 2 % 2], 1 + j % 2))
    return ops


SCAN_READS = {f"ops{n}": alternating(n) for n in (63, 64, 65, 127, 128, 129)}
SCAN_READS.update({
    "m200": [(MM, 200)],
    "m200_in_many": alternating(70) + [(MM, 200)] + alternating(70),
    # an op batch with no reference event: 64 / 70 query-only or empty ops between two M
    "quiet64": [(MM, 5)] + [((I, P, S, H)[j % 4], 1 + j % 3) for j in range(64)] + [(MM, 7)],
    "quiet70": [(S, 3), (MM, 5)] + [((I, P, H)[j % 3], 1 + j % 2) for j in range(70)] + [(MM, 7)],
    "quiet_aligned": alternating(64) + [((I, P)[j % 2], 2) for j in range(64)] + alternating(5),
    "zero_len": [(MM, 4), (DEL, 0), (MM, 0), (I, 0), (SKIP, 0), (MM, 4), (MM, 0)] + alternating(66) + [(DEL, 0)],
    "ins_del": [(MM, 6), (I, 2), (DEL, 3), (MM, 6), (DEL, 2), (I, 3), (MM, 6)] + alternating(9),
    "del300": [(MM, 10), (DEL, 300), (MM, 10)] + alternating(12),
    "skip5000": alternating(11) + [(SKIP, 5000), (MM, 9)],
    "lead_ins": [(I, 4), (MM, 20)] + alternating(10),
    "lead_clip_ins": [(H, 2), (S, 3), (I, 4), (MM, 20)] + alternating(10),
    "del_only": [(DEL, 70)],
    "no_ref": [(S, 2), (I, 10), (P, 1), (S, 1)],
    "no_cigar": [],
})


@pytest.fixture(scope="module")
def scan_batch():
    rng = np.random.default_rng(77)
    reads = []
    for rep in range(3):
        for i, (name, ops) in enumerate(SCAN_READS.items()):
            reads.append(SB.random_read(rng, (131 * i + 517 * rep) % 2500, ops))
    reads.append(SB.random_read(rng, 9000, [(MM, 8)]))  # (the read without a CIGAR is not the last)
    return SB.pack_batch(reads)


def test_scan_boundaries(ctx, scan_batch):
    for name, ops in SCAN_READS.items():
        if name.startswith("ops"):
            assert len(ops) == int(name[3:])
    L = SB.max_end(scan_batch) + 3
    check_ops(ctx, scan_batch, L)
    check_ops(ctx, scan_batch, L, mbqs=(20,), ks=(6,), rpb=1)  # every read its own block and window


# ------------------------------------------------------------------------------- window edges
@pytest.fixture(scope="module")
def edge_batch():
    """One block (reads_per_block 32768): its window is [100, 100 + 4096).  Reads start at window
    offsets 4000-4095 with spans 50-600: part of each in LDS, part in the overhang."""
    rng = np.random.default_rng(78)
    reads = [SB.random_read(rng, 100, alternating(21))]
    for j in range(96):
        span = 50 + (j * 37) % 551
        ops = alternating(9 + j % 40)
        ops.append((MM, max(1, span - SB.ref_span(ops))))
        reads.append(SB.random_read(rng, 100 + 4000 + j, ops))
    reads += [SB.random_read(rng, 100 + WIN - 1, [(MM, 2)]), SB.random_read(rng, 100 + WIN, alternating(15))]
    return SB.pack_batch(reads)


@pytest.mark.parametrize("pad", [0, 1, 64])
def test_window_edge_reads(ctx, edge_batch, pad):
    end = SB.max_end(edge_batch)
    assert end > 100 + WIN + 400
    L = end + pad if pad < 64 else (end + 63) // 64 * 64  # the last read ends at L; L % 64 != 0; == 0
    assert (L % 64 == 0) == (pad == 64)
    check_ops(ctx, edge_batch, L, rpb=32768)
    check_ops(ctx, edge_batch, L, mbqs=(0,), ks=(6,))


def test_span_65536_and_the_long_catalogue(ctx):
    b = SB.catalogue_batch("long", "embedded", 70_000)
    assert int(SB.spans(b).max()) == 65536
    check_ops(ctx, b, 70_000, ks=(6,))
    check_ops(ctx, b, 70_000, mbqs=(20,), ks=(5,), rpb=32768)


@pytest.mark.parametrize("L", [1000, 999, 65, 1])
def test_reference_shorter_than_the_window(ctx, L):
    rng = np.random.default_rng(79 + L)
    reads = []
    for j in range(60):
        ops = alternating(9 + j % 30)
        span = SB.ref_span(ops)
        if span <= L:
            reads.append(SB.random_read(rng, int(rng.integers(0, L - span + 1)), ops))
    reads.append(SB.random_read(rng, L - 1, [(MM, 1)]))
    check_ops(ctx, SB.pack_batch(reads), L, rpb=32768)


# -------------------------------------------------------------------------------- range errors
@pytest.mark.parametrize("where", ["window", "overhang"])
def test_range_errors(ctx, edge_batch, where):
    """Reads overhanging L inside the block's window and past it: the oracle's first bad read,
    exact counts below L, and the error word cleared by its read."""
    L = 100 + 4050 if where == "window" else 100 + WIN + 300
    cnt6, br = SB.expect(edge_batch, L, 0)
    assert br > 0 and SB.max_end(edge_batch) > L
    check_ops(ctx, edge_batch, L, rpb=32768)
    check_ops(ctx, edge_batch, L, mbqs=(0,), ks=(5,), rpb=16)


def test_range_error_unsorted_smallest_index(ctx, edge_batch):
    L = 100 + WIN + 300
    bu = SB.permuted(edge_batch)
    cnt6, br = SB.expect(bu, L, 0)
    ctx.set_shape("ops")
    r = D.DeviceReads(ctx, bu)
    assert r.r.sorted == 0
    got, bad = SB.count_on(ctx, r, L, 0, 6)
    assert bad == br and br >= 0
    assert np.array_equal(got, cnt6.T.astype(np.int32))
    assert ctx.range_error() == -1
    r.free()


# --------------------------------------------------------------------------------------- depth
@pytest.mark.parametrize("d", [1023, 1025, 2047])
def test_depth_complex_blocks(ctx, d):
    b = SB.hot_complex_batch(d)
    want = SB.complex_closed_form(d)
    ctx.set_shape("ops")
    r = D.DeviceReads(ctx, b)
    for k in (5, 6):
        got, bad = SB.count_on(ctx, r, SB.COMPLEX_L, 1, k)
        assert bad == -1
        assert np.array_equal(got, want[:, :k].T.astype(np.int32)), (d, k)
    r.free()


def test_depth_40000_identical_reads_over_block_cuts(ctx):
    """40,000 identical 9-op reads at one start (and 40,000 more at another): more than the 32768
    reads one block may take, so the run is cut, and a 16-bit half of the window reaches 32768."""
    d = 40_000
    b = SB.hot_complex_batch(d)
    want = SB.complex_closed_form(d)[:, :6].T.astype(np.int32)
    for rpb in (32768, 0):
        ctx.set_shape("ops", 0, rpb)
        r = D.DeviceReads(ctx, b)
        got, bad = SB.count_on(ctx, r, SB.COMPLEX_L, 0, 6)
        assert bad == -1
        assert np.array_equal(got, want), rpb
        r.free()


# ------------------------------------------------------------------------------------ unsorted
@pytest.mark.parametrize("with_qual", [False, True])
def test_unsorted(ctx, ont, with_qual):
    """The ONT-like reads shuffled: bc_count directly (k_ops on global atomics), and bc_reads_sort
    then bc_pileup (the fields-only view without qualities, the copied view with them)."""
    L, k = 6000, 6
    mbq = 20 if with_qual else 0
    cnt6, br = SB.expect(ont, L, mbq)
    assert br == -1
    bu = SB.permuted(ont)
    if not with_qual:
        bu = dict(bu, qual=None)
    ctx.set_shape("ops")
    r = D.DeviceReads(ctx, bu)
    try:
        assert r.r.sorted == 0
        SB.launched(ctx)
        got, bad = SB.count_on(ctx, r, L, mbq, k)
        assert SB.launched(ctx) == {"count"} and bad == -1
        assert np.array_equal(got, cnt6.T.astype(np.int32))
        nb = ctx.sort_bytes(r)
        mem = ctx.alloc(nb)
        s = ctx.sort(r, mem.ptr, nb)
        assert s.sorted == 1 and s.n_reads == r.r.n_reads
        assert (s.seq == r.r.seq) == (not with_qual)  # fields-only view: the sequence stays in place
        SB.launched(ctx)
        out, bad = SB.pileup_on(ctx, s, L, mbq, k)
        assert SB.launched(ctx) == {"count", "stats"} and bad == -1
        SB.same(out, SB.expect_stats(cnt6, k), with_qual)
        mem.free()
    finally:
        r.free()


# ---------------------------------------------------------------------------------- every tail
def _tails(ctx, shape, b, L, mbq, k, tiles):
    """Every entry point that runs kernel 1 + a tail, under ``shape``: downloaded results."""
    nf, nf2 = norm_factors(k)
    ctx.set_shape(shape)
    r = D.DeviceReads(ctx, b)
    bufs = [ctx.alloc(n) for n in (4 * k * L, 4 * L, 8 * L, 8 * L)]
    counts, cov, ent, sec = [x.ptr for x in bufs]
    work, dout = ctx.alloc(D.summary_work_bytes(L)), ctx.alloc(32)
    lo = np.array([t[0] for t in tiles], np.int64)
    hi = np.array([t[1] for t in tiles], np.int64)
    dlo, dhi, damp = ctx.alloc(lo.nbytes).upload(lo), ctx.alloc(hi.nbytes).upload(hi), ctx.alloc(48 * len(tiles))
    res = {}

    def outs():
        return (bufs[0].download(np.int32, k * L).tobytes(), bufs[1].download(np.int32, L).tobytes(),
                bufs[2].download(np.float64, L).tobytes(), bufs[3].download(np.float64, L).tobytes())

    try:
        ctx.pileup_summary(r, L, mbq, k, nf, nf2, counts, cov, None, ent, sec, work.ptr, dout.ptr)
        res["summary"] = (dout.download(np.float64, 4).tolist(), outs())
        dout.zero()
        ctx.pileup_summary(r, L, mbq, k, nf, nf2, None, None, None, None, None, work.ptr, dout.ptr)
        res["summary_only"] = dout.download(np.float64, 4).tolist()
        dout.zero()
        for x in bufs:
            x.zero()
        ctx.pileup_partials(r, L, mbq, k, nf, nf2, counts, cov, None, ent, sec, work.ptr)
        ctx.summary_fold([L], [work.ptr], [dout.ptr])
        res["partials"] = (dout.download(np.float64, 4).tolist(), outs())
        dout.zero()
        ctx.pileup_partials(r, L, mbq, k, nf, nf2, None, None, None, None, None, work.ptr)
        ctx.summary_fold([L], [work.ptr], [dout.ptr])
        res["partials_only"] = dout.download(np.float64, 4).tolist()
        dout.zero()
        for x in bufs:
            x.zero()
        ctx.pileup_summary_amplicons(r, L, mbq, k, nf, nf2, counts, cov, ent, sec, work.ptr, dout.ptr, dlo.ptr,
                                     dhi.ptr, len(tiles), damp.ptr)
        res["amplicons"] = (dout.download(np.float64, 4).tolist(),
                            damp.download(np.float64, 6 * len(tiles)).reshape(-1, 6).tolist(), outs())
        assert ctx.range_error() == -1
    finally:
        for x in bufs + [work, dout, dlo, dhi, damp]:
            x.free()
        r.free()
        ctx.set_shape("auto")
    return res


@pytest.mark.parametrize("mbq, k", [(0, 5), (20, 6)])
def test_every_tail_equals_rc_and_oracle(ctx, mbq, k):
    L = 8192 + 700
    b = ont_batch(L, 300, seed=23, mean_len=600, indel_every=14)
    tiles = [(30 + 1100 * i, 30 + 1100 * i + 420) for i in range(8)]
    cnt6, br = SB.expect(b, L, mbq)
    assert br == -1
    ocov, _, oent, osec = O.stats(cnt6, k == 6)
    c64 = ocov.astype(np.int64)
    want = [float(np.mean(c64)), float(np.mean(oent)), float(np.count_nonzero(ocov)), float(c64.sum())]
    want_outs = (cnt6[:, :k].T.astype(np.int32).tobytes(), ocov.astype(np.int32).tobytes(), oent.tobytes(),
                 osec.tobytes())
    SB.launched(ctx)
    got = _tails(ctx, "ops", b, L, mbq, k, tiles)
    ran = SB.launched(ctx)
    assert "count" in ran and "rc" not in ran and not ran & {"pileup", "solo"}
    rc = _tails(ctx, "rc", b, L, mbq, k, tiles)
    assert "rc" in SB.launched(ctx)
    assert got == rc  # every number and every output array, bit for bit
    for name in ("summary", "partials"):
        assert got[name][0] == want and got[name][1] == want_outs, name
    assert got["summary_only"] == want and got["partials_only"] == want
    assert got["amplicons"][0] == want and got["amplicons"][2] == want_outs
    for i, e in enumerate(O.amplicons(ocov, oent, osec, tiles)):
        assert got["amplicons"][1][i] == [float(x) for x in e], tiles[i]


def _segments(ctx, shape, rs, k, mbq):
    n = len(rs.lengths)
    lens = np.asarray(rs.lengths, np.int64)
    per = [synth.batch_arrays(rs, t) for t in range(n)]
    allb = dict(per[0], **{f: np.concatenate([p[f] for p in per]) for f in ("pos", "cig_beg", "cig_n", "seq_nib")})
    read_beg = np.concatenate([[0], np.cumsum([p["pos"].size for p in per])]).astype(np.int64)
    voff = D.segments_layout(lens)
    Lv = int(voff[-1])
    ctx.set_shape(shape)
    reads = D.DeviceReads(ctx, allb)
    tab = ctx.alloc(8 * (3 * n + 2)).upload(np.concatenate([lens, read_beg, voff]))
    vpos = ctx.alloc(4 * int(read_beg[-1]))
    bufs = [ctx.alloc(x) for x in (4 * k * Lv, 4 * Lv, 8 * k * Lv, 8 * Lv, 8 * Lv, 32 * n)]
    nf, nf2 = norm_factors(k)
    t = tab.ptr
    try:
        ctx.pileup_segments(reads, n, t, t + 8 * n, t + 8 * (2 * n + 1), Lv, vpos.ptr, mbq, k, nf, nf2,
                            *[x.ptr for x in bufs])
        assert ctx.range_error() == -1
        return (bufs[0].download(np.int32, k * Lv).reshape(k, Lv), bufs[1].download(np.int32, Lv),
                bufs[2].download(np.float64, k * Lv).reshape(k, Lv), bufs[3].download(np.float64, Lv),
                bufs[4].download(np.float64, Lv), bufs[5].download(np.float64, 4 * n).reshape(n, 4)), voff, per
    finally:
        for x in bufs + [tab, vpos]:
            x.free()
        reads.free()
        ctx.set_shape("auto")


def test_segments_of_ont_like_references(ctx):
    contigs = [("s0", 700), ("s1", 1500), ("s2", 320), ("s3", 2049), ("s4", 900)]
    rs = synth.make_long_reads(contigs, 40, seed=29, mean_len=90, indel_every=5, skip_frac=0.0)
    k, mbq = 6, 20
    SB.launched(ctx)
    got, voff, per = _segments(ctx, "ops", rs, k, mbq)
    assert SB.launched(ctx) == {"count", "stats", "summary"}
    rc, _, _ = _segments(ctx, "rc", rs, k, mbq)
    for a, b in zip(got, rc):
        assert np.array_equal(a, b)
    cnt, cov, pc, ent, sec, sums = got
    for i, (_, L) in enumerate(contigs):
        sl = slice(int(voff[i]), int(voff[i]) + L)
        oc, (br, _) = O.bcount(L, mbq, per[i])
        assert br == -1
        ocov, opc, oent, osec = O.stats(oc, True)
        assert np.array_equal(cnt[:, sl], oc.T.astype(np.int32)), i
        assert np.array_equal(cov[sl], ocov) and np.array_equal(pc[:, sl], opc), i
        assert np.array_equal(ent[sl], oent) and np.array_equal(sec[sl], osec), i
        assert sums[i, 0] == np.mean(ocov.tolist()) and sums[i, 1] == np.mean(oent.tolist()), i
        assert sums[i, 2] == np.count_nonzero(ocov) and sums[i, 3] == int(ocov.astype(np.int64).sum()), i


# --------------------------------------------------------------------------------------- graph
def test_pileup_is_capturable(ctx, ont):
    L, k, mbq = 6000, 6, 20
    cnt6, _ = SB.expect(ont, L, mbq)
    exp = SB.expect_stats(cnt6, k)
    nf, nf2 = norm_factors(k)
    ctx.set_shape("ops")
    r = D.DeviceReads(ctx, ont)
    bufs = [ctx.alloc(n) for n in (4 * k * L, 4 * L, 8 * k * L, 8 * L, 8 * L)]

    def step():
        ctx.pileup(r, L, mbq, k, nf, nf2, *[x.ptr for x in bufs])

    step()  # (the accumulation scratch grows here, outside the capture)
    g = ctx.capture(step)  # a synchronisation or an allocation inside would fail the capture
    for _ in range(3):
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


# ----------------------------------------------------------------------------------- CLI / API
def _run_cli(argv):
    buf = io.BytesIO()
    txt = io.TextIOWrapper(buf, encoding="utf-8", write_through=True)
    with contextlib.redirect_stdout(txt):
        M.run(argv)
        txt.flush()
    return buf.getvalue()


def _ont_manifest():
    with open(os.path.join(ONT, "manifest.json")) as fh:
        return json.load(fh)


def _golden(c):
    with open(os.path.join(ONT, c["stdout"]), "rb") as fh:
        return gzip.decompress(fh.read())


@pytest.mark.parametrize("setting", ["default", "routed", "off", "batches"])
def test_cli_ont_goldens(monkeypatch, setting):
    """Every ont case byte-identical to the reference's output: default routing (the rule routes
    both references), BASECOUNT_LONG_READS=1, routing off, and the accumulate path (50-record
    batches, each routed by the rule on its own reads)."""
    monkeypatch.chdir(ONT)
    monkeypatch.delenv("BASECOUNT_LONG_READS", raising=False)
    monkeypatch.delenv("BASECOUNT_BATCH_RECORDS", raising=False)
    if setting == "off":
        monkeypatch.setenv("BASECOUNT_LONG_READS", "0")
    if setting == "routed":
        monkeypatch.setenv("BASECOUNT_LONG_READS", "1")
    if setting == "batches":
        monkeypatch.setenv("BASECOUNT_BATCH_RECORDS", "50")
    for name, c in sorted(_ont_manifest().items()):
        # in this process the two references come in this interpreter's set order (main.py:92):
        # header and each reference's block byte for byte (the subprocess test below: whole output)
        summ = "--summarise" in c["args"] or "--summarise-with-bed" in c["args"]
        got = O.split_blocks(_run_cli([c["bam"]] + c["args"]).decode(), summ)
        assert got == O.split_blocks(_golden(c).decode(), summ), (setting, name)
        assert set(got[1]) == {"ontA", "ontB"}
        routed = sorted(M.PLAN["ops"])
        if setting == "off":
            assert routed == []
        else:
            assert routed == ["ontA", "ontB"], (setting, name)


def test_cli_subprocess_and_short_reads_not_routed(monkeypatch):
    """`python -m basecount_amd` itself with every reference routed, and c1.bam never routed by the
    rule."""
    c = _ont_manifest()["ont_shown_long"]
    env = dict(os.environ, PYTHONPATH=REPO, BASECOUNT_LONG_READS="1", PYTHONHASHSEED="0")
    p = subprocess.run([sys.executable, "-m", "basecount_amd", c["bam"]] + c["args"], cwd=ONT, env=env,
                       capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout == _golden(c)
    monkeypatch.delenv("BASECOUNT_LONG_READS", raising=False)
    monkeypatch.setattr(M, "OPS_RULE_DEFAULT", True)  # the rule itself, whatever the shipped default
    _run_cli([os.path.join(REPO, "tests", "golden", "c1.bam"), "--summarise"])
    assert M.PLAN["ops"] == [] and M.PLAN["single"] == ["ref"]
    _run_cli([os.path.join(ONT, "ont.bam"), "--summarise"])
    assert sorted(M.PLAN["ops"]) == ["ontA", "ontB"]
