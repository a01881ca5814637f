"""Grouped references on the GPU: many small references counted as one virtual reference
(bc_pileup_segments) must give, per reference, exactly what the per-reference path gives -- in the
library (against bc_pileup / bc_summary on each reference alone and against the oracle) and through
the CLI (against the run with BASECOUNT_GROUP_REFS=0 and the oracle's text)."""
import contextlib
import io

import numpy as np
import pytest

import oracle as O
from basecount_amd import device as D
from basecount_amd import main as M
from basecount_amd import synth
from basecount_amd.main import norm_factors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return D.Context(0)


@pytest.fixture(autouse=True)
def _auto_shape(request):
    yield
    if "ctx" in request.fixturenames:
        request.getfixturevalue("ctx").set_shape("auto")


# ------------------------------------------------------------------ the library on one group
SEG_LENS = [1, 2, 63, 64, 65, 127, 128, 129, 150, 151, 8191, 8192, 8193, 20000] * 3
SEG_EMPTY = {0, 7, 20, 21, 41}  # first, last, single and adjacent ones between


def _segment_reads(rng, L, n):
    """Reads of 1-150 bp inside [0, L): mixed CIGARs, some non-ACGT letters, plus the edge reads:
    one starting at 0, one ending exactly at L, one whose deletion runs to the last position."""
    reads = []

    def add(pos, ops):
        q = sum(ln for op, ln in ops if op in (0, 1, 4, 7, 8))
        codes = synth.ACGT[rng.integers(0, 4, q)]
        codes[rng.random(q) < 0.05] = rng.choice([15, 0, 5])
        reads.append((int(pos), ops, codes, rng.integers(0, 45, q).astype(np.uint8)))

    top = min(L, 150)
    for _ in range(n):
        if top >= 16 and rng.random() < 0.7:
            m1 = int(rng.integers(1, top // 2))
            kind, bl = int(rng.choice([0, 1, 2, 3, 7, 8])), int(rng.integers(1, 4))
            m2 = int(rng.integers(1, top - m1 - 3))
            ops = [(0, m1), (kind, bl), (0, m2)]
            if rng.random() < 0.4:
                ops.insert(0, (4, int(rng.integers(1, 6))))
            if rng.random() < 0.4:
                ops.append((4, int(rng.integers(1, 6))))
        else:
            ops = [(0, int(rng.integers(1, top + 1)))]
        span = sum(ln for op, ln in ops if op in (0, 2, 3, 7, 8))
        add(rng.integers(0, L - span + 1), ops)
    m = int(rng.integers(1, top + 1))
    add(0, [(0, m)])
    add(L - m, [(0, m)])
    if L >= 2:
        d = int(rng.integers(1, min(L - 1, 5) + 1))
        m = int(rng.integers(1, min(L - d, 100) + 1))
        add(L - d - m, [(0, m), (2, d)])
    return reads


def _batch(reads):
    """bc_reads-layout host arrays of (pos, ops, codes, quals) reads, in the given order."""
    nib = np.zeros(len(reads) + 1, np.int64)
    nib[1:] = np.cumsum([len(r[2]) + (len(r[2]) & 1) for r in reads])
    allc = np.zeros(int(nib[-1]) + 2, np.uint8)
    qual = np.zeros(int(nib[-1]) + 2, np.uint8)
    for i, (_, _, s, q) in enumerate(reads):
        allc[nib[i]: nib[i] + len(s)] = s
        qual[nib[i]: nib[i] + len(q)] = q
    cig_n = np.array([len(r[1]) for r in reads], np.uint32)
    cig_beg = np.zeros(len(reads), np.uint32)
    if len(reads):
        cig_beg[1:] = np.cumsum(cig_n)[:-1]
    qstart = np.array([r[1][0][1] if r[1][0][0] == 4 else 0 for r in reads], np.int64)
    return dict(pos=np.array([r[0] for r in reads], np.int32), cig_beg=cig_beg, cig_n=cig_n,
                seq_nib=(nib[:-1] + qstart).astype(np.uint32),
                cigar=np.array([(ln << 4) | op for r in reads for op, ln in r[1]], np.uint32),
                seq=((allc[0::2] << 4) | allc[1::2]).astype(np.uint8), qual=qual)


@pytest.fixture(scope="module")
def group():
    rng = np.random.default_rng(20260)
    segs = []
    for i, L in enumerate(SEG_LENS):
        rd = [] if i in SEG_EMPTY else _segment_reads(rng, L, 3 if L < 64 else 40)
        rd.sort(key=lambda r: r[0])
        segs.append(rd)
    read_beg = np.zeros(len(segs) + 1, np.int64)
    read_beg[1:] = np.cumsum([len(s) for s in segs])
    assert read_beg[-1] <= 20_000
    return dict(lens=np.array(SEG_LENS, np.int64), segs=segs, read_beg=read_beg,
                all=_batch([r for s in segs for r in s]), per=[_batch(s) if s else None for s in segs])


_EXPECT: dict = {}


def _expected(ctx, group, k, mbq):
    """Per segment, computed once per (k, mbq) with the automatic shape and never changed: bc_pileup
    on that reference alone and bc_summary on its outputs, the oracle's counts and statistics."""
    key = (k, mbq)
    if key in _EXPECT:
        return _EXPECT[key]
    ctx.set_shape("auto")
    nf, nf2 = norm_factors(k)
    out = []
    for L, b in zip(group["lens"].tolist(), group["per"]):
        bufs = [ctx.alloc(max(8, n)) for n in (4 * k * L, 4 * L, 8 * k * L, 8 * L, 8 * L)]
        if b is None:
            r = M._no_reads()
            ctx.pileup(r, L, mbq, k, nf, nf2, *[x.ptr for x in bufs])
            oc = np.zeros((L, 6), np.uint32)
        else:
            dr = D.DeviceReads(ctx, b)
            assert dr.r.sorted == 1
            ctx.pileup(dr, L, mbq, k, nf, nf2, *[x.ptr for x in bufs])
            oc, (br, _) = O.bcount(L, mbq, b)
            assert br == -1
        assert ctx.range_error() == -1
        work, dsum = ctx.alloc(D.summary_work_bytes(L)), ctx.alloc(32)
        ctx.summary(bufs[1].ptr, bufs[3].ptr, L, work.ptr, dsum.ptr)
        dev = (bufs[0].download(np.int32, k * L).reshape(k, L), bufs[1].download(np.int32, L),
               bufs[2].download(np.float64, k * L).reshape(k, L), bufs[3].download(np.float64, L),
               bufs[4].download(np.float64, L), dsum.download(np.float64, 4))
        if b is not None:
            dr.free()
        out.append((dev, oc, O.stats(oc, k == 6)))
    _EXPECT[key] = out
    return out


class _GroupOnDevice:
    """The group uploaded once: reads with their own starts, the segment table, outputs at virtual
    size."""

    def __init__(self, ctx, group, k):
        self.ctx, self.k = ctx, k
        self.lens = group["lens"]
        self.n = int(self.lens.size)
        self.voff = D.segments_layout(self.lens)
        self.Lv = Lv = int(self.voff[-1])
        self.reads = D.DeviceReads(ctx, group["all"]) if group["all"] is not None else M._no_reads()
        table = np.concatenate([self.lens, group["read_beg"], self.voff])
        self.tab = ctx.alloc(table.nbytes).upload(table)
        self.vpos = ctx.alloc(max(4, 4 * int(group["read_beg"][-1])))
        self.bufs = [ctx.alloc(n) for n in (4 * k * Lv, 4 * Lv, 8 * k * Lv, 8 * Lv, 8 * Lv)]
        self.sum = ctx.alloc(32 * self.n)

    def run(self, mbq, want_pc=True, want_sum=True):
        nf, nf2 = norm_factors(self.k)
        b, t, n = self.bufs, self.tab.ptr, self.n
        self.ctx.pileup_segments(self.reads, n, t, t + 8 * n, t + 8 * (2 * n + 1), self.Lv, self.vpos.ptr, mbq,
                                 self.k, nf, nf2, b[0].ptr, b[1].ptr, b[2].ptr if want_pc else None, b[3].ptr,
                                 b[4].ptr, self.sum.ptr if want_sum else None)

    def poison(self):
        for x in self.bufs + [self.sum]:
            check = D.lib().bc_memset(self.ctx.h, x.ptr, 0x5A, x.nbytes)
            assert check == 0

    def download(self):
        k, Lv = self.k, self.Lv
        b = self.bufs
        return (b[0].download(np.int32, k * Lv).reshape(k, Lv), b[1].download(np.int32, Lv),
                b[2].download(np.float64, k * Lv).reshape(k, Lv), b[3].download(np.float64, Lv),
                b[4].download(np.float64, Lv), self.sum.download(np.float64, 4 * self.n).reshape(self.n, 4))


@pytest.mark.parametrize("shape", ["auto", "tile", "tile_no_solo", "rc"])
@pytest.mark.parametrize("k,mbq", [(5, 0), (5, 20), (6, 0), (6, 20)])
def test_segments_match_each_reference_alone_and_the_oracle(ctx, group, k, mbq, shape):
    exp = _expected(ctx, group, k, mbq)
    g = _GroupOnDevice(ctx, group, k)
    ctx.set_shape(shape)
    g.poison()
    g.run(mbq)
    assert ctx.range_error() == -1  # every read lies inside its segment
    cnt, cov, pc, ent, sec, sums = g.download()
    vpos = g.vpos.download(np.int32, int(group["read_beg"][-1]))
    seg_of_read = np.repeat(np.arange(g.n), np.diff(group["read_beg"]))
    assert np.array_equal(vpos, group["all"]["pos"] + g.voff[seg_of_read].astype(np.int32))
    in_seg = np.zeros(g.Lv, bool)
    for i, L in enumerate(g.lens.tolist()):
        sl = slice(int(g.voff[i]), int(g.voff[i]) + L)
        in_seg[sl] = True
        (dcnt, dcov, dpc, dent, dsec, dsum), oc, (ocov, opc, oent, osec) = exp[i]
        # the reference alone (bc_pileup, bc_summary), bit for bit
        assert np.array_equal(cnt[:, sl], dcnt), i
        assert np.array_equal(cov[sl], dcov) and np.array_equal(pc[:, sl], dpc), i
        assert np.array_equal(ent[sl], dent) and np.array_equal(sec[sl], dsec), i
        assert np.array_equal(sums[i], dsum), (i, sums[i], dsum)
        # the oracle, and numpy over the lists the reference builds
        assert np.array_equal(cnt[:, sl], oc[:, :k].T.astype(np.int32)), i
        assert np.array_equal(cov[sl], ocov) and np.array_equal(pc[:, sl], opc), i
        assert np.array_equal(ent[sl], oent) and np.array_equal(sec[sl], osec), i
        assert sums[i, 0] == np.mean(ocov.tolist()) and sums[i, 1] == np.mean(oent.tolist()), i
        assert sums[i, 2] == np.count_nonzero(ocov) and sums[i, 3] == int(ocov.astype(np.int64).sum()), i
    assert not cov[~in_seg].any() and not cnt[:, ~in_seg].any()  # nothing lands in a pad


def test_segments_without_percentages_or_summary(ctx, group):
    """d_pc and d_sum are optional: the other outputs are the same and the two stay untouched."""
    g = _GroupOnDevice(ctx, group, 5)
    g.run(0)
    full = g.download()
    g.poison()
    g.run(0, want_pc=False, want_sum=False)
    got = g.download()
    for j in (0, 1, 3, 4):
        assert np.array_equal(got[j], full[j])
    assert np.all(got[2].view(np.uint8) == 0x5A) and np.all(got[5].view(np.uint8) == 0x5A)


@pytest.mark.parametrize("shape", ["auto", "rc"])
def test_segments_call_is_capturable(ctx, group, shape):
    g = _GroupOnDevice(ctx, group, 6)
    ctx.set_shape(shape)
    g.run(20)  # (the k_rc scratch grows here, outside the capture)
    direct = g.download()
    graph = ctx.capture(lambda: g.run(20))
    for _ in range(2):
        g.poison()
        graph.launch()
        replay = g.download()
        for a, b in zip(replay, direct):
            assert np.array_equal(a, b)
    assert ctx.range_error() == -1


def test_segments_all_empty_group(ctx):
    """A group of references without reads (n_reads = 0): coverage 0, entropy 1 everywhere."""
    lens = np.array([5, 64, 8193, 100], np.int64)
    g = _GroupOnDevice(ctx, dict(lens=lens, read_beg=np.zeros(5, np.int64), all=None), 5)
    g.poison()
    g.run(0)
    cnt, cov, pc, ent, sec, sums = g.download()
    for i, L in enumerate(lens.tolist()):
        sl = slice(int(g.voff[i]), int(g.voff[i]) + L)
        assert not cnt[:, sl].any() and not cov[sl].any()
        assert np.all(pc[:, sl] == -1.0) and np.all(ent[sl] == 1.0) and np.all(sec[sl] == 1.0)
        assert sums[i].tolist() == [0.0, 1.0, 0.0, 0.0]


# ------------------------------------------------------------------ the CLI on many references
N_REFS, READ_LEN, PER_REF = 300, 50, 40


def _many_refs(bad=None):
    """300 references of 60-400 positions, 20 of them header-only, 40 mixed-CIGAR reads each.
    bad: "unsorted" shuffles the reads of reference 201; "both" also gives reference 140 a read
    overhanging its end."""
    rng = np.random.default_rng(77)
    lens = rng.integers(60, 401, N_REFS)
    lens[[3, 50, 51, 299]] = [64, 128, 65, 320]
    contigs = [(f"tx{i:03d}", int(L)) for i, L in enumerate(lens)]
    rs = synth.make_reads(contigs, PER_REF, mixed=True, seed=78, read_len=READ_LEN)
    empty = set(rng.choice(np.arange(1, N_REFS - 1), 18, replace=False).tolist()) | {0, N_REFS - 1}
    order = np.nonzero(~np.isin(rs.tid, list(empty)))[0]
    over = unsorted = None
    if bad:
        over, unsorted = 140, 201
        while over in empty:
            over += 1
        while unsorted in empty:
            unsorted += 1
        if bad == "both":
            last = np.nonzero(rs.tid == over)[0][-1]
            rs.pos[last] = lens[over] - 10  # still the largest start; its >= 40 aligned bases overhang
        idx = np.nonzero(rs.tid[order] == unsorted)[0]
        order[idx] = order[idx][rng.permutation(idx.size)]
    rs = synth.subset(rs, order)
    assert rs.n <= 20_000
    return rs, sorted(empty), over, unsorted


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    rs, empty, _, _ = _many_refs()
    path = str(tmp_path_factory.mktemp("segments") / "many.bam")
    synth.write_bam(rs, path)
    return dict(rs=rs, bam=path, empty=empty, counts={})


def _oracle_counts(many, mbq, mmq):
    """{reference: (oracle counts, accepted reads)}, once per (mbq, mmq)."""
    key = (mbq, mmq)
    if key not in many["counts"]:
        rs, out = many["rs"], {}
        for t, (name, L) in enumerate(zip(rs.references, rs.lengths)):
            b = synth.batch_arrays(rs, t, mmq)
            oc, (br, _) = O.bcount(L, mbq, b)
            assert br == -1
            out[name] = (oc, int(b["pos"].size))
        many["counts"][key] = out
    return many["counts"][key]


def _run_cli(argv):
    buf = io.BytesIO()
    txt = io.TextIOWrapper(buf, encoding="utf-8", write_through=True)
    with contextlib.redirect_stdout(txt):
        M.run(argv)
        txt.flush()
    return buf.getvalue()


def _plan():
    return [list(g) for g in M.PLAN["groups"]], set(M.PLAN["single"])


CLI_CASES = {
    "rows": ([], 0, 0), "long": (["--long-format"], 0, 0), "shown": (["--show-n-bases"], 0, 0),
    "summary": (["--summarise"], 0, 0),
    "rows_q20_m30": (["--min-base-quality", "20", "--min-mapping-quality", "30"], 20, 30),
    "summary_q20_m30": (["--summarise", "--min-base-quality", "20", "--min-mapping-quality", "30"], 20, 30),
}


@pytest.mark.parametrize("case", sorted(CLI_CASES))
def test_cli_grouped_output_is_the_ungrouped_output(many, monkeypatch, case):
    """Small groups (>= 4) and batches that cut references: byte-identical to the run with grouping
    off in the same process (same hash seed, so the same reference order), and every reference's
    block byte-identical to the oracle's text."""
    args, mbq, mmq = CLI_CASES[case]
    argv = [many["bam"]] + args
    monkeypatch.setenv("BASECOUNT_BATCH_RECORDS", "1500")
    monkeypatch.setenv("BASECOUNT_GROUP_MAX", "8192")
    monkeypatch.setenv("BASECOUNT_GROUP_REFS", "1")
    got = _run_cli(argv)
    groups, single = _plan()
    assert len(groups) >= 4 and all(len(g) > 1 for g in groups)
    assert single  # the references cut by a batch boundary are accumulated as before
    grouped_refs = [r for g in groups for r in g]
    assert len(grouped_refs) == len(set(grouped_refs)) and not set(grouped_refs) & single
    assert set(grouped_refs) | single == set(many["rs"].references)
    assert set(many["empty"]) & {many["rs"].references.index(r) for r in grouped_refs}  # header-only ones too
    monkeypatch.setenv("BASECOUNT_GROUP_REFS", "0")
    plain = _run_cli(argv)
    assert M.PLAN["groups"] == []
    assert got == plain
    summ = "--summarise" in args
    show_n, long_format = "--show-n-bases" in args, "--long-format" in args
    _, blocks = O.split_blocks(got.decode(), summ)
    assert set(blocks) == set(many["rs"].references)
    for name, (oc, nreads) in _oracle_counts(many, mbq, mmq).items():
        exp = O.summary_text(name, oc, show_n, nreads, 3) if summ else O.rows_text(name, oc, show_n, long_format, 3)
        assert blocks[name] == exp, name


def test_cli_one_batch_default_cap_is_one_group(many, monkeypatch):
    """Defaults: the whole file is one batch and one group, header-only references included."""
    for v in ("BASECOUNT_BATCH_RECORDS", "BASECOUNT_GROUP_MAX", "BASECOUNT_GROUP_REFS"):
        monkeypatch.delenv(v, raising=False)
    got = _run_cli([many["bam"], "--summarise"])
    groups, single = _plan()
    # (header-only references before the first / after the last one with reads are taken at the
    # end of the file: grouped when adjacent, else alone)
    assert sum(len(g) for g in groups) + len(single) == N_REFS and len(single) <= 2 and len(groups) <= 3
    monkeypatch.setenv("BASECOUNT_GROUP_REFS", "0")
    assert _run_cli([many["bam"], "--summarise"]) == got


def _outcome(argv):
    """(stdout, exception type, message) of a CLI run."""
    buf = io.BytesIO()
    txt = io.TextIOWrapper(buf, encoding="utf-8", write_through=True)
    err = None
    with contextlib.redirect_stdout(txt):
        try:
            M.run(argv)
        except BaseException as e:  # noqa: BLE001 - compared, not handled
            err = (type(e), str(e))
        txt.flush()
    return buf.getvalue(), err


@pytest.mark.parametrize("bad", ["both", "unsorted"])
def test_cli_routing_of_overhanging_and_unsorted_references(tmp_path, monkeypatch, bad):
    """A reference with a read past its end and one with unsorted reads keep the per-reference path
    (the IndexError timeline, the device sort); everything else is grouped around them.  "both":
    the run ends in the reference's IndexError; "unsorted": it prints every reference."""
    rs, _, over, unsorted = _many_refs(bad)
    bam = str(tmp_path / "bad.bam")
    synth.write_bam(rs, bam)
    names = rs.references
    monkeypatch.delenv("BASECOUNT_BATCH_RECORDS", raising=False)
    monkeypatch.setenv("BASECOUNT_GROUP_MAX", "16384")
    monkeypatch.setenv("BASECOUNT_GROUP_REFS", "1")
    got = _outcome([bam])
    groups, single = _plan()
    grouped_refs = {r for g in groups for r in g}
    assert len(groups) >= 2 and len(grouped_refs) >= N_REFS - 30
    assert grouped_refs | single == set(names) and not grouped_refs & single
    assert names[unsorted] in single
    assert (names[over] in single) == (bad == "both")
    monkeypatch.setenv("BASECOUNT_GROUP_REFS", "0")
    plain = _outcome([bam])
    assert got == plain
    if bad == "both":
        L = rs.lengths[over]
        assert got[1] == (IndexError, f"vector::_M_range_check: __n (which is {L}) >= this->size() (which is {L})")
    else:
        assert got[1] is None and len(got[0]) > 100_000


@pytest.mark.parametrize("mode", ["rows", "summary"])
def test_launch_count_is_groups_plus_ungrouped(many, monkeypatch, mode):
    """The condition that the feature is on: one kernel-1 launch per group, not per reference."""
    monkeypatch.delenv("BASECOUNT_BATCH_RECORDS", raising=False)
    monkeypatch.setenv("BASECOUNT_GROUP_MAX", "8192")
    c = M.context()

    def launches(on):
        monkeypatch.setenv("BASECOUNT_GROUP_REFS", "1" if on else "0")
        c.timing(True)
        try:
            M.get_basecounts(many["bam"], _mode=mode)
            rep = c.timing_report()
        finally:
            c.timing(False)
        return sum(rep.get(name, (0, 0.0))[0] for name in ("pileup", "solo", "rc", "count")), rep

    k1, rep = launches(True)
    groups, single = _plan()
    assert len(groups) >= 4
    assert k1 <= len(groups) + len(single), (k1, len(groups), len(single), rep)
    assert k1 < N_REFS // 10
    if mode == "summary":
        assert len(groups) <= rep["summary"][0] < N_REFS // 10  # one segmented reduction per group
    k1_off, _ = launches(False)
    assert k1_off >= N_REFS
