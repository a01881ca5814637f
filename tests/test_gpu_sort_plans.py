"""bc_reads_sort (basecount_amd/csrc/bc_sort.hip) on every plan, rank path and copy branch, checked
read by read.

The inputs are tests/sort_plans.py's cases; tests/test_sort_plans_host.py proves on the CPU that each
holds the decisions it is named for (count and scatter rounds, both count_rows instances with more
than one bucket group and row iteration, one and two perm passes and buckets past the registers,
wbits 0, the counting sort's first size, its scan carries and its relay tails, full and shrunk
slots, bump allocations, big records).  Every case is sorted twice: copied (with qualities) and
fields-only (no qualities under shape "rc"; the counting sort copies all the same).  Each run

  * pins sort_plans.layout_bytes to bc_reads_sort_bytes and the batch's max_end to the restated one;
  * wants bc_reads_sort_check clean and the view's sequence pointer as the mode says;
  * downloads the batch and the view as they lie in device memory and applies
    sort_plans.sorted_view_matches: sorted starts, the same reads as a multiset (start, CIGAR, bases,
    qualities), nibble parity kept, no two reads' bytes overlapping and all below room (copied), the
    source's very sequence and seq_nib (fields-only);
  * where max_end < 65,536, counts the view with bc_count under "auto", "rc" and "tile", k 5 and 6,
    min_base_quality 0 and (with qualities) 20, against the oracle's counts of the unsorted batch.

The flagged caller errors (a start outside [0, max_end], overlapping sequences), a d_mem reused for
a smaller layout, and a fields-only view under the tiled kernel and the sparse sweep (L far above
the max_end the sort decided on) have tests of their own."""
import functools

import numpy as np
import pytest

import oracle as O
import sort_plans as SP
from basecount_amd import device as D
from basecount_amd.main import norm_factors

pytestmark = pytest.mark.gpu

COUNT_MAX_END = 65_536  # above it the structural check stands alone (no histogram of a long reference)


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    try:
        yield c
    finally:
        c.set_shape("auto")


@pytest.fixture(autouse=True)
def _auto_shape(ctx):
    """Every test starts and ends with the automatic kernel shape."""
    ctx.set_shape("auto")
    yield
    ctx.set_shape("auto")


def fetch(ctx, ptr, dtype, count):
    out = np.empty(int(count), dtype)
    if out.nbytes:
        D.check(D.lib().bc_memcpy_d2h(ctx.h, out.ctypes.data, ptr, out.nbytes))
        ctx.sync()
    return out


def host_copy(ctx, r, seq_bytes):
    """The arrays of a device batch (a BcReads) as they lie in device memory."""
    n = int(r.n_reads)
    return dict(pos=fetch(ctx, r.pos, np.int32, n), cig_beg=fetch(ctx, r.cig_beg, np.uint32, n),
                cig_n=fetch(ctx, r.cig_n, np.uint32, n), seq_nib=fetch(ctx, r.seq_nib, np.uint32, n),
                cigar=fetch(ctx, r.cigar, np.uint32, r.n_cigar_words), seq=fetch(ctx, r.seq, np.uint8, seq_bytes),
                qual=fetch(ctx, r.qual, np.uint8, r.qual_bytes) if r.qual else None)


def source_copy(ctx, r):
    return host_copy(ctx, r, D.seq_event_bytes(r.seq_bytes))


def view_copy(ctx, r, s):
    """The sorted view s of batch r; a copied view's padding past room must be zero."""
    fields = s.seq == r.seq
    if fields:
        return dict(host_copy(ctx, s, D.seq_event_bytes(r.seq_bytes)), fields=True, room=None)
    room = int(s.seq_bytes)
    v = host_copy(ctx, s, D.seq_event_bytes(room))
    assert not v["seq"][room:].any(), "the copy's padding past room is not zero"
    assert (s.qual_bytes == 2 * room) if r.qual else (not s.qual)
    return dict(v, fields=False, room=room)


def sort_into(ctx, r, mem=None, check=True):
    """bc_reads_sort of r (a BcReads) into a fresh buffer of bc_reads_sort_bytes (or mem) -> (view, mem)."""
    nb = ctx.sort_bytes(r)
    if mem is None:
        mem = ctx.alloc(nb)
    assert mem.nbytes >= nb
    s = ctx.sort(r, mem.ptr, mem.nbytes, check_flags=check)
    assert s.sorted == 1 and s.n_reads == r.n_reads and s.seq_layout == D.BC_SEQ_EVENT
    return s, mem


@functools.lru_cache(maxsize=8)
def want_counts(name, L, mbq):
    exp, (bad, _) = O.bcount(L, mbq, SP.case(name))
    assert bad == -1
    return exp


def count_view(ctx, s, L, mbq, k):
    nbi = ctx.index_bytes(s, L)
    imem = ctx.alloc(max(16, nbi))
    if nbi:
        ctx.index(s, L, imem.ptr, nbi)
    hist = ctx.alloc(4 * k * L)
    hist.zero()
    try:
        ctx.count(s, L, mbq, k, hist.ptr)
        assert ctx.range_error() == -1
        return hist.download(np.int32, k * L).reshape(k, L)
    finally:
        hist.free()
        imem.free()


def counts_match(ctx, s, L, mbqs, want):
    """bc_count of the view under every shape, k 5 and 6, against want(mbq) (the oracle's [L][6])."""
    for shape in ("auto", "rc", "tile"):
        ctx.set_shape(shape)
        for mbq in mbqs:
            for k in (5, 6):
                v = D.BcReads.from_buffer_copy(s)  # (bc_reads_index sets the index fields in place)
                got = count_view(ctx, v, L, mbq, k)
                assert np.array_equal(got, want(mbq)[:, :k].T.astype(np.int32)), (shape, mbq, k)
    ctx.set_shape("auto")


def run_case(ctx, name, mode):
    b = SP.case(name)
    batch = b if mode == "copied" else dict(b, qual=None)
    ctx.set_shape("auto" if mode == "copied" else "rc")
    reads = D.DeviceReads(ctx, batch)
    mem = None
    try:
        r = reads.r
        n, me = int(r.n_reads), SP.max_end_of(b)
        assert r.max_end == me
        P = SP.plan(n, me)
        fields = mode == "fields" and P["kind"] == "bucket"
        assert ctx.sort_bytes(r) == SP.layout_bytes(n, me, b["seq"].size, mode == "copied", mode == "fields")
        s, mem = sort_into(ctx, r)  # (check_flags: bc_reads_sort_check is clean)
        assert (s.seq == r.seq) == fields, (name, mode, P["kind"])
        src = source_copy(ctx, r)
        view = view_copy(ctx, r, s)
        assert view["fields"] == fields
        if not fields:
            assert view["room"] == SP.copy_plan(b)["room"]
        SP.sorted_view_matches(src, view)
        if me < COUNT_MAX_END:
            counts_match(ctx, s, me + 3, (0, 20) if mode == "copied" else (0,),
                         lambda mbq: want_counts(name, me + 3, mbq))
    finally:
        if mem is not None:
            mem.free()
        reads.free()


@pytest.mark.parametrize("mode", ["copied", "fields"])
@pytest.mark.parametrize("name", SP.cases())
def test_sort_case(ctx, name, mode):
    run_case(ctx, name, mode)


def test_copied_without_qualities_under_tile(ctx):
    """The other way to a copy: no qualities, shape "tile" (the sort decides by the shape in force)."""
    b = dict(SP.case("rank_edges"), qual=None)
    ctx.set_shape("tile")
    reads = D.DeviceReads(ctx, b)
    r = reads.r
    assert ctx.sort_bytes(r) == SP.layout_bytes(r.n_reads, r.max_end, b["seq"].size, False, False)
    s, mem = sort_into(ctx, r)
    try:
        assert s.seq != r.seq and not s.qual
        SP.sorted_view_matches(source_copy(ctx, r), view_copy(ctx, r, s))
        L = int(r.max_end) + 3
        counts_match(ctx, s, L, (0,), lambda mbq: want_counts("rank_edges", L, 0))
    finally:
        mem.free()
        reads.free()


def set_starts(ctx, r, pairs):
    """Starts written straight into the device batch (bc_reads_upload refuses a negative start)."""
    for i, p in pairs:
        v = np.array([p], np.int32)
        D.check(D.lib().bc_memcpy_h2d(ctx.h, r.pos + 4 * int(i), v.ctypes.data, 4))
        ctx.sync()


@pytest.mark.parametrize("mode", ["copied", "fields"])
@pytest.mark.parametrize("name", list(SP.BAD_START_BASE))
def test_bad_starts_are_flagged_and_clamped(ctx, name, mode):
    """One negative start and one above max_end: bc_reads_sort_check says "outside", and the view is
    the batch's with those two starts at 0 (safe to count)."""
    b = SP.case(SP.BAD_START_BASE[name])
    batch = b if mode == "copied" else dict(b, qual=None)
    ctx.set_shape("auto" if mode == "copied" else "rc")
    reads = D.DeviceReads(ctx, batch)
    r = reads.r
    bad = SP.bad_starts(b)
    set_starts(ctx, r, bad)
    s, mem = sort_into(ctx, r, check=False)
    try:
        with pytest.raises(D.BcError, match="outside"):
            ctx.sort_check(r, mem.ptr)
        src = source_copy(ctx, r)
        assert [int(src["pos"][i]) for i, _ in bad] == [p for _, p in bad]
        src["pos"][[i for i, _ in bad]] = 0
        SP.sorted_view_matches(src, view_copy(ctx, r, s))
        if r.max_end < COUNT_MAX_END:
            L = int(r.max_end) + 3
            clamped = dict(batch, pos=src["pos"])
            counts_match(ctx, s, L, (0, 20) if mode == "copied" else (0,), lambda mbq: O.bcount(L, mbq, clamped)[0])
    finally:
        mem.free()
        reads.free()


def test_overlap_is_flagged_and_dropped_reads_have_no_cigar(ctx):
    """Reads whose claimed bytes sum to far more than the sequence buffer: the slots shrink, the
    bump allocator runs out, bc_reads_sort_check says "overlap"; the view's starts are sorted, every
    read of it has no CIGAR or is its source read, and it counts as its kept reads do."""
    b = SP.case("overlap")
    reads = D.DeviceReads(ctx, b)
    r = reads.r
    s, mem = sort_into(ctx, r, check=False)
    try:
        with pytest.raises(D.BcError, match="overlap"):
            ctx.sort_check(r, mem.ptr)
        src, view = source_copy(ctx, r), view_copy(ctx, r, s)
        kept = SP.kept_reads_match(src, view)
        assert 0 < kept.size < b["pos"].size
        L = int(r.max_end) + 3
        sub = SP.sub_batch(b, kept)
        counts_match(ctx, s, L, (0, 20), lambda mbq: O.bcount(L, mbq, sub)[0])
    finally:
        mem.free()
        reads.free()


@pytest.mark.parametrize("mode", ["copied", "fields"])
def test_reused_d_mem(ctx, mode):
    """capped_rounds, then w0_tiny into the same d_mem (a larger layout, then a smaller one): the
    second sort's check is clean and its view matches -- no stale bump, flag or qmax word."""
    ctx.set_shape("auto" if mode == "copied" else "rc")
    mem = None
    for name in ("capped_rounds", "w0_tiny"):
        b = SP.case(name)
        reads = D.DeviceReads(ctx, b if mode == "copied" else dict(b, qual=None))
        try:
            s, mem = sort_into(ctx, reads.r, mem)
            assert (s.seq == reads.r.seq) == (mode == "fields")
            SP.sorted_view_matches(source_copy(ctx, reads.r), view_copy(ctx, reads.r, s))
        finally:
            reads.free()
    mem.free()


def test_reused_d_mem_after_flags(ctx):
    """A flagged sort (overlap: bump far past room, flag bit 0, a large qmax), then a clean one into the
    same d_mem."""
    first = D.DeviceReads(ctx, SP.case("overlap"))
    big = ctx.alloc(max(ctx.sort_bytes(first.r), 1 << 20))
    try:
        sort_into(ctx, first.r, big, check=False)
        with pytest.raises(D.BcError, match="overlap"):
            ctx.sort_check(first.r, big.ptr)
        second = D.DeviceReads(ctx, SP.case("w0_tiny"))
        try:
            s, _ = sort_into(ctx, second.r, big)
            SP.sorted_view_matches(source_copy(ctx, second.r), view_copy(ctx, second.r, s))
        finally:
            second.free()
    finally:
        big.free()
        first.free()


# ------------------------------------------------------------- the fields-only view downstream
DOWN_N, DOWN_END = 40_000, 3_000


@functools.lru_cache(maxsize=1)
def downstream_batch():
    rng = np.random.default_rng(611)
    return dict(SP.spread(rng, DOWN_N, DOWN_END, 100, 151), qual=None)


@functools.lru_cache(maxsize=2)
def downstream_want(L):
    cnt, (bad, _) = O.bcount(L, 0, downstream_batch())
    assert bad == -1
    return cnt


@pytest.mark.parametrize("shape", ["auto", "tile"])
@pytest.mark.parametrize("L,kernel", [(30_000, "tiles"), (2_000_000, "solo")])
def test_fields_only_view_downstream(ctx, L, kernel, shape):
    """A deep quality-free batch sorted under "auto" keeps its sequence where it is (the sort takes it
    for k_rc's); counted on a reference far longer than its max_end the view reaches the multi-wave
    tiled kernel (L = 30,000) and the sparse sweep (L = 2,000,000) instead: bc_pileup_summary with no
    per-position output and bc_pileup_summary_amplicons must give numpy's numbers over the oracle's
    arrays, bit for bit."""
    b = downstream_batch()
    reads = D.DeviceReads(ctx, b)
    s, mem = sort_into(ctx, reads.r)
    bufs = []
    try:
        assert s.seq == reads.r.seq and D.pileup_plan(s, DOWN_END)["kernel"] == "rc"
        ctx.set_shape(shape)
        plan = D.pileup_plan(s, L, shape)
        assert plan["kernel"] == kernel and (kernel == "solo" or plan["waves_per_tile"] > 1), plan
        cnt = downstream_want(L)
        rng = np.random.default_rng(L)
        tiles = [(int(a), int(a + w)) for a, w in zip(rng.integers(-20, DOWN_END + 200, 40), rng.integers(-3, 420, 40))]
        tiles += [(0, 0), (L - 1, L + 10), (5, 4), (100, 1_600), (0, L - 1), (2, 2 + 512), (DOWN_END - 10, DOWN_END + 900)]
        lo, hi = np.array([t[0] for t in tiles], np.int64), np.array([t[1] for t in tiles], np.int64)
        for k in (5, 6):
            cov, _, ent, sec = O.stats(cnt, k == 6)
            want = [np.mean(cov.astype(np.int64)), np.mean(ent), float(np.count_nonzero(cov)),
                    float(cov.astype(np.int64).sum())]
            nf, nf2 = norm_factors(k)
            work, dout = ctx.alloc(D.summary_work_bytes(L)), ctx.alloc(32)
            bufs += [work, dout]
            work.zero()
            ctx.timing(True)
            ctx.timing_report()
            ctx.pileup_summary(s, L, 0, k, nf, nf2, None, None, None, None, None, work.ptr, dout.ptr)
            assert ctx.range_error() == -1
            ran = set(ctx.timing_report())
            assert ("solo" if kernel == "solo" else "pileup") in ran and "rc" not in ran, ran
            assert dout.download(np.float64, 4).tolist() == want, (k, "summary only")
            outs = [ctx.alloc(x) for x in (4 * k * L, 4 * L, 8 * L, 8 * L)]
            dlo, dhi, damp = ctx.alloc(lo.nbytes).upload(lo), ctx.alloc(hi.nbytes).upload(hi), ctx.alloc(48 * len(tiles))
            bufs += outs + [dlo, dhi, damp]
            dout.zero()
            ctx.pileup_summary_amplicons(s, L, 0, k, nf, nf2, *[x.ptr for x in outs], work.ptr, dout.ptr, dlo.ptr,
                                         dhi.ptr, len(tiles), damp.ptr)
            assert ctx.range_error() == -1
            ran = set(ctx.timing_report())
            assert ("solo" if kernel == "solo" else "pileup") in ran and "rc" not in ran, ran
            ctx.timing(False)
            assert dout.download(np.float64, 4).tolist() == want, (k, "amplicons' summary")
            assert np.array_equal(outs[0].download(np.int32, k * L).reshape(k, L), cnt[:, :k].T.astype(np.int32))
            assert np.array_equal(outs[1].download(np.int32, L), cov)
            assert np.array_equal(outs[2].download(np.float64, L), ent)
            assert np.array_equal(outs[3].download(np.float64, L), sec)
            got = damp.download(np.float64, 6 * len(tiles)).reshape(-1, 6)
            for i, e in enumerate(O.amplicons(cov, ent, sec, tiles)):
                assert got[i].tolist() == [float(x) for x in e], (k, i, tiles[i])
            while bufs:
                bufs.pop().free()
    finally:
        ctx.timing(False)
        for x in bufs:
            x.free()
        mem.free()
        reads.free()
