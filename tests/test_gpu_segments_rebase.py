"""bc_segments_rebase on the GPU: a cohort batch's cig_beg / seq_nib moved by their file's bases.
Segments of 0, 1, 64, 65 and 257 reads (waves inside one segment and waves that straddle several),
bases near 2^32 against numpy's uint32 arithmetic, in place and to separate outputs; and the call
captured in a graph together with bc_pileup_segments over two files' reads in shared buffers, whose
replay must give what bc_pileup gives on each file alone."""
import numpy as np
import pytest

from basecount_amd import bam
from basecount_amd import device as D
from basecount_amd import synth
from basecount_amd.main import norm_factors

pytestmark = pytest.mark.gpu

SEG_READS = [0, 1, 64, 65, 0, 0, 257, 64, 3, 0]


@pytest.fixture(scope="module")
def ctx():
    return D.Context(0)


def _table(ctx, read_beg, cig_base, nib_base):
    blob = np.concatenate([np.asarray(read_beg, np.int64).view(np.uint64), np.asarray(cig_base, np.uint64),
                           np.asarray(nib_base, np.uint64)])
    d = ctx.alloc(blob.nbytes).upload(blob)
    n = len(cig_base)
    return d, d.ptr, d.ptr + 8 * (n + 1), d.ptr + 8 * (2 * n + 1)


@pytest.mark.parametrize("in_place", [False, True])
def test_rebase_equals_numpy_uint32_with_bases_near_2_32(ctx, in_place):
    rng = np.random.default_rng(41)
    n_seg = len(SEG_READS)
    read_beg = np.zeros(n_seg + 1, np.int64)
    read_beg[1:] = np.cumsum(SEG_READS)
    n = int(read_beg[-1])
    # per segment: a base, and values that reach exactly up to 2^32 - 1 with it
    cig_base = np.sort(rng.integers(0, 1 << 32, n_seg, dtype=np.uint64))
    cig_base[0], cig_base[-2], cig_base[-1] = 0, (1 << 32) - 1 - 5, (1 << 32) - 1  # (the last segment is empty)
    nib_base = (np.sort(rng.integers(0, 1 << 27, n_seg, dtype=np.uint64)) * 32).astype(np.uint64)
    nib_base[-2] = (1 << 32) - 32
    seg = np.repeat(np.arange(n_seg), SEG_READS)
    room_c, room_n = (1 << 32) - 1 - cig_base[seg], (1 << 32) - 1 - nib_base[seg]
    cig = (rng.integers(0, 1 << 32, n, dtype=np.uint64) % (room_c + 1)).astype(np.uint32)
    nib = (rng.integers(0, 1 << 32, n, dtype=np.uint64) % (room_n + 1)).astype(np.uint32)
    first = read_beg[:-1][np.array(SEG_READS) > 0]
    cig[first], nib[first] = room_c[first].astype(np.uint32), room_n[first].astype(np.uint32)  # sum = 2^32 - 1
    exp_c = (cig.astype(np.uint64) + cig_base[seg]).astype(np.uint32)
    exp_n = (nib.astype(np.uint64) + nib_base[seg]).astype(np.uint32)
    assert int((cig.astype(np.uint64) + cig_base[seg]).max()) == (1 << 32) - 1
    _, p_rb, p_cb, p_nb = keep = _table(ctx, read_beg, cig_base, nib_base)
    # 64 guard bytes after each array: a lane past n writes nothing
    dc, dn = ctx.alloc(4 * n + 64), ctx.alloc(4 * n + 64)
    oc, on = ctx.alloc(4 * n + 64), ctx.alloc(4 * n + 64)
    for b in (dc, dn, oc, on):
        assert D.lib().bc_memset(ctx.h, b.ptr, 0x5A, b.nbytes) == 0
    dc.upload(cig)
    dn.upload(nib)
    total = (1 << 32) - 1
    if in_place:
        ctx.segments_rebase(n, n_seg, p_rb, p_cb, p_nb, total, total, dc.ptr, dn.ptr)
        got_c, got_n = dc, dn
    else:
        ctx.segments_rebase(n, n_seg, p_rb, p_cb, p_nb, total, total, dc.ptr, dn.ptr, oc.ptr, on.ptr)
        got_c, got_n = oc, on
        assert np.array_equal(dc.download(np.uint32, n), cig) and np.array_equal(dn.download(np.uint32, n), nib)
    rc, rn = got_c.download(np.uint32, n + 16), got_n.download(np.uint32, n + 16)
    assert np.array_equal(rc[:n], exp_c) and np.array_equal(rn[:n], exp_n)
    assert np.all(rc[n:] == 0x5A5A5A5A) and np.all(rn[n:] == 0x5A5A5A5A)
    del keep


def test_no_reads_is_a_no_op(ctx):
    _, p_rb, p_cb, p_nb = keep = _table(ctx, [0, 0], [0], [0])
    ctx.segments_rebase(0, 1, p_rb, p_cb, p_nb, 0, 0, None, None)
    ctx.sync()
    del keep


def _spans(b):
    out = np.zeros(b["pos"].size, np.int64)
    for i, (c0, cn) in enumerate(zip(b["cig_beg"].tolist(), b["cig_n"].tolist())):
        w = b["cigar"][c0:c0 + cn]
        out[i] = int((w >> 4)[np.isin(w & 0xF, (0, 2, 3, 7, 8))].sum())
    return out


def test_rebase_and_pileup_segments_are_capturable_together(ctx):
    """Two files' reads in shared buffers: rebase (to separate outputs, so that a replay starts from
    the same inputs) + bc_pileup_segments captured in one graph; each file's slice of the replay
    equals bc_pileup on that file alone."""
    k, mbq = 6, 20
    nf, nf2 = norm_factors(k)
    files = []
    for seed, L, n in ((5, 700, 257), (6, 513, 130)):
        rs = synth.make_reads([("r", L)], n, mixed=True, seed=seed, read_len=100)
        b = synth.batch_arrays(rs, 0, 0)
        order = np.argsort(b["pos"], kind="stable")
        for name in ("pos", "cig_beg", "cig_n", "seq_nib"):
            b[name] = b[name][order]
        b["seq_event"] = bam.seq_to_event(b["seq"])
        files.append((L, b))
    lens = np.array([L for L, _ in files], np.int64)
    voff = D.segments_layout(lens)
    Lv = int(voff[-1])
    # the shared buffers: CIGAR words end to end, sequences at multiples of 16, qualities by nibble
    cig_base = np.cumsum([0] + [b["cigar"].size for _, b in files])
    seq_base = np.cumsum([0] + [b["seq_event"].size for _, b in files])
    assert all(int(x) % 16 == 0 for x in seq_base)
    cigar = np.concatenate([b["cigar"] for _, b in files])
    seq = np.concatenate([b["seq_event"] for _, b in files])
    qual = np.zeros(2 * int(seq_base[-1]), np.uint8)
    for (_, b), o in zip(files, seq_base[:-1]):
        qual[2 * int(o):2 * int(o) + b["qual"].size] = b["qual"]
    per = {name: np.concatenate([b[name] for _, b in files]) for name in ("pos", "cig_beg", "cig_n", "seq_nib")}
    read_beg = np.cumsum([0] + [b["pos"].size for _, b in files]).astype(np.int64)
    n = int(read_beg[-1])
    dev = {name: ctx.alloc(a.nbytes).upload(a) for name, a in
           dict(per, cigar=cigar, seq=seq, qual=qual).items()}
    cb2, sn2, vpos = ctx.alloc(4 * n), ctx.alloc(4 * n), ctx.alloc(4 * n)
    _, p_rb, p_cb, p_nb = keep = _table(ctx, read_beg, cig_base[:-1], 2 * seq_base[:-1])
    seg_tab = np.concatenate([lens, read_beg, voff])
    d_tab = ctx.alloc(seg_tab.nbytes).upload(seg_tab)
    r = D.BcReads()
    r.n_reads, r.pos, r.cig_n = n, dev["pos"].ptr, dev["cig_n"].ptr
    r.cig_beg, r.seq_nib = cb2.ptr, sn2.ptr
    r.cigar, r.n_cigar_words = dev["cigar"].ptr, cigar.size
    r.seq, r.seq_bytes, r.seq_layout = dev["seq"].ptr, int(seq_base[-1]) - 16, D.BC_SEQ_EVENT
    r.qual, r.qual_bytes = dev["qual"].ptr, qual.size
    r.sorted, r.max_span = 1, int(max(_spans(b).max() for _, b in files))
    bufs = [ctx.alloc(x) for x in (4 * k * Lv, 4 * Lv, 8 * k * Lv, 8 * Lv, 8 * Lv)]

    def run():
        ctx.segments_rebase(n, 2, p_rb, p_cb, p_nb, cigar.size, 2 * seq.size, dev["cig_beg"].ptr, dev["seq_nib"].ptr,
                            cb2.ptr, sn2.ptr)
        ctx.pileup_segments(r, 2, d_tab.ptr, d_tab.ptr + 16, d_tab.ptr + 40, Lv, vpos.ptr, mbq, k, nf, nf2,
                            *[x.ptr for x in bufs])

    run()  # (any scratch grows here, outside the capture)
    ctx.sync()
    graph = ctx.capture(run)
    for x in bufs + [cb2, sn2]:
        assert D.lib().bc_memset(ctx.h, x.ptr, 0x5A, x.nbytes) == 0
    graph.launch()
    assert ctx.range_error() == -1
    cnt = bufs[0].download(np.int32, k * Lv).reshape(k, Lv)
    ent = bufs[3].download(np.float64, Lv)
    seg = np.repeat([0, 1], np.diff(read_beg))
    assert np.array_equal(cb2.download(np.uint32, n), per["cig_beg"] + cig_base[seg].astype(np.uint32))
    assert np.array_equal(sn2.download(np.uint32, n), per["seq_nib"] + (2 * seq_base[seg]).astype(np.uint32))
    for i, (L, b) in enumerate(files):
        dr = D.DeviceReads(ctx, dict(b, sorted=1))
        one = [ctx.alloc(x) for x in (4 * k * L, 4 * L, 8 * k * L, 8 * L, 8 * L)]
        ctx.pileup(dr, L, mbq, k, nf, nf2, *[x.ptr for x in one])
        assert ctx.range_error() == -1
        sl = slice(int(voff[i]), int(voff[i]) + L)
        assert np.array_equal(cnt[:, sl], one[0].download(np.int32, k * L).reshape(k, L)), i
        assert np.array_equal(ent[sl], one[3].download(np.float64, L)), i
        assert cnt[:, sl].any()
        dr.free()
    del keep
