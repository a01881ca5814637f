"""BAM record decode on the device (bc_bam_index / bc_bam_fill, basecount_amd/csrc/bc_bam.hip)
against the host decoder: every array bit for bit, on inflated bytes resident in HBM, in batches
cut by max_records and carried, with sentinel-filled outputs between guard regions."""
import os

import numpy as np
import pytest

import bam_decode_inputs as B
from basecount_amd import device as D
from basecount_amd import synth
from basecount_amd.bam import BamFile
from basecount_amd.main import norm_factors

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0xEE
NO_LIMIT = (1 << 63) - 1
LIMITED_BATCHES = 32  # batches taken at a record limit before the rest goes in one


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """name -> (inflated bytes, the host decoder's arrays), decoded once."""
    d = tmp_path_factory.mktemp("gpubam")
    out = {}
    for name, rel in B.GOLDEN_BAMS.items():
        path = os.path.join(B.GOLDEN, rel)
        out[name] = (B.inflated(path), B.host_arrays(path))
    trap, _ = B.trap_builder()
    for name, b in (("layout", B.layout_builder()), ("trap", trap)):
        path = str(d / (name + ".bam"))
        B.write_bam(path, b)
        out[name] = (b.raw(), B.host_arrays(path))
    return out


class Guarded:
    """The output arrays of one batch, each between two guard regions, all bytes pre-filled."""

    def __init__(self, ctx, batch, want_qual):
        n, cw, sb = int(batch.n), int(batch.cigar_words), int(batch.seq_bytes)
        self.arrays, self.bufs, self.sizes = D.BcBamArrays(), {}, {}
        for name, dt, cnt in D.BAM_ARRAYS:
            nbytes = int(cnt(n, cw, sb)) * np.dtype(dt).itemsize
            buf = ctx.alloc(nbytes + 2 * GUARD)
            D.check(D.lib().bc_memset(ctx.h, buf.ptr, SENTINEL, buf.nbytes))
            self.bufs[name], self.sizes[name] = buf, nbytes
            setattr(self.arrays, name, buf.ptr + GUARD)
        self.arrays.n_cap, self.arrays.cigar_cap, self.arrays.seq_cap = n, cw, sb
        self.want_qual = want_qual

    def download(self):
        """The arrays; asserts the guards (and a qual array not asked for) still hold the sentinel."""
        out = {}
        for name, dt, _ in D.BAM_ARRAYS:
            raw = self.bufs[name].download(np.uint8, self.sizes[name] + 2 * GUARD)
            assert (raw[:GUARD] == SENTINEL).all() and (raw[GUARD + self.sizes[name]:] == SENTINEL).all(), name
            body = raw[GUARD:GUARD + self.sizes[name]]
            if name == "qual" and not self.want_qual:
                assert (body == SENTINEL).all(), "qual written without want_qual"
            out[name] = body.view(dt)
        return out

    def free(self):
        for b in self.bufs.values():
            b.free()


def decode_all(ctx, raw: bytes, seg: int, limit: int, want_qual=True, final=True, first=None):
    """The whole buffer in batches: LIMITED_BATCHES at `limit` records, the rest in one.  Odd batches
    index the carried bytes as a buffer of their own (d_raw + used, offset 0: any alignment), even
    ones the whole buffer at `first` = used.  Returns the concatenated arrays and the counters."""
    hdr_first, n_refs = B.header_info(raw)
    first = hdr_first if first is None else first
    N = len(raw)
    d_raw = ctx.alloc(max(16, N)).upload(np.frombuffer(raw, np.uint8))
    work = ctx.alloc(D.bam_index_bytes(N, seg))
    parts, used, stats = [], first, dict(device=0, declined=0, repaired=0, batches=0, status=0, err_off=0)
    while True:
        lim = NO_LIMIT if limit < 0 or stats["batches"] >= LIMITED_BATCHES else limit
        base = used if stats["batches"] % 2 else 0
        b = ctx.bam_index(d_raw.ptr + base, N - base, used - base, lim, final, n_refs, work.ptr, work.nbytes, seg)
        stats["batches"] += 1
        stats["repaired"] += int(b.repaired)
        if b.status != 0:
            stats.update(declined=stats["declined"] + 1, status=int(b.status), err_off=base + int(b.err_off))
            break
        stats["device"] += 1
        assert b.raw_bytes == N - base and b.segments >= 1
        g = Guarded(ctx, b, want_qual)
        ctx.bam_fill(d_raw.ptr + base, work.ptr, b, g.arrays, want_qual)
        parts.append((int(b.n), int(b.cigar_words), int(b.seq_bytes), g.download()))
        g.free()
        used = base + int(b.used)
        if b.n == 0 or used >= N:
            break
    d_raw.free()
    work.free()
    stats["used"] = used
    return concat(parts), stats


def concat(parts) -> dict:
    out = {k: [] for k in B.ARRAYS}
    cig = seq = 0
    cig_off, seq_off = [np.zeros(1, np.uint64)], [np.zeros(1, np.uint64)]
    for n, cw, sb, a in parts:
        assert a["cig_off"][0] == 0 and a["seq_off"][0] == 0
        assert a["cig_off"][n] == cw and a["seq_off"][n] == sb
        assert not a["seq_event"][sb:].any() and a["seq_event"].size == D.seq_event_bytes(sb)  # the zero tail
        for k in B.ARRAYS[:9] + ("cigar", "seq", "qual"):
            out[k].append(a[k])
        out["seq_event"].append(a["seq_event"][:sb])
        cig_off.append(a["cig_off"][1:] + np.uint64(cig))
        seq_off.append(a["seq_off"][1:] + np.uint64(seq))
        cig, seq = cig + cw, seq + sb
    res = {k: np.concatenate(v) if v else np.zeros(0, B.DTYPES[k]) for k, v in out.items()}
    res["cig_off"], res["seq_off"] = np.concatenate(cig_off), np.concatenate(seq_off)
    res["n"] = sum(p[0] for p in parts)
    return res


@pytest.mark.parametrize("seg", B.SEGS)
@pytest.mark.parametrize("name", ["c1", "edge", "mixed", "ont", "layout"])
def test_arrays_equal_the_host_decoders(ctx, inputs, name, seg):
    raw, exp = inputs[name]
    for limit in B.LIMITS:
        got, st = decode_all(ctx, raw, seg, limit)
        what = "%s seg_bytes=%d max_records=%d" % (name, seg, limit)
        assert st["declined"] == 0 and st["device"] == st["batches"], "%s: %r" % (what, st)  # a valid file
        assert st["used"] == len(raw), what
        B.assert_arrays_equal(got, exp, True, what)
        if limit > 0:
            assert st["batches"] >= min(exp["n"] // limit, LIMITED_BATCHES), what


def test_qual_is_written_only_when_asked_for(ctx, inputs):
    raw, exp = inputs["edge"]
    got, st = decode_all(ctx, raw, 1024, -1, want_qual=False)
    assert st["declined"] == 0
    B.assert_arrays_equal(got, exp, False, "edge without qual")


def test_partial_last_record_is_left_for_the_next_fill(ctx, inputs):
    raw, exp = inputs["layout"]
    b = B.layout_builder()
    for seg in B.SEGS:
        got, st = decode_all(ctx, raw[:-5], seg, -1, final=False)
        assert st["declined"] == 0 and st["used"] == b.starts[-1], (seg, st)
        B.assert_arrays_equal(got, B.first_records(exp, exp["n"] - 1), True, "partial seg_bytes=%d" % seg)


def test_trap_records_inside_a_qual_field_are_not_believed(ctx, inputs):
    raw, exp = inputs["trap"]
    for seg in B.SEGS:
        got, st = decode_all(ctx, raw, seg, -1)
        B.assert_arrays_equal(got, exp, True, "trap seg_bytes=%d" % seg)
        if seg == 1024:  # the segment behind the field starts inside it, on copied records
            assert st["repaired"] + st["declined"] >= 1, st
    for limit in (1, 3):
        got, st = decode_all(ctx, raw, 1024, limit)
        B.assert_arrays_equal(got, exp, True, "trap max_records=%d" % limit)


@pytest.mark.parametrize("name", sorted(B.refusals()))
def test_rule_violations_decline_the_fill_with_the_hosts_reason(ctx, name, tmp_path):
    raw, msg = B.refusals()[name]
    path = str(tmp_path / "bad.bam")
    with open(path, "wb") as f:
        f.write(B.bgzf(raw))
    with pytest.raises(Exception) as ei:
        BamFile(path)
    assert msg in str(ei.value)
    for seg in B.SEGS:
        for limit in (3, -1):
            got, st = decode_all(ctx, raw, seg, limit)
            assert st["declined"] == 1 and B.STATUS_MESSAGE[st["status"]] == msg, (name, seg, limit, st)
    bad_at = {"truncated_last_record": None, "ends_in_length_prefix": None}
    got, st = decode_all(ctx, raw, 256, -1, final=False)
    if name in bad_at:  # more bytes may follow: the complete records are taken
        assert st["declined"] == 0 and got["n"] == 9
    else:
        assert st["declined"] == 1 and B.STATUS_MESSAGE[st["status"]] == msg


def test_fill_and_pileup_replay_in_one_captured_graph(ctx, tmp_path):
    """bc_bam_fill is stream-ordered and does not allocate: with bc_pileup on the decoded batch it is
    captured into one graph whose replays match the eager result from the host decoder's arrays."""
    L, k, mbq = 3000, 6, 20
    rs = synth.make_reads([("g", L)], 700, mixed=True, seed=11)
    path = str(tmp_path / "g.bam")
    synth.write_bam(rs, path)
    nf, nf2 = norm_factors(k)
    with BamFile(path) as f:
        sel = f.select(0, [1])
        hb = dict(pos=sel.pos.copy(), cig_beg=sel.cig_beg.copy(), cig_n=sel.cig_n.copy(), seq_nib=sel.seq_nib.copy(),
                  cigar=f.cigar.copy(), seq=f.seq.copy(), seq_event=f.seq_event.copy(), qual=f.qual.copy(), sorted=1,
                  max_span=int(sel.span.max()))
        max_end = int((sel.pos.astype(np.int64) + sel.span).max())
    outs = [ctx.alloc(n) for n in (4 * k * L, 4 * L, 8 * k * L, 8 * L, 8 * L)]

    def results():
        return (outs[0].download(np.int32, k * L), outs[1].download(np.int32, L), outs[2].download(np.float64, k * L),
                outs[3].download(np.float64, L), outs[4].download(np.float64, L))

    eager = D.DeviceReads(ctx, hb)
    ctx.pileup(eager, L, mbq, k, nf, nf2, *[x.ptr for x in outs])
    exp = results()
    assert ctx.range_error() == -1 and exp[1].max() > 0
    eager.free()

    raw = B.inflated(path)
    first, n_refs = B.header_info(raw)
    d_raw = ctx.alloc(len(raw)).upload(np.frombuffer(raw, np.uint8))
    work = ctx.alloc(D.bam_index_bytes(len(raw), 1024))
    b = ctx.bam_index(d_raw.ptr, len(raw), first, NO_LIMIT, True, n_refs, work.ptr, work.nbytes, 1024)
    assert b.status == 0 and b.n == hb["pos"].size
    dec = D.DeviceBamBatch(ctx, b, True)
    per_read = {k_: ctx.alloc(4 * b.n).upload(hb[k_]) for k_ in ("pos", "cig_beg", "cig_n", "seq_nib")}
    r = D.BcReads()
    r.n_reads = int(b.n)
    for k_, buf in per_read.items():
        setattr(r, k_, buf.ptr)
    r.cigar, r.n_cigar_words = dec.buffers["cigar"].ptr, int(b.cigar_words)
    r.seq, r.seq_bytes, r.seq_layout = dec.buffers["seq_event"].ptr, int(b.seq_bytes), D.BC_SEQ_EVENT
    r.qual, r.qual_bytes = dec.buffers["qual"].ptr, 2 * int(b.seq_bytes)
    r.sorted, r.max_span, r.max_end = 1, hb["max_span"], max_end

    def step():
        ctx.bam_fill(d_raw.ptr, work.ptr, b, dec.arrays, True)
        ctx.pileup(r, L, mbq, k, nf, nf2, *[x.ptr for x in outs])

    step()  # (context scratch grows here, outside the capture)
    ctx.sync()
    g = ctx.capture(step)  # a synchronisation or an allocation inside would fail the capture
    for _ in range(2):
        for x in outs:
            x.zero()
        for name in ("cigar", "seq_event", "qual"):  # the replayed fill has to write them again
            D.check(D.lib().bc_memset(ctx.h, dec.buffers[name].ptr, SENTINEL, dec.buffers[name].nbytes))
        g.launch()
        for a, e in zip(results(), exp):
            assert np.array_equal(a, e)
    assert ctx.range_error() == -1
    for x in outs + list(per_read.values()) + [d_raw, work]:
        x.free()
    dec.free()
