"""bc_bgzf_deflate on the device against its host twin (bc_bgzf_deflate_host, the same schedule lane
by lane) byte for byte, and against zlib's inflate: tiny spans at odd offsets, the block cuts, the
stored fallback between compressible blocks, a real text as one span and as seven, surplus waves, a
small compressed buffer, the gate, decreasing offsets, and the call captured in a graph behind
bc_fmt_rows.  Every buffer the call writes is pre-filled with a sentinel; 64 guard bytes on each side
of d_comp and of d_work must survive every call."""
import gzip
import os

import numpy as np
import pytest

import fmt_inputs as F
from basecount_amd import device as D

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT, GUARD = 0xEE, 64
TINY = [0, 1, 2, 3, 4, 63, 64, 65, 257, 258, 259, 260]


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    yield c
    c.close()


def rows(n_bytes: int, seed: int) -> bytes:
    """TSV-like text of exactly n_bytes."""
    rng = np.random.default_rng(seed)
    out, size, pos = [], 0, 1
    while size < n_bytes:
        c = rng.integers(0, 40, 5)
        line = b"chr%d\t%d\t%s\t%.2f\n" % (seed, pos, b"\t".join(b"%d" % v for v in c), rng.random())
        out.append(line)
        size += len(line)
        pos += 1
    return b"".join(out)[:n_bytes]


def incompressible(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(144, 256, n).astype(np.uint8).tobytes()


_MIXED = []


def mixed_text() -> bytes:
    if not _MIXED:
        _MIXED.append(gzip.open(os.path.join(REPO, "tests", "golden", "cli", "mixed_default.out.gz")).read())
    return _MIXED[0]


_TWIN = {}


def twin(text: bytes, off) -> tuple:
    key = (hash(text), tuple(int(o) for o in off))
    if key not in _TWIN:
        comp, coff = D.bgzf_deflate_host(text, off)
        assert gzip.decompress(comp.tobytes()) == text[int(off[0]):int(off[-1])] if comp.size else off[0] == off[-1]
        _TWIN[key] = (comp.tobytes(), coff)
    return _TWIN[key]


class Call:
    """One bc_bgzf_deflate call's buffers: the text and the offsets uploaded, the outputs poisoned."""

    def __init__(self, ctx, text: bytes, off, text_cap=None, comp_cap=None, gate=None, comp_shift=0):
        self.ctx = ctx
        off = np.ascontiguousarray(off, np.int64)
        self.n = off.size - 1
        self.text_cap = len(text) if text_cap is None else int(text_cap)
        self.comp_cap = int(comp_cap)
        self.shift = comp_shift
        self.bufs = []
        t = np.frombuffer(text, np.uint8)
        self.d_text = ctx.alloc(max(16, t.size))
        if t.size:
            self.d_text.upload(t)
        self.d_off = ctx.alloc(off.nbytes).upload(off)
        self.d_gate = None
        if gate is not None:
            self.d_gate = ctx.alloc(16).upload(np.array([gate, 0, 0, 0], np.int32))
        self.wb, self.ob = D.bgzf_deflate_bytes(self.text_cap, self.n)
        self.work = ctx.alloc(self.wb + 2 * GUARD)
        self.out = ctx.alloc(self.ob)
        self.comp = ctx.alloc(self.comp_cap + 2 * GUARD + 16)
        self.bufs += [self.d_text, self.d_off, self.work, self.out, self.comp] + ([self.d_gate] if self.d_gate else [])

    def poison(self):
        for b in (self.work, self.out, self.comp):
            D.check(D.lib().bc_memset(self.ctx.h, b.ptr, SENT, b.nbytes))

    def call(self):
        self.ctx.bgzf_deflate(self.d_text.ptr, self.text_cap, self.d_off.ptr, self.n,
                              self.d_gate.ptr if self.d_gate else None, self.work.ptr + GUARD, self.wb, self.out.ptr,
                              self.comp.ptr + GUARD + self.shift, self.comp_cap)

    def download(self):
        raw = self.out.download(np.uint8, self.ob)
        h = raw[:64].view(D.DFL_HEADER_DTYPE)[0]
        work = self.work.download(np.uint8, self.wb + 2 * GUARD)
        comp = self.comp.download(np.uint8, self.comp_cap + 2 * GUARD, self.shift)
        guards = [work[:GUARD], work[GUARD + self.wb:], comp[:GUARD], comp[GUARD + self.comp_cap:]]
        assert all((g == SENT).all() for g in guards), "a guard byte was written"
        return {"status": int(h["status"]), "total": int(h["total_bytes"]), "blocks": int(h["n_blocks"]),
                "stored": int(h["n_stored"]), "text_bytes": int(h["text_bytes"]), "raw_small": raw,
                "coff": raw[64:].view(np.int64), "comp": comp[GUARD:GUARD + self.comp_cap].tobytes(), "work": work}

    def free(self):
        self.ctx.sync()
        for b in self.bufs:
            b.free()


def run(ctx, text, off, **kw):
    k = Call(ctx, text, off, **kw)
    try:
        k.poison()
        k.call()
        return k.download()
    finally:
        k.free()


def spans_of(lens, start=0):
    off = np.zeros(len(lens) + 1, np.int64)
    off[0] = start
    np.cumsum(lens, out=off[1:])
    off[1:] += start
    return off


def _cases():
    mixed = mixed_text()
    cuts = np.linspace(0, len(mixed), 8).astype(np.int64)
    cuts[1:-1] += np.array([-70001, 13, 65280 * 3 - int(cuts[3]) % 65280, 1, -7, 40000])  # unequal, one on a cut
    return {
        "tiny_spans_odd_offsets": (rows(1 + sum(TINY) + 5, 1), spans_of(TINY, 1)),
        "block_cuts": (rows(65279 + 65280 + 65281, 2), spans_of([65279, 65280, 65281])),
        "stored_between": (rows(65280, 3) + incompressible(65280, 4) + rows(30000, 5), spans_of([65280 * 2 + 30000])),
        "stored_short_spans": (rows(300, 6) + incompressible(1500, 7) + rows(300, 8), spans_of([300, 1500, 300])),
        "mixed_one_span": (mixed, spans_of([len(mixed)])),
        "mixed_seven_spans": (mixed, cuts),
    }


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_device_bytes_equal_the_host_twin(ctx, name):
    text, off = CASES[name]
    comp, coff = twin(text, off)
    got = run(ctx, text, off, comp_cap=len(comp) + 40)
    assert got["status"] == D.DFL_OK and got["total"] == len(comp)
    assert got["text_bytes"] == int(off[-1] - off[0])
    assert np.array_equal(got["coff"], coff)
    assert got["comp"][:len(comp)] == comp
    assert got["comp"][len(comp):] == bytes([SENT]) * 40  # nothing at or beyond total_bytes
    assert gzip.decompress(got["comp"][:len(comp)]) == text[int(off[0]):int(off[-1])]
    assert got["stored"] == (1 if name.startswith("stored") else 0)
    assert got["blocks"] == sum(-(-int(b - a) // 65280) for a, b in zip(off[:-1], off[1:]))


@pytest.mark.parametrize("shift", [1, 7, 13])
def test_a_compressed_buffer_at_any_alignment(ctx, shift):
    text, off = CASES["block_cuts"]
    comp, _ = twin(text, off)
    got = run(ctx, text, off, comp_cap=len(comp), comp_shift=shift)
    assert got["status"] == D.DFL_OK and got["comp"] == comp


def test_surplus_waves_exit(ctx):
    text, off = CASES["stored_short_spans"]
    comp, coff = twin(text, off)
    got = run(ctx, text + bytes(4 * 65280), off, text_cap=len(text) + 4 * 65280, comp_cap=len(comp))
    assert got["status"] == D.DFL_OK and got["blocks"] == 3 and got["comp"] == comp
    assert np.array_equal(got["coff"], coff)


def test_too_small_reports_the_exact_total_and_leaves_the_buffer(ctx):
    text, off = CASES["block_cuts"]
    comp, coff = twin(text, off)
    got = run(ctx, text, off, comp_cap=len(comp) - 1)
    assert got["status"] == D.DFL_TOO_SMALL and got["total"] == len(comp)
    assert np.array_equal(got["coff"], coff)
    assert got["comp"] == bytes([SENT]) * (len(comp) - 1)
    again = run(ctx, text, off, comp_cap=got["total"])
    assert again["status"] == D.DFL_OK and again["comp"] == comp


def test_a_gate_leaves_everything_but_the_header(ctx):
    text, off = CASES["tiny_spans_odd_offsets"]
    got = run(ctx, text, off, comp_cap=4096, gate=1)
    assert got["status"] == D.DFL_GATED and got["total"] == 0 and got["blocks"] == 0
    assert got["comp"] == bytes([SENT]) * 4096
    assert (got["work"] == SENT).all() and (got["raw_small"][64:] == SENT).all()
    comp, _ = twin(text, off)
    open_gate = run(ctx, text, off, comp_cap=4096, gate=0)
    assert open_gate["status"] == D.DFL_OK and open_gate["comp"][:len(comp)] == comp


@pytest.mark.parametrize("off", [[0, 500, 400, 900], [-1, 500], [0, 901]], ids=["decreasing", "negative", "past_text_cap"])
def test_bad_offsets_are_a_status(ctx, off):
    got = run(ctx, rows(900, 9), off, comp_cap=4096)
    assert got["status"] == D.DFL_OFFSETS and got["total"] == 0 and got["blocks"] == 0
    assert got["comp"] == bytes([SENT]) * 4096


def test_captured_behind_the_formatter_and_replayed_twice(ctx):
    """bc_fmt_rows then bc_bgzf_deflate on its seg_off, gated on its status, in one graph."""
    case = next(c for c in F.cases() if c["name"] == "segments_40")
    text, seg_off = F.rows_ref(case)
    comp, coff = twin(text, seg_off)
    tab, names = F.table(case)
    bufs = []

    def up(arr):
        b = ctx.alloc(max(16, arr.nbytes))
        if arr.nbytes:
            b.upload(arr)
        bufs.append(b)
        return b

    a = D.BcFmtArgs()
    a.counts, a.pc = up(np.ascontiguousarray(case["counts"], np.int32)).ptr, up(np.ascontiguousarray(case["pc"], np.float64)).ptr
    a.ent, a.sec = up(np.ascontiguousarray(case["ent"], np.float64)).ptr, up(np.ascontiguousarray(case["sec"], np.float64)).ptr
    a.segs, a.names = up(tab).ptr, up(names).ptr
    a.stride, a.n, a.n_seg, a.names_bytes = case["stride"], case["n"], len(tab), names.size
    a.k, a.dp, a.long_format = case["k"], case["dp"], case["long"]
    fwb, fob = D.fmt_rows_bytes(case["n"], len(tab))
    text_cap = len(text) + 100
    dwb, dob = D.bgzf_deflate_bytes(text_cap, len(tab))
    fwork, fout, dtext = up(np.zeros(fwb, np.uint8)), up(np.zeros(fob, np.uint8)), up(np.zeros(text_cap, np.uint8))
    dwork, dout, dcomp = up(np.zeros(dwb, np.uint8)), up(np.zeros(dob, np.uint8)), up(np.zeros(len(comp) + 64, np.uint8))

    def both():
        ctx.fmt_rows(a, fwork.ptr, fwb, fout.ptr, dtext.ptr, text_cap)
        ctx.bgzf_deflate(dtext.ptr, text_cap, fout.ptr + 64, len(tab), fout.ptr, dwork.ptr, dwb, dout.ptr, dcomp.ptr,
                         len(comp) + 64)

    try:
        ctx.sync()
        g = ctx.capture(both)
        for _ in range(2):
            for b in (dtext, dout, dcomp, dwork):
                D.check(D.lib().bc_memset(ctx.h, b.ptr, SENT, b.nbytes))
            g.launch()
            raw = dout.download(np.uint8, dob)
            h = raw[:64].view(D.DFL_HEADER_DTYPE)[0]
            assert int(h["status"]) == D.DFL_OK and int(h["total_bytes"]) == len(comp)
            assert np.array_equal(raw[64:].view(np.int64), coff)
            assert dcomp.download(np.uint8, len(comp) + 64).tobytes() == comp + bytes([SENT]) * 64
        del g
    finally:
        ctx.sync()
        for b in bufs:
            b.free()
