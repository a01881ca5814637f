"""The C-ABI of the device deflate where no device is needed: the three symbols and their arguments,
bc_bgzf_deflate_bytes' arithmetic, every BC_E_ARG case of bc_bgzf_deflate (refused before any device
is touched: the context is a dummy), and bc_bgzf_deflate_host on spans with an empty one between."""
import ctypes as C
import gzip

import numpy as np
import pytest

from basecount_amd import bgzf
from basecount_amd import device as D

BC_E_ARG = -1


def test_the_symbols_are_exported_with_their_arguments():
    L = D.lib()
    assert len(L.bc_bgzf_deflate_bytes.argtypes) == 4
    assert len(L.bc_bgzf_deflate.argtypes) == 11
    assert len(L.bc_bgzf_deflate_host.argtypes) == 8
    assert D.DFL_STATUS == ("ok", "too_small", "gated", "offsets") and D.DFL_HEADER_DTYPE.itemsize == 64


def test_bytes_is_monotone_in_both_arguments():
    prev = None
    for cap in (0, 1, 65279, 65280, 65281, 10**6, 10**9, (1 << 40) - 1):
        w, o = D.bgzf_deflate_bytes(cap, 1)
        assert o == 64 + 16 and w >= 65536 * (cap // 65280 + 1)
        assert prev is None or w >= prev
        prev = w
    prev = None
    for n in (1, 2, 3, 100, 10**5):
        w, o = D.bgzf_deflate_bytes(10**6, n)
        assert o == 64 + 8 * (n + 1) and w >= 65536 * (10**6 // 65280 + n)
        assert prev is None or w > prev
        prev = w


def test_bytes_refuses_bad_sizes():
    w, o = C.c_size_t(0), C.c_size_t(0)
    L = D.lib()
    for cap, n in ((-1, 1), (10, 0), (10, -1), (1 << 40, 1), (10, 1 << 31)):
        assert L.bc_bgzf_deflate_bytes(cap, n, C.byref(w), C.byref(o)) == BC_E_ARG
    assert L.bc_bgzf_deflate_bytes(10, 1, None, C.byref(o)) == BC_E_ARG
    assert L.bc_bgzf_deflate_bytes(10, 1, C.byref(w), None) == BC_E_ARG


def test_every_bad_argument_is_refused_without_a_device():
    L = D.lib()
    wb, _ = D.bgzf_deflate_bytes(1000, 2)
    ctx, p = 0x1000, 0x10000  # never dereferenced: every case below is refused first
    good = dict(ctx=ctx, text=p, cap=1000, off=p, n=2, gate=None, work=p, wb=wb, out=p, comp=p, ccap=100)

    def call(**kw):
        a = dict(good, **kw)
        return L.bc_bgzf_deflate(a["ctx"], a["text"], a["cap"], a["off"], a["n"], a["gate"], a["work"], a["wb"], a["out"],
                                 a["comp"], a["ccap"])

    for bad in (dict(ctx=None), dict(text=None), dict(off=None), dict(work=None), dict(out=None), dict(comp=None),
                dict(cap=-1), dict(cap=1 << 40), dict(n=0), dict(n=-3), dict(ccap=-1), dict(wb=wb - 1), dict(wb=0),
                dict(work=p + 8), dict(off=p + 4), dict(out=p + 4), dict(gate=p + 2)):
        assert call(**bad) == BC_E_ARG, bad
        assert L.bc_last_error()


def test_host_refuses_bad_arguments():
    L = D.lib()
    t, off = np.zeros(16, np.uint8), np.array([0, 16], np.int64)
    comp, coff, total = np.zeros(128, np.uint8), np.zeros(2, np.int64), C.c_int64(0)
    ok = [t.ctypes.data, off.ctypes.data, 1, comp.ctypes.data, 128, coff.ctypes.data, C.byref(total), 1]
    assert L.bc_bgzf_deflate_host(*ok) == D.DFL_OK and total.value == int(coff[1]) > 26
    for i in (0, 1, 3, 5, 6):
        bad = list(ok)
        bad[i] = None
        assert L.bc_bgzf_deflate_host(*bad) == BC_E_ARG
    assert L.bc_bgzf_deflate_host(*(ok[:2] + [0] + ok[3:])) == BC_E_ARG
    assert L.bc_bgzf_deflate_host(*(ok[:4] + [-1] + ok[5:])) == BC_E_ARG
    dec = np.array([0, 10, 5], np.int64)
    coff3 = np.zeros(3, np.int64)
    assert L.bc_bgzf_deflate_host(t.ctypes.data, dec.ctypes.data, 2, comp.ctypes.data, 128, coff3.ctypes.data,
                                  C.byref(total), 1) == D.DFL_OFFSETS


def rows(n):
    return b"".join(b"chr1\t%d\t%d\t0\t3\t0\t0.25\n" % (i, i % 17) for i in range(n))


def test_two_spans_with_an_empty_one_between():
    text = rows(9000)  # more than two blocks
    cut = 70001
    off = np.array([0, cut, cut, len(text)], np.int64)
    comp1, coff1 = D.bgzf_deflate_host(text, off, nthreads=1)
    comp16, coff16 = D.bgzf_deflate_host(text, off, nthreads=16)
    assert np.array_equal(comp1, comp16) and np.array_equal(coff1, coff16)
    assert coff1[0] == 0 and coff1[1] == coff1[2] and coff1[3] == comp1.size  # the empty span: no block
    assert gzip.decompress(comp1[:coff1[1]].tobytes()) == text[:cut]
    assert gzip.decompress(comp1[coff1[2]:].tobytes()) == text[cut:]
    bl = bgzf.blocks(comp1.tobytes())
    assert [b[2] for b in bl] == [65280, cut - 65280] + [65280] * ((len(text) - cut) // 65280) + [(len(text) - cut) % 65280]
    assert coff1[1] in [b[0] for b in bl]  # every span a run of whole blocks
    # one byte short: the exact total, and the same offsets
    L = D.lib()
    t = np.frombuffer(text, np.uint8)
    small, coff, total = np.full(comp1.size - 1, 0xEE, np.uint8), np.zeros(4, np.int64), C.c_int64(0)
    rc = L.bc_bgzf_deflate_host(t.ctypes.data, off.ctypes.data, 3, small.ctypes.data, small.size, coff.ctypes.data,
                                C.byref(total), 4)
    assert rc == D.DFL_TOO_SMALL and total.value == comp1.size and np.array_equal(coff, coff1)
    assert (small == 0xEE).all()


def test_the_writer_and_the_parser(capfdbinary):
    text = rows(5000)
    with bgzf.Writer() as w:
        w.write(b"head\n")
        w.write(b"")
        w.write_blocks(bgzf.compress(text))
    out = capfdbinary.readouterr().out
    assert gzip.decompress(out) == b"head\n" + text and out[-28:] == bgzf.EOF
    bl = bgzf.blocks(out)
    assert bl[0][2] == 5 and bl[-1][2] == 0 and sum(b[2] for b in bl) == 5 + len(text)
    assert w.text_bytes == 5 and w.comp_bytes == len(out)
    with pytest.raises(ValueError):
        bgzf.blocks(out[:-1])
    with pytest.raises(ValueError):
        bgzf.blocks(b"x" + out)


def test_the_twin_cuts_a_long_reference_at_the_formatter_slices(monkeypatch):
    from basecount_amd import main as M

    text = rows(1000)
    assert M.bgzf_text(text) is text  # the switch off: the text itself
    monkeypatch.setenv("BASECOUNT_BGZF", "1")
    monkeypatch.setattr(M, "FORMAT_SLICE", 300)
    for per, want in ((1, [300, 300, 300, 100]), (2, [600, 400])):
        out = bytes(M.bgzf_text(text, per))
        assert gzip.decompress(out) == text
        assert [gzip.decompress(out[o:o + b]).count(b"\n") for o, b, _, _ in bgzf.blocks(out)] == want
    assert bytes(M.bgzf_text(b"")) == b""
