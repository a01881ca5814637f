"""bc_fmt_rows' argument checks and sizes that need no GPU: BC_E_ARG comes before any device is
touched, each with a message naming the limit, and the buffer sizes follow the schedule (two int64
and 64 lane lengths per tile of 64 positions; a 64-byte header and seg_off[n_seg + 1])."""
import ctypes as C

import pytest

from basecount_amd import device as D


def args(**kw):
    a = D.BcFmtArgs()
    a.counts = a.pc = a.ent = a.sec = a.segs = a.names = 0x1000  # never dereferenced on the host
    a.stride, a.n, a.n_seg, a.names_bytes, a.k, a.dp, a.long_format = 100, 100, 1, 4, 5, 3, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_the_symbols_exist_and_the_abi_version_stays():
    L = D.lib()
    assert L.bc_fmt_rows_bytes and L.bc_fmt_rows
    assert L.bc_abi_version() == 8
    assert C.sizeof(D.BcFmtArgs) == 96 and D.FMT_HEADER_DTYPE.itemsize == 64 and D.FMT_SEG_DTYPE.itemsize == 32


def test_byte_counts():
    assert D.fmt_rows_bytes(0, 1) == (272, 64 + 16)
    assert D.fmt_rows_bytes(1, 1) == (272, 80)
    assert D.fmt_rows_bytes(64, 1) == (272, 80)
    assert D.fmt_rows_bytes(65, 3) == (544, 64 + 32)
    assert D.fmt_rows_bytes(1 << 22, 2000) == (272 << 16, 64 + 8 * 2001)
    assert D.fmt_rows_bytes(2**31 - 1, 1) == (272 << 25, 80)


@pytest.mark.parametrize("n, n_seg, word", [(-1, 1, b"negative"), (1, -1, b"negative"), (2**31, 1, b"2^31"),
                                            (10, 0, b"n_seg")])
def test_bytes_argument_errors(n, n_seg, word):
    L = D.lib()
    w, o = C.c_size_t(0), C.c_size_t(0)
    assert L.bc_fmt_rows_bytes(n, n_seg, C.byref(w), C.byref(o)) == D.BC_E_ARG and word in L.bc_last_error()
    assert L.bc_fmt_rows_bytes(1, 1, None, C.byref(o)) == D.BC_E_ARG and b"NULL" in L.bc_last_error()
    assert L.bc_fmt_rows_bytes(1, 1, C.byref(w), None) == D.BC_E_ARG


def test_a_null_context_is_refused_first():
    L = D.lib()
    assert L.bc_fmt_rows(None, None, None, 0, None, None, -1) == D.BC_E_ARG
    assert b"ctx is NULL" in L.bc_last_error()


@pytest.mark.parametrize("kw, word", [
    (dict(counts=None), b"NULL"), (dict(pc=None), b"NULL"), (dict(ent=None), b"NULL"), (dict(sec=None), b"NULL"),
    (dict(segs=None), b"NULL"), (dict(names=None), b"NULL"),
    (dict(k=4), b"k must be 5 or 6"), (dict(k=7), b"k must be 5 or 6"),
    (dict(dp=-1), b"[0, 4]"), (dict(dp=5), b"[0, 4]"),
    (dict(n=-1), b"negative"), (dict(n=2**31, stride=2**31), b"2^31"), (dict(n_seg=0), b"n_seg"),
    (dict(n_seg=-3), b"negative"), (dict(names_bytes=-1), b"negative"), (dict(stride=99), b"stride"),
])
def test_argument_errors_come_before_any_device(kw, word):
    """A context handle that is not one: the checks must fail before it is looked at."""
    L = D.lib()
    fake = C.c_void_p(0x10)
    rc = L.bc_fmt_rows(fake, C.byref(args(**kw)), 0x2000, 1 << 20, 0x3000, 0x4000, 1 << 20)
    assert rc == D.BC_E_ARG and word in L.bc_last_error(), L.bc_last_error()


def test_buffer_errors():
    L = D.lib()
    fake = C.c_void_p(0x10)
    a = args()
    assert L.bc_fmt_rows(fake, None, 0x2000, 544, 0x3000, 0x4000, 10) == D.BC_E_ARG and b"NULL" in L.bc_last_error()
    assert L.bc_fmt_rows(fake, C.byref(a), None, 32, 0x3000, 0x4000, 10) == D.BC_E_ARG and b"NULL" in L.bc_last_error()
    assert L.bc_fmt_rows(fake, C.byref(a), 0x2000, 544, None, 0x4000, 10) == D.BC_E_ARG
    assert L.bc_fmt_rows(fake, C.byref(a), 0x2000, 544, 0x3000, None, 10) == D.BC_E_ARG
    assert L.bc_fmt_rows(fake, C.byref(a), 0x2000, 544, 0x3000, 0x4000, -1) == D.BC_E_ARG and b"text_cap" in L.bc_last_error()
    assert L.bc_fmt_rows(fake, C.byref(a), 0x2000, 543, 0x3000, 0x4000, 10) == D.BC_E_ARG and b"d_work" in L.bc_last_error()
    assert L.bc_fmt_rows(fake, C.byref(a), 0x2004, 544, 0x3000, 0x4000, 10) == D.BC_E_ARG and b"aligned" in L.bc_last_error()


def test_fmt_supported():
    assert D.fmt_supported(0, ["a"]) and D.fmt_supported(4, ["x" * 255, "y"])
    assert not D.fmt_supported(5, ["a"]) and not D.fmt_supported(-1, ["a"]) and not D.fmt_supported(17, [])
    assert not D.fmt_supported(3, ["a", "x" * 256]) and not D.fmt_supported(3, ["é" * 128])
