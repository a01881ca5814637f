"""Argument checks of the device BAM decode calls come first and need no device (BC_E_ARG)."""
import ctypes as C

import pytest

from basecount_amd import device as D


@pytest.fixture(scope="module")
def L():
    return D.lib()


def test_index_bytes_checks_and_layout(L):
    n = C.c_size_t(0)
    assert L.bc_bam_index_bytes(1000, 0, None) == D.BC_E_ARG and b"NULL" in L.bc_last_error()
    for bad in (1, 63, (1 << 24) + 1):
        assert L.bc_bam_index_bytes(1000, bad, C.byref(n)) == D.BC_E_ARG
        assert b"seg_bytes" in L.bc_last_error()
    assert L.bc_bam_index_bytes(0, 0, C.byref(n)) == 0 and n.value >= 128
    small = n.value
    assert L.bc_bam_index_bytes(1 << 20, 256, C.byref(n)) == 0 and n.value > small
    assert D.bam_index_bytes(1 << 20, 256) == n.value
    assert L.bc_bam_index_bytes(1 << 33, 0, C.byref(n)) == 0 and n.value == 128  # declined: header only


def test_index_and_fill_reject_bad_arguments_without_a_device(L):
    # a stand-in for a context: every check below fails before the context is looked at
    ctx = C.create_string_buffer(4096)
    raw, work = C.create_string_buffer(64), C.create_string_buffer(1 << 16)
    b, a = D.BcBamBatch(), D.BcBamArrays()
    wp = (C.addressof(work) + 15) & ~15
    ok = dict(ctx=C.addressof(ctx), raw=C.addressof(raw), raw_bytes=64, first=0, lim=10, final=1, n_refs=1, seg=0,
              work=wp, work_bytes=1 << 15, out=C.byref(b))

    def index(**kw):
        k = dict(ok, **kw)
        return L.bc_bam_index(k["ctx"], k["raw"], k["raw_bytes"], k["first"], k["lim"], k["final"], k["n_refs"],
                              k["seg"], k["work"], k["work_bytes"], k["out"])

    for kw, word in ((dict(ctx=None), b"ctx"), (dict(raw=None), b"NULL"), (dict(work=None), b"NULL"),
                     (dict(out=None), b"NULL"), (dict(first=65), b"first"), (dict(lim=-1), b"max_records"),
                     (dict(n_refs=-1), b"n_refs"), (dict(seg=32), b"seg_bytes"), (dict(work_bytes=64), b"smaller"),
                     (dict(work=wp + 4), b"aligned")):
        assert index(**kw) == D.BC_E_ARG, kw
        assert word in L.bc_last_error(), (kw, L.bc_last_error())
    # more bytes than 32-bit offsets index: declined with a status, no device touched
    assert index(raw_bytes=1 << 32, work_bytes=128) == 0
    assert b.status == D.BAM_STATUS.index("too_large") and b.n == 0

    b = D.BcBamBatch()
    b.raw_bytes, b.seg_bytes = 64, 65536
    assert L.bc_bam_fill(None, ok["raw"], wp, C.byref(b), C.byref(a), 0) == D.BC_E_ARG
    assert L.bc_bam_fill(ok["ctx"], None, wp, C.byref(b), C.byref(a), 0) == D.BC_E_ARG
    assert L.bc_bam_fill(ok["ctx"], ok["raw"], wp, None, C.byref(a), 0) == D.BC_E_ARG
    assert L.bc_bam_fill(ok["ctx"], ok["raw"], wp, C.byref(b), None, 0) == D.BC_E_ARG
    assert L.bc_bam_fill(ok["ctx"], ok["raw"], wp, C.byref(b), C.byref(a), 0) == D.BC_E_ARG
    assert b"missing output array" in L.bc_last_error()
    b.status = 3
    assert L.bc_bam_fill(ok["ctx"], ok["raw"], wp, C.byref(b), C.byref(a), 0) == D.BC_E_ARG
    assert b"declined" in L.bc_last_error()
    b.status, b.n = 0, 5
    assert L.bc_bam_fill(ok["ctx"], ok["raw"], wp, C.byref(b), C.byref(a), 0) == D.BC_E_ARG
    assert b"smaller than the batch" in L.bc_last_error()
