"""bc_segments_rebase's and bc_amplicons_segments' argument checks, which need no GPU: BC_E_ARG
comes before any device is touched, each with a message naming the limit."""
import ctypes as C

import pytest

from basecount_amd import device as D

P = 0x1000  # a device pointer that is never dereferenced on the host
FAKE = C.c_void_p(0x10)  # a context handle that is not one: the checks must fail before it is looked at


def test_the_symbols_exist_and_the_abi_version_stays():
    L = D.lib()
    assert L.bc_segments_rebase and L.bc_amplicons_segments
    assert L.bc_abi_version() == 8


def rebase(ctx=FAKE, n=10, n_seg=2, rb=P, cb=P, nb=P, cw=100, nt=100, c=P, q=P, oc=P, oq=P):
    return D.lib().bc_segments_rebase(ctx, n, n_seg, rb, cb, nb, cw, nt, c, q, oc, oq)


@pytest.mark.parametrize("kw, word", [
    (dict(ctx=None), b"ctx is NULL"),
    (dict(n=-1), b"n_reads"), (dict(n=2**31), b"n_reads"),
    (dict(n_seg=0), b"n_seg"), (dict(n_seg=-4), b"n_seg"),
    (dict(cw=2**32), b"2^32"), (dict(nt=2**32), b"2^32"), (dict(cw=2**40, nt=2**40), b"2^32"),
    (dict(rb=None), b"NULL"), (dict(cb=None), b"NULL"), (dict(nb=None), b"NULL"),
    (dict(c=None), b"NULL"), (dict(q=None), b"NULL"), (dict(oc=None), b"NULL"), (dict(oq=None), b"NULL"),
    (dict(n=0, rb=None, c=None, q=None, oc=None, oq=None), b"NULL"),  # the table is needed even without reads
])
def test_rebase_argument_errors_come_before_any_device(kw, word):
    assert rebase(**kw) == D.BC_E_ARG and word in D.lib().bc_last_error(), D.lib().bc_last_error()


def amplicons(ctx=FAKE, cov=P, ent=P, sec=P, n_seg=2, ln=P, voff=P, lo=P, hi=P, n_tiles=3, out=P):
    return D.lib().bc_amplicons_segments(ctx, cov, ent, sec, n_seg, ln, voff, lo, hi, n_tiles, out)


@pytest.mark.parametrize("kw, word", [
    (dict(ctx=None), b"ctx is NULL"),
    (dict(n_seg=0), b"n_seg"), (dict(n_seg=-1), b"n_seg"),
    (dict(n_tiles=-1), b"n_tiles"), (dict(n_seg=1 << 20, n_tiles=1 << 20), b"2^31"),
    (dict(cov=None), b"NULL"), (dict(ent=None), b"NULL"), (dict(sec=None), b"NULL"), (dict(ln=None), b"NULL"),
    (dict(voff=None), b"NULL"), (dict(lo=None), b"NULL"), (dict(hi=None), b"NULL"), (dict(out=None), b"NULL"),
    (dict(n_tiles=0, n_seg=0), b"n_seg"),  # the counts are checked before "no windows: nothing to do"
])
def test_amplicons_segments_argument_errors_come_before_any_device(kw, word):
    assert amplicons(**kw) == D.BC_E_ARG and word in D.lib().bc_last_error(), D.lib().bc_last_error()


def test_the_largest_buffers_that_fit_pass_the_size_check():
    """2^32 - 1 words and nibbles are accepted by the size rule: the next check (a NULL array) answers."""
    assert rebase(cw=2**32 - 1, nt=2**32 - 1, c=None) == D.BC_E_ARG
    assert b"NULL per-read array" in D.lib().bc_last_error()
