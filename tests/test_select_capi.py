"""bc_bam_select's argument checks and layouts that need no GPU: BC_E_ARG comes before any device
is touched, and the work-buffer size follows the schedule (three int64 columns of one entry per
run of 1,024 records, the compacted tid and rec_err)."""
import ctypes as C

import numpy as np

from basecount_amd import device as D


def test_select_bytes_and_argument_errors():
    L = D.lib()
    b = C.c_size_t(0)
    assert L.bc_bam_select_bytes(-1, 0, C.byref(b)) == D.BC_E_ARG
    assert L.bc_bam_select_bytes(0, -1, C.byref(b)) == D.BC_E_ARG
    assert L.bc_bam_select_bytes(2**31, 0, C.byref(b)) == D.BC_E_ARG and b"2^31" in L.bc_last_error()
    assert L.bc_bam_select_bytes(1, 1, None) == D.BC_E_ARG
    assert D.bam_select_bytes(0, 0) == 3 * 16 + 2 * 16
    assert D.bam_select_bytes(1024, 7) == 3 * 16 + 2 * 4096
    assert D.bam_select_bytes(1025, 7) == 3 * 16 + 2 * 4112
    assert D.bam_select_bytes(1 << 24, 100000) == 3 * 8 * (1 << 14) + 2 * 4 * (1 << 24)
    # a NULL context is refused first, whatever else is passed
    assert L.bc_bam_select(None, None, 0, 0, None, None, 0, None, 0, None) == D.BC_E_ARG
    assert b"NULL" in L.bc_last_error()


def test_output_layout_is_aligned_and_disjoint():
    for n, nr in ((0, 0), (1, 1), (1000, 3), (4097, 1000)):
        off, small, total = D.sel_layout(n, nr)
        spans = [(off["header"], 64)]
        spans += [(off[k], (nr + 1) * np.dtype(dt).itemsize) for k, dt in D.SEL_REF_ARRAYS]
        spans += [(off[k], max(1, n) * np.dtype(dt).itemsize) for k, dt in D.SEL_READ_ARRAYS]
        spans.sort()
        for (a, la), (b2, _) in zip(spans, spans[1:]):
            assert a % 256 == 0 and a + la <= b2
        assert spans[-1][0] + spans[-1][1] <= total and small <= total
        assert all(off[k] < small for k, _ in D.SEL_REF_ARRAYS) and all(off[k] >= small for k, _ in D.SEL_READ_ARRAYS)
        assert C.sizeof(D.BcSelHeader) == 64 == D.SEL_HEADER_DTYPE.itemsize
