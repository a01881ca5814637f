"""bc_bam_select on the device against select_ref (tests/select_inputs.py): every per-read array,
ref_beg, the header and every per-reference fact, on the generated inputs (each the smallest that
can break one mechanism: ballot ranks at wave / step / workgroup boundaries, the order tests, the
64-bit sums, the declines) with poisoned outputs; the argument checks; a captured graph replayed
over re-poisoned outputs; and the device-decoded arrays of c1, mixed and ont."""
import ctypes as C
import os

import numpy as np
import pytest

import bam_decode_inputs as B
import select_inputs as S
from basecount_amd import device as D
from basecount_amd.bam import BamFile

pytestmark = pytest.mark.gpu

CASES = S.cases()


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    yield c
    c.close()


class Selection:
    """One bc_bam_select call's buffers: the record arrays uploaded (or a decoded batch's), the
    outputs in one poisoned buffer."""

    def __init__(self, ctx, n, mmq, ref_sel, ref_len, rec=None, arrays=None):
        self.ctx, self.n, self.nr, self.mmq = ctx, int(n), len(ref_sel), mmq
        self.bufs = []
        if rec is None:
            rec = D.BcBamArrays()
            for k, dt, extra in S.REC_FIELDS:
                setattr(rec, k, self._up(np.ascontiguousarray(arrays[k], dt)))
            rec.n_cap = self.n
        self.rec = rec
        self.d_sel = self._up(np.ascontiguousarray(ref_sel, np.uint8))
        self.d_len = self._up(np.ascontiguousarray(ref_len, np.int64))
        self.work = ctx.alloc(D.bam_select_bytes(self.n, self.nr))
        self.off, self.small, self.total = D.sel_layout(self.n, self.nr)
        self.out = ctx.alloc(self.total)
        self.arrays = D.sel_arrays(self.out.ptr, self.n, self.nr)
        self.bufs += [self.work, self.out]

    def _up(self, a):
        b = self.ctx.alloc(max(16, a.nbytes))
        if a.nbytes:
            b.upload(a)
        self.bufs.append(b)
        return b.ptr

    def poison(self):
        D.check(D.lib().bc_memset(self.ctx.h, self.out.ptr, S.POISON, self.total))
        D.check(D.lib().bc_memset(self.ctx.h, self.work.ptr, S.POISON, self.work.nbytes))

    def call(self):
        self.ctx.bam_select(self.rec, self.n, self.mmq, self.d_sel, self.d_len, self.nr, self.work.ptr,
                            self.work.nbytes, self.arrays)

    def download(self):
        raw = self.out.download(np.uint8, self.total)
        h = raw[:64].view(D.SEL_HEADER_DTYPE)[0]
        got = {k: int(h[k]) for k in ("status", "n_accepted", "n_selected", "keyerror_rec", "keyerror_ordinal")}
        got["batch_err_or"] = int(h["err_or"])
        for k, dt in S.READ_ARRAYS:
            got[k] = raw[self.off[k]:self.off[k] + self.n * np.dtype(dt).itemsize].view(dt)
        got["ref_beg"] = raw[self.off["ref_beg"]:self.off["ref_beg"] + 8 * (self.nr + 1)].view(np.int64)
        for k, dt in S.REF_ARRAYS:
            got[k] = raw[self.off[k]:self.off[k] + self.nr * np.dtype(dt).itemsize].view(dt)
        return got

    def free(self):
        self.ctx.sync()
        for b in self.bufs:
            b.free()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_generated_inputs_equal_the_reference_selection(ctx, case):
    name, a, mmq, ref_sel, ref_len, status = case
    exp = S.select_ref(a, mmq, ref_sel, ref_len)
    assert exp["status"] == status
    s = Selection(ctx, a["tid"].size, mmq, ref_sel, ref_len, arrays=a)
    try:
        s.poison()
        s.call()
        got = s.download()
    finally:
        s.free()
    assert got["status"] == status, "%s: status %d" % (name, got["status"])  # the declines return theirs
    S.assert_matches(got, exp, name)


def test_a_captured_selection_replays_over_poisoned_outputs(ctx):
    name, a, mmq, ref_sel, ref_len, _ = next(c for c in CASES if c[0] == "n%d" % (3 * S.RUN + 17))
    exp = S.select_ref(a, mmq, ref_sel, ref_len)
    s = Selection(ctx, a["tid"].size, mmq, ref_sel, ref_len, arrays=a)
    try:
        ctx.sync()
        g = ctx.capture(s.call)
        for replay in range(2):
            s.poison()
            g.launch()
            S.assert_matches(s.download(), exp, "%s replay %d" % (name, replay))
        del g
    finally:
        s.free()


def test_argument_errors_touch_no_device(ctx):
    """BC_E_ARG before any launch: the pointers below are never dereferenced."""
    L = D.lib()
    name, a, mmq, ref_sel, ref_len, _ = CASES[2]
    s = Selection(ctx, a["tid"].size, mmq, ref_sel, ref_len, arrays=a)
    try:
        s.poison()
        ctx.sync()
        n, nr, wb = s.n, s.nr, s.work.nbytes
        rec, out = C.byref(s.rec), C.byref(s.arrays)

        def call(c=ctx.h, rec=rec, n=n, sel=s.d_sel, ln=s.d_len, nr=nr, work=s.work.ptr, wb=wb, out=out):
            return L.bc_bam_select(c, rec, n, 0, sel, ln, nr, work, wb, out)

        assert call(c=None) == D.BC_E_ARG
        for kw in (dict(rec=None), dict(sel=None), dict(ln=None), dict(work=None), dict(out=None), dict(n=-1),
                   dict(nr=-1), dict(n=2**31), dict(wb=wb - 1), dict(work=s.work.ptr + 8), dict(n=n + 1)):
            assert call(**kw) == D.BC_E_ARG, kw
            assert L.bc_last_error()
        small = D.sel_arrays(s.out.ptr, n, nr)
        small.n_cap = n - 1
        assert call(out=C.byref(small)) == D.BC_E_ARG
        small.n_cap, small.ref_cap = n, nr - 1
        assert call(out=C.byref(small)) == D.BC_E_ARG
        small.ref_cap, small.flags = nr, None
        assert call(out=C.byref(small)) == D.BC_E_ARG
        b = C.c_size_t(0)
        assert L.bc_bam_select_bytes(-1, 0, C.byref(b)) == D.BC_E_ARG
        assert L.bc_bam_select_bytes(0, -1, C.byref(b)) == D.BC_E_ARG
        assert L.bc_bam_select_bytes(2**31, 0, C.byref(b)) == D.BC_E_ARG
        assert L.bc_bam_select_bytes(5, 5, None) == D.BC_E_ARG
        # nothing ran: the outputs are still poison
        raw = s.out.download(np.uint8, s.total)
        assert bool(np.all(raw == S.POISON))
    finally:
        s.free()


GOLDEN_FILES = {"c1": "c1.bam", "mixed": "mixed.bam", "ont": "ont/ont.bam"}


@pytest.mark.parametrize("name", sorted(GOLDEN_FILES))
def test_device_decoded_goldens_select_like_the_host(ctx, name):
    """bc_bam_index + bc_bam_fill + bc_bam_select with nothing in between: the selection of the
    device's own record arrays equals bcio_select on the file."""
    path = os.path.join(B.GOLDEN, GOLDEN_FILES[name])
    raw = B.inflated(path)
    first, n_refs = B.header_info(raw)
    d_raw = ctx.alloc(max(16, len(raw))).upload(np.frombuffer(raw, np.uint8))
    work = ctx.alloc(D.bam_index_bytes(len(raw), 0))
    b = ctx.bam_index(d_raw.ptr, len(raw), first, (1 << 63) - 1, True, n_refs, work.ptr, work.nbytes, 0)
    assert b.status == 0 and b.used == len(raw)
    batch = D.DeviceBamBatch(ctx, b, True)
    ctx.bam_fill(d_raw.ptr, work.ptr, b, batch.arrays, True)
    with BamFile(path) as f:
        assert f.n_records == b.n
        for mmq, every_second in ((0, False), (30, True)):
            ref_sel = np.ones(n_refs, np.uint8)
            if every_second:
                ref_sel[1::2] = 0
            exp = S.select_ref({k: getattr(f, k) for k, _, _ in S.REC_FIELDS}, mmq, ref_sel, f.lengths)
            want = f.select(mmq, ref_sel)
            s = Selection(ctx, b.n, mmq, ref_sel, f.lengths, rec=batch.arrays)
            try:
                s.poison()
                s.call()
                got = s.download()
            finally:
                s.free()
            what = "%s mmq=%d" % (name, mmq)
            assert got["status"] == S.ST_OK, what
            S.assert_matches(got, exp, what)
            m = got["n_selected"]
            for k, _ in S.READ_ARRAYS:
                assert np.array_equal(got[k][:m], getattr(want, k)), "%s: %s against bcio_select" % (what, k)
            assert np.array_equal(got["ref_beg"], want.ref_beg), what
    ctx.sync()
    batch.free()
    work.free()
    d_raw.free()
