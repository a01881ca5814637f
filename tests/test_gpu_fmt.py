"""bc_fmt_rows on the device against rows_ref (tests/fmt_inputs.py: the host formatter per
segment): every generated case byte for byte, with the text buffer pre-filled with a sentinel that
must survive at and beyond total_bytes; a buffer one byte short; a declined value and its position;
and the call captured once in a graph and replayed twice."""
import numpy as np
import pytest

import fmt_inputs as F
from basecount_amd import device as D

pytestmark = pytest.mark.gpu

CASES = F.cases()
SLACK = 64  # sentinel bytes kept behind text_cap


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    yield c
    c.close()


class Call:
    """One bc_fmt_rows call's buffers: the arrays and the table uploaded, the outputs poisoned."""

    def __init__(self, ctx, c, text_cap):
        self.ctx, self.c, self.cap = ctx, c, int(text_cap)
        self.bufs = []
        tab, names = F.table(c)
        a = self.args = D.BcFmtArgs()
        a.counts = self._up(np.ascontiguousarray(c["counts"], np.int32))
        a.pc = self._up(np.ascontiguousarray(c["pc"], np.float64))
        a.ent = self._up(np.ascontiguousarray(c["ent"], np.float64))
        a.sec = self._up(np.ascontiguousarray(c["sec"], np.float64))
        a.segs, a.names = self._up(tab), self._up(names)
        a.stride, a.n, a.n_seg, a.names_bytes = c["stride"], c["n"], len(tab), names.size
        a.k, a.dp, a.long_format = c["k"], c["dp"], c["long"]
        wb, self.ob = D.fmt_rows_bytes(c["n"], len(tab))
        self.work, self.out = ctx.alloc(wb), ctx.alloc(self.ob)
        self.text = ctx.alloc(self.cap + SLACK + 16)
        self.bufs += [self.work, self.out, self.text]

    def _up(self, arr):
        b = self.ctx.alloc(max(16, arr.nbytes))
        if arr.nbytes:
            b.upload(arr)
        self.bufs.append(b)
        return b.ptr

    def poison(self):
        for b in (self.work, self.out, self.text):
            D.check(D.lib().bc_memset(self.ctx.h, b.ptr, F.SENTINEL, b.nbytes))

    def call(self, shift=0):
        self.ctx.fmt_rows(self.args, self.work.ptr, self.work.nbytes, self.out.ptr, self.text.ptr + shift, self.cap)

    def download(self, shift=0):
        raw = self.out.download(np.uint8, self.ob)
        h = raw[:64].view(D.FMT_HEADER_DTYPE)[0]
        return {"status": int(h["status"]), "total": int(h["total_bytes"]), "declined": int(h["declined_pos"]),
                "seg_off": raw[64:].view(np.int64),
                "text": self.text.download(np.uint8, self.cap + SLACK, shift).tobytes()}

    def free(self):
        self.ctx.sync()
        for b in self.bufs:
            b.free()


def run(ctx, c, cap, shift=0):
    k = Call(ctx, c, cap)
    try:
        k.poison()
        k.call(shift)
        return k.download(shift)
    finally:
        k.free()


REFS = {}


def ref_of(c):
    if c["name"] not in REFS:
        REFS[c["name"]] = F.rows_ref(c)
    return REFS[c["name"]]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_text_equals_the_host_formatter(ctx, case):
    text, seg_off = ref_of(case)
    got = run(ctx, case, len(text))
    assert got["status"] == case["status"] and got["declined"] == case["declined"]
    if case["status"] == F.ST_OK:
        assert got["total"] == len(text)
        assert np.array_equal(got["seg_off"], seg_off)
        assert got["text"][:len(text)] == text
        assert got["text"][len(text):] == bytes([F.SENTINEL]) * SLACK  # nothing at or beyond total_bytes
    else:
        assert got["text"] == bytes([F.SENTINEL]) * (len(text) + SLACK)


@pytest.mark.parametrize("shift", [1, 7, 13])
def test_a_text_buffer_at_any_alignment(ctx, shift):
    case = next(c for c in CASES if c["name"] == "segments_40_long")
    text, _ = ref_of(case)
    got = run(ctx, case, len(text), shift)
    assert got["status"] == F.ST_OK and got["text"][:len(text)] == text
    assert got["text"][len(text):] == bytes([F.SENTINEL]) * SLACK


def test_a_larger_buffer_keeps_its_tail(ctx):
    case = next(c for c in CASES if c["name"] == "n257_k5_wide_dp3")
    text, _ = ref_of(case)
    got = run(ctx, case, len(text) + 40)
    assert got["status"] == F.ST_OK and got["total"] == len(text)
    assert got["text"] == text + bytes([F.SENTINEL]) * (40 + SLACK)


@pytest.mark.parametrize("name", ["n65_k6_long_dp2", "n1025_k5_wide_dp4", "segments_pads_wide", "name255_long",
                                  "scan_runs"])
def test_one_byte_short_is_too_small_with_the_exact_total(ctx, name):
    case = next(c for c in CASES if c["name"] == name)
    text, seg_off = ref_of(case)
    got = run(ctx, case, len(text) - 1)
    assert got["status"] == F.ST_TOO_SMALL and got["total"] == len(text) and got["declined"] == -1
    assert np.array_equal(got["seg_off"], seg_off)
    assert got["text"] == bytes([F.SENTINEL]) * (len(text) - 1 + SLACK)
    assert run(ctx, case, len(text))["status"] == F.ST_OK


def test_a_declined_value_wins_over_a_small_buffer(ctx):
    case = next(c for c in CASES if c["name"] == "decline_nan")
    got = run(ctx, case, 5)
    assert got["status"] == F.ST_VALUE and got["declined"] == case["declined"]
    assert got["text"] == bytes([F.SENTINEL]) * (5 + SLACK)


def test_a_name_that_leaves_the_names_array_is_declined(ctx):
    case = dict(next(c for c in CASES if c["name"] == "n129_k5_wide_dp2"))
    text, _ = ref_of(case)
    k = Call(ctx, case, len(text))
    try:
        tab, names = F.table(case)
        tab["name_len"][0] = 300
        bad = ctx.alloc(64).upload(tab)
        k.bufs.append(bad)
        k.args.segs = bad.ptr
        k.poison()
        k.call()
        got = k.download()
    finally:
        k.free()
    assert got["status"] == F.ST_VALUE and got["declined"] == 0
    assert got["text"] == bytes([F.SENTINEL]) * (len(text) + SLACK)


def test_captured_once_and_replayed_twice(ctx):
    case = next(c for c in CASES if c["name"] == "segments_40")
    text, seg_off = ref_of(case)
    k = Call(ctx, case, len(text))
    try:
        k.poison()
        ctx.sync()
        g = ctx.capture(k.call)
        for _ in range(2):
            k.poison()
            g.launch()
            got = k.download()
            assert got["status"] == F.ST_OK and got["total"] == len(text)
            assert np.array_equal(got["seg_off"], seg_off)
            assert got["text"] == text + bytes([F.SENTINEL]) * SLACK
        del g
    finally:
        k.free()
