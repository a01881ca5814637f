"""The stream's decoder seam (bcio_stream_set_decoder) without a device: decoders made of ctypes
callbacks that take the fills (inflating them with zlib into their own pending bytes) and then
decline, at the fill or at the batch.  Whatever a decoder declines the stream decodes itself, so the
batches equal a plain stream's and the fills are counted under the host."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import bam_decode_inputs as B
from basecount_amd import _native as N
from basecount_amd.bam import BamStream

GOLDEN = B.GOLDEN
ZBLOCK = np.dtype([("coff", "<u8"), ("clen", "<u4"), ("isize", "<u4"), ("uoff", "<u8")])

FILL = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                   C.c_int64, C.c_uint64)
NEXT = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int32, C.c_void_p)
PENDING = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64))
RELEASE = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)


class Decliner:
    """Takes fills while ``take_fills`` says so, never produces a batch."""

    def __init__(self, take_fills=True):
        self.pend = b""
        self.take_fills = take_fills
        self.calls = {"fill": 0, "next": 0, "pull": 0}
        self._cb = (FILL(self.fill), NEXT(self.next), PENDING(self.pending), RELEASE(lambda u, h: None))
        self.struct = N.BcioDecoder(None, *[C.cast(f, C.c_void_p).value for f in self._cb])

    def fill(self, user, append, carry, carry_bytes, comp, comp_bytes, blocks, n, inflated):
        self.calls["fill"] += 1
        if not self.take_fills:
            return 1
        keep = self.pend if append else C.string_at(carry, carry_bytes) if carry_bytes else b""
        zb = np.frombuffer(C.string_at(blocks, 24 * n), ZBLOCK) if n else np.zeros(0, ZBLOCK)
        out = bytearray(inflated)
        for z in zb:
            data = zlib.decompress(C.string_at(comp + int(z["coff"]), int(z["clen"])), -15)
            assert len(data) == z["isize"]
            out[int(z["uoff"]):int(z["uoff"]) + len(data)] = data
        self.pend = keep + bytes(out)
        return 0

    def next(self, user, max_records, final, n_refs, out):
        self.calls["next"] += 1
        return 2

    def pending(self, user, dst, nbytes):
        nbytes[0] = len(self.pend)
        if dst:
            self.calls["pull"] += 1
            C.memmove(dst, self.pend, len(self.pend))
            self.pend = b""
        return 0


def batches(path, bsz, dec=None):
    out = []
    with BamStream(path) as s:
        if dec is not None:
            N.bcio_check(N.bcio().bcio_stream_set_decoder(s._h, C.byref(dec.struct)))
        for b in s.batches(bsz):
            assert b.device_arrays is None
            out.append({k: np.array(getattr(b, k), copy=True) for k in B.ARRAYS})
        dev, host = C.c_int64(0), C.c_int64(0)
        N.bcio_check(N.bcio().bcio_stream_decode_stats(s._h, C.byref(dev), C.byref(host)))
        if dec is not None:
            N.bcio_check(N.bcio().bcio_stream_set_decoder(s._h, None))
    return out, (dev.value, host.value)


@pytest.mark.parametrize("name,bsz", [("edge", 3), ("edge", 1 << 20), ("c1", 300), ("ont", 50)])
@pytest.mark.parametrize("take_fills", [True, False])
def test_declined_fills_and_batches_are_decoded_by_the_host(name, bsz, take_fills):
    path = os.path.join(GOLDEN, B.GOLDEN_BAMS[name])
    want, st0 = batches(path, bsz)
    assert st0 == (0, 0)
    dec = Decliner(take_fills)
    got, (dev, host) = batches(path, bsz, dec)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        for k in B.ARRAYS:
            assert np.array_equal(a[k], b[k]), k
    assert dev == 0 and host >= 1  # every fill ended up the host's
    assert dec.calls["fill"] >= 1
    if take_fills:
        assert dec.calls["next"] >= 1 and dec.calls["pull"] == dec.calls["next"]
        assert dec.pend == b""


def test_set_decoder_checks_its_arguments():
    lib = N.bcio()
    assert lib.bcio_stream_set_decoder(None, None) == -4
    with BamStream(os.path.join(GOLDEN, "edge.bam")) as s:
        bad = N.BcioDecoder(None, None, None, None, None)
        assert lib.bcio_stream_set_decoder(s._h, C.byref(bad)) == -4
        assert b"callback" in lib.bcio_last_error()
        assert lib.bcio_device_handle(None) is None
