"""The stream's inflater seam (bcio_stream_set_inflater) on the CPU: a ctypes callback backed by zlib
stands in for the device.  Records are the plain stream's, blocks the callback refuses are inflated
on the host, and hostile files fail exactly as they do without an inflater."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from basecount_amd.bam import BamStream

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BAMS = sorted(f for f in os.listdir(GOLDEN) if f.endswith(".bam"))
FIELDS = ("tid", "pos", "flag", "mapq", "l_seq", "qstart", "qend", "rec_err", "ref_span")


class ZBlock(C.Structure):
    _fields_ = [("coff", C.c_uint64), ("clen", C.c_uint32), ("isize", C.c_uint32), ("uoff", C.c_uint64)]


INFLATE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(ZBlock), C.c_int64,
                         C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.c_uint8))


def make_inflater(fail_every=0, rc=0, log=None):
    """A bcio_inflate_fn: zlib per block; every fail_every-th block (counted over the calls) gets
    status 1 and garbage for output; `rc` is the call's own return value."""
    seen = [0]

    def fn(user, comp, comp_bytes, blocks, n, out, out_bytes, status):
        assert C.sizeof(ZBlock) == 24
        for i in range(n):
            b = blocks[i]
            assert b.coff + b.clen <= comp_bytes and b.uoff + b.isize <= out_bytes
            seen[0] += 1
            if log is not None:
                log.append((b.coff, b.clen, b.isize))
            dst = C.addressof(out.contents) + b.uoff
            if fail_every and seen[0] % fail_every == 0:
                C.memset(dst, 0xD7, b.isize)
                status[i] = 1
                continue
            raw = C.string_at(C.addressof(comp.contents) + b.coff, b.clen)
            try:
                data = zlib.decompress(raw, -15)
            except zlib.error:
                status[i] = 2
                continue
            if len(data) != b.isize:
                status[i] = 3
                continue
            C.memmove(dst, data, len(data))
            status[i] = 0
        return rc

    return INFLATE_FN(fn)


def bgzf_blocks(path):
    """Number of BGZF blocks of a well-formed file."""
    blob, off, n = open(path, "rb").read(), 0, 0
    while off < len(blob):
        off += struct.unpack_from("<H", blob, off + 16)[0] + 1
        n += 1
    return n


def read_all(path, batch, **kw):
    """(records by field, cigars, sequences, inflate stats after open, at the end)."""
    got = {k: [] for k in FIELDS}
    cig, seq = [], []
    with BamStream(path, **kw) as s:
        at_open = s.inflate_stats()
        for b in s.batches(batch):
            for k in FIELDS:
                got[k].append(getattr(b, k).copy())
            cig += [b.cigartuples(i) for i in range(b.n_records)]
            seq += [b.query_alignment_sequence(i) for i in range(b.n_records)]
        stats = s.inflate_stats()
    return {k: np.concatenate(v) if v else np.empty(0) for k, v in got.items()}, cig, seq, at_open, stats


def same_records(a, b):
    for k in FIELDS:
        assert np.array_equal(a[0][k], b[0][k]), k
    assert a[1] == b[1] and a[2] == b[2]


@pytest.fixture(scope="module")
def plain():
    return {(bam, batch): read_all(os.path.join(GOLDEN, bam), batch) for bam in BAMS for batch in (3, 10 ** 9)}


@pytest.mark.parametrize("batch", [3, 10 ** 9])
@pytest.mark.parametrize("bam", BAMS)
def test_records_equal_and_every_later_block_by_callback(plain, bam, batch):
    path = os.path.join(GOLDEN, bam)
    ref = plain[(bam, batch)]
    total = bgzf_blocks(path)
    assert ref[4] == {"callback": 0, "host": total}
    fn = make_inflater()
    got = read_all(path, batch, inflater=(fn, None))
    same_records(got, ref)
    header = got[3]["host"]  # inflated by the open, before the inflater was set
    assert got[3]["callback"] == 0 and 1 <= header < total
    assert got[4] == {"callback": total - header, "host": header}


@pytest.mark.parametrize("bam", BAMS)
def test_blocks_the_callback_refuses_are_inflated_on_the_host(plain, bam):
    path = os.path.join(GOLDEN, bam)
    total = bgzf_blocks(path)
    fn = make_inflater(fail_every=3)
    got = read_all(path, 3, inflater=(fn, None))
    same_records(got, plain[(bam, 3)])
    later = total - got[3]["host"]
    assert got[4] == {"callback": later - later // 3, "host": got[3]["host"] + later // 3}


@pytest.mark.parametrize("bam", BAMS)
def test_a_failing_call_sends_every_block_to_the_host(plain, bam):
    path = os.path.join(GOLDEN, bam)
    fn = make_inflater(rc=-2)
    got = read_all(path, 10 ** 9, inflater=(fn, None))
    same_records(got, plain[(bam, 10 ** 9)])
    assert got[4] == {"callback": 0, "host": bgzf_blocks(path)}


def test_range_streams_use_the_inflater():
    from basecount_amd.bam import find_ref_start

    path = os.path.join(GOLDEN, "mixed.bam")
    beg = find_ref_start(path, 0)
    ref = read_all(path, 10 ** 9, voff_range=(beg, None))
    log = []
    fn = make_inflater(log=log)
    got = read_all(path, 10 ** 9, voff_range=(beg, None), inflater=(fn, None))
    same_records(got, ref)
    assert got[4]["callback"] == len(log) > 0


# ---- hostile files: the same error with and without an inflater ------------------------------------
def _block(raw, *, cdata=None, isize=None):
    if cdata is None:
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        cdata = c.compress(raw) + c.flush()
    bs = 12 + 6 + len(cdata) + 8 - 1
    head = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255]) + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bs)
    return head + cdata + struct.pack("<II", zlib.crc32(raw), len(raw) if isize is None else isize)


def _header():
    text = b"@HD\tVN:1.6\n"
    return b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chrA\0" + \
        struct.pack("<i", 1000)


def _record(pos=10, block_size=None):
    body = struct.pack("<iiBBHHHiiii", 0, pos, 2, 60, 4680, 1, 0, 4, -1, -1, 0) + b"r\0" + struct.pack("<I", 4 << 4)
    body += bytes([0x12, 0x48]) + bytes([30] * 4)
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


_RECS = b"".join(_record(pos=10 + i) for i in range(50))
_GOOD = _block(_RECS)
HOSTILE = {
    "control": _block(_RECS),
    "isize_mismatch": _block(_RECS, isize=len(_RECS) + 3),
    "isize_short": _block(_RECS, isize=len(_RECS) - 1),
    "deflate_bit_flip": _block(_RECS, cdata=bytes([_GOOD[18] ^ 0x06]) + _GOOD[19:-8]),
    "deflate_truncated": _block(_RECS, cdata=_GOOD[18:-8][:20]),
    "deflate_btype3": _block(_RECS, cdata=b"\x07\x00"),
    "record_past_data": _block(_RECS + _record(block_size=10_000)),
    "second_block_bad": _block(_RECS) + _block(_RECS, cdata=b"\x07\x00"),
    "cut_block": _block(_RECS)[:-9],
}


def _outcome(path, **kw):
    try:
        n = 0
        with BamStream(path, **kw) as s:
            for b in s.batches(7):
                n += b.n_records
        return ("ok", n)
    except Exception as e:  # noqa: BLE001 - the outcome IS the exception
        return (type(e).__name__, getattr(e, "code", None), str(e))


@pytest.mark.parametrize("case", sorted(HOSTILE))
def test_hostile_files_fail_the_same_with_an_inflater(tmp_path, case):
    p = tmp_path / "x.bam"
    p.write_bytes(_block(_header()) + HOSTILE[case] + _block(b""))
    want = _outcome(str(p))
    assert (want[0] == "ok") == (case == "control"), want
    for kw in (dict(), dict(fail_every=2), dict(rc=1)):
        fn = make_inflater(**kw)
        assert _outcome(str(p), inflater=(fn, None)) == want, kw
