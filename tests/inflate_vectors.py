"""Raw-DEFLATE vectors shared by the inflate tests (host core, device kernel).

VALID:   streams zlib accepts; `expect` is zlib.decompress(stream, -15).  The decoder under test must
         answer status 0 and the same bytes.
INVALID: hostile or damaged streams (and wrong sizes).  `expect` is what zlib makes of the stream
         with exactly `isize` bytes of room: the bytes, or None where it refuses.  The rule for
         these: status 0 => zlib accepts too and the bytes are equal.
Each vector asserts its own first block's BTYPE, so none can silently test something else.
"""
import gzip
import os
import random
import struct
import zlib
from collections import namedtuple

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Vec = namedtuple("Vec", "name comp isize expect")

STORED, FIXED, DYNAMIC = 0, 1, 2


def btype(stream):
    return (stream[0] >> 1) & 3


def deflate(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def zlib_verdict(stream, isize):
    """What zlib's inflate gives with room for exactly isize bytes: the bytes, or None."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream, isize + 1)
    except zlib.error:
        return None
    if not d.eof or len(out) != isize:
        return None
    return out


# ---- a fixed-Huffman bit writer (RFC 1951 3.2.6): the edges zlib's deflate never emits ------------
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
             227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
              4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class FixedWriter:
    def __init__(self, final=True, kind=FIXED):
        self.acc, self.n, self.out = 0, 0, bytearray()
        self.bits(1 if final else 0, 1)
        self.bits(kind, 2)

    def bits(self, v, n):  # n bits of v, least significant first
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):  # a Huffman code: most significant bit first
        self.bits(int(format(c, "0%db" % n)[::-1], 2), n)

    def sym(self, s):
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def lit(self, data):
        for b in bytes(data):
            self.sym(b)

    def match(self, length, dist):
        li = max(i for i in range(29) if _LEN_BASE[i] <= length and (i != 28 or length == 258))
        if length == 258:
            li = 28
        self.sym(257 + li)
        self.bits(length - _LEN_BASE[li], _LEN_EXTRA[li])
        di = max(i for i in range(30) if _DIST_BASE[i] <= dist)
        self.code(di, 5)
        self.bits(dist - _DIST_BASE[di], _DIST_EXTRA[di])

    def end(self):
        self.sym(256)
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)


def _mixed_bytes():
    with gzip.open(os.path.join(REPO, "tests", "golden", "mixed.bam"), "rb") as f:
        return f.read()


def _valid():
    rnd = random.Random(1951)
    v = []

    def add(name, stream, kind):
        assert btype(stream) == kind, (name, btype(stream))
        v.append(Vec(name, stream, None, zlib.decompress(stream, -15)))

    period = bytes((i * 7 + 3) % 251 for i in range(100)) * 50  # 5,000 bytes of period 100
    add("stored", deflate(period, 0), STORED)
    for lvl in (1, 6, 9):
        add("period_l%d" % lvl, deflate(period, lvl), FIXED)
    add("period_fixed", deflate(period, 6, zlib.Z_FIXED), FIXED)
    skew = bytes(rnd.choice(b"AAAAAAAACCCCGGGTTN#IIIIJJ!5") for _ in range(20000))
    add("huffman_only", deflate(skew, 6, zlib.Z_HUFFMAN_ONLY), DYNAMIC)
    runs = b"".join(bytes([rnd.choice(b"ACGT")]) * rnd.randint(1, 40) for _ in range(1500))
    add("rle", deflate(runs, 6, zlib.Z_RLE), DYNAMIC)
    mixed = _mixed_bytes()[:65536]
    for lvl in (1, 6, 9):
        add("mixed_l%d" % lvl, deflate(mixed, lvl), DYNAMIC)
    # several deflate blocks per BGZF block, empty stored blocks, non-byte-aligned starts
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    s = c.compress(mixed[:3000]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(skew[:700]) + c.flush(zlib.Z_SYNC_FLUSH)
    s += c.compress(period[:900]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(mixed[3000:9000]) + c.flush()
    add("flushes", s, DYNAMIC)
    # sizes around the wave width and at the BGZF limit
    body = bytes(rnd.choice(b"ACGTACGTACGTNNIIII#5") for _ in range(65536))
    for n in (1, 2, 63, 64, 65, 65535, 65536):
        add("size_%d_l6" % n, deflate(body[:n], 6), FIXED if n <= 2 else DYNAMIC)
        add("size_%d_l0" % n, deflate(body[:n], 0), STORED)
    add("eof_block", b"\x03\x00", FIXED)
    assert v[-1].expect == b""

    # hand-assembled fixed-Huffman streams
    w = FixedWriter()
    far = bytes(rnd.getrandbits(8) for _ in range(32768))
    w.lit(far)
    rem = 32768
    while rem:
        n = min(258, rem)
        if 0 < rem - n < 3:
            n = rem - 3
        w.match(n, 32768)
        rem -= n
    add("dist_32768", w.end(), FIXED)
    assert v[-1].expect == far + far
    w = FixedWriter()
    w.lit(b"x")
    w.match(258, 1)
    w.match(3, 1)
    add("rle_258_3", w.end(), FIXED)
    assert v[-1].expect == b"x" * 262
    w = FixedWriter()
    w.lit(bytes(rnd.getrandbits(8) for _ in range(65)))
    for dist in (2, 3, 63, 64, 65):
        for n in (3, 64, 65, 258):
            w.match(n, dist)
    add("overlaps", w.end(), FIXED)
    w = FixedWriter()
    w.lit(b"abcd")
    w.match(4, 4)
    add("match_to_the_end", w.end(), FIXED)
    assert v[-1].expect == b"abcdabcd"
    return [Vec(x.name, x.comp, len(x.expect), x.expect) for x in v]


def _invalid(valid):
    by = {x.name: x for x in valid}
    v = []

    def add(name, stream, isize):
        v.append(Vec(name, stream, isize, zlib_verdict(stream, isize)))

    w = FixedWriter()
    w.lit(b"x")
    w.match(3, 2)
    add("distance_before_start", w.end(), 4)
    assert v[-1].expect is None
    add("btype3", b"\x07\x00", 0)
    assert btype(b"\x07") == 3 and v[-1].expect is None
    add("stored_bad_nlen", b"\x01\x05\x00\xfb\xff" + b"hello", 5)
    assert v[-1].expect is None and zlib_verdict(b"\x01\x05\x00\xfa\xff" + b"hello", 5) == b"hello"
    short = [by["size_65_l6"], by["flushes"], by["size_64_l0"]]
    dyn = deflate(_mixed_bytes()[:1500], 9)
    assert btype(dyn) == DYNAMIC
    short[1] = Vec("short_dynamic", dyn, 1500, zlib.decompress(dyn, -15))
    for x in short[:2]:
        for n in range(len(x.comp)):
            add("%s_prefix_%d" % (x.name, n), x.comp[:n], x.isize)
    for x in list(valid[:12]) + short:
        add(x.name + "_isize_minus", x.comp, x.isize - 1) if x.isize else None
        add(x.name + "_isize_plus", x.comp, x.isize + 1)
    for x in short:
        for bit in range(8 * min(64, len(x.comp))):
            s = bytearray(x.comp)
            s[bit >> 3] ^= 1 << (bit & 7)
            add("%s_flip_%d" % (x.name, bit), bytes(s), x.isize)
    return v


VALID = _valid()
INVALID = _invalid(VALID)


def check_rule(vec, status, out):
    """The rule every vector obeys; the valid ones the other direction too."""
    if status == 0:
        assert vec.expect is not None, "%s: accepted, zlib refuses" % vec.name
        assert bytes(out) == vec.expect, "%s: bytes differ from zlib's" % vec.name


def pack_file(vecs):
    """The input of tests/native/inflate_check.cpp."""
    parts = [struct.pack("<I", len(vecs))]
    for x in vecs:
        parts.append(struct.pack("<II", len(x.comp), x.isize))
        parts.append(x.comp)
    return b"".join(parts)


def unpack_results(blob, vecs):
    """[(status, guards_ok, bytes)] from inflate_check's output."""
    res, q = [], 0
    for x in vecs:
        res.append((blob[q], blob[q + 1], blob[q + 2:q + 2 + x.isize]))
        q += 2 + x.isize
    assert q == len(blob)
    return res
