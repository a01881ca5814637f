"""Raw-DEFLATE vectors shared by the inflate tests (host core, device kernel).

VALID:   streams zlib accepts; `expect` is zlib.decompress(stream, -15).  The decoder under test must
         answer status 0 and the same bytes.
INVALID: hostile or damaged streams (and wrong sizes).  `expect` is what zlib makes of the stream
         with exactly `isize` bytes of room: the bytes, or None where it refuses.  The rule for
         these is the contract's equivalence: status 0 exactly where zlib accepts, and then the
         same bytes.
Each vector asserts its own first block's BTYPE, so none can silently test something else; the
hand-assembled ones assert the feature they are there for (tests/test_inflate_vector_coverage.py
finds each feature again in the finished streams, with a parser of its own).
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


# ---- bit and block writers (RFC 1951 3.2.4 - 3.2.6): the edges zlib's deflate never emits ---------
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
             227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
              4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def _rev(c, n):  # the low n bits of c, reversed
    return int(format(c, "0%db" % n)[::-1], 2) if n else 0


class BitStream:
    """The bit sink that block writers share, so that a block can start in the middle of a byte.
    marks (kept on request): (kind, bit position, bits) of the fields written, for the structured
    mutations."""

    def __init__(self, marks=False):
        self.acc, self.n, self.out, self.marks = 0, 0, bytearray(), [] if marks else None

    def bits(self, v, n):  # n bits of v, least significant first; whole bytes leave eight at a time
        self.acc |= v << self.n
        self.n += n
        if self.n >= 64:
            self.out += (self.acc & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")
            self.acc >>= 64
            self.n -= 64

    def code(self, c, n):  # a Huffman code: most significant bit first
        self.bits(_rev(c, n), n)

    def pos(self):
        return 8 * len(self.out) + self.n

    def mark(self, kind, nbits=0):
        if self.marks is not None:
            self.marks.append((kind, self.pos(), nbits))

    def align(self):  # zero bits up to the next byte boundary; how many
        pad = -self.n % 8
        self.bits(0, pad)
        self.out += self.acc.to_bytes(self.n // 8, "little")
        self.acc = self.n = 0
        return pad

    def stored(self, data, final=False):
        """A stored block; returns the number of padding bits in front of LEN."""
        self.bits(1 if final else 0, 1)
        self.bits(STORED, 2)
        pad = self.align()
        self.mark("stored_len", 16)
        self.bits(len(data), 16)
        self.bits(len(data) ^ 0xFFFF, 16)
        self.align()
        self.out += data
        return pad

    def finish(self):
        self.align()
        return bytes(self.out)


def len_symbol(length, long258=False):
    """(litlen symbol, extra value) of a match length; long258: 258 as symbol 284 with extra 31."""
    if length == 258:
        return (284, 31) if long258 else (285, 0)
    li = max(i for i in range(28) if _LEN_BASE[i] <= length)
    return 257 + li, length - _LEN_BASE[li]


def dist_symbol(dist):
    di = max(i for i in range(30) if _DIST_BASE[i] <= dist)
    return di, dist - _DIST_BASE[di]


class _BlockWriter:
    """What the fixed and the dynamic writer share: symbols through self.lcode / self.dcode, which
    map a symbol to (code as the stream carries it, bits)."""

    def sym(self, s):
        if self.s.marks is not None:
            self.s.mark("sym")
        self.bits(*self.lcode[s])

    def lit(self, data):
        for b in bytes(data):
            self.bits(*self.lcode[b])

    def raw_match(self, lsym, lextra, dsym, dextra):
        self.sym(lsym)
        n = _LEN_EXTRA[lsym - 257]
        if n:
            self.s.mark("len_extra", n)
            self.bits(lextra, n)
        self.bits(*self.dcode[dsym])
        n = _DIST_EXTRA[dsym]
        if n:
            self.s.mark("dist_extra", n)
            self.bits(dextra, n)

    def match(self, length, dist, long258=False):
        self.raw_match(*(len_symbol(length, long258) + dist_symbol(dist)))

    def close(self):  # end-of-block; the stream stays open for the next block
        self.sym(256)
        self.s.mark("sym")

    def end(self):
        self.close()
        return self.s.finish()


def canonical(lens):
    """{symbol: (bit-reversed code, length)} by RFC 1951 3.2.2; the set need not be complete."""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (_rev(nxt[n] & ((1 << n) - 1), n), n)
            nxt[n] += 1
    return out


def kraft(lens):
    """The code space a set of lengths takes, in units of 2**-15: complete at 32768."""
    return sum(1 << (15 - n) for n in lens if n)


_FIXED_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_LCODE, _FIXED_DCODE = canonical(_FIXED_LENS), canonical([5] * 32)


class FixedWriter(_BlockWriter):
    def __init__(self, final=True, kind=FIXED, stream=None):
        self.s = stream if stream is not None else BitStream()
        self.bits, self.code = self.s.bits, self.s.code
        self.lcode, self.dcode = _FIXED_LCODE, _FIXED_DCODE
        self.bits(1 if final else 0, 1)
        self.bits(kind, 2)


# ---- a dynamic-Huffman block writer (RFC 1951 3.2.7) ----------------------------------------------
_CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
_REP_EXTRA = {16: 2, 17: 3, 18: 7}


def run_length(seq):
    """Greedy code-length symbols [(sym, extra)] for a sequence of code lengths."""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run, i = j - i, j
        if v == 0:
            while run >= 11:
                n = min(run, 138)
                out.append((18, n - 11))
                run -= n
            if run >= 3:
                out.append((17, run - 3))
                run = 0
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                n = min(run, 6)
                out.append((16, n - 3))
                run -= n
        out += [(v, 0)] * run
    return out


def crossing_repeats(cl_syms, hlit):
    """The repeat codes (16/17/18) of a code-length symbol sequence whose run covers lengths on both
    sides of the litlen/distance boundary."""
    have, found = 0, set()
    for sym, extra in cl_syms:
        rep = 1 if sym < 16 else (3 if sym < 18 else 11) + extra
        if sym >= 16 and have < hlit < have + rep:
            found.add(sym)
        have += rep
    return found


def limited_lengths(freq, limit):
    """A complete code of at most `limit` bits over the symbols with freq > 0 (two at the least:
    a single symbol gets a partner).  Starts flat and shortens the frequent symbols while the code
    space allows; not optimal, always complete."""
    used = sorted((s for s, f in enumerate(freq) if f), key=lambda s: -freq[s])
    if len(used) == 1:
        used.append((used[0] + 1) % len(freq))
    flat = (len(used) - 1).bit_length()
    assert 1 <= flat <= limit
    lens = {s: flat for s in used}
    space = lambda: sum(1 << (limit - n) for n in lens.values())
    moved = True
    while moved:
        moved = False
        for s in used:
            while lens[s] > 1 and space() + (1 << (limit - lens[s])) <= 1 << limit:
                lens[s] -= 1
                moved = True
    assert space() == 1 << limit
    return [lens.get(s, 0) for s in range(len(freq))]


class DynWriter(_BlockWriter):
    """litlens / distlens: code lengths by symbol.  hlit / hdist: how many of each the header carries
    (default: up to the last used symbol, 257 / 1 at the least).  cl_syms: the code-length symbols
    [(sym, extra)] (default: greedy run lengths over litlen + distance as ONE sequence when `cross`,
    over each of them when not).  cl_lens: the code-length code's 19 lengths (default: a complete
    code of at most 7 bits over the symbols cl_syms uses).  hclen: how many of them the header
    carries (default: up to the last non-zero one in header order, 4 at the least).  hdr_delta:
    (index, d) adds d to the header's length `index` of the sequence only: the symbols are still
    written with the codes of the lengths given, which is what a damaged header looks like."""

    def __init__(self, litlens, distlens, hlit=None, hdist=None, hclen=None, cl_lens=None, cl_syms=None, cross=True,
                 final=True, stream=None, hdr_delta=None):
        self.s = stream if stream is not None else BitStream()
        self.bits, self.code = self.s.bits, self.s.code
        last = lambda a: max([i + 1 for i, n in enumerate(a) if n], default=0)
        self.hlit = max(257, last(litlens)) if hlit is None else hlit
        self.hdist = max(1, last(distlens)) if hdist is None else hdist
        assert last(litlens) <= self.hlit and last(distlens) <= self.hdist
        lit = (list(litlens) + [0] * 288)[:self.hlit]
        dist = (list(distlens) + [0] * 32)[:self.hdist]
        self.litlens, self.distlens = lit, dist
        self.lcode, self.dcode = canonical(lit), canonical(dist)
        if cl_syms is None:
            seq = lit + dist
            if hdr_delta is not None:
                seq[hdr_delta[0]] = min(15, max(0, seq[hdr_delta[0]] + hdr_delta[1]))
            cl_syms = run_length(seq) if cross else run_length(seq[:self.hlit]) + run_length(seq[self.hlit:])
        self.cl_syms = cl_syms
        self.crossing = crossing_repeats(cl_syms, self.hlit)
        if cl_lens is None:
            freq = [0] * 19
            for sym, _ in cl_syms:
                freq[sym] += 1
            cl_lens = limited_lengths(freq, 7)
        self.cl_lens = cl_lens
        need = max([i + 1 for i in range(19) if cl_lens[_CLEN_ORDER[i]]], default=0)
        self.hclen = max(4, need) if hclen is None else hclen
        assert need <= self.hclen <= 19
        self.bits(1 if final else 0, 1)
        self.bits(DYNAMIC, 2)
        for name, v, n in (("hlit", self.hlit - 257, 5), ("hdist", self.hdist - 1, 5), ("hclen", self.hclen - 4, 4)):
            assert 0 <= v < 1 << n
            self.s.mark(name, n)
            self.bits(v, n)
        for i in range(self.hclen):
            self.s.mark("cl_len", 3)
            self.bits(cl_lens[_CLEN_ORDER[i]], 3)
        clcode = canonical(cl_lens)
        for sym, extra in cl_syms:
            self.s.mark("cl_sym")
            self.bits(*clcode[sym])
            if sym >= 16:
                self.s.mark("rep_extra", _REP_EXTRA[sym])
                self.bits(extra, _REP_EXTRA[sym])


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
    _dynamic_edges(add, rnd)
    _stored_edges(add, rnd)
    named = len(v)
    for name, stream in _fuzz_valid():
        v.append(Vec(name, stream, None, zlib.decompress(stream, -15)))
    FUZZ_NAMES.extend(x.name for x in v[named:])
    assert sum(len(x.comp) for x in v[named:]) < 1 << 20
    return [Vec(x.name, x.comp, len(x.expect), x.expect) for x in v]


def flat_lens(symbols, n):
    """n code lengths: a complete code over `symbols` (two or more), as flat as it can be."""
    m = len(symbols)
    k = m.bit_length() - 1
    lens = [0] * n
    for i, s in enumerate(symbols):
        lens[s] = k if i < (2 << k) - m else k + 1
    assert kraft(lens) == 32768
    return lens


def _max_bits_sets():
    """litlen lengths 1..15,15 over 13 literals, 256, 285, 284; distance lengths 1..15,15 over
    symbols 0..13, 28, 29: both tables at 15 bits, the longest codes on the symbols with the most
    extra bits."""
    lits = list(b"ACGTNacgtn=#!")
    lit, dist = [0] * 286, [0] * 30
    for n, s in enumerate(lits + [256, 285, 284], 1):
        lit[s] = min(n, 15)
    for n, s in enumerate(list(range(14)) + [28, 29], 1):
        dist[s] = min(n, 15)
    assert kraft(lit) == 32768 and kraft(dist) == 32768 and lit[284] == 15 and dist[29] == 15
    return lits, lit, dist


def _many_15bit_sets():
    """seven litlen codes of 1..7 bits and 256 of 15 bits (252 of them literals): the ballot ranks
    of one length run over five 64-lane passes, the canonical walk indexes sorted[] beyond 256."""
    lit = [15] * 252 + [0] * 34
    for n, s in enumerate((252, 257, 253, 258, 254, 265, 255), 1):
        lit[s] = n
    for s in (256, 270, 280, 285):
        lit[s] = 15
    assert kraft(lit) == 32768 and lit.count(15) == 256
    return lit, [2, 2, 2, 2]


def _repeat_crosses_sets():
    lit, dist = [9] * 172 + [8] * 106 + [5] * 8, [5] * 28 + [4] * 2
    assert kraft(lit) == 32768 and kraft(dist) == 32768
    return lit, dist


def _random_symbols(rnd, w, at, goal, lits, lsyms, dsyms, pmatch):
    """Literals and matches drawn from the given symbols until `goal` output bytes; valid by
    construction: a distance never reaches before the stream's first byte."""
    while at < goal:
        if lsyms and at and rnd.random() < pmatch:
            ls = rnd.choice(lsyms)
            lextra = rnd.getrandbits(_LEN_EXTRA[ls - 257]) if _LEN_EXTRA[ls - 257] else 0
            length = _LEN_BASE[ls - 257] + lextra
            ds = [d for d in dsyms if _DIST_BASE[d] <= at]
            if ds and length <= goal - at:
                d = rnd.choice(ds)
                dextra = rnd.getrandbits(_DIST_EXTRA[d]) if _DIST_EXTRA[d] else 0
                w.raw_match(ls, lextra, d, min(dextra, at - _DIST_BASE[d]))
                at += length
                continue
        w.sym(rnd.choice(lits))
        at += 1
    return at


def _dynamic_edges(add, rnd):
    """Dynamic-Huffman headers and codes no encoder emits."""
    lits, lit, dist = _max_bits_sets()
    w = DynWriter(lit, dist)
    w.lit(bytes(rnd.choice(lits) for _ in range(33000)))
    for d in _DIST_BASE[:14]:  # every distance code of 1..14 bits; 284 and 285 are the only lengths
        w.match(227 + d % 7, d)
    w.match(257, 32768)  # a 15-bit code + 5 extra bits, then a 15-bit code + 13 extra bits, all ones
    w.match(258, 32768)
    w.match(230, 24577)
    w.match(258, 32768, long258=True)  # 258 as 284 + 31: every bit of both extra fields set
    w.match(258, 1, long258=True)
    for _ in range(40):  # the 48-bit worst case again behind codes of 1..13 bits: other positions in the word
        w.lit(bytes(rnd.choice(lits) for _ in range(rnd.randint(1, 3))))
        w.match(258, 32768, long258=True)
    add("max_bits", w.end(), DYNAMIC)

    # neighbours in the list (and so on one wave after each other when the list is cycled): no
    # distance code, 256 codes of 15 bits, a single distance code
    w = DynWriter(flat_lens(list(range(64, 128)) + [256], 257), [0], hdist=1)
    assert kraft(w.distlens) == 0
    w.lit(bytes(rnd.randrange(64, 128) for _ in range(700)))
    add("no_dist_code", w.end(), DYNAMIC)
    lit, dist = _many_15bit_sets()
    w = DynWriter(lit, dist)
    _random_symbols(rnd, w, 0, 4000, list(range(252)), [257, 258, 265], [0, 1, 2, 3], 0.1)
    add("many_15bit", w.end(), DYNAMIC)
    lit = flat_lens(list(b"abcdefgh") + [256, 257, 258, 259, 264, 270, 285], 286)
    w = DynWriter(lit, [1])
    assert w.hdist == 1 and kraft(w.distlens) == 16384
    w.lit(b"abcdefgh")
    for n in (3, 4, 5, 10, 23, 258, 3):
        w.match(n, 1)
        w.lit(b"hgf")
    one_dist_code = w.end()
    add("one_dist_code", one_dist_code, DYNAMIC)
    w = DynWriter(lit, [0, 0, 0, 0, 0, 1])
    assert w.hdist == 6 and kraft(w.distlens) == 16384
    w.lit(b"abcdefgh")
    for n, d in ((3, 7), (4, 8), (258, 8), (10, 7), (5, 8)):
        w.match(n, d)
        w.lit(b"dc")
    add("one_dist_code_sym5", w.end(), DYNAMIC)
    w = DynWriter([0] * 256 + [1], [0])  # and the litlen set that is one code: end-of-block alone
    assert kraft(w.litlens) == 16384
    add("only_eob_code", w.end(), DYNAMIC)
    assert zlib.decompress(w.s.finish(), -15) == b""

    # 257 codes of 8..10 bits in front of longer ones: the canonical walk (codes longer than the
    # primary table's index) reads sorted[257] and beyond
    lit = [8] * 255 + [9, 10, 11, 12, 13, 14, 15, 15]
    assert kraft(lit) == 32768
    w = DynWriter(lit, [2, 2, 2, 2])
    for _ in range(60):
        w.lit(bytes(rnd.getrandbits(8) for _ in range(rnd.randint(1, 9))))
        w.match(rnd.randint(3, 8), rnd.randint(1, 4))
    add("walk_past_256", w.end(), DYNAMIC)

    lit, dist = _repeat_crosses_sets()
    w = DynWriter(lit, dist)
    assert w.crossing == {16}
    _random_symbols(rnd, w, 0, 6000, list(range(256)), list(range(257, 286)), list(range(30)), 0.08)
    add("repeat_crosses", w.end(), DYNAMIC)
    w = DynWriter(lit, dist, cross=False)
    assert not w.crossing
    _random_symbols(rnd, w, 0, 1500, list(range(256)), list(range(257, 286)), list(range(30)), 0.08)
    add("repeat_stops_at_boundary", w.end(), DYNAMIC)
    # 26 trailing litlen zeros and 20 leading distance zeros: one code-18 run of 46
    w = DynWriter(flat_lens(list(range(256)) + [256, 257, 258, 259], 286), [0] * 20 + [1, 1], hlit=286)
    assert w.hlit == 286 and w.hdist == 22 and w.crossing == {18} and (18, 46 - 11) in w.cl_syms
    w.lit(bytes(rnd.getrandbits(8) for _ in range(1600)))
    for n, d in ((3, 1025), (4, 1536), (5, 1537), (3, 1600)):
        w.match(n, d)
    add("zero_run_crosses", w.end(), DYNAMIC)
    # 3 trailing litlen zeros and 4 leading distance zeros: one code-17 run of 7
    w = DynWriter(flat_lens(list(range(256)) + list(range(256, 283)), 286), [0] * 4 + [1, 1], hlit=286)
    assert w.hlit == 286 and w.hdist == 6 and w.crossing == {17} and (17, 7 - 3) in w.cl_syms
    w.lit(bytes(rnd.getrandbits(8) for _ in range(300)))
    for n, d in ((3, 5), (30, 6), (100, 7), (194, 8)):
        w.match(n, d)
    add("zero_run_crosses_17", w.end(), DYNAMIC)

    # HCLEN 5: only 16, 17, 18, 0 and 8 can have a code.  255 literals and end-of-block at 8 bits.
    cl = [0] * 19
    cl[8], cl[0], cl[16] = 1, 2, 2
    w = DynWriter([8] * 255 + [0, 8], [0], cl_lens=cl)
    assert w.hclen == 5 and w.hlit == 257 and kraft(w.litlens) == 32768
    w.lit(bytes(rnd.randrange(255) for _ in range(900)))
    add("hclen5", w.end(), DYNAMIC)
    # a code-length code of 1,2,...,7,7 bits: eight code-length symbols, no repeat codes
    lit = [0] * 258
    for n, s in zip((1, 2, 3, 4, 5, 6, 7, 7), list(b"ACGTN") + [256, 257, 35]):
        lit[s] = n
    cl = [0] * 19
    for n, s in zip((1, 2, 3, 4, 5, 6, 7, 7), (0, 1, 2, 3, 4, 5, 6, 7)):
        cl[s] = n
    w = DynWriter(lit, [1], cl_lens=cl, cl_syms=[(n, 0) for n in lit + [1]])
    assert kraft(lit) == 32768 and sum(1 << (7 - n) for n in cl if n) == 128 and w.hclen == 18
    w.lit(bytes(rnd.choice(b"AAAACCGTN#") for _ in range(500)))
    w.match(3, 1)
    add("clen_7bit", w.end(), DYNAMIC)

    # three dynamic blocks with very different code sets and a stored block, none but the one after
    # the stored block (which cannot) starting on a byte boundary: the tables of the block before
    s = BitStream()
    FixedWriter(final=False, stream=s).close()
    starts = [s.pos()]
    lits, lit, dist = _max_bits_sets()
    w = DynWriter(lit, dist, final=False, stream=s)
    w.lit(bytes(rnd.choice(lits) for _ in range(800)))
    w.match(257, 100)
    w.close()
    starts.append(s.pos())
    lit, dist = _many_15bit_sets()
    w = DynWriter(lit, dist, final=False, stream=s)
    at = _random_symbols(rnd, w, 1057, 2500, list(range(252)), [257, 258, 265], [0, 1, 2, 3], 0.1)
    w.close()
    starts.append(s.pos())
    s.stored(bytes(rnd.getrandbits(8) for _ in range(77)))
    lit, dist = _repeat_crosses_sets()
    w = DynWriter(lit, dist, stream=s)
    _random_symbols(rnd, w, at + 77, 5000, list(range(256)), list(range(257, 286)), list(range(30)), 0.1)
    assert all(p % 8 for p in starts), starts
    add("dyn_dyn_stored_dyn", w.end(), FIXED)


def _stored_edges(add, rnd):
    """Stored blocks behind compressed ones at every bit alignment, matches into stored bytes."""
    pads = set()
    for k in range(8):
        s = BitStream()
        w = FixedWriter(final=False, stream=s)
        w.lit(bytes(rnd.randrange(144, 256) for _ in range(k)) + b"ab")  # k nine-bit codes
        w.close()
        raw = bytes(rnd.getrandbits(8) for _ in range(300))
        pads.add(s.stored(raw))
        w = FixedWriter(stream=s)
        w.lit(b"QQQQQ")
        w.match(258, 300)
        w.match(3, 1)
        w.match(200, 310)
        add("stored_align_%d" % k, w.end(), FIXED)
    assert pads == set(range(8))
    # a full 64-byte literal buffer and 6 pending, an empty stored block, a 65-byte one, matches back
    s = BitStream()
    w = FixedWriter(final=False, stream=s)
    w.lit(bytes(rnd.getrandbits(8) for _ in range(70)))
    w.close()
    s.stored(b"")
    s.stored(bytes(rnd.getrandbits(8) for _ in range(65)))
    w = FixedWriter(stream=s)
    w.match(64, 65)
    w.match(130, 1)
    add("lit70_empty_stored_stored65", w.end(), FIXED)


# ---- structured fuzz: random code sets, headers and block mixes, valid by construction -----------
FUZZ_NAMES = []
_FUZZ_STREAMS, _FUZZ_BIG, _FUZZ_MUTATED = 300, (65535, 65536, 65535, 65536), 40


def random_code(rnd, n, maxbits, tail):
    """The n >= 2 code lengths of a random complete set: leaves of a binary tree split at random,
    the deepest one with probability `tail` (long-tailed sets reach maxbits)."""
    count = [0] * (maxbits + 1)
    count[1] = 2
    for _ in range(n - 2):
        deep = [d for d in range(1, maxbits) if count[d]]
        d = deep[-1] if rnd.random() < tail else rnd.choices(deep, [count[d] for d in deep])[0]
        count[d] -= 1
        count[d + 1] += 2
    lens = [d for d in range(1, maxbits + 1) for _ in range(count[d])]
    rnd.shuffle(lens)
    assert len(lens) == n and kraft(lens) == 32768
    return lens


def _fuzz_dynamic(rnd, s, final, want_matches, hdr_delta):
    """A dynamic block header with random sets; returns (writer, literals, length symbols, distance symbols)."""
    nlit = rnd.choice((1, 2, 5, 20, 80, 200, 256))
    nlen = rnd.choice((1, 3, 29) if want_matches else (0, 0, 1, 3, 10, 29))
    lits, lsyms = rnd.sample(range(256), nlit), rnd.sample(range(257, 286), nlen)
    ndist = rnd.choice((1, 2, 8, 30) if want_matches else (0, 1, 1, 2, 3, 8, 20, 30)) if nlen else rnd.choice((0, 0, 1, 4))
    dsyms = [0] if want_matches and ndist == 1 else rnd.sample(range(30), ndist)
    lit, dist = [0] * 286, [0] * 30
    used = lits + [256] + lsyms
    for sym, n in zip(used, random_code(rnd, len(used), 15, rnd.choice((0.0, 0.2, 0.6, 0.9)))):
        lit[sym] = n
    if ndist == 1:
        dist[dsyms[0]] = 1
    elif ndist:
        for sym, n in zip(dsyms, random_code(rnd, ndist, 15, rnd.choice((0.0, 0.3, 0.8, 1.0)))):
            dist[sym] = n
    hlit = rnd.randint(max(257, max(used) + 1), 286)
    hdist = rnd.randint(max([1] + [d + 1 for d in dsyms]), 30)
    cross, seed = rnd.random() < 0.5, rnd.getrandbits(32)
    if hdr_delta is not None:
        hdr_delta = (int(hdr_delta[0] * (hlit + hdist)), hdr_delta[1])
    w = DynWriter(lit, dist, hlit=hlit, hdist=hdist, cross=cross, final=final, stream=BitStream(), hdr_delta=hdr_delta)
    # the same header again into the stream, now with a random code-length code and HCLEN
    sub, cl = random.Random(seed), [0] * 19
    csyms = sorted(set(sym for sym, _ in w.cl_syms))
    if len(csyms) == 1:
        csyms.append((csyms[0] + 1) % 19)
    for sym, n in zip(csyms, random_code(sub, len(csyms), 7, sub.choice((0.0, 0.5, 1.0)))):
        cl[sym] = n
    need = max(i + 1 for i in range(19) if cl[_CLEN_ORDER[i]])
    w = DynWriter(lit, dist, hlit=hlit, hdist=hdist, cl_lens=cl, cl_syms=w.cl_syms, hclen=sub.randint(max(4, need), 19),
                  final=final, stream=s)
    return w, lits, lsyms, dsyms


def fuzz_stream(seed, size, hdr_delta=None, marks=False):
    """(stream, marks, dynamic blocks): 1..4 blocks of mixed types, `size` output bytes.  hdr_delta
    = (dynamic block, position in 0..1, d) damages one code length of that block's header."""
    rnd = random.Random(seed)
    s, at, ndyn = BitStream(marks), 0, 0
    nblocks = rnd.randint(1, 4)
    goals = sorted(rnd.randint(0, size) for _ in range(nblocks - 1)) + [size]
    big = size > 4096
    pmatch = 0.9 if big else rnd.choice((0.0, 0.05, 0.3, 0.9))
    for k, goal in enumerate(goals):
        final = k == nblocks - 1
        kind = rnd.choice((DYNAMIC, DYNAMIC, DYNAMIC, FIXED, STORED))
        if kind == STORED and goal - at <= (4096 if big else 65535):
            s.stored(bytes(rnd.getrandbits(8) for _ in range(goal - at)), final)
            at = goal
            continue
        if kind == DYNAMIC:
            delta = None
            if hdr_delta is not None and hdr_delta[0] == ndyn:
                delta = hdr_delta[1:]
            w, lits, lsyms, dsyms = _fuzz_dynamic(rnd, s, final, big, delta)
            ndyn += 1
        else:
            w, lits, lsyms, dsyms = FixedWriter(final, stream=s), range(256), range(257, 286), range(30)
        at = _random_symbols(rnd, w, at, goal, lits, lsyms, dsyms, pmatch)
        w.close()
    return s.finish(), s.marks, ndyn


def _fuzz_valid():
    rnd = random.Random(3951)
    for i in range(_FUZZ_STREAMS + len(_FUZZ_BIG)):
        size = rnd.randint(0, 4096) if i < _FUZZ_STREAMS else _FUZZ_BIG[i - _FUZZ_STREAMS]
        stream, _, _ = fuzz_stream(i, size)
        assert zlib_verdict(stream, size) is not None, i
        yield "fuzz_%d_%d" % (i, size), stream


def patch_field(stream, pos, nbits, d):
    """The stream with d added to the nbits-wide field at bit position pos (modulo the field)."""
    x = int.from_bytes(stream, "little")
    v = (x >> pos) & ((1 << nbits) - 1)
    x ^= (v ^ ((v + d) & ((1 << nbits) - 1))) << pos
    return x.to_bytes(len(stream), "little")


def _fuzz_mutations(add, fuzz):
    """Single-field damage in the structured parts of the first fuzz streams: what zlib makes of
    each is the verdict, so some stay valid (another distance of the same code, say)."""
    rnd = random.Random(7951)
    for i in range(_FUZZ_MUTATED):
        size = fuzz[i].isize
        stream, marks, ndyn = fuzz_stream(i, size, marks=True)
        assert stream == fuzz[i].comp
        pick = lambda kinds: [m for m in marks if m[0] in kinds and m[2]]
        for rep in range(2):
            if ndyn:  # one code length of a dynamic header, one up or down
                hd = (rnd.randrange(ndyn), rnd.random(), rnd.choice((-1, 1)))
                add("fuzz_%d_codelen_%d" % (i, rep), fuzz_stream(i, size, hd)[0], size)
            for what, kinds in (("header", ("hlit", "hdist", "hclen", "cl_len", "stored_len")),
                                ("extra", ("rep_extra", "len_extra", "dist_extra"))):
                fields = pick(kinds)
                if fields:
                    _, pos, nbits = rnd.choice(fields)
                    add("fuzz_%d_%s_%d" % (i, what, rep), patch_field(stream, pos, nbits, rnd.choice((-1, 1))), size)
            cuts = [m[1] for m in marks if m[0] in ("sym", "cl_sym")]
            if cuts:  # the stream cut at a symbol boundary (to the byte that holds it)
                add("fuzz_%d_cut_%d" % (i, rep), stream[:(rnd.choice(cuts) + 7) // 8], size)


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
    _named_invalid(add)
    assert [x.name for x in v[-len(NAMED_INVALID) + 3:]] == list(NAMED_INVALID[3:])
    _fuzz_mutations(add, [by[name] for name in FUZZ_NAMES])
    return v


def zlib_complaint(stream):
    """zlib's own words for why it refuses a stream."""
    try:
        zlib.decompressobj(-15).decompress(stream)
    except zlib.error as e:
        return str(e)
    return ""


NAMED_INVALID = ("distance_before_start", "btype3", "stored_bad_nlen", "litlen_oversubscribed", "litlen_incomplete",
                 "no_end_of_block_code", "two_dist_codes_incomplete", "one_dist_code_of_2_bits", "hclen4",
                 "repeat_16_first", "repeat_past_the_end", "hlit_30", "hdist_30", "one_clen_code", "fixed_litlen_286",
                 "fixed_dist_30", "one_dist_code_missing_half")


def _named_invalid(add0):
    """Streams that zlib refuses, each for the reason its name gives."""
    def add(name, stream, why, isize=3):
        assert why in zlib_complaint(stream), (name, zlib_complaint(stream))
        add0(name, stream, isize)
        assert zlib_verdict(stream, isize) is None

    def body(w, eob=True):
        w.lit(b"abc")
        return w.end() if eob else w.s.finish()

    lit8 = [8] * 255 + [0, 8]  # complete: 255 literals and end-of-block
    add("litlen_oversubscribed", body(DynWriter([8] * 257, [1])), "invalid literal/lengths set")
    assert kraft([8] * 257) == 32768 + 128
    add("litlen_incomplete", body(DynWriter([8] * 254 + [0, 0, 8], [1])), "invalid literal/lengths set")
    add("no_end_of_block_code", body(DynWriter([8] * 256, [1], hlit=257), eob=False), "missing end-of-block")
    add("two_dist_codes_incomplete", body(DynWriter(lit8, [1, 2])), "invalid distances set")
    add("one_dist_code_of_2_bits", body(DynWriter(lit8, [2])), "invalid distances set")
    # HCLEN 4: only 16, 17, 18 and 0 can have a code, so no symbol can get a length
    cl = [0] * 19
    cl[18], cl[0] = 1, 1
    w = DynWriter([], [], cl_lens=cl, cl_syms=[(18, 127), (18, 120 - 11)])
    assert w.hclen == 4
    add("hclen4", w.s.finish(), "missing end-of-block")
    cl = [0] * 19
    cl[16], cl[8], cl[0] = 1, 2, 2
    w = DynWriter(lit8, [0], cl_lens=cl, cl_syms=[(16, 3)] + [(8, 0)] * 249 + [(0, 0), (8, 0), (0, 0)])
    add("repeat_16_first", body(w), "invalid bit length repeat")
    w = DynWriter(lit8, [0], cl_lens=cl, cl_syms=[(8, 0)] + [(16, 3)] * 42 + [(8, 0), (8, 0), (0, 0), (8, 0), (16, 0)])
    add("repeat_past_the_end", body(w), "invalid bit length repeat")
    add("hlit_30", body(DynWriter(lit8, [1], hlit=287)), "too many length or distance symbols")
    add("hdist_30", body(DynWriter(lit8, [1], hdist=31)), "too many length or distance symbols")
    cl = [0] * 19
    cl[18] = 1
    w = DynWriter([], [], cl_lens=cl, cl_syms=[(18, 127), (18, 120 - 11)])
    add("one_clen_code", w.s.finish(), "invalid code lengths set")
    w = FixedWriter()
    w.lit(b"abc")
    w.sym(286)
    add("fixed_litlen_286", w.end(), "invalid literal/length code")
    w = FixedWriter()
    w.lit(b"abc")
    w.sym(257)
    w.code(30, 5)
    add("fixed_dist_30", w.end(), "invalid distance code", 6)
    # one_dist_code's set (a single distance code, '0'): the bit that is no code
    w = DynWriter(flat_lens(list(b"abcdefgh") + [256, 257, 258, 259, 264, 270, 285], 286), [1])
    w.lit(b"abcdefgh")
    w.match(3, 1)
    w.sym(258)
    w.bits(1, 1)
    add("one_dist_code_missing_half", w.end(), "invalid distance code", 15)


VALID = _valid()
INVALID = _invalid(VALID)


def check_rule(vec, status, out):
    """The rule every vector obeys, in both directions: accepted exactly where zlib accepts."""
    if vec.expect is None:
        assert status != 0, "%s: accepted, zlib refuses" % vec.name
    else:
        assert status == 0, "%s: refused with status %d, zlib accepts" % (vec.name, status)
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
