"""Inputs of the BAM record decode tests (bc_bam.h on the host, bc_bam.hip on the device): a BAM
builder that controls every record's byte offset, the synthetic layout and trap files, the refusal
buffers, and the file formats of tests/native/bamdecode_check.cpp.

Offsets here come from the builder's own arithmetic (``Builder.starts``), never from a decoder."""
import gzip
import os
import struct
import zlib

import numpy as np

SEGS = (256, 1024, 0)  # seg_bytes of the tests; 0 = the default
DEFAULT_SEG = 65536
LIMITS = (1, 3, -1)  # max_records; -1 = no limit
REFS = (("chrA", 400_000), ("chrB", 50_000))
ARRAYS = ("tid", "pos", "flag", "mapq", "l_seq", "qstart", "qend", "rec_err", "ref_span", "cig_off", "seq_off",
          "cigar", "seq", "seq_event", "qual")
DTYPES = {"tid": np.int32, "pos": np.int32, "flag": np.uint16, "mapq": np.uint8, "l_seq": np.int32,
          "qstart": np.int32, "qend": np.int32, "rec_err": np.uint32, "ref_span": np.int64, "cig_off": np.uint64,
          "seq_off": np.uint64, "cigar": np.uint32, "seq": np.uint8, "seq_event": np.uint8, "qual": np.uint8}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_BAMS = {"c1": "c1.bam", "edge": "edge.bam", "mixed": "mixed.bam", "ont": os.path.join("ont", "ont.bam")}


# ---- bytes ----
def bam_header(refs=REFS) -> bytes:
    h = b"BAM\1" + struct.pack("<i", 0) + struct.pack("<i", len(refs))
    for name, ln in refs:
        nm = name.encode() + b"\0"
        h += struct.pack("<i", len(nm)) + nm + struct.pack("<i", ln)
    return h


def record(tid=0, pos=0, mapq=60, flag=0, name=b"r", cigar=(), seq=None, l_seq=None, qual=None, aux=b"",
           block_size=None) -> bytes:
    """One serialized alignment.  cigar: (op, len) pairs; seq: 4-bit codes per base (default: a
    pattern of l_seq bases); qual: l_seq bytes (default a pattern; b"" keeps whatever l_seq says).
    l_seq / block_size override the written fields (for the refusal buffers)."""
    if seq is None:
        seq = (np.arange(l_seq or 0) * 7 % 16).astype(np.uint8) if l_seq and l_seq > 0 else np.zeros(0, np.uint8)
    seq = np.asarray(seq, np.uint8)
    n = seq.size
    pad = np.concatenate([seq, np.zeros(n & 1, np.uint8)])
    packed = ((pad[0::2] << 4) | pad[1::2]).astype(np.uint8).tobytes()
    if qual is None:
        qual = (np.arange(n) * 5 % 41).astype(np.uint8).tobytes()
    cig = b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar)
    nm = name + b"\0"
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(nm), mapq, 0, len(cigar), flag, n if l_seq is None else l_seq,
                       -1, -1, 0) + nm + cig + packed + qual + aux
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


class Builder:
    """Records laid back to back after the header; ``starts[i]`` / ``ends[i]`` are record i's offsets."""

    def __init__(self, refs=REFS):
        self.refs = refs
        self.head = bam_header(refs)
        self.recs = []

    @property
    def first(self):
        return len(self.head)

    @property
    def size(self):
        return len(self.head) + sum(len(r) for r in self.recs)

    def add(self, **kw):
        self.recs.append(bytearray(record(**kw)))
        return self

    def add_bytes(self, b):
        self.recs.append(bytearray(b))
        return self

    def pad_to(self, offset):
        """Lengthen the last record with auxiliary bytes so that the next record starts at offset."""
        more = offset - self.size
        assert more >= 0, (offset, self.size)
        r = self.recs[-1]
        r += b"A" * more
        r[0:4] = struct.pack("<I", len(r) - 4)
        return self

    @property
    def starts(self):
        out, q = [], self.first
        for r in self.recs:
            out.append(q)
            q += len(r)
        return out

    @property
    def ends(self):
        return [s + len(r) for s, r in zip(self.starts, self.recs)]

    def raw(self) -> bytes:
        return self.head + b"".join(bytes(r) for r in self.recs)


def bgzf(raw: bytes, level: int = 6, chunk: int = 65280) -> bytes:
    out = []
    for i in list(range(0, len(raw), chunk)) + [None]:
        data = b"" if i is None else raw[i:i + chunk]  # the last one: the EOF block
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = z.compress(data) + z.flush()
        out.append(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25) + comp +
                   struct.pack("<II", zlib.crc32(data), len(data)))
    return b"".join(out)


def inflated(path: str) -> bytes:
    with open(path, "rb") as f:
        return gzip.decompress(f.read())


def header_info(raw: bytes):
    """(offset of the first record, n_ref) of inflated BAM bytes."""
    assert raw[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", raw, 4)
    q = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, q)
    q += 4
    for _ in range(n_ref):
        ln, = struct.unpack_from("<i", raw, q)
        q += 4 + ln + 4
    return q, n_ref


# ---- the synthetic files ----
K64 = 65536


def _small_records(b: Builder, seed: int, n: int):
    rng = np.random.default_rng(seed)
    for i in range(n):
        ls = int(rng.integers(1, 180))
        b.add(tid=int(rng.integers(0, 2)), pos=int(rng.integers(0, 40_000)), mapq=int(rng.integers(0, 61)),
              flag=int(rng.choice([0, 16, 99, 147])), name=b"read%d" % i, cigar=[(0, ls)],
              seq=rng.integers(0, 16, ls).astype(np.uint8), qual=rng.integers(0, 42, ls).astype(np.uint8).tobytes())


def layout_builder() -> Builder:
    """Every piece of the layout test at seg_bytes 256, 1024 and 65536 at once: the placements are
    multiples of 65536 (minus 0..3), which are multiples of the smaller sizes too."""
    b = Builder()
    _small_records(b, 1, 12)
    # the record kinds the field extraction distinguishes
    b.add(name=b"odd", cigar=[(4, 3), (0, 10), (4, 4)], l_seq=17)
    b.add(name=b"nocigar", l_seq=8)
    b.add(name=b"noseq", cigar=[(0, 5)], l_seq=0, qual=b"")
    b.add(name=b"noseq_clip", cigar=[(4, 2), (0, 5), (1, 2), (4, 1)], l_seq=0, qual=b"")
    b.add(name=b"noqual", cigar=[(0, 9)], l_seq=9, qual=b"\xff" * 9)
    b.add(name=b"hardclip", cigar=[(5, 4), (4, 2), (0, 10), (4, 1), (5, 2)], l_seq=13)
    b.add(name=b"badclip", cigar=[(4, 2), (5, 4), (0, 10), (5, 1), (4, 2)], l_seq=14)
    b.add(name=b"negpos", pos=-5, cigar=[(0, 6)], l_seq=6)
    b.add(name=b"unmapped", tid=-1, pos=-1, flag=4, mapq=0, l_seq=11)
    b.add(name=b"ops", cigar=[(0, 5), (2, 3), (0, 5), (3, 100), (7, 4), (8, 1), (1, 2), (6, 1)], l_seq=17)
    b.add(name=b"iupac", cigar=[(0, 16)], seq=np.arange(16, dtype=np.uint8))
    # a record spanning three and more segments of 256 and 1024 bytes
    b.add(name=b"span", cigar=[(0, 2100)], l_seq=2100)
    _small_records(b, 2, 5)
    # one read of about 70 kb (longer than the default segment and than a BGZF block), 300 ops;
    # lengthened to end one byte before a multiple of 65536: it spans segments 0, 1 and 2 at 65536
    ops = [(0, 150), (1, 3), (0, 150), (2, 2)] * 75 + [(4, 23_000)]
    ls = sum(n for op, n in ops if op in (0, 1, 4))
    rng = np.random.default_rng(3)
    b.add(name=b"long70k", pos=1000, cigar=ops, seq=rng.integers(0, 16, ls).astype(np.uint8),
          qual=rng.integers(0, 42, ls).astype(np.uint8).tobytes())
    b.pad_to(3 * K64 - 1)  # the next start: in the last byte of a segment
    b.add(name=b"last1", cigar=[(0, 30)], l_seq=30).pad_to(4 * K64 - 2)
    b.add(name=b"last2", cigar=[(0, 31)], l_seq=31).pad_to(5 * K64 - 3)
    b.add(name=b"last3", cigar=[(0, 32)], l_seq=32).pad_to(6 * K64)
    b.add(name=b"onboundary", cigar=[(0, 33)], l_seq=33)
    _small_records(b, 4, 6)
    return b


def trap_builder():
    """One long read whose QUAL bytes are genuine serialized records of the same file, tiling the
    field exactly to its end (what the stitch must not believe).  Returns the builder
    and the index of the trap record."""
    b = Builder()
    _small_records(b, 5, 40)
    # enough copies to cross four boundaries of 1024; a few bytes of aux in front shift where the
    # field ends inside its segment
    fake = b"".join(bytes(r) for r in b.recs[5:35]) * 2
    ls = len(fake)
    rng = np.random.default_rng(6)
    b.add(name=b"trap", pos=100, cigar=[(0, ls)], seq=rng.integers(1, 16, ls).astype(np.uint8), qual=fake)
    trap = len(b.recs) - 1
    _small_records(b, 7, 20)
    return b, trap


def write_bam(path: str, b: Builder, level: int = 6) -> None:
    with open(path, "wb") as f:
        f.write(bgzf(b.raw(), level))


# what the record rules refuse, as inflated buffers: name -> (raw, the host decoder's message)
def refusals() -> dict:
    out = {}
    base = Builder()
    _small_records(base, 8, 10)
    good = base.raw()
    last = base.starts[-1]
    out["truncated_last_record"] = (good[:-7], "truncated BAM record")
    out["ends_in_length_prefix"] = (good[:last + 2], "truncated record length")
    for name, kw, msg in (("block_size_31", dict(block_size=31), "truncated BAM record"),
                          ("negative_l_seq", dict(l_seq=-1), "negative l_seq"),
                          ("fields_past_record", dict(block_size=40), "BAM record shorter than its fields")):
        b = Builder()
        _small_records(b, 9, 6)
        b.add_bytes(record(name=b"bad", cigar=[(0, 20)], seq=np.ones(20, np.uint8), **kw))
        _small_records(b, 10, 3)
        out[name] = (b.raw(), msg)
    return out


STATUS_MESSAGE = {1: "truncated record length", 2: "truncated BAM record", 3: "truncated BAM record",
                  4: "negative l_seq", 5: "BAM record shorter than its fields"}


# ---- the host decoder's arrays: the oracle ----
def host_arrays(path: str) -> dict:
    from basecount_amd.bam import BamFile

    with BamFile(path) as f:
        out = {k: np.array(getattr(f, k), copy=True) for k in ARRAYS}
        out["seq_event"] = out["seq_event"][:out["seq"].size]  # batches pad their own tails
        out["n"] = int(f.n_records)
        out["n_refs"] = len(f.references)
    return out


def first_records(exp: dict, n: int) -> dict:
    """The arrays of the first n records."""
    cw, sb = int(exp["cig_off"][n]), int(exp["seq_off"][n])
    out = {k: exp[k][:n] for k in ARRAYS[:9]}
    out.update(cig_off=exp["cig_off"][:n + 1], seq_off=exp["seq_off"][:n + 1], cigar=exp["cigar"][:cw],
               seq=exp["seq"][:sb], seq_event=exp["seq_event"][:sb], qual=exp["qual"][:2 * sb], n=n)
    return out


# ---- tests/native/bamdecode_check.cpp ----
def pack_input(raw: bytes, first: int, n_refs: int, configs) -> bytes:
    """configs: (seg_bytes, max_records, trunc, final, want_qual) each."""
    out = [struct.pack("<QQiI", len(raw), first, n_refs, len(configs)), raw]
    out += [struct.pack("<IqIII", *c) for c in configs]
    return b"".join(out)


def unpack_results(buf: bytes, configs) -> list:
    res, q = [], 0
    for c in configs:
        guards, status, err_off, n, cw, sb, repaired, batches, used = struct.unpack_from("<IiQqQQqqQ", buf, q)
        q += 64
        r = dict(guards=guards, status=status, err_off=err_off, n=n, repaired=repaired, batches=batches, used=used)
        for k in ARRAYS:
            cnt = {"cig_off": n + 1, "seq_off": n + 1, "cigar": cw, "seq": sb, "seq_event": sb,
                   "qual": 2 * sb if c[4] else 0}.get(k, n)
            r[k] = np.frombuffer(buf, DTYPES[k], cnt, q)
            q += cnt * np.dtype(DTYPES[k]).itemsize
        res.append(r)
    assert q == len(buf), (q, len(buf))
    return res


def assert_arrays_equal(got: dict, exp: dict, want_qual: bool, what: str) -> None:
    assert got["n"] == exp["n"], "%s: %d records, the host decoder has %d" % (what, got["n"], exp["n"])
    for k in ARRAYS:
        if k == "qual" and not want_qual:
            continue
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), "%s: %s differs" % (what, k)
