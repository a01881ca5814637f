"""Helpers for the 64-bit-index instances of the tiled kernels (a plain module, no fixtures).

k_pileup and k_pileup_solo are compiled over an index type IT: int32_t while ``tiles_fit_i32``
(basecount_amd/csrc/bc_pileup.hip) holds, int64_t otherwise.  ``fits_i32`` restates the predicate;
``widen`` raises a device batch's ``max_end`` (documented as an upper bound of pos + span: the
kernels size their tile loop by it and nothing else), which is the cheap way to the wide side;
``is_wide`` reads the decision back from the library: k_pileup's static range hand-off is
``IT rng[8][2]``, so bc_pileup_launch_info reports exactly 64 B more LDS for a 64-bit instance.
tests/test_wide_index_host.py pins all of it without a device."""
import ctypes as C

import numpy as np

from basecount_amd import device as D

TILE = 64
I32_LIMIT = 0x7FFFFF00        # tiles_fit_i32: n_reads and the furthest position touched stay below
WIDE_END = 2**31 - 1          # the largest end an int32 start can have
RNG_BYTES_I32 = 8 * 2 * 4     # rng[8][2] of int32_t; of int64_t: twice that


def fits_i32(n_reads, reach, max_span):
    """tiles_fit_i32 restated; reach = max(max_end, ref_len)."""
    n_tiles = -(-int(reach) // TILE)
    return int(n_reads) < I32_LIMIT and n_tiles * TILE + int(max_span) + 2 * TILE < I32_LIMIT


def last_narrow_end(max_span, L):
    """The largest max_end at which a batch of few reads on L positions still takes int32_t."""
    end = (I32_LIMIT - int(max_span) - 2 * TILE - 1) // TILE * TILE
    assert L <= end, "the reference alone is wide"
    return end


def first_wide_end(max_span, L):
    """The smallest max_end for which the predicate fails (few reads, L positions)."""
    return last_narrow_end(max_span, L) + 1


def _struct(reads):
    return reads.r if isinstance(reads, D.DeviceReads) else reads


def with_end(reads, max_end):
    """A copy of a batch header (a DeviceReads, a BcReads or a header dict) with another max_end."""
    if isinstance(reads, dict):
        return dict(reads, max_end=int(max_end))
    r = D.BcReads.from_buffer_copy(_struct(reads))
    r.max_end = int(max_end)
    return r


def widen(reads, max_end=WIDE_END):
    """The BcReads of a DeviceReads (or a BcReads) with max_end raised: still an upper bound, so the
    batch stays truthful; index_tag no longer matches, so the kernels search instead of reading
    the upload's tile index.  The device arrays stay the original object's (free that one)."""
    old = int(_struct(reads).max_end)
    assert max_end >= old, (max_end, old)
    r = with_end(reads, max_end)
    assert C.sizeof(r) == C.sizeof(D.BcReads) and r.pos == _struct(reads).pos
    return r


def header_of(reads):
    r = _struct(reads)
    if isinstance(r, dict):
        return int(r["n_reads"]), int(r["max_span"]), int(r["max_end"])
    return int(r.n_reads), int(r.max_span), int(r.max_end)


def append_reads(b, reads):
    """The batch dict b with reads (pos, [(op, len)], base codes, qualities) appended in the given
    order: each read's bases start on a byte boundary after b's sequence, its qualities at the
    same nibble index.  The starts must not lie before b's last."""
    assert b["qual"].size == 2 * b["seq"].size
    pos, cig_beg, cig_n, seq_nib = [list(b[f]) for f in ("pos", "cig_beg", "cig_n", "seq_nib")]
    cigar, seq, qual = list(b["cigar"]), [b["seq"]], [b["qual"]]
    at = 2 * int(b["seq"].size)  # the next read's first nibble
    for p, ops, codes, q in reads:
        assert p >= pos[-1] and len(codes) == len(q) == sum(ln for op, ln in ops if op in (0, 1, 4, 7, 8))
        c = np.zeros(len(codes) + 2 + (len(codes) & 1), np.uint8)
        c[:len(codes)] = codes
        qq = np.zeros(c.size, np.uint8)
        qq[:len(q)] = q
        pos.append(int(p))
        cig_beg.append(len(cigar))
        cig_n.append(len(ops))
        seq_nib.append(at + (ops[0][1] if ops[0][0] == 4 else 0))
        cigar += [(ln << 4) | op for op, ln in ops]
        seq.append(((c[0::2] << 4) | c[1::2]).astype(np.uint8))
        qual.append(qq)
        at += c.size
    return dict(pos=np.array(pos, np.int32), cig_beg=np.array(cig_beg, np.uint32), cig_n=np.array(cig_n, np.uint32),
                seq_nib=np.array(seq_nib, np.uint32), cigar=np.array(cigar, np.uint32), seq=np.concatenate(seq),
                qual=np.concatenate(qual))


# the reads of a batch that reaches the end of the int32 range by its own data: two `150M`, the last
# one ending at 2^31 - 1, and one with an insertion and a deletion
FAR_READS = ((WIDE_END - 400, [(0, 40), (2, 20), (0, 40), (1, 5), (0, 45)]),
             (WIDE_END - 150 - 64, [(0, 150)]),
             (WIDE_END - 150, [(0, 150)]))


def far_batch(near, rng):
    """``near`` with FAR_READS (random A C G T, qualities 0-44) appended: they sort last."""
    reads = []
    for p, ops in FAR_READS:
        q = sum(ln for op, ln in ops if op in (0, 1, 4, 7, 8))
        reads.append((p, ops, np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, q)], rng.integers(0, 45, q).astype(np.uint8)))
    return append_reads(near, reads)


def _kind(info):
    return "slice" if info["slice"] else "lean" if info["lean"] else "general"


def is_wide(reads, L, shape, waves=0, instance="auto", mbq=0, k=5):
    """Whether bc_pileup / bc_count on a context set to (shape, waves, instance) launch a 64-bit
    instance for this batch on L positions.  k_pileup: lds_bytes of bc_pileup_launch_info against
    the same call on a copy whose max_end is last_narrow_end: 64 B more, or nothing.  (Where the
    width itself changes the instance -- no slice instance and, with a threshold, no lean one is
    built at 64 bits -- both sides are asked for the general instance: the width does not depend
    on it.)  The sweep's plan has no such term: there the predicate is evaluated, which
    launch_pileup_tiles applies identically on both branches."""
    n, span, end = header_of(reads)
    info = D.pileup_launch_info(reads, L, shape, waves, instance, mbq, k)
    assert info["kernel"] in ("solo", "tiles"), info
    if info["kernel"] == "solo":
        return not fits_i32(n, max(end, L), span)
    narrow = with_end(reads, last_narrow_end(span, L))
    if isinstance(narrow, dict):
        narrow = dict(narrow, n_reads=min(n, I32_LIMIT - 1))
    base = D.pileup_launch_info(narrow, L, shape, waves, instance, mbq, k)
    if _kind(base) != _kind(info):
        info = D.pileup_launch_info(reads, L, shape, waves, "general", mbq, k)
        base = D.pileup_launch_info(narrow, L, shape, waves, "general", mbq, k)
    assert (base["kernel"], base["waves_per_tile"]) == (info["kernel"], info["waves_per_tile"]), (info, base)
    extra = info["lds_bytes"] - base["lds_bytes"]
    assert extra in (0, RNG_BYTES_I32), (info, base)
    return extra == RNG_BYTES_I32
