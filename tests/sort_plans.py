"""The device sort's decisions (basecount_amd/csrc/bc_sort.hip) restated on the CPU, the batches that
reach each of them, and a structural yardstick for a sorted view.

``plan`` restates bkt_plan and what follows from it (rounds of k_bkt_count and k_bkt_scatter, the
count_rows instance and its loop counts, the counting sort's scan passes); ``layout_bytes`` restates
sort_layout's total; ``copy_plan`` restates copy_slot / read_words (full or shrunk slots, the reads
that take bump-allocator bytes, the "big records" of k_bkt_copy); ``rank_plan`` gives every bucket's
size and its path through k_bkt_rank.  ``make_batch`` builds a batch (the dict of
test_gpu_parity.build_batch) without a Python loop over the reads; ``case`` names the batches
tests/test_sort_plans_host.py proves and tests/test_gpu_sort_plans.py runs.

``sorted_view_matches(source, view)`` checks a sorted view read by read against the batch it was
sorted from: both are host copies of the arrays as they lie in device memory, so the sequence's
BC_SEQ_EVENT code map is not restated.  ``model_view`` is a plain CPU sort producing such a view
(the host tests corrupt it).  Nothing here imports the device library."""
import functools

import numpy as np

M, I, DEL, SKIP, S, EQ, X = 0, 1, 2, 3, 4, 7, 8  # CIGAR ops
ACGT = np.array([1, 2, 4, 8], np.uint8)          # BAM 4-bit base codes
OTHER = np.array([15, 0, 5, 3], np.uint8)        # N and codes no column counts

# bc_sort.hip's constants
BKT_THREADS = 1024     # kBktThreads
COUNT_B, SCATTER_B = 8, 4  # reads per thread and round of k_bkt_count / k_bkt_scatter
BKT_MAX = 4096         # kBktMax
BKT_TARGET = 256       # kBktTarget
BKT_CHUNK = 4096       # kBktChunk
MAT_WORDS = 65536      # the count rows' bound (blocks x buckets)
RANK_REGS = 8 * 1024   # kRankRegs * kRankThreads: a bucket's records held in registers
PERM_SLOTS = 4096      # kPermSlots (BC_SORT_RUNS == 0)
QLEN_MAX = 0xFFFF      # kQlenMax
SORT_CAP_MAX = 0x55555550  # kSortCapMax
SCAN_TILE = 1024       # kScanTile
RELAY_READS = 4        # kRelayReads
RELAY_BASES = 160      # kRelayWords * 4 lanes * 8 bases: the copy's unrolled part


def cdiv(a, b):
    return -(-a // b)


def seq_event_bytes(n):
    """bc_seq_event_bytes / bam.seq_event_bytes: the device's sequence buffer for n packed bytes."""
    return (max(int(n), 0) + 15) // 16 * 16 + 16


# ------------------------------------------------------------------------------- the decisions
def plan(n, max_end):
    """bkt_plan(n_reads, max_end) and the loop counts its numbers give the kernels."""
    n, nbins = int(n), int(max_end) + 2
    assert 0 < n < 0xFFFFFFFF and nbins > 0
    w = 0
    while w < 12 and cdiv(nbins, 1 << w) > BKT_TARGET:
        w += 1
    H = cdiv(nbins, 1 << w)
    if H > BKT_MAX:
        tiles = cdiv(nbins, SCAN_TILE)
        return dict(kind="counting", n=n, nbins=nbins, scan_tiles=tiles, scan_passes=cdiv(tiles, SCAN_TILE),
                    relay_groups=cdiv(n, RELAY_READS), relay_tail=n % RELAY_READS)
    nblk = max(1, min(cdiv(n, BKT_CHUNK), MAT_WORDS // H))
    chunk = cdiv(n, nblk)
    nblk = cdiv(n, chunk)
    inst = "4x16" if H <= 256 else "8x4"
    g, r = (4, 16) if inst == "4x16" else (8, 4)
    return dict(kind="bucket", n=n, nbins=nbins, wbits=w, W=1 << w, nbkt=H, nblk=nblk, chunk=chunk,
                count_rounds=cdiv(chunk, COUNT_B * BKT_THREADS), scatter_rounds=cdiv(chunk, SCATTER_B * BKT_THREADS),
                rows=inst, h0_iters=cdiv(H, 64 * g), row_iters=(nblk - 1) // (16 * r) + 1)


def layout_bytes(n, max_end, seq_bytes, has_qual, fields):
    """sort_layout(...).total: what bc_reads_sort_bytes answers."""
    n = int(n)
    if n <= 0:
        return 0
    P = plan(n, max_end)
    bkt = P["kind"] == "bucket"
    fields = bool(fields) and bkt
    cap = min(int(seq_bytes) + 5 * n + 16, SORT_CAP_MAX)
    room = (cap + cap // 2 + 15) // 16 * 16
    pieces = [16]
    if not bkt:
        pieces.append(4 * P["nbins"])
    pieces += [32 * n, 4 * n, 4 * n, 4 * n, 4 * n]
    if fields:
        pieces.append(16 * n)
    if not bkt:
        pieces.append(4 * (cdiv(P["nbins"], SCAN_TILE) + 1))
    if not fields:
        pieces.append(seq_event_bytes(room))
        if has_qual:
            pieces.append(2 * room + 32)
    pieces += [4 * P["nbkt"] * P["nblk"], 8 * P["nblk"], 4 * (P["nbkt"] + 1)] if bkt else [0, 0, 0]
    return sum(cdiv(x, 256) * 256 for x in pieces)


def ragged(starts, lens):
    """Indices starts[i] .. starts[i] + lens[i] - 1 of every i, one after the other."""
    lens = np.asarray(lens, np.int64)
    ends = np.cumsum(lens)
    return np.repeat(np.asarray(starts, np.int64) - (ends - lens), lens) + np.arange(int(ends[-1]) if lens.size else 0)


def query_lengths(b):
    """Every read's aligned query length: the sum of its M / I / = / X (bc_runs.h qcons)."""
    cn = np.asarray(b["cig_n"], np.int64)
    words = np.asarray(b["cigar"], np.uint32)[ragged(b["cig_beg"], cn)].astype(np.int64)
    ln = np.where(np.isin(words & 15, (M, I, EQ, X)), words >> 4, 0)
    q = np.zeros(cn.size, np.int64)
    np.add.at(q, np.repeat(np.arange(cn.size), cn), ln)
    return q


def read_words(sn, q):
    """read_words: 32-bit words of a read's copy at its nibble parity."""
    return ((((np.asarray(sn, np.int64) & 1) + q + 1) >> 1) + 3) >> 2


def copy_plan(b):
    """copy_slot / copy_reads for a batch: cap, room, the slot size and whether the slots are the
    longest read's ("full") or shrunk, the reads that take bump-allocator bytes, whether those
    bytes overflow room (the "overlap" flag), and k_bkt_copy's big records."""
    n = int(np.asarray(b["pos"]).size)
    q = query_lengths(b)
    qmax = int(q.max()) if n else 0
    cap = min(int(np.asarray(b["seq"]).size) + 5 * n + 16, SORT_CAP_MAX)
    room = (cap + cap // 2 + 15) // 16 * 16
    full = ((qmax + 2) // 2 + 3) & ~3
    shrunk = full * n > room
    slot = (cap // (2 * n)) & ~3 if shrunk else full
    nbytes = 4 * read_words(b["seq_nib"], q)
    bump = nbytes > slot
    return dict(n=n, q=q, qmax=qmax, cap=cap, room=room, slots="shrunk" if shrunk else "full", slot=int(slot),
                bump=np.flatnonzero(bump), bump_bytes=int(nbytes[bump].sum()),
                overflows=bool(slot * n + int(nbytes[bump].sum()) > room),
                big=np.flatnonzero((np.asarray(b["cig_n"], np.int64) > 0xFFFF) | (q >= QLEN_MAX)),
                past_unrolled=np.flatnonzero(read_words(b["seq_nib"], q) > RELAY_BASES // 8))


def rank_plan(b, P):
    """The bucket sizes of a batch under a bucketed plan and each bucket's way through k_bkt_rank:
    "empty", "regs1" / "regs2" (in registers; the fields-only sort writes it in one or two passes of
    kPermSlots) or "past_regs" (more than kRankRegs * kRankThreads records)."""
    assert P["kind"] == "bucket"
    pos = np.asarray(b["pos"], np.int64)
    pos = np.where((pos < 0) | (pos >= P["nbins"] - 1), 0, pos)  # bkt_pos
    sizes = np.bincount(pos >> P["wbits"], minlength=P["nbkt"])
    assert sizes.size == P["nbkt"]
    path = np.where(sizes == 0, "empty", np.where(sizes <= PERM_SLOTS, "regs1",
                                                  np.where(sizes <= RANK_REGS, "regs2", "past_regs")))
    return dict(sizes=sizes, path=path, empty=int((sizes == 0).sum()),
                counts={k: int((path == k).sum()) for k in ("empty", "regs1", "regs2", "past_regs")})


# ------------------------------------------------------------------------------- the builder
def make_batch(rng, pos, m1, clip=0, ins=0, m2=0, nib0=None, qual=True, tight=False):
    """The batch dict of test_gpu_parity.build_batch, built with array operations only.  Read i:
    start pos[i], CIGAR [clip[i] S] m1[i] M [ins[i] I m2[i] M] (the bracketed parts where the number
    is non-zero), random bases with 5 % non-ACGT codes, qualities 0-44.  Its sequence starts at
    nibble nib0[i] of ``seq`` (default: one read after the other, each on a byte boundary) and
    ``seq_nib`` points past the soft clip.  ``tight``: the arrays end with the last read's last base
    (its quality is ``qual``'s last byte); else two nibbles later."""
    pos = np.asarray(pos, np.int64)
    n = pos.size
    m1, clip, ins, m2 = (np.broadcast_to(np.asarray(x, np.int64), (n,)) for x in (m1, clip, ins, m2))
    m2 = np.where(ins > 0, m2, 0)
    assert np.all(m1 > 0) and np.all((ins == 0) | (m2 > 0))
    words = np.stack([clip << 4 | S, m1 << 4 | M, ins << 4 | I, m2 << 4 | M], 1).astype(np.uint32)
    have = np.stack([clip > 0, m1 > 0, ins > 0, ins > 0], 1)
    cig_n = have.sum(1).astype(np.uint32)
    cig_beg = np.zeros(n, np.uint32)
    cig_beg[1:] = np.cumsum(cig_n)[:-1]
    lseq = clip + m1 + ins + m2
    if nib0 is None:
        nib0 = np.zeros(n, np.int64)
        nib0[1:] = np.cumsum(lseq + (lseq & 1))[:-1]
    nib0 = np.asarray(nib0, np.int64)
    total = int((nib0 + lseq).max()) + (0 if tight else 2)
    codes = ACGT[rng.integers(0, 4, total + (total & 1))]
    other = rng.random(codes.size) < 0.05
    codes[other] = OTHER[rng.integers(0, 4, int(other.sum()))]
    return dict(pos=pos.astype(np.int32), cig_beg=cig_beg, cig_n=cig_n, seq_nib=(nib0 + clip).astype(np.uint32),
                cigar=words[have], seq=((codes[0::2] << 4) | codes[1::2]).astype(np.uint8),
                qual=rng.integers(0, 45, total).astype(np.uint8) if qual else None)


def max_end_of(b):
    """max(start + reference span): bc_reads_upload's max_end."""
    cn = np.asarray(b["cig_n"], np.int64)
    words = np.asarray(b["cigar"], np.uint32)[ragged(b["cig_beg"], cn)].astype(np.int64)
    span = np.zeros(cn.size, np.int64)
    np.add.at(span, np.repeat(np.arange(cn.size), cn), np.where(np.isin(words & 15, (M, DEL, SKIP, EQ, X)), words >> 4, 0))
    return int((np.asarray(b["pos"], np.int64) + span).max())


def mixed_reads(rng, pos, lo, hi):
    """Reads of lo..hi - 1 aligned bases: 40 % with a soft clip, 30 % with an insertion."""
    n = len(pos)
    m1 = rng.integers(lo, hi, n)
    clip = np.where(rng.random(n) < 0.4, rng.integers(1, 6, n), 0)
    ins = np.where((rng.random(n) < 0.3) & (m1 > 3), rng.integers(1, 4, n), 0)
    m2 = np.where(ins > 0, rng.integers(1, 4, n), 0)
    return dict(m1=m1, clip=clip, ins=ins, m2=m2)


def spread(rng, n, max_end, lo=8, hi=13, mixed=True, starts=None):
    """n shuffled reads with starts uniform on the reference (or ``starts``); the last one ends at
    max_end exactly, so the uploaded batch's max_end is the one asked for."""
    kw = mixed_reads(rng, np.zeros(n), lo, hi) if mixed else dict(m1=rng.integers(lo, hi, n))
    span = kw["m1"] + kw.get("m2", 0)
    pos = rng.integers(0, max(1, max_end - hi - 4), n) if starts is None else np.asarray(starts, np.int64).copy()
    pos[-1] = max_end - span[-1]
    assert np.all(pos >= 0) and int((pos + span).max()) == max_end
    return make_batch(rng, pos, **kw)


CASES = {}


def _case(fn):
    CASES[fn.__name__.lstrip("_")] = fn
    return fn


@_case
def _one_read(rng):
    return make_batch(rng, [3], [7])


@_case
def _two_reads_same_start(rng):
    return make_batch(rng, [3, 3], [7, 5], clip=[0, 2])


@_case
def _w0_tiny(rng):
    return spread(rng, 700, 254, 1, 50)


@_case
def _all_one_start(rng):
    m1 = rng.integers(50, 101, 9_000)
    m1[17] = 100
    return make_batch(rng, np.full(9_000, 100), m1)


@_case
def _h256_edge(rng):
    return spread(rng, 5_000, (1 << 20) - 2)


@_case
def _h257_edge(rng):
    return spread(rng, 5_000, (1 << 20) - 1)


@_case
def _h_gt_512(rng):
    return spread(rng, 10_000, 3_000_000)


@_case
def _rows_gt_64(rng):
    return spread(rng, 270_000, 1_200_000)


@_case
def _rows_gt_256(rng):
    return spread(rng, 1_050_000, 3_198, 10, 11, mixed=False)


@_case
def _capped_rounds(rng):
    return spread(rng, 140_000, (1 << 24) - 2)


RANK_EDGE_BUCKETS = {10: 4096, 50: 4097, 100: 8192, 200: 8193}


@_case
def _rank_edges(rng):
    starts = [16 * h + rng.integers(0, 16, k) for h, k in RANK_EDGE_BUCKETS.items()]
    starts.append(16 * rng.integers(120, 181, 5_400) + rng.integers(0, 16, 5_400))  # the others: buckets 120-180
    starts = rng.permutation(np.concatenate(starts))
    return spread(rng, starts.size + 1, 4_000, starts=np.append(starts, 0))  # (+ the read that ends at max_end)


ALIGN_QLENS = list(range(1, 41)) + list(range(150, 176))


@_case
def _alignments(rng):
    offs, qs = np.meshgrid(np.arange(8), ALIGN_QLENS, indexing="ij")
    order = rng.permutation(offs.size)  # the order in the buffer
    offs, qs = offs.ravel()[order], qs.ravel()[order]
    nib0, cur = np.zeros(offs.size, np.int64), 0
    for i in range(offs.size):
        nib0[i] = cur + (offs[i] - cur) % 8
        cur = nib0[i] + qs[i]
    pos = rng.integers(0, 300, offs.size)
    shuffle = rng.permutation(offs.size)  # the order of the reads
    return make_batch(rng, pos[shuffle], qs[shuffle], nib0=nib0[shuffle], tight=True)


SHRUNK_LONG = (7_000, 8_800, 9_000, 9_000, 9_000)


@_case
def _shrunk_many_long(rng):
    """3,000 reads of 8 bases and five long ones: the slots shrink to 8 bytes (half the mean), which
    hold every short read; exactly the long ones take bump-allocator bytes."""
    m1 = np.concatenate([np.full(3_000, 8), SHRUNK_LONG])
    pos = rng.integers(0, 10_000, m1.size)
    order = rng.permutation(m1.size)
    return make_batch(rng, pos[order], m1[order])


@_case
def _big_records(rng):
    """2,000 reads of 50 bases (in their shrunk slots), one of 70,000 bases and one of exactly 0xFFFF:
    the two whose query length does not fit the bucketed record's 16 bits."""
    m1 = np.concatenate([np.full(2_000, 50), [70_000, QLEN_MAX]])
    clip = np.concatenate([np.full(2_000, 3), [0, 0]])
    pos = np.concatenate([rng.integers(0, 119_800, 2_000), [1_000, 20_000]])
    order = rng.permutation(m1.size)
    return make_batch(rng, pos[order], m1[order], clip=clip[order])


@_case
def _counting_edge(rng):
    return spread(rng, 2_003, (1 << 24) - 1)


COUNTING_LONG = (1 << 24) + 4_096


@_case
def _counting_spread(rng):
    n = 4_001
    starts = rng.integers(0, COUNTING_LONG - 20, n)
    starts[:18] = np.arange(18) * (SCAN_TILE * SCAN_TILE) + 5  # a start in the first tile of every pass of k_scan_sums
    starts[:18] = np.minimum(starts[:18], COUNTING_LONG - 20)
    return spread(rng, n, COUNTING_LONG, starts=rng.permutation(starts))


@_case
def _counting_tiny1(rng):
    return spread(rng, 1, COUNTING_LONG)


@_case
def _counting_tiny3(rng):
    return spread(rng, 3, COUNTING_LONG)


@_case
def _overlap(rng):
    """200 reads that each claim 6,000 bases of one 4,000-byte sequence: a caller's error (the
    reads' bytes sum to far more than the buffer's), flagged by the copy."""
    n = 200
    codes = ACGT[rng.integers(0, 4, 8_000)]
    return dict(pos=rng.integers(0, 2_000, n).astype(np.int32), cig_beg=np.arange(n, dtype=np.uint32),
                cig_n=np.ones(n, np.uint32), seq_nib=rng.integers(0, 2_001, n).astype(np.uint32),
                cigar=np.full(n, 6_000 << 4 | M, np.uint32), seq=((codes[0::2] << 4) | codes[1::2]).astype(np.uint8),
                qual=rng.integers(0, 45, 8_000).astype(np.uint8))


FLAG_CASES = ("overlap",)  # caller errors: not part of the clean catalogue
BAD_START_BASE = {"bad_start_bucket": "rank_edges", "bad_start_counting": "counting_edge"}


def cases():
    return [c for c in CASES if c not in FLAG_CASES]


@functools.lru_cache(maxsize=4)
def case(name):
    """The named batch (read-only arrays; the same for every caller)."""
    b = CASES[name](np.random.default_rng(sorted(CASES).index(name) + 500))
    for v in b.values():
        if v is not None:
            v.setflags(write=False)
    return b


def bad_starts(b):
    """(read, start) pairs that make a batch untruthful: one negative start, one above max_end."""
    n, me = b["pos"].size, max_end_of(b)
    return [(n // 3, -5), (2 * n // 3, me + 1)] if n // 3 != 2 * n // 3 else [(0, -5)]


# what test_gpu_parity.py's test_device_sort_* sorted before this catalogue, and full-size C3: (n, reference
# length); a batch's max_end lies within a read's span below its reference length
OLD_SUITE = {"unsorted71": (20_000, 3_000), "unsorted72": (60_000, 30_000), "unsorted73": (5, 500),
             "unsorted74": (3_000, 2_000_000), "unsorted75": (40_000, 6_000), "unsorted76": (60_000, 3_000),
             "unsorted77": (3, 500), "hot_start": (30_000, 5_000), "shrunk_slots": (3_001, 20_000),
             "longer_than_16_bits": (2_001, 120_000), "flags_deferred": (5_000, 4_000), "in_a_graph": (120_000, 6_000),
             "c3_full_size": (1_000_000, 6_000)}
OLD_SUITE_COUNTING = {"long_reference": (2_000, (1 << 24) + 4_096)}


# ------------------------------------------------------------------------------- the yardstick
def _nibbles(seq, idx):
    """Nibble idx of a device sequence buffer: byte idx >> 1, the low half when idx is even."""
    byte = seq[idx >> 1]
    return np.where(idx & 1, byte >> 4, byte & 15).astype(np.uint8)


def read_table(d, what="batch", keep=None, extra=None):
    """{(cig_n, q): rows} of a batch's reads: one row of bytes per read, its start, its CIGAR words,
    its q bases (one per byte) and, with qualities, its q quality bytes; rows sorted bytewise.
    ``keep``: a mask of the reads to take; ``extra``: one more number per read for its row.  Raises
    AssertionError for a read outside its arrays."""
    pos = np.asarray(d["pos"]).astype(np.int32)
    n = pos.size
    cb, cn, sn = (np.asarray(d[k]).astype(np.int64) for k in ("cig_beg", "cig_n", "seq_nib"))
    cigar, seq, qual = np.asarray(d["cigar"], np.uint32), np.asarray(d["seq"], np.uint8), d.get("qual")
    assert np.all(cb + cn <= cigar.size), f"{what}: a CIGAR outside the cigar buffer"
    q = query_lengths(dict(cig_beg=cb, cig_n=cn, cigar=cigar))
    assert np.all((q == 0) | (sn + q <= 2 * seq.size)), f"{what}: a read's bases outside the sequence buffer"
    if qual is not None:
        qual = np.asarray(qual, np.uint8)
        assert np.all((q == 0) | (sn + q <= qual.size)), f"{what}: a read's qualities outside the quality buffer"
    key = cn << 32 | q
    sel = np.arange(n) if keep is None else np.flatnonzero(keep)
    order = sel[np.argsort(key[sel], kind="stable")]
    cuts = np.flatnonzero(np.diff(key[order])) + 1
    table = {}
    for idx in np.split(order, cuts) if order.size else []:
        c, ql = int(cn[idx[0]]), int(q[idx[0]])
        parts = [pos[idx].view(np.uint8).reshape(-1, 4)]
        if extra is not None:
            parts.append(np.asarray(extra, np.int64)[idx].view(np.uint8).reshape(-1, 8))
        if c:
            w = cigar[cb[idx, None] + np.arange(c)]
            parts.append(np.ascontiguousarray(w).view(np.uint8).reshape(idx.size, 4 * c))
        if ql:
            at = sn[idx, None] + np.arange(ql)
            parts.append(_nibbles(seq, at))
            if qual is not None:
                parts.append(qual[at])
        rows = np.ascontiguousarray(np.concatenate(parts, 1))
        void = rows.view(np.dtype((np.void, rows.shape[1]))).ravel()
        table[(c, ql)] = np.sort(void)
    return table, q


def _same_tables(a, b):
    if a.keys() != b.keys():
        return False
    return all(a[k].size == b[k].size and a[k].tobytes() == b[k].tobytes() for k in a)


def sorted_view_matches(source, view):
    """Raises AssertionError unless ``view`` is a sorted view of ``source``.  Both are dicts of host
    arrays: pos, cig_beg, cig_n, seq_nib, the shared cigar, and seq / qual (None without qualities)
    as they lie in device memory.  ``view`` also says ``fields`` (True: the sort left the sequence in
    place) and, for a copied view, ``room`` (bytes of its sequence buffer the reads may use).

      * the view's starts are non-decreasing;
      * its reads are the source's as a multiset, a read being its start, its CIGAR words, its
        aligned query length q and the q bases and q qualities at nibbles seq_nib .. seq_nib + q - 1
        (the order among equal starts is unspecified: both sides are compared sorted);
      * seq_nib keeps its parity (as a multiset with the read: the parity is part of the comparison);
      * copied: no two reads' bytes overlap and all lie below room;
      * fields-only: the view's sequence is the source's and every read keeps its seq_nib."""
    vpos = np.asarray(view["pos"]).astype(np.int64)
    assert vpos.size == np.asarray(source["pos"]).size, "read count differs"
    assert np.all(vpos[1:] >= vpos[:-1]), "starts out of order at %d" % int(np.argmax(vpos[1:] < vpos[:-1]))
    # seq_nib's parity (fields-only: seq_nib itself) is part of the read's row
    word = (lambda d: np.asarray(d["seq_nib"]).astype(np.int64) & (-1 if view["fields"] else 1))
    st, _ = read_table(source, "source", extra=word(source))
    vt, q = read_table(view, "view", extra=word(view))
    if not _same_tables(st, vt):
        plain = _same_tables(read_table(source, "source")[0], read_table(view, "view")[0])
        assert plain, "reads differ as a multiset (start, CIGAR, bases, qualities)"
        raise AssertionError("seq_nib differs (fields-only view)" if view["fields"] else "seq_nib parity differs")
    if view["fields"]:
        assert np.array_equal(np.asarray(view["seq"]), np.asarray(source["seq"])), "fields-only view: sequence differs"
        return
    sn = np.asarray(view["seq_nib"]).astype(np.int64)
    lo, hi = sn >> 1, (sn + q + 1) >> 1
    live = q > 0
    assert np.all(hi[live] <= int(view["room"])), "a read's bytes reach past room"
    order = np.argsort(lo[live], kind="stable")
    lo, hi = lo[live][order], hi[live][order]
    assert np.all(lo[1:] >= hi[:-1]), "two reads' bytes overlap"


def kept_reads_match(source, view):
    """For a view the copy flagged ("overlap"): every read of the view either has no CIGAR
    (dropped) or is a source read; the starts are sorted.  Returns the source indices of the kept
    reads (found through cig_beg, which must be distinct per source read)."""
    vpos = np.asarray(view["pos"]).astype(np.int64)
    assert np.all(vpos[1:] >= vpos[:-1]), "starts out of order"
    scb = np.asarray(source["cig_beg"]).astype(np.int64)
    assert np.unique(scb).size == scb.size
    back = np.argsort(scb)
    which = back[np.searchsorted(scb[back], np.asarray(view["cig_beg"]).astype(np.int64))]
    assert np.unique(which).size == which.size, "a source read appears twice"
    assert np.array_equal(np.asarray(source["pos"])[which], np.asarray(view["pos"])), "a read's start changed"
    kept = np.asarray(view["cig_n"]) != 0
    src_mask = np.zeros(scb.size, bool)
    src_mask[which[kept]] = True
    st, _ = read_table(source, "source", keep=src_mask)
    vt, _ = read_table(view, "view", keep=kept)
    assert _same_tables(st, vt), "a kept read differs from its source read"
    return np.sort(which[kept])


def sub_batch(b, idx):
    """The batch of reads idx of b (the buffers shared)."""
    return dict(b, pos=b["pos"][idx], cig_beg=b["cig_beg"][idx], cig_n=b["cig_n"][idx], seq_nib=b["seq_nib"][idx])


def model_view(source, fields=False):
    """A correct sorted view of ``source`` made on the CPU (stable sort by start): fields-only, or
    copied into slots of the longest read's bytes, each read at its old nibble parity."""
    pos = np.asarray(source["pos"]).astype(np.int64)
    order = np.argsort(pos, kind="stable")
    v = {k: np.asarray(source[k])[order].copy() for k in ("pos", "cig_beg", "cig_n", "seq_nib")}
    v["cigar"] = source["cigar"]
    if fields:
        return dict(v, seq=np.asarray(source["seq"]).copy(), qual=None if source.get("qual") is None else
                    np.asarray(source["qual"]).copy(), fields=True, room=None)
    q = query_lengths(v)
    n = pos.size
    slot = ((int(q.max()) + 2) // 2 + 3) & ~3
    room = slot * n
    sn = v["seq_nib"].astype(np.int64)
    new = 2 * slot * np.arange(n) + (sn & 1)
    src, dst = ragged(sn, q), ragged(new, q)
    nib = np.zeros(2 * room, np.uint8)
    nib[dst] = _nibbles(np.asarray(source["seq"]), src)
    qual = None
    if source.get("qual") is not None:
        qual = np.zeros(2 * room, np.uint8)
        qual[dst] = np.asarray(source["qual"])[src]
    return dict(v, seq_nib=new.astype(np.uint32), seq=nib[0::2] | nib[1::2] << 4, qual=qual, fields=False, room=room)
