"""Sequence layouts for the tile walk's staging decisions (process_chunk, basecount_amd/csrc/bc_tile.h)
and a CPU model of those decisions.

``place`` builds a batch whose reads' bases lie at chosen byte offsets of ``seq``; ``chunk_plan``
restates, from the header's comments, what process_chunk decides for every chunk of every tile
(speculative copy, speculation holds, restage, unstaged, complex; gap; largest run count);
``cases`` names the layouts tests/test_stage_layouts_host.py proves and
tests/test_gpu_stage_layouts.py runs.  Nothing here imports the device library.

A read is (pos, [(op, len)], base codes, qualities) as in test_gpu_tile_tail.build_batch."""
import functools

import numpy as np

M, I, DEL, SKIP, S, EQ, X = 0, 1, 2, 3, 4, 7, 8  # CIGAR ops
ACGT = np.array([1, 2, 4, 8], np.uint8)          # BAM 4-bit base codes
OTHER = np.array([15, 0, 5, 3], np.uint8)        # N and codes no column counts
TILE = 64
STG, LEAN_STG = 6144, 6016  # kStage, kLeanStage: a wave's stage in bytes
SPEC_SLACK = 128            # kSpecSlack: bytes copied beyond the last read's first base
K_PRE, MAX_RUNS = 8, 4      # bc_runs.h: CIGAR words decoded per read, runs per table
KINDS = ("spec_hit", "restaged", "staged_no_spec", "unstaged", "complex")
NP_BUF = 8192               # numpy's pairwise-sum buffer: the read-parallel summary needs L >= this
FAR = 40_000                # bytes between a far straggler and its chunk


def seq_event_bytes(n):
    """bc_seq_event_bytes: the device's sequence buffer for n packed bytes."""
    return (n + 15) // 16 * 16 + 16


def query_len(ops):
    return sum(ln for op, ln in ops if op in (M, I, S, EQ, X))


def ref_span(ops):
    return sum(ln for op, ln in ops if op in (M, DEL, SKIP, EQ, X))


def read_of(rng, pos, ops):
    """A read with the given CIGAR: random bases with 5 % non-ACGT codes, qualities 0-44."""
    q = query_len(ops)
    codes = ACGT[rng.integers(0, 4, q)]
    other = rng.random(q) < 0.05
    codes[other] = OTHER[rng.integers(0, 4, int(other.sum()))]
    return (int(pos), list(ops), codes, rng.integers(0, 45, q).astype(np.uint8))


def nbytes_of(read):
    return (len(read[2]) + 1) // 2


def place(reads, offsets, tail_pad=2, seq_bytes=None, with_qual=True):
    """The batch dict of test_gpu_parity.build_batch for reads in start order, read i's first byte at
    byte ``offsets[i]`` of ``seq`` (its first base in that byte's high nibble) and its qualities
    at the same nibble index of ``qual``.  The arrays end ``tail_pad`` nibbles after the last base
    of the read that lies last: with 0 that base is the arrays' last nibble and ``qual``'s last
    byte is its quality.  ``seq_bytes`` asks for a larger (zero-filled) ``seq``; ``with_qual``
    False leaves ``qual`` out (min_base_quality 0 only)."""
    pos = [r[0] for r in reads]
    assert pos == sorted(pos) and len(offsets) == len(reads)
    offsets = [int(o) for o in offsets]
    spans = sorted((o, o + nbytes_of(r)) for o, r in zip(offsets, reads))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "reads overlap in seq"
    nibbles = max(2 * o + len(r[2]) for o, r in zip(offsets, reads)) + tail_pad
    size = (nibbles + 1) // 2
    assert seq_bytes is None or seq_bytes >= size
    seq = np.zeros(size if seq_bytes is None else seq_bytes, np.uint8)
    qual = np.zeros(nibbles if seq_bytes is None else 2 * seq_bytes, np.uint8) if with_qual else None
    for o, (_, _, codes, q) in zip(offsets, reads):
        c = np.zeros(2 * nbytes_of((0, 0, codes)), np.uint8)
        c[:len(codes)] = codes
        seq[o: o + c.size // 2] = (c[0::2] << 4) | c[1::2]
        if with_qual:
            qual[2 * o: 2 * o + len(q)] = q
    cig_n = np.array([len(r[1]) for r in reads], np.uint32)
    cig_beg = np.zeros(len(reads), np.uint32)
    cig_beg[1:] = np.cumsum(cig_n)[:-1]
    clip = [r[1][0][1] if r[1][0][0] == S else 0 for r in reads]
    b = dict(pos=np.array(pos, np.int32), cig_beg=cig_beg, cig_n=cig_n,
             seq_nib=np.array([2 * o + c for o, c in zip(offsets, clip)], np.uint32),
             cigar=np.array([(ln << 4) | op for r in reads for op, ln in r[1]], np.uint32), seq=seq)
    if with_qual:
        b["qual"] = qual
    return b


# ---------------------------------------------------------------- the model of process_chunk
def decode_runs(ops):
    """bc_runs.h decode_runs over a read's first K_PRE ops -> (nrun, gap, complex, span, qlen):
    M / = / X ops with the same query delta merge into one run, a read is complex with more than
    K_PRE ops, more than MAX_RUNS runs, a delta outside +-32767 or a span of 0x1FFF or more."""
    cx, gap = len(ops) > K_PRE, False
    rc = qc = nrun = 0
    last_en, last_qd = None, 0
    for op, ln in ops[:K_PRE]:
        m, d = op in (M, EQ, X) and ln != 0, op in (DEL, SKIP) and ln != 0
        qd = qc - rc
        new = m and not (last_en == rc and last_qd == qd)
        cx = cx or (m and not -32768 <= qd <= 32767) or (new and nrun >= MAX_RUNS)
        nrun += new
        gap = gap or d
        if m:
            last_en, last_qd = rc + ln, qd
        if m or d:
            rc += ln
        if m or op == I:
            qc += ln
    return nrun, gap, cx or rc >= 0x1FFF, rc, qc


def cigars(b):
    w, beg, n = b["cigar"], b["cig_beg"].astype(np.int64), b["cig_n"].astype(np.int64)
    return [[(int(x) & 15, int(x) >> 4) for x in w[beg[i]: beg[i] + n[i]]] for i in range(n.size)]


def max_span_of(b):
    return max(ref_span(c) for c in cigars(b))


def max_end_of(b):
    return max(int(p) + ref_span(c) for p, c in zip(b["pos"], cigars(b)))


class _Fields:
    """Per-read inputs of the chunk decisions."""

    def __init__(self, b, lean):
        dec = [decode_runs(c) for c in cigars(b)]
        self.sn = [int(x) for x in b["seq_nib"]]
        self.nrun = [d[0] for d in dec]
        self.gap = [d[1] for d in dec]
        self.cx = [d[2] for d in dec]
        self.qlen = [d[4] for d in dec]
        self.slow = [lean and (d[2] or d[1] or d[0] > 1) for d in dec]
        end = seq_event_bytes(int(b["seq"].size))
        self.buf_end = end if end < 0xFFFFFFFF else 0xFFFFFFF0


def _classify(F, i0, i1, lean, qual):
    """process_chunk's decisions for the reads [i0, i1) taken as one chunk."""
    stg = LEAN_STG if lean else STG
    spec, spec_lo, spec_hi, clamped = False, 0, 0, False
    if not qual:
        spec_lo = (F.sn[i0] >> 1) & ~15
        spec_hi = (F.sn[i1 - 1] >> 1) + SPEC_SLACK
        clamped = spec_hi > F.buf_end
        spec_hi = min(spec_hi, F.buf_end)
        spec = spec_hi > spec_lo and spec_hi - spec_lo <= stg
    rng = range(i0, i1)
    cx = not lean and any(F.cx[i] for i in rng)
    gap = not lean and any(F.gap[i] for i in rng)
    mr = 1 if lean else max(F.nrun[i] for i in rng)
    lo, hi = 0xFFFFFFFF, 0
    for i in rng:
        if F.qlen[i] and not F.slow[i]:
            lo = min(lo, F.sn[i] >> 1)
            hi = max(hi, (F.sn[i] + F.qlen[i] + 1) >> 1)
    lo = lo & ~15 if hi > lo else 0
    spec_ok = spec and not cx and (hi <= lo or (lo >= spec_lo and hi <= spec_hi))
    staged = not cx and (spec_ok or hi - lo <= stg)
    kind = ("complex" if cx else "unstaged" if not staged else "spec_hit" if spec_ok else
            "restaged" if spec else "staged_no_spec")
    return dict(base=i0, nr=i1 - i0, kind=kind, gap=gap, maxrun=1 if mr <= 1 else 2 if mr == 2 else 4, seg_len=hi - lo,
                seg_lo=lo, seg_hi=hi, spec=spec, spec_lo=spec_lo, spec_hi=spec_hi, clamped=clamped,
                slow=sum(F.slow[i] for i in rng))


def chunk_plan(b, L, lean=False, qual=False, windows=False):
    """What process_chunk decides for every chunk of every tile of the batch on a reference of L
    positions: a list of dicts with tile, base (first read), nr, kind (one of KINDS), gap, maxrun
    (1, 2, 4), seg_len (bytes of the exact segment from its 16-byte rounded start), spec (a
    speculative copy was issued), clamped (its end was cut at the buffer's), slow (lean: reads
    walked alone).  The chunks of tile t are the reads [lo + 64 j, min(lo + 64 j + 64, hi)), lo the
    first pos > 64 t - max_span, hi the first pos >= 64 t + 64.

    lean: the lean instance (6,016-byte stage; slow reads leave the segment, the chunk is never
    "complex" or gapped; "unstaged" means the whole chunk goes to walk_complex).  qual: a quality
    threshold is set (no speculation: every staged chunk is "staged_no_spec").

    windows: the sweep kernels start their chunks at a cursor this model does not follow, so
    instead of tiles every window of 2-64 consecutive reads is classified (tile = -1): a class
    that holds for all of them holds for whatever chunks the sweep forms."""
    F = _Fields(b, lean)
    n = len(F.sn)
    out = []
    if windows:
        for i0 in range(n):
            for i1 in range(i0 + 2, min(i0 + 64, n) + 1):
                out.append(dict(_classify(F, i0, i1, lean, qual), tile=-1))
        return out
    pos = b["pos"].astype(np.int64)
    span = max_span_of(b)
    reach = max(int(L), max_end_of(b))
    for t in range((reach + TILE - 1) // TILE):
        lo = int(np.searchsorted(pos, TILE * t - span, "right"))
        hi = int(np.searchsorted(pos, TILE * t + TILE, "left"))
        for i0 in range(lo, hi, 64):
            out.append(dict(_classify(F, i0, min(i0 + 64, hi), lean, qual), tile=t))
    return out


def header(b):
    """What bc_pileup_plan reads of a batch."""
    return dict(n_reads=int(b["pos"].size), max_span=max_span_of(b), max_end=max_end_of(b),
                n_cigar_words=int(b["cigar"].size))


def sparse_length(b, L):
    """The shortest reference of whole 8,192-position buffers + 100 on which the batch is sparse
    enough for the one-wave sweep (bc_internal.h: at most 48 reads walked per tile on average) and
    long enough for the read-parallel summary: the reads keep their places, the rest is empty."""
    h = header(b)
    m = 1
    while h["n_reads"] * (h["max_span"] + 63) / (NP_BUF * m + 100) > 47.0:
        m += 1
    return max(NP_BUF * m + 100, L)


# ---------------------------------------------------------------- layouts
def packed(reads, start=0):
    """Byte offsets of reads laid one after the other from ``start``."""
    off, at = [], start
    for r in reads:
        off.append(at)
        at += nbytes_of(r)
    return off


def cluster_spacing(span):
    """Clusters of reads that start within 40 positions, this far apart, share no tile: a cluster of
    m reads is walked as the chunks [64 j, min(64 j + 64, m)) of its own reads by each of its tiles."""
    return TILE * -(-(40 + span) // TILE)


def clustered(rng, cigar_lists, spacing, width=40):
    """Reads in clusters: cluster c's reads (one per CIGAR of cigar_lists[c]) start in
    [c * spacing, c * spacing + width), sorted; -> (reads, [first read of each cluster] + [n])."""
    reads, first = [], [0]
    for c, cl in enumerate(cigar_lists):
        pos = np.sort(rng.integers(0, width, len(cl))) + c * spacing
        reads += [read_of(rng, p, ops) for p, ops in zip(pos, cl)]
        first.append(len(reads))
    return reads, first


def straggle(reads, first, far, rng, start=0):
    """Offsets with one straggler per chunk of every cluster: the chunk's other reads lie in order,
    the straggler (an all-M read, never the chunk's first or last) just before them, or FAR bytes
    behind everything (far)."""
    off = [0] * len(reads)
    at, late = start, []
    for c0, c1 in zip(first, first[1:]):
        for i0 in range(c0, c1, 64):
            i1 = min(i0 + 64, c1)
            cand = [i for i in range(i0 + 1, i1 - 1) if len(reads[i][1]) == 1]
            s = cand[int(rng.integers(0, len(cand)))] if cand else -1
            if s >= 0 and far:
                late.append(s)
            elif s >= 0:
                off[s] = at
                at += nbytes_of(reads[s])
            for i in range(i0, i1):
                if i != s:
                    off[i] = at
                    at += nbytes_of(reads[i])
    at += FAR
    for s in late:
        off[s] = at
        at += nbytes_of(reads[s])
    return off


def uniform_reads(rng, n, L, lengths):
    pos = np.sort(rng.integers(0, L - max(lengths), n))
    return [read_of(rng, p, [(M, int(lengths[i % len(lengths)]))]) for i, p in enumerate(pos)]


def _in_order_150(rng):
    reads = uniform_reads(rng, 1200, 1024, [150])
    return place(reads, packed(reads)), 1024


def _reversed_stride256(rng):
    reads = uniform_reads(rng, 600, 1024, [150])
    return place(reads, [(len(reads) - 1 - i) * 256 for i in range(len(reads))]), 1024


STRAGGLER_SIZES = (64, 94, 128, 17, 133)  # reads per cluster: full chunks, short ones, a last cluster of three


def _straggler(rng, far, L=None):
    sp = cluster_spacing(150)
    reads, first = clustered(rng, [[[(M, 150)]] * m for m in STRAGGLER_SIZES], sp)
    return place(reads, straggle(reads, first, far, rng)), L or sp * len(STRAGGLER_SIZES)


def _round_down(rng):
    """The 16-byte round-down of the speculative copy's start: a 16-base read in the 8 bytes before
    the chunk's first read, which starts 8 mod 16 (first cluster: the copy covers the small read) or
    0 mod 16 (second cluster: it does not)."""
    sp = cluster_spacing(150)
    cl = [[[(M, 150)]] * 5 + [[(M, 16)]] + [[(M, 150)]] * 30] * 2
    reads, first = clustered(rng, cl, sp)
    off, at = [0] * len(reads), 0
    for c, (c0, c1) in enumerate(zip(first, first[1:])):
        small = next(i for i in range(c0, c1) if len(reads[i][2]) == 16)
        assert small not in (c0, c1 - 1)
        at = (at + 15) // 16 * 16 + 16 + (0 if c == 0 else 8)  # the small read: 0 / 8 mod 16
        off[small] = at
        at += 8
        for i in range(c0, c1):
            if i != small:
                off[i] = at
                at += nbytes_of(reads[i])
    return place(reads, off), 640


def _long_tail_300(rng):
    sp = cluster_spacing(300)
    cl = [[[(M, 300)]] * 20, [[(M, 300)]] * 7, [[(M, 150)]] * 12 + [[(M, 256)]], [[(M, 150)]] * 12 + [[(M, 258)]],
          [[(M, 300)]]]
    reads, first = clustered(rng, cl, sp)
    # a cluster's longest read lies last in seq (sorted starts: make it the last read as well)
    for c0, c1 in zip(first, first[1:]):
        grp = sorted(reads[c0:c1], key=lambda r: len(r[2]))
        for i, p in enumerate(sorted(r[0] for r in grp)):
            reads[c0 + i] = (p,) + grp[i][1:]
    # every cluster's last read starts on a 16-byte boundary: the copy ends at the slack's end to the
    # byte (LDS-DMA moves 16-byte pieces: an unaligned end would bring the bytes behind it along)
    off, at = [], 0
    for c0, c1 in zip(first, first[1:]):
        before = sum(nbytes_of(r) for r in reads[c0:c1 - 1])
        off += packed(reads[c0:c1], (at + 15) // 16 * 16 + -before % 16)
        at = off[-1] + nbytes_of(reads[c1 - 1])
    return place(reads, off), sp * len(cl)


def exact_fit_chunks(lean):
    """(first byte mod 16, read lengths) of the 64-read chunks of exact_fit: segments of exactly the
    stage and of 1, 16, 8 and 15 bytes more, at each alignment one that fits."""
    n = 188 if lean else 192  # 64 reads of n bases fill the stage
    full = lambda k: [n - 1, n] * 16 + [n] * (32 - k) + [n + 1] * k  # 64 reads, k of them a byte longer
    return [(0, full(0)), (0, full(1)), (0, full(16)), (8, full(0)), (15, full(0)),
            (8, full(0)[:63] + [n - 16]), (15, full(0)[:63] + [n - 30])]


def _exact_fit(rng, lean):
    chunks = exact_fit_chunks(lean)
    sp = cluster_spacing(194)
    # (starts within 4 positions: no tile sees only the reads that start late in a cluster)
    reads, first = clustered(rng, [[[(M, ln)] for ln in lens] for _, lens in chunks], sp, width=4)
    off, at = [], 0
    for (al, _), c0, c1 in zip(chunks, first, first[1:]):
        at = (at + 15) // 16 * 16 + 256 + al
        off += packed(reads[c0:c1], at)
        at = off[-1] + nbytes_of(reads[c1 - 1])
    return place(reads, off), sp * len(chunks)


EDGE_VARIANTS = ((0, 0), (1, 1), (15, 0), (0, 1))  # (first byte of the buffer's first read, odd total)


def _buffer_edges(rng, start, odd):
    sp = cluster_spacing(150)
    cl = [[[(M, 150)]] * 40, [[(M, 150)]] * 64, [[(M, 150)]] * 9 + [[(M, 149 if odd else 150)]]]
    reads, first = clustered(rng, cl, sp)
    c0 = first[2]
    grp = sorted(reads[c0:], key=lambda r: -len(r[2]))  # the odd read last
    for i, p in enumerate(sorted(r[0] for r in grp)):
        reads[c0 + i] = (p,) + grp[i][1:]
    return place(reads, packed(reads, start), tail_pad=0), 640


def _kind_ops(kind, n=150):
    a = n // 4
    return {"plain": [(M, n)],
            "clip": [(S, 4), (M, n - 6), (S, 2)],
            "ins": [(M, a), (I, 2), (M, n - a - 2)],                               # two runs, no gap
            "tail_skip": [(M, n), (SKIP, 6)],                                      # one run, a gap
            "del": [(M, a), (DEL, 3), (EQ, n - a)],                                # two runs, a gap
            "ins2": [(M, a), (I, 1), (X, a), (I, 3), (M, n - 2 * a - 4)],          # three runs, no gap
            "ins3": [(M, a), (I, 1), (M, a), (I, 1), (M, a), (I, 2), (M, n - 3 * a - 4)],  # four runs
            "del_ins": [(M, a), (DEL, 2), (M, a), (I, 2), (M, n - 2 * a - 2)],     # three runs, a gap
            "del_skip": [(M, a), (DEL, 1), (M, a), (SKIP, 5), (M, a), (I, 1), (M, n - 3 * a - 1)],  # four runs, a gap
            "many": [(M, 20), (I, 1), (M, 20), (DEL, 1), (M, 20), (I, 1), (M, 20), (DEL, 2), (M, 20), (I, 1),
                     (M, n - 103)]}[kind]                                          # more than 8 ops


# cluster -> the kinds salted into plain reads: (gap, maxrun) = (F,1) (F,2) (T,1) (T,2) (F,4) (T,4), complex
MATRIX = (("plain", "clip"), ("ins",), ("tail_skip",), ("del",), ("ins2", "ins3"), ("del_ins", "del_skip"), ("many",))
MATRIX_SIZE = 84  # reads per cluster: a full chunk and one of 20


def _runs_matrix(rng, far):
    cl = []
    for kinds in MATRIX:
        ks = ["plain" if i % 3 else kinds[(i // 3) % len(kinds)] for i in range(MATRIX_SIZE)]
        if kinds == ("many",):  # a few complex reads, in the full chunk only
            ks = ["many" if i in (5, 40, 63) else "plain" for i in range(MATRIX_SIZE)]
        cl.append([_kind_ops(k) for k in ks])
    sp = cluster_spacing(max(ref_span(o) for c in cl for o in c))
    reads, first = clustered(rng, cl, sp)
    off = straggle(reads, first, True, rng) if far else packed(reads)
    return place(reads, off), sp * len(cl)


HIGH_SEQ_BYTES = (1 << 30) + 65_536
HIGH_FIRST_BYTE = (1 << 30) + 2_048 + 16  # every base above nibble 2^31 + 4,096


def high_nibbles(layout, with_qual):
    """Reads of 150 and of 250 bases on L = 2,048 whose bases all lie above nibble 2^31 + 4,096 of a
    seq array of 2^30 + 65,536 bytes: 560 reads in order (staged), or 240 reads, read i's bytes at
    (n - 1 - i) * 256 from there (what the array holds at that stride; unstaged).  Not cached: the
    arrays are 1 GiB (and 2 GiB of qualities)."""
    rng = np.random.default_rng(77 + (layout == "reversed"))
    n = 560 if layout == "in_order" else 240
    reads = uniform_reads(rng, n, 2048, [150, 250])
    off = packed(reads, HIGH_FIRST_BYTE)
    if layout == "reversed":
        off = [HIGH_FIRST_BYTE + (n - 1 - i) * 256 for i in range(n)]
    b = place(reads, off, seq_bytes=HIGH_SEQ_BYTES, with_qual=with_qual)
    assert int(b["seq_nib"].min()) > (1 << 31) + 4096
    return b, 2048


def _cut(b, L):
    """A reference cut inside the last cluster's reach: its reads run past the end."""
    return b, int(b["pos"][-1]) + 100


BUILDERS = {
    "in_order_150": _in_order_150,
    "reversed_stride256": _reversed_stride256,
    "straggler_near": lambda rng: _straggler(rng, False),
    "straggler_far": lambda rng: _straggler(rng, True),
    "round_down": _round_down,
    "long_tail_300": _long_tail_300,
    "exact_fit": lambda rng: _exact_fit(rng, False),
    "exact_fit_lean": lambda rng: _exact_fit(rng, True),
    **{f"buffer_edges_{s}_{'odd' if o else 'even'}": (lambda rng, s=s, o=o: _buffer_edges(rng, s, o))
       for s, o in EDGE_VARIANTS},
    "runs_matrix_in_order": lambda rng: _runs_matrix(rng, False),
    "runs_matrix_far": lambda rng: _runs_matrix(rng, True),
    "cut_short_near": lambda rng: _cut(*_straggler(rng, False)),
    "cut_short_far": lambda rng: _cut(*_straggler(rng, True)),
}
EDGE_CASES = tuple(n for n in BUILDERS if n.startswith("buffer_edges"))
CUT_CASES = ("cut_short_near", "cut_short_far")


def cases():
    """The named cases (high_nibbles apart: high_nibbles())."""
    return tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """(batch, L) of a named case; built once, never changed."""
    b, L = BUILDERS[name](np.random.default_rng(sum(map(ord, name))))
    assert 640 <= L <= 2048 and b["pos"].size <= 1500
    for a in b.values():
        a.setflags(write=False)
    return b, L


@functools.lru_cache(maxsize=None)
def expected(name, L, mbq):
    """The oracle's counts [L][6] and (first offending read, position) of a case on L positions."""
    import oracle as O
    cnt, bad = O.bcount(L, mbq, case(name)[0])
    cnt.setflags(write=False)
    return cnt, bad
