"""Batch builders and launch helpers shared by test_gpu_saturation.py, test_gpu_cigar_edges.py,
test_gpu_quality_range.py and test_saturation_inputs.py (a plain module, no fixtures).

Three families of deterministic inputs, all in the bc_reads layout of include/basecount_hip.h:

* ``hot_batch(d)``: blocks of d identical short reads, 128 positions apart, one content each, so
  that one (position, column) takes the whole depth d and the kernels' narrow counters (4-bit
  nibbles, byte sums, the event image's digits, 16-bit LDS halves) reach their stated bounds;
  ``hot_complex_batch(d)``: d identical 9-op reads per block (the six 10-bit fields of
  walk_complex / flush_acc).
* ``catalogue_ops()`` / ``catalogue_batch()``: hand-written reads on either side of every threshold of
  decode_runs / decode_fast2 / pack_runs (bc_runs.h).
* ``quality_batch()``: quality bytes over the whole 0..255 range.

Everything the GPU tests expect comes from oracle.bcount / oracle.stats; where a closed form
exists (hot blocks) ``hot_closed_form`` gives it without the oracle."""
import functools

import numpy as np

import oracle as O
import wide_index as WI
from basecount_amd import device as D
from basecount_amd.main import norm_factors

A, C_, G, T, N, IUPAC_M, EQ = 1, 2, 4, 8, 15, 3, 0     # BAM 4-bit base codes ('M' = A/C, '=')
LETTERS = np.array([A, C_, G, T, N, IUPAC_M, EQ], np.uint8)
M, I, DEL, SKIP, S, H, P, EQOP, X, B = range(10)        # CIGAR ops
REF_OPS, STORED_OPS = (M, DEL, SKIP, EQOP, X), (M, I, S, EQOP, X)

K_TILE_MAX_SPAN = 4096  # bc_internal.h kTileMaxSpan: longer spans always take k_rc
K_WIN_MAX = 4096        # bc_internal.h kWinMax: k_count's LDS window

# depths of Part A, each next to a bound of the packed counters (see test_gpu_saturation.py)
DEPTHS = (14, 15, 16, 17, 31, 32, 33, 112, 113, 120, 128, 129, 255, 256, 257, 511, 512, 513,
          1022, 1023, 1024, 1025, 2047, 4096, 65535, 65536, 65537)
COMPLEX_DEPTHS = (1022, 1023, 1024, 1025, 2047)

# (shape, tile_waves, k_rc input mode): every launch shape of a sorted batch
TILED_SHAPES = (("tile", 1, None), ("tile_no_solo", 1, None), ("tile", 2, None), ("tile", 4, None),
                ("tile", 8, None))
RC_SHAPES = (("rc", 0, "records+summaries"), ("rc", 0, "cigars"), ("rc", 0, "records"))


def w(op, ln):
    return (ln << 4) | op


def stored_len(ops):
    """Bases a read's record stores: M / I / S / = / X."""
    return sum(ln for op, ln in ops if op in STORED_OPS)


def ref_span(ops):
    return sum(ln for op, ln in ops if op in REF_OPS)


def pack_batch(reads, sort=True, tight=False):
    """The batch dict of reads given as (pos, [(op, len)], codes, quals); each read's SEQ starts
    on a byte boundary; coordinate-sorted (stable) unless ``sort`` is False.  ``tight``: no padding
    after the last read, so qual ends with (or one byte after) the last base."""
    if sort:
        reads = sorted(reads, key=lambda r: r[0])
    nib = np.zeros(len(reads) + 1, np.int64)
    nib[1:] = np.cumsum([len(r[2]) + (len(r[2]) & 1) for r in reads])
    pad = 0 if tight else 2
    allc = np.zeros(int(nib[-1]) + pad, np.uint8)
    qual = np.zeros(int(nib[-1]) + pad, np.uint8)
    for i, (_, _, s, q) in enumerate(reads):
        allc[nib[i]: nib[i] + len(s)] = s
        qual[nib[i]: nib[i] + len(q)] = q
    cig_n = np.array([len(r[1]) for r in reads], np.uint32)
    cig_beg = np.zeros(len(reads), np.uint32)
    cig_beg[1:] = np.cumsum(cig_n)[:-1]
    qstart = np.array([r[1][0][1] if r[1] and r[1][0][0] == S else 0 for r in reads], np.int64)
    return dict(pos=np.array([r[0] for r in reads], np.int32), cig_beg=cig_beg, cig_n=cig_n,
                seq_nib=(nib[:-1] + qstart).astype(np.uint32),
                cigar=np.array([w(op, ln) for r in reads for op, ln in r[1]], np.uint32),
                seq=((allc[0::2] << 4) | allc[1::2]).astype(np.uint8), qual=qual)


def spans(b):
    """Every read's reference span (M / D / N / = / X bases)."""
    cg = b["cigar"].astype(np.int64)
    ref = np.where(np.isin(cg & 15, REF_OPS), cg >> 4, 0)
    cs = np.concatenate([[0], np.cumsum(ref)])
    beg = b["cig_beg"].astype(np.int64)
    return cs[beg + b["cig_n"].astype(np.int64)] - cs[beg]


def max_end(b):
    return int((b["pos"].astype(np.int64) + spans(b)).max())


def permuted(b, seed=5):
    """The same reads in a random order (an unsorted batch: bc_count takes k_count)."""
    p = np.random.default_rng(seed).permutation(b["pos"].size)
    return dict(b, pos=b["pos"][p], cig_beg=b["cig_beg"][p], cig_n=b["cig_n"][p], seq_nib=b["seq_nib"][p])


# ------------------------------------------------------------------------------- hot batches
HOT_FIRST, HOT_STEP, HOT_LEN = 60, 128, 16  # first block at 60 (mod 64): over a window and a tile edge
# block contents: letter(s) and whether every / every other read is `1M 14D 1M`
HOT_BLOCKS = ("A", "C", "G", "T", "N", "del", "A/N", "T/del")
HOT_L = HOT_FIRST + HOT_STEP * (len(HOT_BLOCKS) - 1) + HOT_LEN  # the last block ends exactly here


def hot_starts():
    return [HOT_FIRST + HOT_STEP * j for j in range(len(HOT_BLOCKS))]


RUNS3_OPS = ((M, 5), (DEL, 1), (M, 5), (DEL, 1), (M, 4))  # span 16, three runs, 14 bases


@functools.lru_cache(maxsize=4)
def hot_batch(d, runs3=False, qual=40):
    """Coordinate-sorted blocks of d short reads, 128 positions apart, each block one content:
    all A / C / G / T / N (`16M`), all `1M 14D 1M` (letter A), A and N reads interleaved read by
    read, T reads and `1M 14D 1M` (letter T) reads interleaved.  Every quality is ``qual``.
    The last block ends exactly at HOT_L; counting with ref_len = HOT_L - 3 makes its reads run 3
    positions past the end.
    ``runs3``: every `16M` read is `5M 1D 5M 1D 4M` instead: three runs, which the event image of
    k_rc does not take (its chunks walk the run tables) and the tiled kernels walk with four run
    slots."""
    nb = len(HOT_BLOCKS)
    letter = np.zeros((nb, d), np.uint8)
    gap = np.zeros((nb, d), bool)  # the read is 1M 14D 1M
    odd = (np.arange(d) & 1) == 1
    for j, c in enumerate(HOT_BLOCKS):
        letter[j] = {"A": A, "C": C_, "G": G, "T": T, "N": N, "del": A, "A/N": A, "T/del": T}[c]
        if c == "A/N":
            letter[j, odd] = N
        gap[j] = True if c == "del" else (odd if c == "T/del" else False)
    letter, gap = letter.ravel(), gap.ravel()
    n = nb * d
    plain = [w(op, ln) for op, ln in RUNS3_OPS] if runs3 else [w(M, HOT_LEN)]
    qlen = np.where(gap, 2, stored_len(RUNS3_OPS) if runs3 else HOT_LEN).astype(np.int64)  # all even
    seq_nib = np.concatenate([[0], np.cumsum(qlen)[:-1]])
    codes = np.repeat(letter, qlen)
    codes = np.concatenate([codes, np.zeros(2, np.uint8)])
    cig_n = np.where(gap, 3, len(plain)).astype(np.uint32)
    cig_beg = np.concatenate([[0], np.cumsum(cig_n)[:-1]]).astype(np.int64)
    cigar = np.zeros(int(cig_n.sum()), np.uint32)
    for i, word in enumerate(plain):
        cigar[cig_beg[~gap] + i] = word
    for i, word in enumerate((w(M, 1), w(DEL, HOT_LEN - 2), w(M, 1))):
        cigar[cig_beg[gap] + i] = word
    pos = np.repeat(np.array(hot_starts(), np.int32), d)
    b = dict(pos=pos, cig_beg=cig_beg.astype(np.uint32), cig_n=cig_n, seq_nib=seq_nib.astype(np.uint32),
             cigar=cigar, seq=((codes[0::2] << 4) | codes[1::2]).astype(np.uint8),
             qual=np.full(codes.size, qual, np.uint8))
    assert n == pos.size
    return b


def hot_closed_form(d, runs3=False):
    """hot_batch(d, runs3)'s counts [HOT_L][6], written down without the oracle."""
    c = np.zeros((HOT_L, 6), np.uint32)
    col = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 5}
    plain = np.ones(HOT_LEN, bool)  # offsets where a plain read counts its letter (else a deletion)
    if runs3:
        plain[[5, 11]] = False
    gapped = np.zeros(HOT_LEN, bool)
    gapped[[0, HOT_LEN - 1]] = True
    for s, blk in zip(hot_starts(), HOT_BLOCKS):
        # (letter column, letter offsets, reads) of the even-numbered and the odd-numbered reads
        kinds = {"del": [(0, gapped, d)], "A/N": [(0, plain, (d + 1) // 2), (5, plain, d // 2)],
                 "T/del": [(3, plain, (d + 1) // 2), (3, gapped, d // 2)]}.get(blk) or [(col[blk], plain, d)]
        for cl, at, n in kinds:
            c[s: s + HOT_LEN, cl] += np.where(at, n, 0).astype(np.uint32)
            c[s: s + HOT_LEN, 4] += np.where(at, 0, n).astype(np.uint32)
    return c


COMPLEX_OPS = ((S, 2), (M, 5), (I, 1), (M, 5), (DEL, 1), (M, 5), (P, 1), (M, 5), (S, 1))  # 9 ops, 3 runs
COMPLEX_STARTS, COMPLEX_LETTERS = (60, 188), (A, N)
COMPLEX_L = COMPLEX_STARTS[-1] + ref_span(COMPLEX_OPS)


@functools.lru_cache(maxsize=2)
def hot_complex_batch(d, qual=40):
    """Two blocks (all A at 60, all N at 188) of d identical reads `2S 5M 1I 5M 1D 5M 1P 5M 1S`:
    nine ops, so every read takes the kernels' complex path (cig_n > kPre)."""
    st = stored_len(COMPLEX_OPS)  # 24: even
    n = d * len(COMPLEX_STARTS)
    words = np.array([w(op, ln) for op, ln in COMPLEX_OPS], np.uint32)
    codes = np.concatenate([np.repeat(np.array(COMPLEX_LETTERS, np.uint8), d * st), np.zeros(2, np.uint8)])
    return dict(pos=np.repeat(np.array(COMPLEX_STARTS, np.int32), d),
                cig_beg=(np.arange(n) * words.size).astype(np.uint32), cig_n=np.full(n, words.size, np.uint32),
                seq_nib=(np.arange(n) * st + COMPLEX_OPS[0][1]).astype(np.uint32), cigar=np.tile(words, n),
                seq=((codes[0::2] << 4) | codes[1::2]).astype(np.uint8), qual=np.full(codes.size, qual, np.uint8))


def complex_closed_form(d):
    c = np.zeros((COMPLEX_L, 6), np.uint32)
    for s, col in zip(COMPLEX_STARTS, (0, 5)):
        c[s: s + 10, col] = d
        c[s + 10, 4] = d
        c[s + 11: s + 21, col] = d
    return c


def plain_batch(pos, codes, qual):
    """All-M reads of one (even) length: codes [n][len], starts ``pos`` (given in order), qual a
    byte or an array [n * len]."""
    n, ln = codes.shape
    assert ln % 2 == 0
    flat = np.concatenate([codes.ravel().astype(np.uint8), np.zeros(2, np.uint8)])
    q = np.full(flat.size, qual, np.uint8) if np.isscalar(qual) else np.concatenate([qual, np.zeros(2, np.uint8)])
    return dict(pos=np.asarray(pos, np.int32), cig_beg=np.arange(n, dtype=np.uint32), cig_n=np.ones(n, np.uint32),
                seq_nib=(np.arange(n) * ln).astype(np.uint32), cigar=np.full(n, w(M, ln), np.uint32),
                seq=((flat[0::2] << 4) | flat[1::2]).astype(np.uint8), qual=q.astype(np.uint8))


def full_halves_batch(n=32768):
    """Two chunks of n reads: `16M` of the letters C A T G N ... at 60, then n - 1 reads all C and
    one all A at 188."""
    row = np.array([C_, A, T, G, N] * 4, np.uint8)[:16]
    codes = np.concatenate([np.tile(row, (n, 1)), np.full((n - 1, 16), C_, np.uint8), np.full((1, 16), A, np.uint8)])
    return plain_batch(np.repeat([60, 188], n), codes, 40)


def window_batch(wlen, seed=3):
    """Two 64-read chunks of `16M` reads with random letters and quality bytes; chunk 0's
    pos[last] - pos[first] + max_span is ``wlen`` (kWinMax = 4096 is the last that takes LDS)."""
    rng = np.random.default_rng(seed)
    first = 100
    p0 = np.sort(np.concatenate([[first, first + wlen - 16], rng.integers(first, first + wlen - 15, 62)]))
    p1 = np.sort(rng.integers(p0[-1], p0[-1] + 500, 64))
    n = 128
    return plain_batch(np.concatenate([p0, p1]), LETTERS[rng.integers(0, 7, (n, 16))],
                          rng.integers(0, 256, n * 16).astype(np.uint8))


def chunk_window(b, rpb, chunk=0):
    p = b["pos"][chunk * rpb: (chunk + 1) * rpb].astype(np.int64)
    return int(p[-1] - p[0] + spans(b).max())


# ------------------------------------------------------------------------------ random reads
def random_reads(rng, n, lo, hi, qmax=256, letters=LETTERS):
    """n short reads inside [lo, hi): soft clips, an insertion, a deletion or a short skip, letters
    from A C G T N M =, quality bytes uniform below ``qmax``."""
    out = []
    for _ in range(n):
        ops = []
        if rng.random() < 0.3:
            ops.append((S, int(rng.integers(1, 5))))
        ops.append((M, int(rng.integers(3, 40))))
        kind = int(rng.integers(0, 4))
        if kind:
            ops += [((I, DEL, SKIP)[kind - 1], int(rng.integers(1, 6))), (M, int(rng.integers(3, 40)))]
        if rng.random() < 0.3:
            ops.append((S, int(rng.integers(1, 5))))
        span = ref_span(ops)
        if span > hi - lo:
            continue
        q = stored_len(ops)
        out.append((int(rng.integers(lo, hi - span + 1)), ops, letters[rng.integers(0, letters.size, q)],
                    rng.integers(0, qmax, q).astype(np.uint8)))
    return out


# ---------------------------------------------------------------------------- CIGAR catalogue
def catalogue_ops():
    """{name: [(op, len)]}: the read on either side of each decode threshold of bc_runs.h.  Names
    ending in ``@long`` have a span above kTileMaxSpan (k_rc whatever the shape)."""
    c = {}
    # cig_n against kPre = 8, runs against kMaxRuns = 4
    c["ops8_runs3"] = [(S, 2), (M, 5), (I, 1), (M, 5), (DEL, 1), (M, 5), (P, 1), (M, 5)]
    c["ops9_runs3"] = list(COMPLEX_OPS)
    c["ops9_runs2"] = [(S, 1), (M, 4), (P, 1), (M, 4), (H, 1), (M, 4), (DEL, 2), (M, 4), (S, 1)]
    c["ops7_runs4"] = [(M, 4), (DEL, 1), (M, 4), (I, 1), (M, 4), (SKIP, 2), (M, 4)]
    # (five runs need four breaking ops between them, so at least nine ops: with eight ops the
    # most is four runs, here followed by an X that extends the last one)
    c["ops8_runs4"] = [(M, 3), (DEL, 1), (M, 3), (DEL, 1), (M, 3), (I, 1), (M, 3), (X, 3)]
    c["ops9_runs5"] = [(M, 3), (DEL, 1), (M, 3), (DEL, 1), (M, 3), (DEL, 1), (M, 3), (DEL, 1), (M, 3)]
    # zero-length ops: no run, no break (decode_runs' len == 0)
    c["zero_len"] = [(M, 4), (DEL, 0), (M, 4), (I, 0), (M, 0), (M, 4)]
    c["lead_del"] = [(DEL, 3), (M, 9)]
    c["trail_skip"] = [(M, 9), (SKIP, 5)]
    # reads that count no base
    c["del_only"] = [(DEL, 5)]
    c["ins_only"] = [(I, 10)]
    c["clip_only"] = [(S, 10)]
    c["no_cigar"] = []
    # no-op ops between two M, and a mid-read S (the reference does not advance the query)
    c["mid_H"] = [(M, 5), (H, 2), (M, 5)]
    c["mid_P"] = [(M, 5), (P, 2), (M, 5)]
    c["mid_B"] = [(M, 5), (B, 2), (M, 5)]
    c["mid_S"] = [(M, 3), (S, 2), (M, 3)]
    # query delta around int16 in a read of span 8 (stays on the tiled kernels)
    for n in (32767, 32768, 32772):
        c[f"ins{n}"] = [(M, 4), (I, n), (M, 4)]
    # query length around 0xFFFF with every run's delta inside int16 (pack_runs)
    c["qlen65535"] = [(M, 4), (I, 32760), (M, 4), (I, 32767)]
    c["qlen65536"] = [(M, 4), (I, 32760), (M, 4), (I, 32768)]
    # span exactly kTileMaxSpan: the largest the tiled kernel accepts
    c["span4096"] = [(M, 4), (DEL, 4088), (M, 4)]
    # span around 0x1FFF / op lengths around 2^13 (decode_fast2)
    for sp in (8190, 8191, 8192):
        c[f"span{sp}@long"] = [(M, 4), (SKIP, sp - 8), (M, 4)]
    c["op8191@long"] = [(M, 8191)]
    c["op8192@long"] = [(M, 8192)]
    c["m65535@long"] = [(M, 65535)]
    c["m65536@long"] = [(M, 65536)]
    return c


# two-run reads whose run boundaries fall on / next to an 8-position row edge; each is placed at
# every start mod 8
EDGE_TWO_RUN = [[(M, a), (op, ln), (M, 8)] for a in (7, 8, 9) for op, ln in ((DEL, 1), (DEL, 8), (I, 2), (SKIP, 7))]


def host_runs(ops):
    """(cig_n, runs, query deltas of the runs, span, query length, longest op): decode_runs'
    quantities, computed plainly (consecutive M/=/X with one delta merge; zero lengths vanish)."""
    rc = qc = 0
    runs = []
    for op, ln in ops:
        if ln == 0:
            continue
        if op in (M, EQOP, X):
            if runs and runs[-1][1] == rc and runs[-1][2] == qc - rc:
                runs[-1][1] = rc + ln
            else:
                runs.append([rc, rc + ln, qc - rc])
            rc, qc = rc + ln, qc + ln
        elif op == I:
            qc += ln
        elif op in (DEL, SKIP):
            rc += ln
    return dict(cig_n=len(ops), nrun=len(runs), qd=[r[2] for r in runs], span=rc, qlen=qc,
                maxlen=max([ln for _, ln in ops], default=0))


def is_complex(ops):
    """The host statement of bc_runs.h's switch to the complex path."""
    h = host_runs(ops)
    return (h["cig_n"] > 8 or h["nrun"] > 4 or any(q < -32768 or q > 32767 for q in h["qd"])
            or h["span"] >= 0x1FFF or h["qlen"] > 0xFFFF)


def random_read(rng, pos, ops):
    """The read `ops` at `pos` with random letters (A C G T N M =) and random quality bytes."""
    q = stored_len(ops)
    return (pos, list(ops), LETTERS[rng.integers(0, LETTERS.size, q)], rng.integers(0, 256, q).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def catalogue_batch(which, variant, L):
    """The catalogue as a sorted batch on a reference of L positions.
    which: "tiled" (spans <= kTileMaxSpan) or "long" (the @long reads too);
    variant: "embedded" (once, among 300 random reads) or "deep" (8 or 12 copies, more than 300
    reads, and one plain read at the end: every k_rc chunk holds catalogue reads only)."""
    rng = np.random.default_rng(700 + len(which) + len(variant))
    cat = catalogue_ops()
    names = [k for k in cat if which == "long" or not k.endswith("@long")]
    reads = []
    for rep in range(1 if variant == "embedded" else (8 if which == "tiled" else 12)):
        for i, name in enumerate(names):
            span = ref_span(cat[name])
            at = (977 * i + 11 * rep + 5) % (L - span - 64)
            if name == "span4096":
                at = 8192 - 2048 + rep  # over the 8192-position summary buffer edge when L allows
                at = min(at, L - span - 1)
            reads.append(random_read(rng, at, cat[name]))
        if which == "tiled":
            for s in range(8):
                for j, ops in enumerate(EDGE_TWO_RUN):
                    reads.append(random_read(rng, 1024 + 32 * j + s + 256 * (rep % 2), ops))
    # the read without a CIGAR must not be the last (its cig_beg then stays inside the buffer)
    reads.append(random_read(rng, L - 40, [(M, 8)]))
    if variant == "embedded":
        reads += random_reads(rng, 300, 0, L)
    return pack_batch(reads)


# ------------------------------------------------------------------------------ quality range
QUAL_THRESHOLDS = (1, 2, 127, 128, 129, 200, 254, 255, 256, 1000)


@functools.lru_cache(maxsize=None)
def quality_batch(L=3000, n=3000, tight=False, seed=11):
    """A few thousand reads with quality bytes uniform over 0..255, about one read in ten entirely
    0xFF, 0x80 or 0x7F; ``tight``: the qual array ends with the last read's (padded) bases."""
    rng = np.random.default_rng(seed)
    reads = random_reads(rng, n, 0, L, letters=LETTERS[:6])
    for i in range(0, len(reads), 10):
        p, ops, s, q = reads[i]
        reads[i] = (p, ops, s, np.full(q.size, (0xFF, 0x80, 0x7F)[(i // 10) % 3], np.uint8))
    return pack_batch(reads, tight=tight)


# --------------------------------------------------------------------------- expected results
_EXPECTED = {}  # (id(batch), L, mbq) -> (batch, counts, first bad read): computed once, left unchanged


def expect(b, L, mbq):
    """(counts [L][6] of every in-range event, the oracle's first out-of-range read at ref_len L).
    The oracle stops at the first read past the end (count.cpp's .at() throws); the device counts
    every in-range event of every read, so the counts come from a reference long enough for the
    whole batch, cut at L."""
    key = (id(b), L, mbq)
    if key not in _EXPECTED or _EXPECTED[key][0] is not b:  # (the batch kept: its id stays its own)
        end = max(max_end(b), L)
        cnt, (br, _) = O.bcount(end, mbq, b)
        assert br == -1
        if end > L:
            _, (br, _) = O.bcount(L, mbq, b)
        if len(_EXPECTED) >= 12:
            _EXPECTED.clear()
        _EXPECTED[key] = (b, cnt[:L], br)
    return _EXPECTED[key][1:]


def expect_stats(cnt6, k):
    return (cnt6[:, :k].T.astype(np.int32),) + tuple(O.stats(cnt6, k == 6))


# ------------------------------------------------------------------------------ GPU launches
def kernel_for(shape, waves, b):
    """The BC_K_* name bc_count / bc_pileup must pick for a sorted uploaded batch."""
    if shape == "rc" or int(spans(b).max()) > K_TILE_MAX_SPAN:
        return "rc"
    return "solo" if (shape, waves) == ("tile", 1) else "pileup"


def upload(ctx, b, shape="auto", waves=0, mode=None, max_end=None):
    """Set the kernel shape, then upload (the upload builds the index of the shape in force);
    mode: k_rc's inputs -- the upload's run records and chunk summaries, the records only, or its
    own CIGAR decode.
    max_end: the launches are to run on ``r.launch``, the batch with max_end raised to it
    (wide_index.widen: the 64-bit-index instances); without it ``r.launch`` is the batch itself.
    The device batch is freed through the returned object either way."""
    ctx.set_shape(shape, waves)
    r = D.DeviceReads(ctx, b)
    if mode is not None:
        assert r.r.read_runs and r.r.run_chunks > 0
        if mode == "records":
            r.r.run_chunks = 0
        elif mode == "cigars":
            r.r.read_runs = None
    r.launch = r.r if max_end is None else WI.widen(r, max_end)
    return r


def launched(ctx):
    """Names of the kernels timed since the last call (bc_timing_report; index builds left out)."""
    return set(ctx.timing_report()) - {"index"}


def count_on(ctx, r, L, mbq, ncols):
    hist = ctx.alloc(max(16, 4 * ncols * L))
    hist.zero()
    ctx.count(r, L, mbq, ncols, hist.ptr)
    bad = ctx.range_error()
    got = hist.download(np.int32, ncols * L).reshape(ncols, L)
    hist.free()
    return got, bad


def pileup_on(ctx, r, L, mbq, k, fill=None):
    """bc_pileup's five outputs and range error; ``fill``: the byte the outputs hold before the call."""
    bufs = [ctx.alloc(max(16, n)) for n in (4 * k * L, 4 * L, 8 * k * L, 8 * L, 8 * L)]
    if fill is not None:
        for x in bufs:
            D.check(D.lib().bc_memset(ctx.h, x.ptr, fill, x.nbytes))
    nf, nf2 = norm_factors(k)
    ctx.pileup(r, L, mbq, k, nf, nf2, *[x.ptr for x in bufs])
    bad = ctx.range_error()
    out = (bufs[0].download(np.int32, k * L).reshape(k, L), bufs[1].download(np.int32, L),
           bufs[2].download(np.float64, k * L).reshape(k, L), bufs[3].download(np.float64, L),
           bufs[4].download(np.float64, L))
    for x in bufs:
        x.free()
    return out, bad


def same(got, exp, what):
    for name, g, e in zip(("counts", "cov", "pc", "ent", "sec"), got, exp):
        assert np.array_equal(g, e), (what, name)


def check_sorted(ctx, b, L, mbqs, shapes, ks=(5, 6), repeat_last=False, max_end=None):
    """bc_count (accumulate mode) and bc_pileup of the sorted batch b through every given launch
    shape: the kernel the shape names really ran, the oracle's first out-of-range read, counts /
    coverage exact and percentages / entropies bit-identical below L.
    max_end: the launches run on the batch with max_end raised to it, and every tiled launch must
    then be a 64-bit-index instance (wide_index.is_wide)."""
    exp = {mbq: expect(b, L, mbq) for mbq in mbqs}
    for shape, waves, mode in shapes:
        kern = kernel_for(shape, waves, b)
        assert mode is None or kern == "rc"
        r = upload(ctx, b, shape, waves, mode, max_end)
        try:
            assert r.r.sorted == 1
            for mbq in mbqs:
                cnt6, br = exp[mbq]
                for k in ks:
                    what = (shape, waves, mode, mbq, k)
                    if max_end is not None and kern != "rc":
                        assert WI.is_wide(r.launch, L, shape, waves, "auto", mbq, k), what
                    launched(ctx)
                    got, bad = count_on(ctx, r.launch, L, mbq, k)
                    assert launched(ctx) == {kern}, what
                    assert bad == br, what
                    assert np.array_equal(got, cnt6[:, :k].T.astype(np.int32)), what
                    for _ in range(2 if repeat_last and (mbq, k) == (mbqs[-1], ks[-1]) else 1):
                        got, bad = pileup_on(ctx, r.launch, L, mbq, k, fill=None if max_end is None else 0xFF)
                        assert launched(ctx) == ({"rc", "stats"} if kern == "rc" else {kern}), what
                        assert bad == br, what
                        same(got, expect_stats(cnt6, k), what)
        finally:
            r.free()
            ctx.set_shape("auto")


def check_unsorted(ctx, b, L, mbqs, rpbs=(0, 1, 32768), ks=(5, 6)):
    """The batch with its reads permuted: k_count on global atomics at each reads_per_block, then
    bc_reads_sort of the permuted batch and a count of the sorted copy."""
    exp = {mbq: expect(b, L, mbq) for mbq in mbqs}
    bu = permuted(b)
    r = D.DeviceReads(ctx, bu)
    try:
        assert r.r.sorted == 0
        for rpb in rpbs:
            ctx.set_shape("auto", 0, rpb)
            for mbq in mbqs:
                cnt6, br = exp[mbq]
                want_bad = -1 if br == -1 else expect(bu, L, mbq)[1]
                for k in ks:
                    launched(ctx)
                    got, bad = count_on(ctx, r, L, mbq, k)
                    assert launched(ctx) == {"count"}, (rpb, mbq, k)
                    assert bad == want_bad
                    assert np.array_equal(got, cnt6[:, :k].T.astype(np.int32)), (rpb, mbq, k)
        ctx.set_shape("auto")
        nb = ctx.sort_bytes(r)
        mem = ctx.alloc(nb)
        launched(ctx)
        s = ctx.sort(r, mem.ptr, nb)
        assert launched(ctx) == {"sort"}
        assert s.sorted == 1 and s.n_reads == r.r.n_reads
        pos = np.zeros(s.n_reads, np.int32)
        D.check(D.lib().bc_memcpy_d2h(ctx.h, pos.ctypes.data, s.pos, pos.nbytes))
        ctx.sync()
        assert np.array_equal(pos, np.sort(bu["pos"]))
        for mbq in mbqs:
            cnt6, br = exp[mbq]
            hist = ctx.alloc(4 * 6 * L)
            hist.zero()
            ctx.count(s, L, mbq, 6, hist.ptr)
            bad = ctx.range_error()
            assert launched(ctx) & {"rc", "pileup", "solo"}
            assert (bad == -1) == (br == -1)
            assert np.array_equal(hist.download(np.int32, 6 * L).reshape(6, L), cnt6.T.astype(np.int32)), mbq
            hist.free()
        mem.free()
    finally:
        r.free()
        ctx.set_shape("auto")


def check_summaries(ctx, b, L, mbq, k, shapes=(("tile", 1), ("tile_no_solo", 1), ("rc", 0)), max_end=None):
    """bc_pileup_summary, and the summary-only forms (bc_pileup_partials with every output NULL +
    bc_summary_fold; bc_pileup_summary with every output NULL), against bc_pileup followed by
    bc_summary and against numpy over the oracle's coverage and entropy.
    max_end: as for check_sorted (the tiled launches are 64-bit-index instances)."""
    assert L >= 8192  # the sparse summary-only path (bc_sum.hip's own read walk) needs a whole buffer
    cnt6, br = expect(b, L, mbq)
    assert br == -1
    cov, _, ent, _ = O.stats(cnt6, k == 6)
    c64 = cov.astype(np.int64)
    want = [float(np.mean(c64)), float(np.mean(ent)), float(np.count_nonzero(cov)), float(c64.sum())]
    nf, nf2 = norm_factors(k)
    for shape, waves in shapes:
        kern = kernel_for(shape, waves, b)
        r = upload(ctx, b, shape, waves, max_end=max_end)
        assert max_end is None or kern == "rc" or WI.is_wide(r.launch, L, shape, waves, "auto", mbq, k), shape
        bufs =[ctx.alloc(n) for n in (4 * k * L, 4 * L, 8 * L, 8 * L)]
        counts, dcov, dent, dsec = [x.ptr for x in bufs]
        work, out = ctx.alloc(D.summary_work_bytes(L)), ctx.alloc(32)
        if max_end is not None:  # (the wide runs: no output may rely on what the buffer held)
            for x in bufs:
                D.check(D.lib().bc_memset(ctx.h, x.ptr, 0xFF, x.nbytes))
        try:
            ctx.pileup(r.launch, L, mbq, k, nf, nf2, counts, dcov, None, dent, dsec)
            ctx.summary(dcov, dent, L, work.ptr, out.ptr)
            base = out.download(np.float64, 4).tolist()
            assert ctx.range_error() == -1
            assert base == want, (shape, "bc_pileup + bc_summary")
            out.zero()
            launched(ctx)
            ctx.pileup_summary(r.launch, L, mbq, k, nf, nf2, counts, dcov, None, dent, dsec, work.ptr, out.ptr)
            assert out.download(np.float64, 4).tolist() == base, (shape, "bc_pileup_summary")
            assert {kern, "summary"} <= launched(ctx) | ({"summary"} if kern == "rc" else set()), shape
            assert np.array_equal(bufs[0].download(np.int32, k * L).reshape(k, L), cnt6[:, :k].T.astype(np.int32))
            out.zero()
            ctx.pileup_partials(r.launch, L, mbq, k, nf, nf2, None, None, None, None, None, work.ptr)
            ctx.summary_fold([L], [work.ptr], [out.ptr])
            assert out.download(np.float64, 4).tolist() == base, (shape, "summary only: partials + fold")
            assert {kern, "summary"} <= launched(ctx), shape
            out.zero()
            ctx.pileup_summary(r.launch, L, mbq, k, nf, nf2, None, None, None, None, None, work.ptr, out.ptr)
            assert out.download(np.float64, 4).tolist() == base, (shape, "summary only: bc_pileup_summary")
            assert ctx.range_error() == -1
        finally:
            for x in bufs + [work, out]:
                x.free()
            r.free()
            ctx.set_shape("auto")
