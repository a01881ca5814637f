"""Inputs and the yardstick of the device row formatter (basecount_amd/csrc/bc_fmt.h).

``rows_ref`` is the text the host formatter writes: fmt.rows_text (bcio_fmt_rows) per segment,
concatenated, with the position column shifted by the segment's pos0.  ``cases()`` generates output
arrays and segment tables, each the smallest input that can break one mechanism of the kernels (tile
and wave boundaries, every row-start alignment, digit-length changes, windows of the staging area,
the unprinted slots, pads and empty segments, the scan's runs, the declines).  ``pack_input`` /
``unpack_results`` are the file format of tests/native/fmt_check.cpp."""
import struct

import numpy as np

from basecount_amd import fmt

ST_OK, ST_TOO_SMALL, ST_VALUE = 0, 1, 2
SENTINEL = 0xEE
TILE, WIN, SCAN_THREADS = 64, 8192 - 16, 256
SEG_DTYPE = np.dtype([("beg", "<i8"), ("len", "<i8"), ("pos0", "<i8"), ("name_off", "<i4"), ("name_len", "<i4")])
HEADER_DTYPE = np.dtype([("status", "<i4"), ("reserved0", "<i4"), ("total_bytes", "<i8"), ("declined_pos", "<i8"),
                         ("reserved", "<i8", (5,))])


def _shift_positions(text: bytes, pos0: int, rows_per_pos: int) -> bytes:
    """rows_text's body with position p printed as pos0 + p."""
    if pos0 == 0 or not text:
        return text
    out = []
    for i, line in enumerate(text.split(b"\n")[:-1]):
        ref, _, rest = line.split(b"\t", 2)
        out.append(b"%s\t%d\t%s\n" % (ref, pos0 + i // rows_per_pos + 1, rest))
    return b"".join(out)


def rows_ref(c) -> tuple:
    """(text, seg_off) of a case as the host formatter writes it."""
    k, parts = c["k"], []
    for beg, ln, pos0, name in c["segs"]:
        sl = slice(beg, beg + ln)
        t = fmt.rows_text(name, np.ascontiguousarray(c["counts"][:k, sl]), np.ascontiguousarray(c["pc"][:, sl]),
                          np.ascontiguousarray(c["ent"][sl]), np.ascontiguousarray(c["sec"][sl]), c["dp"], bool(c["long"]))
        parts.append(_shift_positions(t, pos0, k if c["long"] else 1))
    off = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    return b"".join(parts), off


def layout(lens) -> list:
    """Segment starts as bc_segments_layout places them: each at the next multiple of 64."""
    beg, at = [], 0
    for ln in lens:
        beg.append(at)
        at += (ln + TILE - 1) // TILE * TILE
    return beg


_TIES = np.array([0.5, 1.5, 2.5, 0.125, 0.375, 0.0625, 0.03125, 2.675, 1.005, 0.045, 33.335, 12.5, 99.995, 0.00005,
                  0.00015, 1.00005, 50.0, 100.0, 0.0, 1e-300, 66.66666666666667, 4.35, 0.285, 1.0000000000000002])


def arrays(rng, n, k, ncols=None, stride=None, hi=60):
    """Outputs as the kernels leave them for ``n`` positions: random counts with all-zero positions
    and positions with one non-zero count, the percentages c / cov * 100, entropies in their ranges
    with decimal and binary ties mixed in, and NaN in every slot that is not printed."""
    ncols = ncols or k
    stride = stride or n
    counts = rng.integers(0, hi, (ncols, stride)).astype(np.int32)
    kind = rng.random(stride)
    counts[:, kind < 0.15] = 0
    one = np.flatnonzero((kind >= 0.15) & (kind < 0.3))
    keep = rng.integers(0, k, one.size)
    v = counts[keep, one] + 1
    counts[:, one] = 0
    counts[keep, one] = v
    if n:
        counts[:, 0] = 0  # the first position always without coverage
    cov = counts[:k].astype(np.int64).sum(0)
    nz = (counts[:k] != 0).sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        pc = counts[:k] / cov * 100
    ent = rng.random(stride) * 2.33
    sec = rng.random(stride) * 3.0
    t = rng.random(stride) < 0.3
    ent[t] = rng.choice(_TIES, int(t.sum()))
    t = rng.random(stride) < 0.3
    sec[t] = rng.choice(_TIES, int(t.sum()))
    pc[:, cov == 0] = np.nan  # never inspected
    ent[cov == 0] = np.nan
    sec[(cov == 0) | (nz <= 1)] = np.nan
    return counts, np.ascontiguousarray(pc), ent, sec


def _case(name, rng, n, k, dp, long, segs, status=ST_OK, declined=-1, **kw):
    counts, pc, ent, sec = arrays(rng, n, k, **kw)
    return {"name": name, "n": n, "k": k, "dp": dp, "long": int(long), "segs": segs, "counts": counts, "pc": pc,
            "ent": ent, "sec": sec, "stride": counts.shape[1], "status": status, "declined": declined}


def _blank_pads(c):
    """NaN and garbage counts at every array position outside the segments: they print nothing."""
    used = np.zeros(c["stride"], bool)
    for beg, ln, _, _ in c["segs"]:
        used[beg:beg + ln] = True
    c["counts"][:, ~used] = -7
    c["pc"][:, ~used] = np.nan
    c["ent"][~used] = np.nan
    c["sec"][~used] = np.nan
    return c


def cases() -> list:
    rng = np.random.default_rng(20260)
    out = []
    shapes = [(5, 0), (6, 0), (5, 1), (6, 1)]
    # the sizes around tile boundaries, every shape, decimal places rotating
    for i, n in enumerate((0, 1, 63, 64, 65, 127, 128, 129, 257, 1025)):
        for j, (k, lg) in enumerate(shapes):
            dp = (i + j) % 5
            out.append(_case("n%d_k%d_%s_dp%d" % (n, k, "long" if lg else "wide", dp), rng, n, k, dp, lg,
                             [(0, n, 0, "chr%d" % j)]))
    # every shape at every dp
    for k, lg in shapes:
        for dp in range(5):
            out.append(_case("full_k%d_%s_dp%d" % (k, "long" if lg else "wide", dp), rng, 129, k, dp, lg,
                             [(0, 129, 0, "MN908947.3")]))
    # names of 1 .. 9 bytes: the row starts take every alignment mod 16; long names: several windows
    for ln in range(1, 10):
        out.append(_case("name%d" % ln, rng, 70, 5 + ln % 2, 3, ln % 3 == 0, [(0, 70, 0, "abcdefghi"[:ln])]))
    for ln in (200, 255):
        for k, lg in ((5, 0), (6, 1)):
            out.append(_case("name%d_%s" % (ln, "long" if lg else "wide"), rng, 130, k, 2, lg,
                             [(0, 130, 0, ("N" * ln))]))
    # a slice of a large reference: the digit-length changes of the position
    for pos0 in (0, 8, 98, 998, 999999990, 2**31 - 70):
        out.append(_case("pos0_%d" % pos0, rng, 130, 5, 3, pos0 % 3 == 0, [(0, 130, pos0, "ref")]))
    # a plane count above the printed columns (the histogram of a run without N has k planes; one with 6)
    out.append(_case("ncols6_k5", rng, 100, 5, 3, 0, [(0, 100, 0, "r")], ncols=6, stride=131))
    # counts at the top of int32: cov has 11 digits; negative counts print signed
    for lg in (0, 1):
        c = _case("int32_max_%s" % ("long" if lg else "wide"), rng, 66, 5, 4, lg, [(0, 66, 0, "big")])
        c["counts"][:, 1:] = 2**31 - 1
        c["pc"][:, 1:] = 20.0
        c["ent"][1:], c["sec"][1:] = 2.321928094887362, 2.0
        out.append(c)
    c = _case("negative_counts", rng, 65, 5, 1, 0, [(0, 65, 0, "neg")])
    c["counts"][:, 1:] = -3
    c["pc"][:, 1:], c["ent"][1:], c["sec"][1:] = -20.0, -0.0, -1e-4
    out.append(c)
    # every position without coverage; every position with one non-zero count
    c = _case("all_zero", rng, 200, 6, 3, 1, [(0, 200, 0, "zero")])
    c["counts"][:] = 0
    c["pc"][:], c["ent"][:], c["sec"][:] = np.nan, np.nan, np.nan
    out.append(c)
    c = _case("all_nz1", rng, 200, 5, 3, 0, [(0, 200, 0, "one")])
    c["counts"][:] = 0
    c["counts"][2] = 9
    c["pc"][:], c["pc"][2], c["ent"][:], c["sec"][:] = 0.0, 100.0, 0.0, np.nan
    out.append(c)
    # segment tables: pads between segments, empty segments, a one-position segment
    for lg in (0, 1):
        lens = [5, 64, 0, 1, 130, 0, 0, 63, 65, 0]
        beg = layout(lens)
        n = beg[-1] + lens[-1]
        segs = [(b, ln, 0, "s%d" % i) for i, (b, ln) in enumerate(zip(beg, lens))]
        out.append(_blank_pads(_case("segments_pads_%s" % ("long" if lg else "wide"), rng, n, 5 + lg, 3, lg, segs)))
    lens = [int(x) for x in rng.integers(1, 301, 40)]
    beg = layout(lens)
    n = beg[-1] + lens[-1]
    segs = [(b, ln, 0, "contig_%d" % (i * 37)) for i, (b, ln) in enumerate(zip(beg, lens))]
    out.append(_blank_pads(_case("segments_40", rng, n, 5, 3, 0, segs)))
    out.append(_blank_pads(_case("segments_40_long", rng, n, 6, 2, 1, segs)))
    out.append(_blank_pads(_case("segment_starts_late", rng, 192, 5, 3, 0, [(0, 0, 0, "e"), (128, 40, 0, "late")])))
    # more tiles than the scan has threads: every thread a run of two tiles
    n = TILE * (SCAN_THREADS + 44) + 5
    out.append(_case("scan_runs", rng, n, 5, 0, 0, [(0, n, 0, "s")]))
    # the declines: a printed value outside the cover, at a known position
    for tag, val, dp in (("nan", np.nan, 3), ("inf", np.inf, 0), ("ninf", -np.inf, 4), ("1e300", 1e300, 2),
                         ("1e15_scaled", 1e11, 4)):
        c = _case("decline_" + tag, rng, 300, 5, dp, 0, [(0, 300, 0, "d")], status=ST_VALUE)
        p = int(np.flatnonzero(~np.isnan(c["sec"]))[70])  # a position whose secondary entropy prints
        c["sec"][p] = val
        c["declined"] = p
        out.append(c)
    c = _case("decline_pc_first_of_two", rng, 300, 6, 3, 1, [(0, 300, 0, "d")], status=ST_VALUE)
    ps = np.flatnonzero(~np.isnan(c["pc"][0]))
    c["pc"][3, ps[40]] = np.nan
    c["ent"][ps[200]] = np.inf
    c["declined"] = int(ps[40])
    out.append(c)
    # just inside the cover: 1e15 is not reached
    c = _case("large_values_inside", rng, 65, 5, 4, 0, [(0, 65, 0, "L")])
    ps = np.flatnonzero(~np.isnan(c["sec"]))
    c["sec"][ps] = 99999999999.99985
    c["ent"][ps] = 123456789.12345
    out.append(c)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def table(c) -> tuple:
    """(segment table, names bytes) of a case."""
    tab = np.zeros(len(c["segs"]), SEG_DTYPE)
    blob = b""
    for i, (beg, ln, pos0, name) in enumerate(c["segs"]):
        b = name.encode()
        tab[i] = (beg, ln, pos0, len(blob), len(b))
        blob += b
    return tab, np.frombuffer(blob, np.uint8)


def pack_input(cs, caps) -> bytes:
    """fmt_check's input: u32 ncases, then per case { i32 k dp long ncols, i64 n stride n_seg names_bytes
    text_cap, counts i32[ncols * stride], pc f64[k * stride], ent f64[stride], sec f64[stride], the
    segment table, the names }."""
    out = [struct.pack("<I", len(cs))]
    for c, cap in zip(cs, caps):
        tab, names = table(c)
        out.append(struct.pack("<4i5q", c["k"], c["dp"], c["long"], c["counts"].shape[0], c["n"], c["stride"], len(tab),
                               names.size, cap))
        out += [np.ascontiguousarray(c["counts"], np.int32).tobytes(), np.ascontiguousarray(c["pc"], np.float64).tobytes(),
                np.ascontiguousarray(c["ent"], np.float64).tobytes(), np.ascontiguousarray(c["sec"], np.float64).tobytes(),
                tab.tobytes(), names.tobytes()]
    return b"".join(out)


def unpack_results(raw: bytes, cs, caps) -> list:
    """Per case { u32 guards_ok, the 64-byte header, seg_off i64[n_seg + 1], text u8[text_cap] }."""
    out, at = [], 0
    for c, cap in zip(cs, caps):
        ns = len(c["segs"])
        g = struct.unpack_from("<I", raw, at)[0]
        h = np.frombuffer(raw, HEADER_DTYPE, 1, at + 4)[0]
        off = np.frombuffer(raw, np.int64, ns + 1, at + 68)
        text = raw[at + 68 + 8 * (ns + 1):at + 68 + 8 * (ns + 1) + cap]
        at += 68 + 8 * (ns + 1) + cap
        out.append({"guards": g, "status": int(h["status"]), "total": int(h["total_bytes"]),
                    "declined": int(h["declined_pos"]), "seg_off": off, "text": text})
    assert at == len(raw)
    return out
