"""Inputs and the yardstick of the device read selection (basecount_amd/csrc/bc_select.h).

``select_ref`` restates the selection (bcio_select) and the per-reference facts in numpy;
tests/test_select_ref.py pins it against BamFile.select and main._reads_inside.  ``cases()`` generates
record arrays, each the smallest input that can break one mechanism of the kernels (ballot ranks,
wave and workgroup boundaries, the order tests, the 64-bit sums, the declines).  ``pack_input`` /
``unpack_results`` are the file format of tests/native/select_check.cpp."""
import struct

import numpy as np

RUN = 1024  # records of one workgroup (BCS_RUN); a wave takes 256 of them, 64 a step
ST_OK, ST_UNGROUPED, ST_TOO_LARGE = 0, 1, 2
F_SORTED, F_INSIDE = 1, 2
POISON = 0xEE

REC_FIELDS = (("tid", np.int32, 0), ("pos", np.int32, 0), ("flag", np.uint16, 0), ("mapq", np.uint8, 0),
              ("qstart", np.int32, 0), ("qend", np.int32, 0), ("rec_err", np.uint32, 0), ("ref_span", np.int64, 0),
              ("cig_off", np.uint64, 1), ("seq_off", np.uint64, 1))
READ_ARRAYS = (("pos", np.int32), ("cig_beg", np.uint32), ("cig_n", np.uint32), ("seq_nib", np.uint32),
               ("qlen", np.uint32), ("span", np.int64), ("rec", np.int64), ("ordinal", np.int64))
REF_ARRAYS = (("max_span", np.int64), ("max_end", np.int64), ("n_reads", np.int64), ("n_complex", np.int64),
              ("sum_ops", np.uint64), ("err_or", np.uint32), ("flags", np.uint32))
HEADER = ("status", "batch_err_or", "n_accepted", "n_selected", "keyerror_rec", "keyerror_ordinal")


def select_ref(a, min_mapq, ref_sel, ref_len):
    """bcio_select and the per-reference facts of the records ``a`` (a mapping with REC_FIELDS'
    arrays), in numpy.  The per-read arrays are bcio_select's whatever the status says."""
    tid = np.asarray(a["tid"], np.int32)
    n, nr = tid.size, len(ref_sel)
    sel_t = np.asarray(ref_sel, np.uint8) != 0
    L = np.asarray(ref_len, np.int64)
    acc = ((np.asarray(a["flag"]) & 4) == 0) & (np.asarray(a["mapq"]).astype(np.int64) >= int(min_mapq))
    inr = (tid >= 0) & (tid < nr)
    want = np.zeros(n, bool)
    want[inr] = sel_t[tid[inr]]
    sel = acc & want
    ordinal_all = np.cumsum(acc) - acc  # accepted records before i
    idx = np.flatnonzero(sel)
    ctid_file = tid[idx]
    order = np.argsort(ctid_file, kind="stable")
    rec = idx[order].astype(np.int64)
    ctid = ctid_file[order]
    cig_off, seq_off = np.asarray(a["cig_off"], np.uint64), np.asarray(a["seq_off"], np.uint64)
    qs, qe = np.asarray(a["qstart"], np.int32)[rec], np.asarray(a["qend"], np.int32)[rec]
    out = {
        "pos": np.asarray(a["pos"], np.int32)[rec],
        "cig_beg": cig_off[rec].astype(np.uint32),
        "cig_n": (cig_off[rec + 1] - cig_off[rec]).astype(np.uint32),
        "seq_nib": (2 * seq_off[rec] + np.maximum(qs, 0).astype(np.uint64)).astype(np.uint32),
        "qlen": np.maximum(qe.astype(np.int64) - qs, 0).astype(np.uint32),
        "span": np.asarray(a["ref_span"], np.int64)[rec],
        "rec": rec,
        "ordinal": ordinal_all[rec].astype(np.int64),
    }
    ref_beg = np.zeros(nr + 1, np.int64)
    np.cumsum(np.bincount(ctid, minlength=nr)[:nr], out=ref_beg[1:])
    out["ref_beg"] = ref_beg
    out["n_accepted"], out["n_selected"] = int(acc.sum()), int(idx.size)
    ke = np.flatnonzero(acc & ~want)
    out["keyerror_rec"] = int(ke[0]) if ke.size else -1
    out["keyerror_ordinal"] = int(ordinal_all[ke[0]]) if ke.size else -1
    err = np.asarray(a["rec_err"], np.uint32)[rec]
    out["batch_err_or"] = int(np.bitwise_or.reduce(err)) if err.size else 0
    status = ST_OK
    if bool(np.any(ctid_file[1:] < ctid_file[:-1])):
        status = ST_UNGROUPED
    if int(cig_off[n]) > 2**32 - 1 or 2 * int(seq_off[n]) > 2**32 - 1:
        status = ST_TOO_LARGE
    out["status"] = status
    # per reference
    p64, span = out["pos"].astype(np.int64), out["span"]
    facts = {k: np.zeros(nr, dt) for k, dt in REF_ARRAYS}
    facts["n_reads"][:] = np.diff(ref_beg)
    facts["flags"][:] = F_SORTED | F_INSIDE
    facts["max_end"][facts["n_reads"] > 0] = np.iinfo(np.int64).min
    np.maximum.at(facts["max_span"], ctid, span)
    np.maximum.at(facts["max_end"], ctid, p64 + span)
    np.add.at(facts["n_complex"], ctid, (out["cig_n"] > 8).astype(np.int64))
    np.add.at(facts["sum_ops"], ctid, out["cig_n"].astype(np.uint64))
    np.bitwise_or.at(facts["err_or"], ctid, err)
    outside = (p64 < 0) | (p64 + span > L[ctid])
    facts["flags"][ctid[outside]] &= ~np.uint32(F_INSIDE)
    if p64.size > 1:
        dec = np.zeros(p64.size, bool)
        dec[1:] = (p64[1:] < p64[:-1]) & (ctid[1:] == ctid[:-1])
        facts["flags"][ctid[dec]] &= ~np.uint32(F_SORTED)
    out.update(facts)
    return out


# ---- generated inputs ----
def records(n, n_refs, seed, tid=None):
    """n records grouped by reference with non-decreasing starts within one, about a third
    unmapped (flag bit 4), mapq over 0..255, 1..12 CIGAR ops, negative qstart and qend < qstart
    here and there, no rec_err."""
    rng = np.random.default_rng(seed)
    if tid is None:
        tid = np.sort(rng.integers(0, max(1, n_refs), n)).astype(np.int32)
    tid = np.asarray(tid, np.int32)
    pos = np.zeros(n, np.int32)
    for t in np.unique(tid):
        m = tid == t
        pos[m] = np.sort(rng.integers(0, 5000, int(m.sum())))
    flag = np.where(rng.random(n) < 1 / 3, 4, 0).astype(np.uint16) | (rng.integers(0, 2, n) * 16).astype(np.uint16)
    mapq = rng.integers(0, 256, n).astype(np.uint8)
    cig_n = rng.integers(1, 13, n)
    cig_n[::7] = 8
    cig_n[3::7] = 9
    l_seq = rng.integers(1, 200, n)
    qstart = rng.integers(0, 20, n).astype(np.int32)
    qstart[5::11] = -3
    qend = (qstart + rng.integers(0, 150, n)).astype(np.int32)
    qend[2::13] = qstart[2::13] - 4
    return {
        "tid": tid, "pos": pos, "flag": flag, "mapq": mapq, "qstart": qstart, "qend": qend,
        "rec_err": np.zeros(n, np.uint32), "ref_span": rng.integers(0, 300, n).astype(np.int64),
        "cig_off": np.concatenate([[0], np.cumsum(cig_n)]).astype(np.uint64),
        "seq_off": np.concatenate([[0], np.cumsum((l_seq + 1) // 2)]).astype(np.uint64),
    }


def _all_accepted(a):
    a["flag"][:] = 0
    a["mapq"][:] = 60
    return a


def cases():
    """[(name, records, min_mapq, ref_sel, ref_len, expected status)]."""
    out = []
    big = np.int64(1) << 40

    def add(name, a, mmq, ref_sel, ref_len, status=ST_OK):
        out.append((name, a, mmq, np.asarray(ref_sel, np.uint8), np.asarray(ref_len, np.int64), status))

    # n: the ballot ranks at every boundary of the schedule
    for n in (0, 1, 63, 64, 65, RUN - 1, RUN, RUN + 1, 3 * RUN + 17):
        add("n%d" % n, records(n, 2, 100 + n), 30, [1, 1], [10000, 10000])
    # acceptance mixes
    n = RUN + 1
    add("all_accepted", _all_accepted(records(n, 2, 1)), 0, [1, 1], [10000, 10000])
    add("none_accepted", records(n, 2, 2), 256, [1, 1], [10000, 10000])
    add("negative_mmq", records(n, 2, 3), -1, [1, 1], [10000, 10000])
    add("none_wanted", records(n, 2, 4), 0, [0, 0], [10000, 10000])
    add("second_wanted", records(n, 2, 5), 10, [0, 1], [10000, 10000])
    # n_refs
    add("one_ref", records(700, 1, 6), 20, [1], [10000])
    few = np.array([0, 17, 18, 400, 401, 998, 999])
    a = records(2 * RUN + 100, 1000, 7, tid=np.sort(few[np.random.default_rng(7).integers(0, 7, 2 * RUN + 100)]))
    add("thousand_refs_seven_with_reads", a, 0, np.ones(1000, np.uint8), np.full(1000, 10000))
    sel = np.ones(1000, np.uint8)
    sel[[17, 400]] = 0
    add("thousand_refs_two_unwanted", {k: v.copy() for k, v in a.items()}, 0, sel, np.full(1000, 10000))
    # keyerror: an accepted record on no reference of the header, first and last
    a = _all_accepted(records(RUN + 70, 2, 8))
    a["tid"][0] = -1
    add("keyerror_first", a, 0, [1, 1], [10000, 10000])
    a = _all_accepted(records(RUN + 70, 2, 9))
    a["tid"][-1] = 2
    add("keyerror_last", a, 0, [1, 1], [10000, 10000])
    a = records(RUN + 70, 2, 10)
    a["flag"][[0, 5, -1]] = 0
    a["mapq"][[0, 5, -1]] = 60
    a["flag"][1:5] = 4
    a["tid"][5] = 7
    a["tid"][-1] = -1
    add("keyerror_after_unmapped", a, 0, [1, 1], [10000, 10000])
    # tid order among the selected reads
    for name, at in (("inside_a_wave", 10), ("wave_boundary", 64), ("step_boundary", 256 + 64),
                     ("workgroup_boundary", RUN), ("second_workgroup_boundary", 2 * RUN)):
        a = _all_accepted(records(2 * RUN + 50, 3, 11 + at))
        a["tid"][:] = 1
        a["tid"][at:] = 0
        add("tid_decrease_" + name, a, 0, [1, 1, 1], [10000] * 3, ST_UNGROUPED)
    a = _all_accepted(records(2 * RUN + 50, 3, 12))
    a["tid"][:] = 1
    a["tid"][RUN - 3:RUN + 2] = 0  # these five are unmapped: the selected reads stay in order
    a["flag"][RUN - 3:RUN + 2] = 4
    add("tid_decrease_only_among_unselected", a, 0, [1, 1, 1], [10000] * 3)
    a = _all_accepted(records(2 * RUN + 50, 3, 13))
    a["tid"][:] = 2
    a["tid"][RUN:] = 0  # reference 2 is not wanted: the selected reads are reference 0's
    add("tid_decrease_from_an_unwanted_reference", a, 0, [1, 1, 0], [10000] * 3)
    # pos order within a reference, at a wave boundary of the compacted order, and across references
    a = _all_accepted(records(300, 2, 14))
    a["tid"][:200] = 0
    a["tid"][200:] = 1
    a["pos"][:] = np.arange(300) + 10
    a["pos"][64] = 5
    add("pos_decrease_at_wave_boundary", a, 0, [1, 1], [10000, 10000])
    a = _all_accepted(records(300, 2, 15))
    a["tid"][:128] = 0
    a["tid"][128:] = 1
    a["pos"][:] = np.arange(300) + 1000
    a["pos"][128:] = np.arange(172)  # a decrease exactly where the reference changes: still sorted
    add("pos_decrease_across_references", a, 0, [1, 1], [10000, 10000])
    # inside
    a = _all_accepted(records(130, 3, 16))
    a["tid"][:] = np.repeat([0, 1, 2], [50, 50, 30])
    a["pos"][:] = 100
    a["ref_span"][:] = 50
    a["ref_span"][49] = 900   # 100 + 900 == L: inside
    a["ref_span"][99] = 901   # == L + 1: not inside
    a["pos"][100:] = 2**31 - 1
    a["ref_span"][100:] = 2**31 - 5  # the sum needs 64 bits
    add("inside_edges", a, 0, [1, 1, 1], [1000, 1000, big])
    a = {k: v.copy() for k, v in a.items()}
    a["pos"][120] = -1
    a["rec_err"][120] = 16
    a["rec_err"][3] = 8
    add("negative_pos_and_rec_err", a, 0, [1, 1, 1], [1000, 1000, 2**32 - 7])
    # a straddling wave: many references inside one wave of the compacted order
    a = _all_accepted(records(RUN + 200, 40, 17))
    add("forty_refs", a, 0, np.arange(40) % 3 != 1, np.full(40, 3000))
    # offsets that do not fit 32 bits
    a = records(200, 2, 18)
    a["cig_off"][-1] = 2**32
    add("cigar_words_too_large", a, 0, [1, 1], [10000, 10000], ST_TOO_LARGE)
    a = records(200, 2, 19)
    a["seq_off"][-1] = 2**31
    add("seq_bytes_too_large", a, 0, [1, 1], [10000, 10000], ST_TOO_LARGE)
    a = records(200, 2, 20)
    a["cig_off"][-1] = 2**32 - 1
    a["seq_off"][-1] = 2**31 - 1
    add("offsets_just_fit", a, 0, [1, 1], [10000, 10000])
    return out


def assert_matches(got, exp, name, n_cap=None):
    """Every output of one selection against select_ref's.  ``got`` holds full-capacity arrays
    that were poisoned before the call: the slots past n_selected must still be poison."""
    assert got["status"] == exp["status"], "%s: status %d, expected %d" % (name, got["status"], exp["status"])
    if exp["status"] != ST_OK:
        return
    for k in HEADER:
        assert int(got[k]) == int(exp[k]), "%s: header %s = %d, expected %d" % (name, k, int(got[k]), int(exp[k]))
    m = exp["n_selected"]
    for k, dt in READ_ARRAYS:
        assert np.array_equal(got[k][:m], exp[k]), "%s: %s differs" % (name, k)
        rest = np.ascontiguousarray(got[k][m:]).view(np.uint8)
        assert bool(np.all(rest == POISON)), "%s: %s written past n_selected" % (name, k)
    assert np.array_equal(got["ref_beg"], exp["ref_beg"]), "%s: ref_beg differs" % name
    for k, dt in REF_ARRAYS:
        assert np.array_equal(got[k], exp[k]), "%s: per-reference %s differs" % (name, k)


# ---- the file format of tests/native/select_check.cpp ----
def pack_input(cs):
    b = [struct.pack("<I", len(cs))]
    for _, a, mmq, ref_sel, ref_len, _ in cs:
        n = a["tid"].size
        b.append(struct.pack("<qiq", n, len(ref_sel), int(mmq)))
        for k, dt, extra in REC_FIELDS:
            arr = np.ascontiguousarray(a[k], dt)
            assert arr.size == n + extra, k
            b.append(arr.tobytes())
        b.append(np.ascontiguousarray(ref_sel, np.uint8).tobytes())
        b.append(np.ascontiguousarray(ref_len, np.int64).tobytes())
    return b"".join(b)


def unpack_results(buf, cs):
    res, at = [], 0
    for _, a, _, ref_sel, _, _ in cs:
        n, nr = a["tid"].size, len(ref_sel)
        r = {}
        r["guards"], = struct.unpack_from("<I", buf, at)
        at += 4
        (r["status"], r["batch_err_or"], r["n_accepted"], r["n_selected"], r["keyerror_rec"],
         r["keyerror_ordinal"]) = struct.unpack_from("<iIqqqq", buf, at)
        at += 64
        for k, dt in READ_ARRAYS:
            r[k] = np.frombuffer(buf, dt, n, at)
            at += n * np.dtype(dt).itemsize
        r["ref_beg"] = np.frombuffer(buf, np.int64, nr + 1, at)
        at += 8 * (nr + 1)
        for k, dt in REF_ARRAYS:
            r[k] = np.frombuffer(buf, dt, nr, at)
            at += nr * np.dtype(dt).itemsize
        res.append(r)
    assert at == len(buf)
    return res
