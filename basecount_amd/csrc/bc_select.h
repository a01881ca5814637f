// bc_select.h — the read selection of a decoded batch, on the device and on the host.
//
// The specification is bcio_select (bcio.cpp), bit for bit: which records the read loop accepts,
// which of them lie on a requested reference, the per-read fields of the GPU batch format and the
// order they come out in (by reference, file order within a reference).  Every decision about a
// record is a function of this header; bc_select.hip runs them on the device, and
// bcs_select_host below (tests/native/select_check.cpp, under AddressSanitizer) runs the same
// functions as plain loops over the kernels' schedule.
//
// The device handles the batches whose SELECTED reads have non-decreasing tid (DESIGN.md §3 "Device
// read selection"): then "by reference, file order within" is the file order of the selected reads,
// so a stable compaction is the whole partition and ref_beg[t] is the lower bound of t in the
// compacted tids.  Any other batch gets status BCS_ST_UNGROUPED, a batch whose CIGAR / SEQ offsets
// do not fit 32 bits BCS_ST_TOO_LARGE; then no output array is to be trusted and the caller runs
// bcio_select.  Whatever the input, no access leaves the arrays: ranks are bounded by the counts.
//
// Schedule (a workgroup is BCS_WAVES waves; wave w of workgroup g takes the BCS_STEPS * 64
// consecutive records from g * BCS_RUN + w * BCS_STEPS * 64, 64 a step):
//   count    per workgroup: accepted and selected records, the first accepted record not wanted
//   scan     exclusive prefix sums of the two columns; the header
//   scatter  rank = workgroup base + waves before + steps before + lanes before; the per-read
//            arrays, the compacted tid and rec_err; the keyerror record's lane writes its ordinal
//   refs     a thread per reference: ref_beg by lower bound, n_reads, the facts' neutral values
//   facts    a thread per selected read: the order test against its predecessor, the per-reference
//            facts (max_span, max_end, n_complex, sum_ops, err_or, the sorted / inside flags)
#pragma once
#include <stdint.h>

#include "bc_bam.h"

#define BCS_ST_OK 0
#define BCS_ST_UNGROUPED 1  /* the selected reads' tids decrease somewhere                  */
#define BCS_ST_TOO_LARGE 2  /* cig_off[n] or 2 * seq_off[n] above 2^32 - 1 (wins over 1)    */

#define BCS_WAVES 4u
#define BCS_STEPS 4u
#define BCS_THREADS (64u * BCS_WAVES)
#define BCS_WAVE_RUN (64u * BCS_STEPS)
#define BCS_RUN (BCS_WAVE_RUN * BCS_WAVES) /* records of one workgroup */
#define BCS_MAX_N 0x7FFFFFFFll

#define BCS_F_SORTED 1u /* pos non-decreasing within the reference */
#define BCS_F_INSIDE 2u /* every read has 0 <= pos and pos + span <= L */

// the header (basecount_hip.h's bc_sel_header has this layout)
struct bcs_header {
    int32_t status;  // BCS_ST_*
    uint32_t err_or; // OR of rec_err over the selected reads
    int64_t n_accepted;
    int64_t n_selected;
    int64_t keyerror_rec;  // first accepted record that is not wanted, else -1
    int64_t keyerror_ordinal;
    int64_t reserved[3];
};

// the outputs (basecount_hip.h's bc_sel_arrays has this layout)
struct bcs_arrays {
    int32_t* pos;  // [n_selected] each, capacity n_cap
    uint32_t* cig_beg;
    uint32_t* cig_n;
    uint32_t* seq_nib;
    uint32_t* qlen;
    int64_t* span;
    int64_t* rec;
    int64_t* ordinal;
    int64_t n_cap;
    int64_t* ref_beg;  // [n_refs + 1]
    int64_t* max_span; // [n_refs] each, capacity ref_cap
    int64_t* max_end;
    int64_t* n_reads;
    int64_t* n_complex;
    uint64_t* sum_ops;
    uint32_t* err_or;
    uint32_t* flags;  // BCS_F_*
    int64_t ref_cap;
    bcs_header* header;
};

// the work buffer: three int64 columns of one entry per workgroup, the compacted tid and rec_err
struct bcs_layout {
    uint32_t nwg;
    uint64_t acc_off, sel_off, ke_off, ctid_off, cerr_off, total;
};

BCB_HD bcs_layout bcs_make_layout(int64_t n, int64_t n_refs) {
    (void)n_refs;
    bcs_layout l;
    const uint64_t un = (uint64_t)n;
    l.nwg = (uint32_t)((un + BCS_RUN - 1) / BCS_RUN);
    if (l.nwg == 0) l.nwg = 1;
    const uint64_t col = ((uint64_t)l.nwg * 8u + 15u) & ~(uint64_t)15u;
    const uint64_t per = ((un > 0 ? un : 1u) * 4u + 15u) & ~(uint64_t)15u;
    l.acc_off = 0;
    l.sel_off = col;
    l.ke_off = 2 * col;
    l.ctid_off = 3 * col;
    l.cerr_off = l.ctid_off + per;
    l.total = l.cerr_off + per;
    return l;
}

struct bcs_work {
    int64_t *acc, *sel, *ke;
    int32_t* ctid;
    uint32_t* cerr;
    uint32_t nwg;
};

BCB_HD bcs_work bcs_bind(void* mem, const bcs_layout& l) {
    uint8_t* p = (uint8_t*)mem;
    bcs_work w;
    w.acc = (int64_t*)(p + l.acc_off);
    w.sel = (int64_t*)(p + l.sel_off);
    w.ke = (int64_t*)(p + l.ke_off);
    w.ctid = (int32_t*)(p + l.ctid_off);
    w.cerr = (uint32_t*)(p + l.cerr_off);
    w.nwg = l.nwg;
    return w;
}

// ---- the decisions ----

// main.py:165: not is_unmapped (flag bit 4 only) and mapping_quality >= min_mapping_quality
BCB_HD bool bcs_accepted(uint16_t flag, uint8_t mapq, int64_t min_mapq) { return !(flag & 4) && (int64_t)mapq >= min_mapq; }

BCB_HD bool bcs_wanted(int32_t tid, int32_t n_refs, const uint8_t* ref_sel) {
    return tid >= 0 && tid < n_refs && ref_sel[tid] != 0;
}

// bit 0: accepted, bit 1: selected (accepted and wanted)
BCB_HD uint32_t bcs_classify(const bcb_arrays& r, int64_t i, int64_t min_mapq, int32_t n_refs, const uint8_t* ref_sel) {
    if (!bcs_accepted(r.flag[i], r.mapq[i], min_mapq)) return 0u;
    return bcs_wanted(r.tid[i], n_refs, ref_sel) ? 3u : 1u;
}

BCB_HD bool bcs_too_large(uint64_t cig_off_n, uint64_t seq_off_n) {
    return cig_off_n > 0xFFFFFFFFull || seq_off_n > 0x7FFFFFFFull;  // 2 * seq_off[n] > 2^32 - 1
}

// record i to slot j of the outputs, with its ordinal
BCB_HD void bcs_store_read(const bcb_arrays& r, int64_t i, int64_t j, int64_t ordinal, const bcs_arrays& o,
                           const bcs_work& w) {
    const int32_t qs = r.qstart[i], ql = r.qend[i] - qs;
    const uint64_t c0 = r.cig_off[i];
    o.pos[j] = r.pos[i];
    o.cig_beg[j] = (uint32_t)c0;
    o.cig_n[j] = (uint32_t)(r.cig_off[i + 1] - c0);
    o.seq_nib[j] = (uint32_t)(2 * r.seq_off[i] + (uint64_t)(qs > 0 ? qs : 0));
    o.qlen[j] = (uint32_t)(ql > 0 ? ql : 0);
    o.span[j] = r.ref_span[i];
    o.rec[j] = i;
    o.ordinal[j] = ordinal;
    w.ctid[j] = r.tid[i];
    w.cerr[j] = r.rec_err[i];
}

// first j in [0, m) with ctid[j] >= t, else m: log2(m) steps whatever the array holds
BCB_HD int64_t bcs_lower_bound(const int32_t* ctid, int64_t m, int32_t t) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ctid[mid] < t)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// reference t's row before any read is seen
BCB_HD void bcs_ref_init(int32_t t, int32_t n_refs, int64_t m, const bcs_arrays& o, const bcs_work& w) {
    const int64_t b0 = t < n_refs ? bcs_lower_bound(w.ctid, m, t) : m;
    o.ref_beg[t] = b0;
    if (t >= n_refs) return;
    const int64_t b1 = t + 1 < n_refs ? bcs_lower_bound(w.ctid, m, t + 1) : m;
    const bool any = b1 > b0;
    o.n_reads[t] = any ? b1 - b0 : 0;
    o.max_span[t] = 0;
    o.max_end[t] = any ? INT64_MIN : 0;  // every read raises it
    o.n_complex[t] = 0;
    o.sum_ops[t] = 0;
    o.err_or[t] = 0;
    o.flags[t] = BCS_F_SORTED | BCS_F_INSIDE;
}

// what selected read j adds to its reference's row
struct bcs_fact {
    int32_t tid;
    int64_t span, end;
    uint32_t ops, complex, err;
    uint32_t clear;      // BCS_F_* bits this read takes away
    uint32_t ungrouped;  // its predecessor's tid is larger
};

BCB_HD bool bcs_inside(int32_t pos, int64_t span, int64_t L) { return pos >= 0 && (int64_t)pos + span <= L; }

BCB_HD bcs_fact bcs_read_fact(int64_t j, const bcs_arrays& o, const bcs_work& w, const int64_t* ref_len) {
    bcs_fact f;
    f.tid = w.ctid[j];
    const int32_t p = o.pos[j];
    f.span = o.span[j];
    f.end = (int64_t)p + f.span;
    f.ops = o.cig_n[j];
    f.complex = f.ops > 8u ? 1u : 0u;
    f.err = w.cerr[j];
    f.clear = bcs_inside(p, f.span, ref_len[f.tid]) ? 0u : BCS_F_INSIDE;
    f.ungrouped = 0;
    if (j > 0) {
        const int32_t tp = w.ctid[j - 1];
        if (tp > f.tid) f.ungrouped = 1;
        if (tp == f.tid && o.pos[j - 1] > p) f.clear |= BCS_F_SORTED;  // (across a boundary: not counted)
    }
    return f;
}

// ---- the whole selection on one lane: the host instantiation ----
#if !defined(__HIP_DEVICE_COMPILE__)
// `work` holds bcs_make_layout(n, n_refs).total bytes.  Returns the header's status.
inline int bcs_select_host(const bcb_arrays& r, int64_t n, int64_t min_mapq, const uint8_t* ref_sel, const int64_t* ref_len,
                           int32_t n_refs, void* work, const bcs_arrays& o) {
    const bcs_layout l = bcs_make_layout(n, n_refs);
    const bcs_work w = bcs_bind(work, l);
    // count: a workgroup's waves and steps in order are its records in order
    for (uint32_t g = 0; g < l.nwg; ++g) {
        int64_t acc = 0, sel = 0, ke = -1;
        for (uint32_t wv = 0; wv < BCS_WAVES; ++wv)
            for (uint32_t s = 0; s < BCS_STEPS; ++s)
                for (uint32_t ln = 0; ln < 64u; ++ln) {
                    const int64_t i = (int64_t)g * BCS_RUN + wv * BCS_WAVE_RUN + s * 64u + ln;
                    if (i >= n) continue;
                    const uint32_t c = bcs_classify(r, i, min_mapq, n_refs, ref_sel);
                    if (c == 1u && ke < 0) ke = i;
                    acc += c & 1u;
                    sel += c >> 1;
                }
        w.acc[g] = acc;
        w.sel[g] = sel;
        w.ke[g] = ke;
    }
    // scan
    bcs_header h{};
    h.keyerror_rec = h.keyerror_ordinal = -1;
    for (uint32_t g = 0; g < l.nwg; ++g) {
        const int64_t a = w.acc[g], s = w.sel[g];
        w.acc[g] = h.n_accepted;
        w.sel[g] = h.n_selected;
        h.n_accepted += a;
        h.n_selected += s;
        if (h.keyerror_rec < 0 && w.ke[g] >= 0) h.keyerror_rec = w.ke[g];
    }
    h.status = bcs_too_large(r.cig_off[n], r.seq_off[n]) ? BCS_ST_TOO_LARGE : BCS_ST_OK;
    *o.header = h;
    // scatter
    for (uint32_t g = 0; g < l.nwg; ++g) {
        int64_t ord = w.acc[g], j = w.sel[g];
        for (int64_t i = (int64_t)g * BCS_RUN, e = i + BCS_RUN < n ? i + BCS_RUN : n; i < e; ++i) {
            const uint32_t c = bcs_classify(r, i, min_mapq, n_refs, ref_sel);
            if (c == 3u) bcs_store_read(r, i, j++, ord, o, w);
            if (c == 1u && i == o.header->keyerror_rec) o.header->keyerror_ordinal = ord;
            ord += c & 1u;
        }
    }
    // refs, facts
    const int64_t m = o.header->n_selected;
    for (int32_t t = 0; t <= n_refs; ++t) bcs_ref_init(t, n_refs, m, o, w);
    for (int64_t j = 0; j < m; ++j) {
        const bcs_fact f = bcs_read_fact(j, o, w, ref_len);
        if (f.ungrouped && o.header->status < BCS_ST_UNGROUPED) o.header->status = BCS_ST_UNGROUPED;
        o.header->err_or |= f.err;
        const int32_t t = f.tid;
        if (f.span > o.max_span[t]) o.max_span[t] = f.span;
        if (f.end > o.max_end[t]) o.max_end[t] = f.end;
        o.n_complex[t] += f.complex;
        o.sum_ops[t] += f.ops;
        o.err_or[t] |= f.err;
        o.flags[t] &= ~f.clear;
    }
    return o.header->status;
}
#endif
