// bc_bam.h — BAM record decode of a buffer of inflated bytes, on the device and on the host.
//
// Every decision about bytes is in this header: the record rules (what bcio.cpp's hop_records
// accepts and refuses, restated), the plausibility predicate of the speculation, the hop over one
// segment, the stitch that proves the chain exact, and the field extraction (bcio.cpp's
// fill_records / query_start / query_end / seq_to_event, restated).  bc_bam.hip runs these functions
// on the device; tests/native/bamdecode_check.cpp runs the same functions as plain loops under
// AddressSanitizer.  The outputs are specified as byte-identical to the host decoder's arrays.
//
// Finding the record chain (DESIGN.md §3 "Device record decode"):
//   speculate  raw[0, N) is cut into segments of seg_bytes.  For each segment the first offset that
//              passes bcb_plausible is its entry (the segment that holds the known first record
//              offset takes that instead); bcb_hop walks from the entry to the first start at or
//              past the segment's end under the record rules only, storing each start with the
//              running CIGAR-word and SEQ-byte counts.
//   stitch     bcb_stitch walks from the known first offset e: the segment that holds e is
//              e / seg_bytes; its speculation counts only if its entry is exactly e, else the segment
//              is hopped again from e (a repair).  Segments the chain jumps over are never looked at.
//              By induction every accepted start is a true start, whatever the predicate let through.
//   fill       each accepted segment's records go to the output arrays at the stitch's prefix sums.
//
// Hard guarantee, whatever the bytes: no read leaves raw[0, N).  bcb_record_at checks q + 4 <= N
// before the length prefix and q + 4 + block_size <= N before any field; every later read of the
// record is inside [q, q + 4 + block_size) by the field rule.  Offsets are 32-bit: N < 2^31 is the
// caller's check (BCB_ST_TOO_LARGE), so sums of offsets and counts cannot wrap.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BCB_HD __host__ __device__ __forceinline__
#else
#define BCB_HD inline
#endif

// status of a fill (bc_bam_batch.status) and of one record / one segment's hop
#define BCB_ST_OK 0
#define BCB_ST_PARTIAL_LEN 1 /* fewer than 4 bytes left: "truncated record length" when final    */
#define BCB_ST_PARTIAL 2     /* the record ends past the buffer: "truncated BAM record" when final */
#define BCB_ST_SHORT 3       /* block_size < 32: "truncated BAM record"                            */
#define BCB_ST_NEG_LSEQ 4    /* "negative l_seq"                                                   */
#define BCB_ST_FIELDS 5      /* "BAM record shorter than its fields"                               */
#define BCB_ST_TOO_LARGE 6   /* raw_bytes >= 2^31: not indexed with 32 bits                        */
#define BCB_ST_REPAIRS 7     /* more wrong segments than the repair bound                          */
#define BCB_ST_INTERNAL 8    /* a segment held more starts than its slots (cannot happen)          */

#define BCB_NO_ENTRY 0xFFFFFFFFu
#define BCB_MAX_RAW 0x7FFFFFFFull
#define BCB_MIN_SEG 64u
#define BCB_CHAIN 3 /* records the plausibility predicate follows */

// per-record status bits: bcio.h's BCIO_REC_* (tests compare the arrays)
#define BCB_REC_NO_CIGAR 1u
#define BCB_REC_NO_SEQ 2u
#define BCB_REC_NO_QUAL 4u
#define BCB_REC_BAD_CLIP 8u
#define BCB_REC_NEG_POS 16u

// what bc_bam_index returns (basecount_hip.h's bc_bam_batch has this layout)
struct bcb_result {
    int64_t n;             // records taken
    uint64_t used;         // offset after the last record taken
    uint64_t cigar_words;  // = cig_off[n]
    uint64_t seq_bytes;    // = seq_off[n]
    int32_t status;        // BCB_ST_*; non-zero: the fill is declined
    int32_t reserved;
    uint64_t err_off;      // the offset the status speaks of
    int64_t segments;
    int64_t repaired;
    uint64_t raw_bytes;    // the arguments the work buffer was laid out for
    uint64_t seg_bytes;
};

struct bcb_seg {
    uint32_t entry;     // first record start the hop began at, BCB_NO_ENTRY if none was found
    uint32_t exit;      // first start at or past the segment's end, or where the hop stopped
    uint32_t nrec;      // starts stored
    uint32_t status;    // BCB_ST_OK, or why the hop stopped at `exit`
    uint32_t take;      // stitch: records of this segment in the batch (0: skipped)
    uint32_t rec_base;  // stitch: prefix sums over the accepted segments before this one
    uint32_t cig_base;
    uint32_t seq_base;
};

// the work buffer: result, segment table, then three slot arrays of nseg * (cap + 1) words
struct bcb_layout {
    uint32_t nseg, cap;  // cap: most starts one segment can hold (records are >= 36 bytes)
    uint64_t segs_off, starts_off, cigx_off, seqx_off, total;
};

BCB_HD bcb_layout bcb_make_layout(uint64_t raw_bytes, uint64_t seg_bytes) {
    bcb_layout l;
    l.nseg = (uint32_t)((raw_bytes + seg_bytes - 1) / seg_bytes);
    if (l.nseg == 0) l.nseg = 1;
    l.cap = (uint32_t)(seg_bytes / 36u) + 1u;
    const uint64_t slots = (uint64_t)l.nseg * (l.cap + 1u);
    l.segs_off = 128;
    l.starts_off = (l.segs_off + (uint64_t)l.nseg * sizeof(bcb_seg) + 15u) & ~(uint64_t)15u;
    l.cigx_off = l.starts_off + ((slots * 4u + 15u) & ~(uint64_t)15u);
    l.seqx_off = l.cigx_off + ((slots * 4u + 15u) & ~(uint64_t)15u);
    l.total = l.seqx_off + ((slots * 4u + 15u) & ~(uint64_t)15u);
    return l;
}

struct bcb_work {
    bcb_result* res;
    bcb_seg* segs;
    uint32_t *starts, *cigx, *seqx;
    uint32_t nseg, cap;
};

BCB_HD bcb_work bcb_bind(void* mem, const bcb_layout& l) {
    uint8_t* p = (uint8_t*)mem;
    bcb_work w;
    w.res = (bcb_result*)p;
    w.segs = (bcb_seg*)(p + l.segs_off);
    w.starts = (uint32_t*)(p + l.starts_off);
    w.cigx = (uint32_t*)(p + l.cigx_off);
    w.seqx = (uint32_t*)(p + l.seqx_off);
    w.nseg = l.nseg;
    w.cap = l.cap;
    return w;
}

// the output arrays (basecount_hip.h's bc_bam_arrays has this layout): bcio_records' arrays
struct bcb_arrays {
    int32_t* tid;
    int32_t* pos;
    uint16_t* flag;
    uint8_t* mapq;
    int32_t* l_seq;
    int32_t* qstart;
    int32_t* qend;
    uint32_t* rec_err;
    int64_t* ref_span;
    uint64_t* cig_off;   // [n + 1]
    uint64_t* seq_off;   // [n + 1]
    uint32_t* cigar;     // [cigar_words]
    uint8_t* seq;        // [seq_bytes] BAM packing; may be NULL (not written)
    uint8_t* seq_event;  // [bcb_seq_event_bytes(seq_bytes)] BC_SEQ_EVENT, zero tail
    uint8_t* qual;       // [2 * seq_bytes] by nibble index; written only with want_qual
    int64_t n_cap;       // what the arrays hold: records, CIGAR words, SEQ bytes
    uint64_t cigar_cap;
    uint64_t seq_cap;
};

BCB_HD uint64_t bcb_seq_event_bytes(uint64_t n) { return (n + 15) / 16 * 16 + 16; }

BCB_HD uint32_t bcb_rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
BCB_HD uint32_t bcb_rd32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

struct bcb_rec {
    uint32_t bs;   // block_size
    uint32_t lrn;  // l_read_name
    uint32_t nc;   // n_cigar_op
    int32_t ls;    // l_seq
};

// The record rules at offset q of raw[0, N), in hop_records' order.  BCB_ST_OK: the whole record
// [q, q + 4 + bs) is inside the buffer and its fields fit it.
BCB_HD int bcb_record_at(const uint8_t* raw, uint32_t N, uint32_t q, bcb_rec* r) {
    if ((uint64_t)q + 4 > N) return BCB_ST_PARTIAL_LEN;
    const uint32_t bs = bcb_rd32(raw + q);
    if (bs < 32) return BCB_ST_SHORT;
    if ((uint64_t)q + 4 + bs > N) return BCB_ST_PARTIAL;
    const uint8_t* f = raw + q + 4;
    const int32_t ls = (int32_t)bcb_rd32(f + 16);
    if (ls < 0) return BCB_ST_NEG_LSEQ;
    const uint32_t lrn = f[8], nc = bcb_rd16(f + 12);
    if (32ull + lrn + 4ull * nc + (((uint64_t)ls + 1) / 2) + (uint64_t)ls > bs) return BCB_ST_FIELDS;
    r->bs = bs;
    r->lrn = lrn;
    r->nc = nc;
    r->ls = ls;
    return BCB_ST_OK;
}

// The speculation's guess that a record starts at q: a short chain of records that pass the rules,
// name a reference of the header (or none) and carry a NUL-terminated name.  The first must be
// complete; the chain may end at the buffer's end.  Free to be wrong either way: see bcb_stitch.
BCB_HD bool bcb_plausible(const uint8_t* raw, uint32_t N, uint32_t q, int32_t n_refs) {
    for (int k = 0; k < BCB_CHAIN; ++k) {
        bcb_rec r;
        const int st = bcb_record_at(raw, N, q, &r);
        if (st == BCB_ST_PARTIAL_LEN || st == BCB_ST_PARTIAL) return k > 0;
        if (st != BCB_ST_OK) return false;
        const uint8_t* f = raw + q + 4;
        const int32_t tid = (int32_t)bcb_rd32(f), ntid = (int32_t)bcb_rd32(f + 20);
        if (tid < -1 || tid >= n_refs || ntid < -1 || ntid >= n_refs) return false;
        if (r.lrn < 1 || f[32 + r.lrn - 1] != 0) return false;
        q += 4 + r.bs;
        if (q == N) return true;
    }
    return true;
}

// Hop from the record start q to the first start at or past seg_end (<= N) under the record rules
// only.  Slot j of the segment gets start j and the CIGAR words / SEQ bytes of the records before
// it; slot nrec gets the exit and the totals.
BCB_HD void bcb_hop(const uint8_t* raw, uint32_t N, uint32_t q, uint32_t seg_end, uint32_t cap, uint32_t* starts,
                    uint32_t* cigx, uint32_t* seqx, bcb_seg* sg) {
    uint32_t n = 0, cg = 0, sq = 0, st = BCB_ST_OK;
    sg->entry = q;
    while (q < seg_end) {
        bcb_rec r;
        st = (uint32_t)bcb_record_at(raw, N, q, &r);
        if (st != BCB_ST_OK) break;
        if (n >= cap) {
            st = BCB_ST_INTERNAL;
            break;
        }
        starts[n] = q;
        cigx[n] = cg;
        seqx[n] = sq;
        ++n;
        cg += r.nc;
        sq += ((uint32_t)r.ls + 1u) / 2u;
        q += 4u + r.bs;
    }
    starts[n] = q;
    cigx[n] = cg;
    seqx[n] = sq;
    sg->exit = q;
    sg->nrec = n;
    sg->status = st;
}

// One segment's speculation for a machine of one lane (the device searches the entry with a wave:
// bc_bam.hip).  Segment `first / seg_bytes` starts at the known first offset.
BCB_HD uint32_t bcb_seg_end(uint32_t s, uint32_t seg_bytes, uint32_t N) {
    const uint64_t e = ((uint64_t)s + 1) * seg_bytes;
    return e < N ? (uint32_t)e : N;
}

BCB_HD void bcb_speculate_from(const uint8_t* raw, uint32_t N, uint32_t s, uint32_t seg_bytes, uint32_t entry,
                               const bcb_work& w) {
    bcb_seg* sg = &w.segs[s];
    const uint64_t slot = (uint64_t)s * (w.cap + 1u);
    sg->take = 0;
    sg->rec_base = sg->cig_base = sg->seq_base = 0;
    if (entry == BCB_NO_ENTRY) {
        sg->entry = BCB_NO_ENTRY;
        sg->exit = 0;
        sg->nrec = 0;
        sg->status = BCB_ST_OK;
        return;
    }
    bcb_hop(raw, N, entry, bcb_seg_end(s, seg_bytes, N), w.cap, w.starts + slot, w.cigx + slot, w.seqx + slot, sg);
}

BCB_HD void bcb_speculate_seg(const uint8_t* raw, uint32_t N, uint32_t s, uint32_t seg_bytes, uint32_t first,
                              int32_t n_refs, const bcb_work& w) {
    uint32_t entry = BCB_NO_ENTRY;
    const uint32_t beg = s * seg_bytes, end = bcb_seg_end(s, seg_bytes, N);
    if (first >= beg && first < end) {
        entry = first;
    } else {
        for (uint32_t q = beg; q < end; ++q)
            if (bcb_plausible(raw, N, q, n_refs)) {
                entry = q;
                break;
            }
    }
    bcb_speculate_from(raw, N, s, seg_bytes, entry, w);
}

BCB_HD uint32_t bcb_repair_bound(uint32_t nseg) { return 16u + nseg / 4u; }

// The verification, from the known first offset.  Uses the record rules and induction only.
// max_records >= 0; hop_records' order: the cut at max_records comes before the next record is
// looked at, so a violation or a partial record behind the cut is not this batch's.
BCB_HD void bcb_stitch(const uint8_t* raw, uint32_t N, uint32_t seg_bytes, uint32_t first, int64_t max_records,
                       bool final, const bcb_work& w) {
    bcb_result* res = w.res;
    uint32_t e = first, n = 0, cg = 0, sq = 0, repaired = 0;
    int32_t status = BCB_ST_OK;
    while (e < N && (int64_t)n < max_records) {
        const uint32_t s = e / seg_bytes;
        bcb_seg* sg = &w.segs[s];
        const uint64_t slot = (uint64_t)s * (w.cap + 1u);
        if (sg->entry != e) {
            if (++repaired > bcb_repair_bound(w.nseg)) {
                status = BCB_ST_REPAIRS;
                break;
            }
            bcb_hop(raw, N, e, bcb_seg_end(s, seg_bytes, N), w.cap, w.starts + slot, w.cigx + slot, w.seqx + slot, sg);
        }
        const int64_t left = max_records - (int64_t)n;
        const uint32_t take = (int64_t)sg->nrec >= left ? (uint32_t)left : sg->nrec;
        sg->rec_base = n;
        sg->cig_base = cg;
        sg->seq_base = sq;
        sg->take = take;
        n += take;
        cg += w.cigx[slot + take];
        sq += w.seqx[slot + take];
        e = w.starts[slot + take];
        if ((int64_t)n >= max_records) break;  // the cut: nothing behind it is looked at
        if (sg->status != BCB_ST_OK) {
            const bool partial = sg->status == BCB_ST_PARTIAL_LEN || sg->status == BCB_ST_PARTIAL;
            if (!partial || final) status = (int32_t)sg->status;
            break;
        }
    }
    res->n = n;
    res->used = e;
    res->cigar_words = cg;
    res->seq_bytes = sq;
    res->status = status;
    res->reserved = 0;
    res->err_off = e;
    res->segments = w.nseg;
    res->repaired = repaired;
    res->raw_bytes = N;
    res->seg_bytes = seg_bytes;
}

// ---- field extraction ----

// BAM 4-bit code -> BC_SEQ_EVENT class: A 1, C 2, G 4, T 8, N(15) 3, others 0; one nibble per code
BCB_HD uint32_t bcb_event_class(uint32_t code) { return (uint32_t)(0x3000000800040210ull >> (4u * code)) & 15u; }
// one packed byte: the nibbles swapped (base 2m to the low nibble) and classified
BCB_HD uint8_t bcb_event_byte(uint8_t b) { return (uint8_t)(bcb_event_class(b >> 4) | (bcb_event_class(b & 15u) << 4)); }

// pysam getQueryStart over the CIGAR words at raw + c
BCB_HD int32_t bcb_query_start(const uint8_t* cig, uint32_t n, int32_t l_qseq, bool* bad) {
    int32_t start = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t w = bcb_rd32(cig + 4 * k), op = w & 0xf;
        if (op == 5) {
            if (start != 0 && start != l_qseq) *bad = true;
        } else if (op == 4) {
            start += (int32_t)(w >> 4);
        } else {
            break;
        }
    }
    return start;
}

// pysam getQueryEnd: walk back from the last op, never looking at op 0
BCB_HD int32_t bcb_query_end(const uint8_t* cig, uint32_t n, int32_t l_qseq, bool* bad) {
    int32_t end = l_qseq;
    if (end == 0) {
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t w = bcb_rd32(cig + 4 * k), op = w & 0xf, len = w >> 4;
            if (op == 0 || op == 1 || op == 7 || op == 8 || (op == 4 && end == 0)) end += (int32_t)len;
        }
    } else {
        for (uint32_t k = n; k-- > 1;) {
            const uint32_t w = bcb_rd32(cig + 4 * k), op = w & 0xf;
            if (op == 5) {
                if (end != l_qseq) *bad = true;
            } else if (op == 4) {
                end -= (int32_t)(w >> 4);
            } else {
                break;
            }
        }
    }
    return end;
}

// the header fields of a record the hop accepted (no rule is checked again)
BCB_HD void bcb_rec_sizes(const uint8_t* raw, uint32_t q, bcb_rec* r) {
    const uint8_t* f = raw + q + 4;
    r->bs = bcb_rd32(raw + q);
    r->lrn = f[8];
    r->nc = bcb_rd16(f + 12);
    r->ls = (int32_t)bcb_rd32(f + 16);
}

// record i's scalars: one lane's work
BCB_HD void bcb_fill_meta(const uint8_t* raw, uint32_t q, uint64_t i, uint64_t co, uint64_t so, const bcb_arrays& o) {
    bcb_rec r;
    bcb_rec_sizes(raw, q, &r);
    const uint8_t* f = raw + q + 4;
    const int32_t ps = (int32_t)bcb_rd32(f + 4);
    o.tid[i] = (int32_t)bcb_rd32(f);
    o.pos[i] = ps;
    o.mapq[i] = f[9];
    o.flag[i] = (uint16_t)bcb_rd16(f + 14);
    o.l_seq[i] = r.ls;
    o.cig_off[i] = co;
    o.seq_off[i] = so;
    const uint8_t* c = f + 32 + r.lrn;
    int64_t span = 0;  // reference-consuming ops M D N = X
    for (uint32_t k = 0; k < r.nc; ++k) {
        const uint32_t w = bcb_rd32(c + 4 * k);
        if ((0x18Du >> (w & 0xf)) & 1) span += w >> 4;
    }
    o.ref_span[i] = span;
    uint32_t err = 0;
    if (r.nc == 0) err |= BCB_REC_NO_CIGAR;
    if (r.ls == 0) err |= BCB_REC_NO_SEQ;
    // QUAL[0] is read only when the record has one (l_seq > 0 puts it inside the record)
    if (r.ls == 0 || c[4ull * r.nc + (((uint64_t)r.ls + 1) / 2)] == 0xFF) err |= BCB_REC_NO_QUAL;
    bool badclip = false;
    o.qstart[i] = bcb_query_start(c, r.nc, r.ls, &badclip);
    o.qend[i] = bcb_query_end(c, r.nc, r.ls, &badclip);
    if (badclip) err |= BCB_REC_BAD_CLIP;
    if (ps < 0) err |= BCB_REC_NEG_POS;
    o.rec_err[i] = err;
}

// a record's CIGAR words, SEQ and QUAL bytes, strided over `nl` lanes (1 on the host); source and
// destination offsets have any alignment
BCB_HD void bcb_fill_bytes(const uint8_t* raw, uint32_t q, uint64_t co, uint64_t so, const bcb_arrays& o,
                           bool want_qual, uint32_t lane, uint32_t nl) {
    bcb_rec r;
    bcb_rec_sizes(raw, q, &r);
    const uint8_t* c = raw + q + 36 + r.lrn;
    for (uint32_t k = lane; k < r.nc; k += nl) o.cigar[co + k] = bcb_rd32(c + 4 * k);
    const uint8_t* s = c + 4ull * r.nc;
    const uint32_t ls = (uint32_t)r.ls, sb = (ls + 1u) / 2u;
    for (uint32_t j = lane; j < sb; j += nl) {
        const uint8_t b = s[j];
        if (o.seq) o.seq[so + j] = b;
        o.seq_event[so + j] = bcb_event_byte(b);
    }
    if (want_qual) {
        const uint8_t* ql = s + sb;
        uint8_t* qd = o.qual + 2 * so;
        for (uint32_t j = lane; j < ls; j += nl) qd[j] = ql[j];
        if ((ls & 1u) && lane == 0) qd[ls] = 0xFF;  // pad byte of an odd-length read
    }
}

// the arrays' ends: the CSR totals and the zero tail of seq_event; strided over nl lanes
BCB_HD void bcb_fill_tail(const bcb_result* res, const bcb_arrays& o, uint32_t lane, uint32_t nl) {
    if (lane == 0) {
        o.cig_off[res->n] = res->cigar_words;
        o.seq_off[res->n] = res->seq_bytes;
    }
    const uint64_t end = bcb_seq_event_bytes(res->seq_bytes);
    for (uint64_t j = res->seq_bytes + lane; j < end; j += nl) o.seq_event[j] = 0;
}

// ---- the whole decode on one lane: the host instantiation (tests/native/bamdecode_check.cpp) ----
#if !defined(__HIP_DEVICE_COMPILE__)
// Index: speculate every segment, stitch.  `work` holds bcb_make_layout(raw_bytes, seg_bytes).total
// bytes.  Returns the result's status.
inline int bcb_index_host(const uint8_t* raw, uint64_t raw_bytes, uint64_t first, int64_t max_records, bool final,
                          int32_t n_refs, uint64_t seg_bytes, void* work) {
    const bcb_layout l = bcb_make_layout(raw_bytes, seg_bytes);
    const bcb_work w = bcb_bind(work, l);
    if (raw_bytes > BCB_MAX_RAW) {
        *w.res = bcb_result{};
        w.res->status = BCB_ST_TOO_LARGE;
        w.res->used = w.res->err_off = first;
        w.res->segments = l.nseg;
        w.res->raw_bytes = raw_bytes;
        w.res->seg_bytes = seg_bytes;
        return BCB_ST_TOO_LARGE;
    }
    const uint32_t N = (uint32_t)raw_bytes;
    for (uint32_t s = 0; s < l.nseg; ++s)
        bcb_speculate_seg(raw, N, s, (uint32_t)seg_bytes, (uint32_t)first, n_refs, w);
    bcb_stitch(raw, N, (uint32_t)seg_bytes, (uint32_t)first, max_records, final, w);
    return w.res->status;
}

inline void bcb_fill_host(const uint8_t* raw, const void* work, const bcb_arrays& o, bool want_qual) {
    const bcb_result* res = (const bcb_result*)work;
    const bcb_layout l = bcb_make_layout(res->raw_bytes, res->seg_bytes);
    const bcb_work w = bcb_bind(const_cast<void*>(work), l);
    for (uint32_t s = 0; s < l.nseg; ++s) {
        const bcb_seg& sg = w.segs[s];
        const uint64_t slot = (uint64_t)s * (w.cap + 1u);
        for (uint32_t j = 0; j < sg.take; ++j) {
            const uint32_t q = w.starts[slot + j];
            const uint64_t co = (uint64_t)sg.cig_base + w.cigx[slot + j], so = (uint64_t)sg.seq_base + w.seqx[slot + j];
            bcb_fill_meta(raw, q, (uint64_t)sg.rec_base + j, co, so, o);
            bcb_fill_bytes(raw, q, co, so, o, want_qual, 0, 1);
        }
    }
    bcb_fill_tail(res, o, 0, 1);
}
#endif
