// bc_fmt.h — the TSV rows of the per-position outputs, on the device and on the host.
//
// The specification is the text bcio_fmt_rows (bcio.cpp) produces, byte for byte: for position p of
// a segment named ref, cov = the 64-bit sum of the k counts and nz = the number of non-zero counts;
//   wide   ref \t pos \t cov, the k counts, the k percentages, entropy, secondary entropy, \n
//   long   k rows  ref \t pos \t cov \t BASE \t count \t pc \t ent \t sec \n   (A C G T DS N)
// a percentage prints as -1 when cov == 0, entropy as 1 when cov == 0, secondary entropy as 1 when
// cov == 0 or nz <= 1, and a value that is not printed is never inspected.  Floats print as
// str(round(x, dp)) for dp 0..4 (bcf_round below).  Every decision about a row is a function of this
// header; bc_fmt.hip runs them on the device, and bcf_rows_host (tests/native/fmt_check.cpp, under
// AddressSanitizer) runs the same functions as plain loops over the kernels' schedule.
//
// Declined, never failed: a printed value that is not finite or reaches 1e15 after scaling, or a
// name that is longer than 255 bytes or leaves the names array, gives status BCF_ST_VALUE and the
// first such array position; a text larger than the caller's buffer gives BCF_ST_TOO_SMALL with the
// exact total and segment offsets.  Then no text byte is to be trusted.  Whatever the arrays and
// the table hold, no access leaves the buffers: a position is read only below n, a name only inside
// the names array, and text is written only below the total of the same call.
//
// Schedule (a tile is 64 consecutive array positions; segments start at multiples of 64, so a
// tile's positions share one segment, found once per tile):
//   measure  a wave per tile: each lane the byte length of its position's row(s), kept in the work
//            buffer for write; the tile's byte count and its first declined position
//   scan     one workgroup: exclusive prefix sums of the tile byte counts, seg_off, the header
//   write    a wave per tile, only when the status is OK: each lane forms its row(s) at its
//            wave-prefix offset in a staging area of BCF_WIN bytes, the wave copies the area out
//            (16-byte stores from consecutive lanes, byte stores at the unaligned head and tail);
//            a tile with more text takes several windows, and a lane writes the part of its text
//            that falls into the current window
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BCF_HD __host__ __device__ __forceinline__
#else
#define BCF_HD inline
#endif

#define BCF_ST_OK 0
#define BCF_ST_TOO_SMALL 1 /* total_bytes > text_cap; total_bytes and seg_off are exact          */
#define BCF_ST_VALUE 2     /* a printed value or a name outside the cover (wins over 1)          */

#define BCF_TILE 64
#define BCF_STAGE 8192u            /* staging bytes of a wave                                     */
#define BCF_WIN (BCF_STAGE - 16u)  /* text bytes of one window: the area less the alignment skew  */
#define BCF_SCAN_THREADS 256u
#define BCF_MAX_NAME 255
#define BCF_MAX_DP 4

// the header (basecount_hip.h's bc_fmt_header has this layout)
struct bcf_header {
    int32_t status;  // BCF_ST_*
    int32_t reserved0;
    int64_t total_bytes;
    int64_t declined_pos;  // array position of the first declined value, else -1
    int64_t reserved[5];
};

// a segment (basecount_hip.h's bc_fmt_seg): array positions [beg, beg + len), printed as positions
// pos0 + 1 .. under the name names[name_off, name_off + name_len)
struct bcf_seg {
    int64_t beg, len, pos0;
    int32_t name_off, name_len;
};

// the inputs (basecount_hip.h's bc_fmt_args has this layout)
struct bcf_args {
    const int32_t* counts;  // [k][.] planes of `stride` elements
    const double* pc;       // [k][.] planes of `stride` elements
    const double* ent;
    const double* sec;
    int64_t stride;
    int64_t n;  // array positions
    const bcf_seg* segs;
    int64_t n_seg;
    const uint8_t* names;
    int64_t names_bytes;
    int32_t k, dp, long_format, reserved;
};

// the work buffer: per tile its byte count (scanned in place into its byte offset) and its first
// declined position (INT64_MAX: none), then per tile and lane the lane's text length (measure
// leaves it for write, which so holds the row function once, over the writer)
BCF_HD uint64_t bcf_tiles(int64_t n) { return ((uint64_t)n + BCF_TILE - 1) / BCF_TILE; }
BCF_HD uint64_t bcf_work_bytes(int64_t n) {
    const uint64_t t = bcf_tiles(n);
    return (16u + 4u * BCF_TILE) * (t ? t : 1u);
}
BCF_HD uint32_t* bcf_work_len(void* work, int64_t n) {
    const uint64_t t = bcf_tiles(n);
    return (uint32_t*)((int64_t*)work + 2u * (t ? t : 1u));
}
BCF_HD int64_t* bcf_work_off(void* work) { return (int64_t*)work; }
BCF_HD int64_t* bcf_work_decl(void* work, int64_t n) {
    const uint64_t t = bcf_tiles(n);
    return (int64_t*)work + (t ? t : 1u);
}

// ---- numbers ---------------------------------------------------------------------------------
// Digits come from 32-bit chunks of nine: no 64-bit division inside a loop.
BCF_HD uint32_t bcf_nd9(uint32_t w) {  // decimal digits of a value below 10^9
    return 1u + (w >= 10u) + (w >= 100u) + (w >= 1000u) + (w >= 10000u) + (w >= 100000u) + (w >= 1000000u) +
           (w >= 10000000u) + (w >= 100000000u);
}

struct bcf_dec {
    uint32_t c0, c1, c2;  // value = c2 * 10^18 + c1 * 10^9 + c0
    uint32_t nd;          // its decimal digits
};

BCF_HD uint32_t bcf_dec_digits(uint32_t c0, uint32_t c1, uint32_t c2) {
    return c2 ? 18u + bcf_nd9(c2) : c1 ? 9u + bcf_nd9(c1) : bcf_nd9(c0);
}

BCF_HD bcf_dec bcf_dec_u64(uint64_t v) {
    bcf_dec d;
    d.c1 = d.c2 = 0;
    if (v < 1000000000ull) {
        d.c0 = (uint32_t)v;
    } else {
        uint64_t hi = v / 1000000000ull;
        d.c0 = (uint32_t)(v - hi * 1000000000ull);
        if (hi >= 1000000000ull) {
            d.c2 = (uint32_t)(hi / 1000000000ull);
            hi -= (uint64_t)d.c2 * 1000000000ull;
        }
        d.c1 = (uint32_t)hi;
    }
    d.nd = bcf_dec_digits(d.c0, d.c1, d.c2);
    return d;
}

// str(round(x, dp)) for 0 <= dp <= 4 as sign, integer part and fraction digits.  bcio's put_round
// takes rintl of the x87 product x * 10^dp, which is exact (53 + 10 bits); here the double product p
// and its exact residual e = fma(x, P, -p) give the same integer: rint(p), unless p lies on a tie that
// the exact product does not (|p - rint(p)| == 0.5 and e != 0), where e's sign decides.  The integer
// n < 10^15 is then split in double arithmetic: floor(n / P) is exact, since a quotient that is not
// an integer lies at least 1 / P from one and half an ulp of it is less, and so is the remainder
// by fma; the same holds for the split of the integer part at 10^9.
struct bcf_num {
    bcf_dec ip;    // integer part
    uint32_t fr;   // fraction, nd digits (trailing zeros stripped; "0" when the fraction is zero)
    uint32_t nd;
    uint32_t neg;  // the sign of x: -0.0 and -0.0001 at dp 3 print -0.0
    uint32_t ok;   // 0: declined (not finite, or 1e15 reached after scaling); prints as 0.0
};

BCF_HD bcf_num bcf_round(double x, int dp) {
    bcf_num r;
    r.ip.c0 = r.ip.c1 = r.ip.c2 = 0;
    r.ip.nd = 1;
    r.fr = 0;
    r.nd = 1;
    r.neg = 0;
    r.ok = 0;
    const double P = dp == 0 ? 1.0 : dp == 1 ? 10.0 : dp == 2 ? 100.0 : dp == 3 ? 1000.0 : 10000.0;
    const double p = x * P;
    double n = rint(p);
    const double e = fma(x, P, -p);
    if (e != 0.0 && fabs(p - n) == 0.5) {
        const double f = floor(p);
        n = e > 0.0 ? f + 1.0 : f;
    }
    const double an = fabs(n);
    if (!(an < 1e15)) return r;  // NaN, infinities and everything too large
    const double ipd = floor(an / P);
    uint32_t fr = (uint32_t)fma(-ipd, P, an), nd = (uint32_t)dp;
    if (ipd < 1e9) {
        r.ip.c0 = (uint32_t)ipd;
    } else {
        const double h = floor(ipd / 1e9);
        r.ip.c1 = (uint32_t)h;
        r.ip.c0 = (uint32_t)fma(-h, 1e9, ipd);
    }
    r.ip.nd = bcf_dec_digits(r.ip.c0, r.ip.c1, 0);
    if (fr == 0) {
        nd = 1;
    } else {
        while (fr % 10u == 0) {
            fr /= 10u;
            --nd;
        }
    }
    r.fr = fr;
    r.nd = nd;
    r.neg = __builtin_signbit(x) ? 1u : 0u;
    r.ok = 1;
    return r;
}

// ---- sinks: the one row function below runs over a counter (measure) or a writer (write) --------
struct bcf_counter {
    uint32_t n;
    BCF_HD void ch(uint8_t) { ++n; }
    BCF_HD void bytes(const uint8_t*, uint32_t len) { n += len; }
    BCF_HD void digits(uint32_t, uint32_t nd) { n += nd; }
    BCF_HD void dec(const bcf_dec& d) { n += d.nd; }
};

// writes the bytes of the tile's text that fall into the window [base, base + cap) at buf
struct bcf_writer {
    uint8_t* buf;
    uint32_t base, cap;
    uint32_t at;  // offset in the tile's text of the next byte
    BCF_HD void st(uint32_t o, uint8_t c) {
        const uint32_t r = o - base;
        if (r < cap) buf[r] = c;
    }
    BCF_HD void ch(uint8_t c) { st(at++, c); }
    BCF_HD void bytes(const uint8_t* p, uint32_t len) {
        for (uint32_t i = 0; i < len; ++i) st(at + i, p[i]);
        at += len;
    }
    BCF_HD void digits(uint32_t v, uint32_t nd) {  // v zero-padded to nd digits
#pragma unroll 1
        for (uint32_t i = nd; i > 0;) {
            st(at + --i, (uint8_t)('0' + v % 10u));
            v /= 10u;
        }
        at += nd;
    }
    BCF_HD void dec(const bcf_dec& d) {
        uint32_t c = d.c0, next = d.c1, left = 9;  // from the last digit back, chunk after chunk
#pragma unroll 1
        for (uint32_t i = d.nd; i > 0;) {
            st(at + --i, (uint8_t)('0' + c % 10u));
            c /= 10u;
            if (--left == 0) {
                c = next;
                next = d.c2;
                left = 9;
            }
        }
        at += d.nd;
    }
};

template <class S>
BCF_HD void bcf_put_i64(S& s, int64_t v) {
    if (v < 0) s.ch('-');
    s.dec(bcf_dec_u64(v < 0 ? 0u - (uint64_t)v : (uint64_t)v));
}

template <class S>
BCF_HD void bcf_put_num(S& s, const bcf_num& r) {
    if (r.neg) s.ch('-');
    s.dec(r.ip);
    s.ch('.');
    s.digits(r.fr, r.nd);
}

// ---- segments and tiles -----------------------------------------------------------------------
// the last segment that begins at or before array position t0, -1 without one (the table is sorted
// by beg; an empty segment shares its beg with the one after it)
BCF_HD int64_t bcf_find_seg(const bcf_seg* segs, int64_t n_seg, int64_t t0) {
    int64_t lo = 0, hi = n_seg;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (segs[mid].beg <= t0)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo - 1;
}

struct bcf_tile {
    uint32_t cnt;       // positions of the tile that print: lanes 0 .. cnt - 1
    uint32_t name_len;  // 0 when the name is declined
    uint32_t name_bad;
    const uint8_t* name;
    uint64_t pos1;  // the printed position of lane 0
};

BCF_HD bcf_tile bcf_tile_of(const bcf_args& a, uint64_t tile) {
    bcf_tile t;
    t.cnt = t.name_len = t.name_bad = 0;
    t.name = a.names;
    t.pos1 = 0;
    const int64_t t0 = (int64_t)(tile * BCF_TILE);
    if (t0 >= a.n) return t;
    const int64_t i = bcf_find_seg(a.segs, a.n_seg, t0);
    if (i < 0) return t;
    const bcf_seg sg = a.segs[i];
    const uint64_t d = (uint64_t)t0 - (uint64_t)sg.beg;
    if (sg.len <= 0 || d >= (uint64_t)sg.len) return t;  // a gap between segments
    uint64_t cnt = (uint64_t)sg.len - d;
    if (cnt > (uint64_t)(a.n - t0)) cnt = (uint64_t)(a.n - t0);
    t.cnt = cnt > BCF_TILE ? BCF_TILE : (uint32_t)cnt;
    t.pos1 = (uint64_t)sg.pos0 + d + 1u;
    if (sg.name_off < 0 || sg.name_len < 0 || sg.name_len > BCF_MAX_NAME ||
        (int64_t)sg.name_off + sg.name_len > a.names_bytes) {
        t.name_bad = 1;
    } else {
        t.name = a.names + sg.name_off;
        t.name_len = (uint32_t)sg.name_len;
    }
    return t;
}

// ---- the rows of one position -----------------------------------------------------------------
// The text of array position p (lane `ln` of tile `t`) into the sink; false when a printed value is
// declined (the text is then well-formed but not to be used).
template <class S>
BCF_HD bool bcf_emit_pos(S& s, const bcf_args& a, const bcf_tile& t, int64_t p, uint32_t ln) {
    const int k = a.k, dp = a.dp;
    const int32_t* c = a.counts + p;
    const double* pc = a.pc + p;
    int64_t cov = 0;
    int nz = 0;
    for (int j = 0; j < k; ++j) {
        const int32_t v = c[(int64_t)j * a.stride];
        cov += v;
        nz += v != 0;
    }
    const bool has = cov != 0, has_sec = has && nz > 1;
    bcf_num en = {{0, 0, 0, 1}, 0, 1, 0, 1}, sn = en;
    if (has) en = bcf_round(a.ent[p], dp);
    if (has_sec) sn = bcf_round(a.sec[p], dp);
    bool ok = en.ok && sn.ok;
    const int64_t pos = (int64_t)(t.pos1 + ln);
    const int rows = a.long_format ? k : 1;
#pragma unroll 1
    for (int row = 0; row < rows; ++row) {
        s.bytes(t.name, t.name_len);
        s.ch('\t');
        bcf_put_i64(s, pos);
        s.ch('\t');
        bcf_put_i64(s, cov);
        const int j0 = a.long_format ? row : 0, j1 = a.long_format ? row + 1 : k;
        if (a.long_format) {
            s.ch('\t');
            if (row == 4) {
                s.ch('D');
                s.ch('S');
            } else {
                s.ch(row == 0 ? 'A' : row == 1 ? 'C' : row == 2 ? 'G' : row == 3 ? 'T' : 'N');
            }
        }
#pragma unroll 1
        for (int j = j0; j < j1; ++j) {
            s.ch('\t');
            bcf_put_i64(s, (int64_t)c[(int64_t)j * a.stride]);
        }
#pragma unroll 1
        for (int j = j0; j < j1; ++j) {
            s.ch('\t');
            if (has) {
                const bcf_num r = bcf_round(pc[(int64_t)j * a.stride], dp);
                ok = ok && r.ok;
                bcf_put_num(s, r);
            } else {
                s.ch('-');
                s.ch('1');
            }
        }
        s.ch('\t');
        if (has)
            bcf_put_num(s, en);
        else
            s.ch('1');
        s.ch('\t');
        if (has_sec)
            bcf_put_num(s, sn);
        else
            s.ch('1');
        s.ch('\n');
    }
    return ok;
}

// ---- the scan's serial pieces (the kernel runs them per thread, the twin once) ------------------
BCF_HD int32_t bcf_status(int64_t declined, int64_t total, int64_t text_cap) {
    if (declined != INT64_MAX) return BCF_ST_VALUE;
    return total > text_cap ? BCF_ST_TOO_SMALL : BCF_ST_OK;
}

// seg_off[i] once the tile byte counts are offsets: the offset of the tile segment i begins at
BCF_HD int64_t bcf_seg_off(const bcf_args& a, const int64_t* off, int64_t total, int64_t i) {
    if (i >= a.n_seg) return total;
    const uint64_t tile = (uint64_t)a.segs[i].beg / BCF_TILE;  // (a negative beg lands past the end)
    return tile >= bcf_tiles(a.n) ? total : off[tile];
}

BCF_HD void bcf_store_header(bcf_header* h, int64_t declined, int64_t total, int64_t text_cap) {
    bcf_header v;
    v.status = bcf_status(declined, total, text_cap);
    v.reserved0 = 0;
    v.total_bytes = total;
    v.declined_pos = declined == INT64_MAX ? -1 : declined;
    for (int i = 0; i < 5; ++i) v.reserved[i] = 0;
    *h = v;
}

// the copy of a staged window: `head` bytes up to the first 16-byte boundary of the destination,
// `body` 16-byte pieces, `tail` bytes
struct bcf_copy {
    uint32_t head, body, tail;
};
BCF_HD bcf_copy bcf_copy_plan(uint32_t skew, uint32_t wlen) {
    bcf_copy c;
    c.head = (16u - skew) & 15u;
    if (c.head > wlen) c.head = wlen;
    c.body = (wlen - c.head) / 16u;
    c.tail = wlen - c.head - 16u * c.body;
    return c;
}

// ---- the host twin: the three launches as loops -------------------------------------------------
#if !defined(__HIPCC__)
inline void bcf_rows_host(const bcf_args& a, void* work, bcf_header* hdr, int64_t* seg_off, uint8_t* text,
                          int64_t text_cap) {
    const uint64_t nt = bcf_tiles(a.n);
    int64_t* off = bcf_work_off(work);
    int64_t* decl = bcf_work_decl(work, a.n);
    uint32_t* lens = bcf_work_len(work, a.n);
    // measure
    for (uint64_t tile = 0; tile < nt; ++tile) {
        const bcf_tile t = bcf_tile_of(a, tile);
        int64_t sum = 0, bad = t.name_bad && t.cnt ? (int64_t)(tile * BCF_TILE) : INT64_MAX;
        for (uint32_t ln = 0; ln < BCF_TILE; ++ln) {
            bcf_counter s;
            s.n = 0;
            const int64_t p = (int64_t)(tile * BCF_TILE + ln);
            if (ln < t.cnt && !bcf_emit_pos(s, a, t, p, ln) && bad == INT64_MAX) bad = p;
            lens[p] = s.n;
            sum += s.n;
        }
        off[tile] = sum;
        decl[tile] = bad;
    }
    // scan
    int64_t total = 0, declined = INT64_MAX;
    for (uint64_t tile = 0; tile < nt; ++tile) {
        const int64_t b = off[tile];
        off[tile] = total;
        total += b;
        if (decl[tile] < declined) declined = decl[tile];
    }
    for (int64_t i = 0; i <= a.n_seg; ++i) seg_off[i] = bcf_seg_off(a, off, total, i);
    bcf_store_header(hdr, declined, total, text_cap);
    if (hdr->status != BCF_ST_OK) return;
    // write
    uint8_t stage[BCF_STAGE];
    for (uint64_t tile = 0; tile < nt; ++tile) {
        const bcf_tile t = bcf_tile_of(a, tile);
        if (!t.cnt) continue;
        uint32_t lane_off[BCF_TILE + 1];
        lane_off[0] = 0;
        for (uint32_t ln = 0; ln < t.cnt; ++ln) lane_off[ln + 1] = lane_off[ln] + lens[tile * BCF_TILE + ln];
        uint64_t tot = lane_off[t.cnt];
        const uint64_t g0 = (uint64_t)off[tile];
        if (tot > (uint64_t)total - g0) tot = (uint64_t)total - g0;
        const uint32_t skew = (uint32_t)((uintptr_t)(text + g0) & 15u);
        for (uint32_t wb = 0; wb < tot; wb += BCF_WIN) {
            const uint32_t wlen = tot - wb < BCF_WIN ? (uint32_t)(tot - wb) : BCF_WIN;
            for (uint32_t ln = 0; ln < t.cnt; ++ln) {
                if (lane_off[ln] >= wb + wlen || lane_off[ln + 1] <= wb) continue;
                bcf_writer w;
                w.buf = stage + skew;
                w.base = wb;
                w.cap = wlen;
                w.at = lane_off[ln];
                bcf_emit_pos(w, a, t, (int64_t)(tile * BCF_TILE + ln), ln);
            }
            const bcf_copy c = bcf_copy_plan(skew, wlen);
            uint8_t* dst = text + g0 + wb;
            const uint8_t* src = stage + skew;
            for (uint32_t i = 0; i < c.head; ++i) dst[i] = src[i];
            for (uint32_t i = 0; i < c.body; ++i) memcpy(dst + c.head + 16u * i, src + c.head + 16u * i, 16);
            for (uint32_t i = 0; i < c.tail; ++i) dst[c.head + 16u * c.body + i] = src[c.head + 16u * c.body + i];
        }
    }
}
#endif
