// bc_inflate.h — raw DEFLATE (RFC 1951) for one BGZF block, on the device and on the host.
//
// Contract: input comp[0, clen), output exactly isize bytes (isize <= 65536), a status back.
// Validity follows zlib's inflate(): whatever it rejects is rejected here, and a stream it accepts
// inflates to the same bytes.  Bytes after the final block's end-of-block inside clen are ignored.
//
// Everything that decides an address or a validity question is in this header: the bit reader and
// its input limit, the stored-block LEN/NLEN check, the code-length alphabet with its repeat codes
// (16/17/18 run across the litlen/dist boundary), canonical code construction, the length and
// distance base/extra tables and the match checks.  The decoder is a template over a "machine" M
// that supplies storage and the data movement only:
//     host   (BczHost below):     one lane, plain loops, bounds-exact byte reads
//     device (bc_inflate.hip):    one wave, tables and copies done by all 64 lanes, input staged
//                                 into LDS by whole 16-byte pieces
// The control flow is the same on both and is wave-uniform on the device: every lane of the wave
// executes it with the same values.
//
// Hard guarantee, whatever the input: M::fetch32 is only asked for words of the padded span
// [0, (head + clen + 3) / 4 + 2) and returns zero bits (host) or unspecified but in-allocation bits
// (device: whole aligned 16-byte pieces that hold at least one byte of the span) outside
// comp[0, clen); a decision taken on such bits is discarded by the input-limit check that follows
// it before anything is written.  No write goes outside out[0, isize): every literal, match and
// stored copy is checked against isize first.  On a non-zero status the block's own output bytes
// are unspecified.
//
// M provides:
//   int lane(), nlanes()                 this lane and the number of lanes (1 on the host)
//   uint64_t ballot(bool), lt_mask()     lanes whose predicate holds; the lanes below this one
//   void sync()                          make the lanes' table writes visible to each other
//   uint32_t fetch32(uint32_t w)         input word w (little endian) of the padded span
//   void seek(uint32_t w)                the next fetch32 is of word w (forward only)
//   T uni(T)                             a value every lane holds alike (the device moves it to a scalar)
//   uint8_t* lens()                      [BCZ_MAXLENS] code lengths: litlen at 0, distance at 288
//   uint8_t* lens_stage()                [BCZ_MAXLENS] a dynamic header's lengths as one sequence
//   uint16_t* lit_table(), dist_table()  [1 << BCZ_LIT_ROOT], [1 << BCZ_DIST_ROOT]
//   uint16_t* lit_sorted(), dist_sorted()[288], [32] symbols in canonical order
//   uint16_t* lit_count(), dist_count()  [16] codes per length
//   void literal(uint32_t at, uint8_t b) output byte `at` is b (may be buffered)
//   void match(uint32_t at, uint32_t len, uint32_t dist)   copy, sources by bcz_match_src
//   void stored(uint32_t at, uint32_t src_byte, uint32_t len)  comp[src_byte ..) -> out[at ..)
//   void flush()                         buffered literals out
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BCZ_HD __host__ __device__ __forceinline__
#else
#define BCZ_HD inline
#endif

// status codes (bc_bgzf_inflate's d_status bytes)
#define BC_Z_OK 0
#define BC_Z_DESC 1        /* descriptor outside its buffers, isize > 65536 or clen > 16 MiB   */
#define BC_Z_BTYPE 2       /* block type 3                                                     */
#define BC_Z_STORED 3      /* stored block: LEN != ~NLEN                                       */
#define BC_Z_HEADER 4      /* dynamic header: more than 286 litlen or 30 distance symbols      */
#define BC_Z_CODELEN 5     /* bad code-length code set, repeat without a previous length or past the end */
#define BC_Z_OVERSUB 6     /* over-subscribed litlen or distance code set                      */
#define BC_Z_INCOMPLETE 7  /* incomplete code set that is not a single code of length 1        */
#define BC_Z_NO_EOB 8      /* litlen code without symbol 256                                   */
#define BC_Z_SYMBOL 9      /* bits that are no code; litlen symbol 286/287; distance code 30/31 */
#define BC_Z_DIST 10       /* distance reaching before the block's first output byte           */
#define BC_Z_INPUT 11      /* input exhausted before the final block's end-of-block            */
#define BC_Z_LONG 12       /* output would pass isize                                          */
#define BC_Z_SHORT 13      /* stream ended with fewer than isize bytes                         */

#define BCZ_MAX_ISIZE 65536u
#define BCZ_MAX_CLEN (1u << 24) /* bit positions stay 32-bit; a BGZF block's data is below 64 KiB  */
#define BCZ_MAXLENS 320     /* 288 litlen + 32 distance code lengths                            */
#define BCZ_LIT_ROOT 10     /* primary table bits: a longer code takes the canonical walk       */
#define BCZ_DIST_ROOT 8

// descriptor check (the descriptors are device data: the kernel checks each block itself)
BCZ_HD int bcz_desc_ok(uint64_t coff, uint32_t clen, uint32_t isize, uint64_t uoff, uint64_t comp_bytes,
                       uint64_t out_bytes) {
    return isize <= BCZ_MAX_ISIZE && clen <= BCZ_MAX_CLEN && coff <= comp_bytes && clen <= comp_bytes - coff && uoff <= out_bytes &&
           isize <= out_bytes - uoff;
}

// RFC 1951 3.2.5: length symbols 257..285, distance symbols 0..29 (base, extra bits)
BCZ_HD uint32_t bcz_len_base(uint32_t i) {  // i = symbol - 257, 0..28
    return i < 8 ? 3 + i : i == 28 ? 258 : 3 + ((4 + (i & 3)) << ((i >> 2) - 1));
}
BCZ_HD uint32_t bcz_len_extra(uint32_t i) { return i < 8 || i == 28 ? 0 : (i >> 2) - 1; }
BCZ_HD uint32_t bcz_dist_base(uint32_t i) {  // i = 0..29
    return i < 4 ? 1 + i : 1 + ((2 + (i & 1)) << ((i >> 1) - 1));
}
BCZ_HD uint32_t bcz_dist_extra(uint32_t i) { return i < 4 ? 0 : (i >> 1) - 1; }
// order of the code-length code's lengths in the dynamic header
BCZ_HD uint32_t bcz_clen_order(uint32_t i) {
    // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                        6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31);
}

// source of a match's byte i (0 <= i < len) written at p with distance dist (1 <= dist <= p): the
// periodic index, so that every source lies below p even when the match overlaps itself
BCZ_HD uint32_t bcz_match_src(uint32_t p, uint32_t dist, uint32_t len, uint32_t i) {
    return p - dist + (dist >= len ? i : i % dist);
}

BCZ_HD uint32_t bcz_popc(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(x);
#else
    return (uint32_t)__builtin_popcountll(x);
#endif
}
BCZ_HD uint32_t bcz_rev(uint32_t code, uint32_t len) {  // the low `len` bits of code, reversed
    uint32_t r = 0;
    for (uint32_t i = 0; i < 15; ++i)
        if (i < len) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// ---- the bit reader -------------------------------------------------------------------------
// Bits come LSB first from 32-bit little-endian words of the padded span; `pos` counts the bits
// consumed from the span's start (the `head` alignment bytes in front of comp[0] included), and
// `end` = 8 * (head + clen) is the input limit: over() after a step means it used bits that are
// not the block's.
struct BczBits {
    uint64_t buf;
    uint32_t cnt, w, pos, end;
};
template <class M>
BCZ_HD void bcz_seek(M& m, BczBits& b, uint32_t bitpos) {
    b.w = bitpos >> 5;
    m.seek(b.w);
    b.buf = (uint64_t)m.fetch32(b.w++) >> (bitpos & 31);
    b.cnt = 32 - (bitpos & 31);
    b.pos = bitpos;
}
// at least 33 bits buffered afterwards: enough for a code (15) with its extra bits (13)
template <class M>
BCZ_HD void bcz_need(M& m, BczBits& b) {
    if (b.cnt <= 32) {
        b.buf |= (uint64_t)m.fetch32(b.w++) << b.cnt;
        b.cnt += 32;
    }
}
BCZ_HD uint32_t bcz_peek(const BczBits& b, uint32_t n) { return (uint32_t)b.buf & ((1u << n) - 1u); }
BCZ_HD void bcz_drop(BczBits& b, uint32_t n) {
    b.buf >>= n;
    b.cnt -= n;
    b.pos += n;
}
BCZ_HD uint32_t bcz_take(BczBits& b, uint32_t n) {
    const uint32_t v = bcz_peek(b, n);
    bcz_drop(b, n);
    return v;
}
BCZ_HD bool bcz_over(const BczBits& b) { return b.pos > b.end; }

// ---- canonical code construction ----------------------------------------------------------------
// lens[0, n) -> count[16] (codes per length), sorted[] (symbols in canonical order) and the primary
// table of `root` bits: entry = symbol << 4 | length for a code of at most root bits at every index
// whose low bits are the code (bit-reversed, as the stream delivers it), 0 elsewhere (longer code,
// or no code).  Lanes take symbols lane, lane + nlanes, ...; ranks among equal lengths come from
// ballots.  allow: 0 = the code-length code (an incomplete set is always an error), 1 = litlen or
// distance code (zlib: an incomplete set is accepted when its longest code has length 1, and so is
// a set without codes).
template <class M>
BCZ_HD int bcz_build(M& m, const uint8_t* lens, uint32_t n, uint32_t root, uint16_t* table, uint16_t* sorted,
                     uint16_t* count, int allow) {
    const uint32_t lane = (uint32_t)m.lane(), nl = (uint32_t)m.nlanes();
    const uint64_t below = m.lt_mask();
    uint32_t cnt[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (uint32_t base = 0; base < n; base += nl) {
        const uint32_t s = base + lane;
        const uint32_t my = s < n ? lens[s] : 0;
#pragma unroll
        for (uint32_t l = 1; l < 16; ++l) cnt[l] += bcz_popc(m.ballot(my == l));
    }
    int32_t left = 1;
    uint32_t maxlen = 0;
#pragma unroll
    for (uint32_t l = 1; l < 16; ++l) {
        left = left * 2 - (int32_t)cnt[l];
        if (left < 0) return BC_Z_OVERSUB;
        if (cnt[l]) maxlen = l;
    }
    if (left > 0 && maxlen != 0 && (!allow || maxlen != 1)) return BC_Z_INCOMPLETE;
    // first code and first sorted slot of each length
    uint32_t first[16], offs[16];
    {
        uint32_t code = 0, o = 0;
#pragma unroll
        for (uint32_t l = 1; l < 16; ++l) {
            code = (code + cnt[l - 1]) << 1;  // cnt[0] is 0
            first[l] = code;
            offs[l] = o;
            o += cnt[l];
        }
    }
    for (uint32_t i = lane; i < (1u << root); i += nl) table[i] = 0;
    if (lane == 0) count[0] = 0;
#pragma unroll
    for (uint32_t l = 1; l < 16; ++l)
        if (nl == 1 || lane == l) count[l] = (uint16_t)cnt[l];
    m.sync();
    uint32_t run[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) run[l] = 0;
    for (uint32_t base = 0; base < n; base += nl) {
        const uint32_t s = base + lane;
        const uint32_t my = s < n ? lens[s] : 0;
        uint32_t rank = 0, f = 0, o = 0;
#pragma unroll
        for (uint32_t l = 1; l < 16; ++l) {
            const uint64_t mask = m.ballot(my == l);
            if (my == l) {
                rank = run[l] + bcz_popc(mask & below);
                f = first[l];
                o = offs[l];
            }
            run[l] += bcz_popc(mask);
        }
        if (my != 0) {
            sorted[o + rank] = (uint16_t)s;
            if (my <= root) {
                const uint16_t e = (uint16_t)(s << 4 | my);
                for (uint32_t i = bcz_rev(f + rank, my); i < (1u << root); i += 1u << my) table[i] = e;
            }
        }
    }
    m.sync();
    return BC_Z_OK;
}

// one symbol: the primary table, else the canonical walk over count[] / sorted[] (codes longer than
// root bits, and bits that are no code at all).  -1: no code.  Consumes the code's bits.
template <class M>
BCZ_HD int32_t bcz_symbol(M& m, BczBits& b, const uint16_t* table, uint32_t root, const uint16_t* sorted,
                          const uint16_t* count) {
    const uint32_t e = m.uni((uint32_t)table[bcz_peek(b, root)]);
    if (e != 0) {
        bcz_drop(b, e & 15u);
        return (int32_t)(e >> 4);
    }
    uint32_t bits = (uint32_t)b.buf, code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        code |= bits & 1u;
        bits >>= 1;
        const uint32_t c = m.uni((uint32_t)count[l]);
        if (code < first + c) {
            bcz_drop(b, l);
            return (int32_t)m.uni((uint32_t)sorted[index + (code - first)]);
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

// ---- the decoder --------------------------------------------------------------------------------
// head: bytes between the padded span's start and comp[0] (the device aligns its loads; 0 on the
// host).  Returns BC_Z_*.
template <class M>
BCZ_HD int bcz_inflate(M& m, uint32_t head, uint32_t clen, uint32_t isize) {
    BczBits b;
    b.end = 8u * (head + clen);
    bcz_seek(m, b, 8u * head);
    uint8_t* lens = m.lens();
    uint32_t at = 0;  // output bytes produced
    const uint32_t lane = (uint32_t)m.lane(), nl = (uint32_t)m.nlanes();
    for (;;) {
        bcz_need(m, b);
        const uint32_t last = bcz_take(b, 1), type = bcz_take(b, 2);
        if (bcz_over(b)) return BC_Z_INPUT;
        if (type == 3) return BC_Z_BTYPE;
        if (type == 0) {
            bcz_drop(b, (8u - (b.pos & 7u)) & 7u);
            bcz_need(m, b);
            const uint32_t len = bcz_take(b, 16);
            bcz_need(m, b);
            const uint32_t nlen = bcz_take(b, 16);
            if (bcz_over(b)) return BC_Z_INPUT;
            if ((len ^ 0xFFFFu) != nlen) return BC_Z_STORED;
            if (len > (b.end - b.pos) / 8u) return BC_Z_INPUT;
            if (len > isize - at) return BC_Z_LONG;
            m.flush();
            m.stored(at, b.pos / 8u - head, len);
            at += len;
            bcz_seek(m, b, b.pos + 8u * len);
        } else {
            uint32_t nlit, ndist;
            if (type == 1) {
                nlit = 288;
                ndist = 32;
                for (uint32_t s = lane; s < 320; s += nl) lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
                m.sync();
            } else {
                nlit = bcz_take(b, 5) + 257;
                ndist = bcz_take(b, 5) + 1;
                const uint32_t ncode = bcz_take(b, 4) + 4;
                if (bcz_over(b)) return BC_Z_INPUT;
                if (nlit > 286 || ndist > 30) return BC_Z_HEADER;
                // the code-length code's 19 lengths borrow the distance lengths' slots
                uint8_t* cl = lens + 288;
                for (uint32_t i = lane; i < 19; i += nl) cl[i] = 0;
                m.sync();
                for (uint32_t i = 0; i < ncode; ++i) {
                    bcz_need(m, b);
                    const uint32_t v = bcz_take(b, 3);
                    if (nl == 1 || lane == 0) cl[bcz_clen_order(i)] = (uint8_t)v;
                }
                if (bcz_over(b)) return BC_Z_INPUT;
                m.sync();
                // its 7-bit table goes into the distance table's storage, its sorted symbols and
                // counts into the distance code's: all three are rebuilt after the lengths are read
                int rc = bcz_build(m, cl, 19, 7, m.dist_table(), m.dist_sorted(), m.dist_count(), 0);
                if (rc != BC_Z_OK) return BC_Z_CODELEN;
                // the lengths, litlen then distance as ONE sequence (repeats cross the boundary),
                // into the staging array; the two parts move to their places in lens[] after
                uint32_t have = 0, prev = 0;
                const uint32_t total = nlit + ndist;
                while (have < total) {
                    bcz_need(m, b);
                    const int32_t sym = bcz_symbol(m, b, m.dist_table(), 7, m.dist_sorted(), m.dist_count());
                    if (sym < 0) return bcz_over(b) ? BC_Z_INPUT : BC_Z_CODELEN;
                    uint32_t rep, val;
                    if (sym < 16) {
                        rep = 1;
                        val = prev = (uint32_t)sym;
                    } else if (sym == 16) {
                        if (have == 0) return bcz_over(b) ? BC_Z_INPUT : BC_Z_CODELEN;
                        rep = 3 + bcz_take(b, 2);
                        val = prev;
                    } else if (sym == 17) {
                        rep = 3 + bcz_take(b, 3);
                        val = prev = 0;
                    } else {
                        rep = 11 + bcz_take(b, 7);
                        val = prev = 0;
                    }
                    if (bcz_over(b)) return BC_Z_INPUT;
                    if (rep > total - have) return BC_Z_CODELEN;
                    for (uint32_t i = lane; i < rep; i += nl) m.lens_stage()[have + i] = (uint8_t)val;
                    have += rep;
                }
                m.sync();
                // staging -> lens: litlen [0, nlit), zero to 288, distance [288, 288 + ndist), zero to 320
                {
                    const uint8_t* st = m.lens_stage();
                    for (uint32_t s = lane; s < 320; s += nl)
                        lens[s] = s < nlit ? st[s] : s < 288 ? 0 : s - 288 < ndist ? st[nlit + (s - 288)] : 0;
                }
                m.sync();
                if (m.uni((uint32_t)lens[256]) == 0) return BC_Z_NO_EOB;
            }
            int rc = bcz_build(m, lens, type == 1 ? 288 : nlit, BCZ_LIT_ROOT, m.lit_table(), m.lit_sorted(), m.lit_count(), 1);
            if (rc != BC_Z_OK) return rc;
            rc = bcz_build(m, lens + 288, ndist, BCZ_DIST_ROOT, m.dist_table(), m.dist_sorted(), m.dist_count(), 1);
            if (rc != BC_Z_OK) return rc;
            const uint16_t *lt = m.lit_table(), *ls = m.lit_sorted(), *lc = m.lit_count();
            const uint16_t *dt = m.dist_table(), *ds = m.dist_sorted(), *dc = m.dist_count();
            // the symbol loop leaves through ONE exit (st says why): several exits would each cost
            // the compiled loop a state test per symbol
            int st = BC_Z_OK;
            for (;;) {
                bcz_need(m, b);
                const int32_t sym = bcz_symbol(m, b, lt, BCZ_LIT_ROOT, ls, lc);
                const bool over = bcz_over(b);
                if (sym >= 0 && sym < 256 && !over && at < isize) {
                    m.literal(at, (uint8_t)sym);
                    ++at;
                    continue;
                }
                if (sym < 0) {
                    st = over ? BC_Z_INPUT : BC_Z_SYMBOL;
                    break;
                }
                if (sym < 256) {
                    st = over ? BC_Z_INPUT : BC_Z_LONG;
                    break;
                }
                if (sym == 256) {
                    st = over ? BC_Z_INPUT : BC_Z_OK;
                    break;
                }
                if (sym > 285) {
                    st = over ? BC_Z_INPUT : BC_Z_SYMBOL;
                    break;
                }
                const uint32_t li = (uint32_t)sym - 257u;
                const uint32_t len = bcz_len_base(li) + bcz_take(b, bcz_len_extra(li));
                bcz_need(m, b);
                const int32_t dsym = bcz_symbol(m, b, dt, BCZ_DIST_ROOT, ds, dc);
                if (dsym < 0 || dsym > 29) {
                    st = bcz_over(b) ? BC_Z_INPUT : BC_Z_SYMBOL;
                    break;
                }
                const uint32_t dist = bcz_dist_base((uint32_t)dsym) + bcz_take(b, bcz_dist_extra((uint32_t)dsym));
                if (bcz_over(b)) {
                    st = BC_Z_INPUT;
                    break;
                }
                if (dist > at) {
                    st = BC_Z_DIST;
                    break;
                }
                if (len > isize - at) {
                    st = BC_Z_LONG;
                    break;
                }
                m.match(at, len, dist);
                at += len;
            }
            if (st != BC_Z_OK) return st;
        }
        if (last) break;
    }
    m.flush();
    return at == isize ? BC_Z_OK : BC_Z_SHORT;
}

// ---- the host machine -------------------------------------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
struct BczHost {
    const uint8_t* comp;
    uint32_t clen;
    uint8_t* out;
    uint8_t lens_[BCZ_MAXLENS], stage_[BCZ_MAXLENS];
    uint16_t lit_table_[1 << BCZ_LIT_ROOT], dist_table_[1 << BCZ_DIST_ROOT];
    uint16_t lit_sorted_[288], dist_sorted_[32], lit_count_[16], dist_count_[16];
    int lane() const { return 0; }
    int nlanes() const { return 1; }
    uint64_t ballot(bool p) const { return p ? 1u : 0u; }
    uint64_t lt_mask() const { return 0; }
    template <class T>
    T uni(T v) const { return v; }
    void sync() {}
    void seek(uint32_t) {}
    uint32_t fetch32(uint32_t w) const {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; ++k) {
            const uint64_t i = (uint64_t)w * 4 + k;
            if (i < clen) v |= (uint32_t)comp[i] << (8 * k);
        }
        return v;
    }
    uint8_t* lens() { return lens_; }
    uint8_t* lens_stage() { return stage_; }
    uint16_t* lit_table() { return lit_table_; }
    uint16_t* dist_table() { return dist_table_; }
    uint16_t* lit_sorted() { return lit_sorted_; }
    uint16_t* dist_sorted() { return dist_sorted_; }
    uint16_t* lit_count() { return lit_count_; }
    uint16_t* dist_count() { return dist_count_; }
    void literal(uint32_t at, uint8_t v) { out[at] = v; }
    void match(uint32_t at, uint32_t len, uint32_t dist) {
        for (uint32_t i = 0; i < len; ++i) out[at + i] = out[bcz_match_src(at, dist, len, i)];
    }
    void stored(uint32_t at, uint32_t src, uint32_t len) {
        for (uint32_t i = 0; i < len; ++i) out[at + i] = comp[src + i];
    }
    void flush() {}
};

// one block on the host: comp[0, clen) -> out[0, isize)
inline int bcz_inflate_host(const uint8_t* comp, uint32_t clen, uint8_t* out, uint32_t isize) {
    if (isize > BCZ_MAX_ISIZE || clen > BCZ_MAX_CLEN) return BC_Z_DESC;
    BczHost m;
    m.comp = comp;
    m.clen = clen;
    m.out = out;
    return bcz_inflate(m, 0, clen, isize);
}
#endif
