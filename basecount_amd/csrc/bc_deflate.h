// bc_deflate.h — one BGZF block written: raw DEFLATE (RFC 1951) with the fixed Huffman codes, the
// CRC-32 and the BGZF framing, on the device and on the host.
//
// Contract: a block is up to BCD_BLOCK = 65,280 input bytes (the cut bcio.cpp's BAM writer and
// htslib use) and becomes 18 header bytes, one DEFLATE block with BFINAL = 1, the CRC-32 and ISIZE:
// at most 65,311 bytes, in the block's own BCD_SLOT = 64 KiB slot.  The compressed bytes are a pure
// function of the input bytes: every rule below says who wins where lanes meet, nothing depends on
// the order in which lanes or atomics land.  The host machine (BcdHost) runs the same schedule lane
// by lane and writes the same bytes, bit for bit.
//
// THE SCHEDULE.  The block is walked in steps of 64 positions; lane l of step s stands on position
// p = 64 s + l.
//   hash      of the four bytes at p: (little-endian word * 2654435761) >> 20, twelve bits, for every
//             p with p + 4 <= len.  The table has 4,096 entries of 16 bits (a position of the block;
//             0xFFFF: empty).
//   lookups   a step's lookups all happen before its inserts, so a candidate comes from an earlier
//             step and lies at distance >= l + 1.  Positions a match of an earlier step covers are
//             not looked up (they start no token).
//   inserts   every hashed position of the step is inserted, covered or not.  Of two inserts that
//             collide the highest position remains.
//   match     one candidate per position.  It is rejected when it lies farther back than 32,768 (a
//             block is longer than the window).  Its length is the common prefix with the candidate,
//             at most 258 and at most len - p, read from the input itself, so a match may overlap its
//             own start; it is accepted from 4 bytes on.
//   parse     inside a step from the first uncovered position on, in position order: the next
//             position j that holds a match takes it, unless j + 1 lies in the step and holds a
//             longer one (then j is a literal and j + 1 is asked the same); positions before j are
//             literals; the parse goes on at j + length.
//   past the step   a match is never cut at the step's end: the positions it covers in later steps
//             start no token and are not looked up, only inserted.
//   bits      LSB first; Huffman codes bit-reversed, extra bits as they are; a token is at most 31
//             bits; the lanes' bit offsets are the prefix sums of their tokens' lengths and the tokens
//             are OR-ed into the zeroed staging area (OR commutes).  The final byte is zero-padded.
//   fallback  payload (3 header bits, tokens, end-of-block, padding) >= len + 5 bytes: the block is
//             written again as one stored block of len + 5 bytes.  The payload only grows, so the
//             test after every step finds it before the staging area or the slot could overflow.
//   CRC-32    each lane the raw CRC (register 0, no final inversion) of a chunk of ceil(len / 64)
//             bytes, the chunks aligned to the block's end (the first lanes' are short or empty);
//             six log-steps fold them: v[l] = v[l] * X^(2^r) + v[l + 2^r] with X = x^(8 chunk) mod P;
//             the initial and final inversions are added as 0xFFFFFFFF * x^(8 len) + 0xFFFFFFFF.
//
// Hard guarantee, whatever the input: nothing is read outside the input's [0, len) but the aligned
// 32-bit words that hold at least one byte of it (device), nothing is written outside the slot's
// first 65,536 bytes.
//
// M provides (NL lanes, PER = 64 / NL positions of a step per lane; a per-lane value is an array of
// PER, which is one register on the device):
//   uint32_t lane()
//   uint32_t load32(uint32_t p)            input bytes p .. p + 3, little endian; p < len; bytes at or
//                                          past len unspecified (every use is capped by len)
//   uint16_t* table(); uint32_t* stage(); uint32_t* crc_table()     [4096], [BCD_STAGE_WORDS], [256]
//   void sync()                            the lanes' table and staging writes are visible to each other
//   uint64_t mask(const bool (&)[PER])     the lanes whose value is true
//   uint32_t get(const uint32_t (&)[PER], uint32_t j)     lane j's value
//   void scan(const uint32_t (&v)[PER], uint32_t (&excl)[PER], uint32_t& total)
//   void down(const uint32_t (&v)[PER], uint32_t (&o)[PER], uint32_t d)   o[l] = v[l + d], 0 past lane 63
//   void insert(const uint32_t (&h)[PER], const uint32_t (&p)[PER], const bool (&on)[PER])
//                                          table[h] = p for the lanes that are on; the highest p remains
//   void stage_or(uint32_t w, uint32_t bits)
//   void flush(uint32_t dst, uint32_t n16) staging bytes [0, 16 n16) to the slot's bytes [dst, ...)
//   void slot_byte(uint32_t off, uint8_t v); void slot_fence()   direct slot writes, after the flushes
#pragma once
#include <stdint.h>

#include "bc_inflate.h"

#define BCD_HD BCZ_HD

#ifndef BC_DFL_OK
#define BC_DFL_OK 0
#define BC_DFL_TOO_SMALL 1 /* total_bytes > comp_cap: total and offsets exact, no compressed byte to be trusted */
#define BC_DFL_GATED 2     /* *d_gate != 0: nothing but the header was written                               */
#define BC_DFL_OFFSETS 3   /* span offsets decreasing, negative or past text_cap: nothing compressed         */
#endif

#define BCD_BLOCK 65280u
#define BCD_SLOT 65536u
#define BCD_HEAD 18u
#define BCD_TAIL 8u
#define BCD_HASH_BITS 12u
#define BCD_EMPTY 0xFFFFu
#define BCD_MIN_MATCH 4u
#define BCD_MAX_MATCH 258u
#define BCD_MAX_DIST 32768u
#define BCD_STEP 64u
#define BCD_FLUSH 1024u        /* bytes that leave the staging area at a time              */
#define BCD_STAGE_WORDS 288u   /* BCD_FLUSH + 128 bytes: a step adds at most 72 (64 x 9 bits) */
#define BCD_STORED_EXTRA 5u    /* a stored block's own bytes: type byte, LEN, NLEN          */
#define BCD_CRC_POLY 0xEDB88320u

// ---- the block cut --------------------------------------------------------------------------------
BCD_HD uint64_t bcd_nblocks(uint64_t span_bytes) { return (span_bytes + BCD_BLOCK - 1u) / BCD_BLOCK; }
BCD_HD uint64_t bcd_max_blocks(uint64_t text_cap, uint64_t n_spans) { return text_cap / BCD_BLOCK + n_spans; }
BCD_HD uint32_t bcd_block_len(uint64_t span_bytes, uint64_t k) {  // block k of a span
    const uint64_t rest = span_bytes - k * BCD_BLOCK;
    return (uint32_t)(rest < BCD_BLOCK ? rest : BCD_BLOCK);
}

// ---- framing ----------------------------------------------------------------------------------------
// 1f 8b 08 04 | mtime 0 | xfl 0 | os ff | xlen 6 | 'B' 'C' 2 0 | BSIZE = block size - 1
BCD_HD uint8_t bcd_header_byte(uint32_t i, uint32_t bsize) {
    const uint64_t lo = 0x00000000'04088B1Full, hi = 0x00024342'0006FF00ull;  // bytes 0-7, 8-15
    return (uint8_t)(i < 8 ? lo >> (8 * i) : i < 16 ? hi >> (8 * (i - 8)) : i == 16 ? bsize : bsize >> 8);
}
BCD_HD uint8_t bcd_eof_byte(uint32_t i) {  // the 28-byte EOF block: an empty fixed-code block
    return i < 18 ? bcd_header_byte(i, 27) : i == 18 ? 3 : 0;
}

// ---- tokens -----------------------------------------------------------------------------------------
BCD_HD uint32_t bcd_hash(uint32_t v) { return (v * 2654435761u) >> (32u - BCD_HASH_BITS); }
BCD_HD uint32_t bcd_ilog2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }
BCD_HD uint32_t bcd_ctz(uint32_t x) { return (uint32_t)__builtin_ctz(x); }
BCD_HD uint32_t bcd_ctz64(uint64_t x) { return (uint32_t)__builtin_ctzll(x); }

struct BcdTok {
    uint32_t bits, nb;
};
// fixed litlen code of symbol s (RFC 1951 3.2.6), bit-reversed
BCD_HD BcdTok bcd_litlen(uint32_t s) {
    BcdTok t;
    if (s < 144) {
        t.nb = 8;
        t.bits = bcz_rev(0x30u + s, 8);
    } else if (s < 256) {
        t.nb = 9;
        t.bits = bcz_rev(0x190u + (s - 144u), 9);
    } else if (s < 280) {
        t.nb = 7;
        t.bits = bcz_rev(s - 256u, 7);
    } else {
        t.nb = 8;
        t.bits = bcz_rev(0xC0u + (s - 280u), 8);
    }
    return t;
}
// the length symbol's index (symbol - 257) and the distance symbol: the inverses of bcz_len_base /
// bcz_dist_base, whose tables stay where they are
BCD_HD uint32_t bcd_len_index(uint32_t len) {  // 3 .. 258
    if (len == 258) return 28;
    if (len < 11) return len - 3u;
    const uint32_t n = len - 3u, hb = bcd_ilog2(n);
    return 4u * (hb - 1u) + ((n >> (hb - 2u)) & 3u);
}
BCD_HD uint32_t bcd_dist_index(uint32_t dist) {  // 1 .. 32768
    if (dist < 5) return dist - 1u;
    const uint32_t n = dist - 1u, hb = bcd_ilog2(n);
    return 2u * hb + ((n >> (hb - 1u)) & 1u);
}
BCD_HD BcdTok bcd_match(uint32_t len, uint32_t dist) {
    const uint32_t li = bcd_len_index(len), di = bcd_dist_index(dist);
    BcdTok t = bcd_litlen(257u + li);
    t.bits |= (len - bcz_len_base(li)) << t.nb;
    t.nb += bcz_len_extra(li);
    t.bits |= bcz_rev(di, 5) << t.nb;
    t.nb += 5;
    t.bits |= (dist - bcz_dist_base(di)) << t.nb;
    t.nb += bcz_dist_extra(di);
    return t;  // at most 8 + 5 + 5 + 13 = 31 bits
}

// ---- CRC-32 arithmetic (reflected: bit 31 is x^0) ------------------------------------------------------
BCD_HD uint32_t bcd_crc_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (BCD_CRC_POLY & (0u - (c & 1u)));
    return c;
}
BCD_HD uint32_t bcd_mulmod(uint32_t a, uint32_t b) {  // a * b mod P
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32; ++i) {
        p ^= b & (0u - ((a >> (31u - i)) & 1u));
        b = (b >> 1) ^ (BCD_CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}
BCD_HD uint32_t bcd_xpow(uint32_t n) {  // x^n mod P
    uint32_t r = 0x80000000u, sq = 0x40000000u;
    for (; n; n >>= 1) {
        if (n & 1u) r = bcd_mulmod(r, sq);
        sq = bcd_mulmod(sq, sq);
    }
    return r;
}

// the lanes' loop: position l of the step (0 .. 63) in slot i of the lane's arrays
#define BCD_LANES(m, i, l) \
    for (uint32_t i = 0, l = (m).lane(); i < M::PER; ++i, l += M::NL)

template <class M>
BCD_HD uint32_t bcd_crc(M& m, uint32_t len) {
    const uint32_t chunk = (len + 63u) / 64u;
    const uint32_t* T = m.crc_table();
    uint32_t v[M::PER], o[M::PER];
    BCD_LANES(m, i, l) {
        const int32_t end = (int32_t)len - (int32_t)((63u - l) * chunk);
        uint32_t c = 0;
        if (end > 0) {
            uint32_t q = end > (int32_t)chunk ? (uint32_t)end - chunk : 0u;
            for (; q + 4u <= (uint32_t)end; q += 4u) {
                c ^= m.load32(q);
                c = T[c & 255u] ^ (c >> 8);
                c = T[c & 255u] ^ (c >> 8);
                c = T[c & 255u] ^ (c >> 8);
                c = T[c & 255u] ^ (c >> 8);
            }
            if (q < (uint32_t)end) {
                uint32_t w = m.load32(q);
                for (; q < (uint32_t)end; ++q, w >>= 8) c = T[(c ^ w) & 255u] ^ (c >> 8);
            }
        }
        v[i] = c;
    }
    uint32_t X = bcd_xpow(8u * chunk);
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        m.down(v, o, d);
        BCD_LANES(m, i, l) v[i] = bcd_mulmod(v[i], X) ^ o[i];
        X = bcd_mulmod(X, X);
    }
    return m.get(v, 0) ^ bcd_mulmod(0xFFFFFFFFu, bcd_xpow(8u * len)) ^ 0xFFFFFFFFu;
}

// the common prefix of the input at c and at p (c < p), at most min(258, len - p)
template <class M>
BCD_HD uint32_t bcd_match_len(M& m, uint32_t c, uint32_t p, uint32_t len) {
    const uint32_t cap = len - p < BCD_MAX_MATCH ? len - p : BCD_MAX_MATCH;
    uint32_t n = 0;
    while (n < cap) {
        const uint32_t x = m.load32(c + n) ^ m.load32(p + n);
        if (x) {
            n += bcd_ctz(x) >> 3;
            break;
        }
        n += 4u;
    }
    return n < cap ? n : cap;
}

// nb bits (at most 32) at bit `at` of the staging area; the words were zero or hold other tokens
template <class M>
BCD_HD void bcd_put(M& m, uint32_t at, uint32_t bits, uint32_t nb) {
    const uint64_t v = (uint64_t)bits << (at & 31u);
    m.stage_or(at >> 5, (uint32_t)v);
    if ((at & 31u) + nb > 32u) m.stage_or((at >> 5) + 1u, (uint32_t)(v >> 32));
}

// One block: input [0, len), 1 <= len <= BCD_BLOCK, into the machine's slot.  Returns the block's
// size; *stored says whether the fallback wrote it.
template <class M>
BCD_HD uint32_t bcd_block(M& m, uint32_t len, bool* stored) {
    uint16_t* tab = m.table();
    uint32_t* stg = m.stage();
    BCD_LANES(m, i, l) {
        for (uint32_t e = l; e < (1u << BCD_HASH_BITS); e += 64u) tab[e] = (uint16_t)BCD_EMPTY;
        for (uint32_t e = l; e < BCD_STAGE_WORDS; e += 64u) stg[e] = 0;
        for (uint32_t e = 4u * l; e < 4u * l + 4u; ++e) m.crc_table()[e] = bcd_crc_entry(e);
    }
    m.sync();
    const uint32_t crc = bcd_crc(m, len);
    // the header (BSIZE comes last) and the block's three header bits: BFINAL = 1, BTYPE = 01
    BCD_LANES(m, i, l) {
        if (l < 16u) bcd_put(m, 8u * l, bcd_header_byte(l, 0), 8);
        if (l == 16u) bcd_put(m, 8u * BCD_HEAD, 3u, 3);
    }
    uint32_t sbits = 8u * BCD_HEAD + 3u;  // bits in the staging area
    uint32_t flushed = 0;                 // bytes of the slot written by whole flushes
    uint32_t cover = 0;                   // the first position no match covers yet
    bool fall = false;
    for (uint32_t base = 0; base < len; base += BCD_STEP) {
        const uint32_t n = len - base < BCD_STEP ? len - base : BCD_STEP;
        uint32_t p[M::PER], h[M::PER], cand[M::PER], byte[M::PER], mlen[M::PER], mdist[M::PER];
        bool can[M::PER], has[M::PER];
        BCD_LANES(m, i, l) {
            p[i] = base + l;
            const uint32_t v = l < n ? m.load32(p[i]) : 0u;
            byte[i] = v & 255u;
            can[i] = p[i] + 4u <= len;
            h[i] = bcd_hash(v);
            cand[i] = can[i] && p[i] >= cover ? (uint32_t)tab[h[i]] : BCD_EMPTY;
        }
        m.sync();
        m.insert(h, p, can);
        m.sync();
        BCD_LANES(m, i, l) {
            mlen[i] = 0;
            mdist[i] = 0;
            if (cand[i] != BCD_EMPTY && p[i] - cand[i] <= BCD_MAX_DIST) {
                const uint32_t ml = bcd_match_len(m, cand[i], p[i], len);
                if (ml >= BCD_MIN_MATCH) {
                    mlen[i] = ml;
                    mdist[i] = p[i] - cand[i];
                }
            }
            has[i] = mlen[i] != 0;
        }
        // the parse: lit and mt are the lanes that start a literal / a match
        const uint64_t M_ = m.mask(has);
        uint64_t lit = 0, mt = 0;
        uint32_t pos = cover > base ? cover - base : 0u;
        while (pos < n) {
            const uint64_t rest = M_ >> pos << pos;
            const uint32_t j = rest ? bcd_ctz64(rest) : n;
            const uint32_t upto = j < n ? j : n;  // literals [pos, upto)
            lit |= ((upto < 64u ? 1ull << upto : 0ull) - 1ull) >> pos << pos;
            if (j >= n) {
                pos = n;
                break;
            }
            const uint32_t lj = m.get(mlen, j);
            if (j + 1u < n && (M_ >> (j + 1u) & 1ull) && m.get(mlen, j + 1u) > lj) {
                lit |= 1ull << j;
                pos = j + 1u;
            } else {
                mt |= 1ull << j;
                pos = j + lj;
            }
        }
        if (base + pos > cover) cover = base + pos;
        uint32_t nb[M::PER], bits[M::PER], off[M::PER], total;
        BCD_LANES(m, i, l) {
            BcdTok t;
            t.bits = t.nb = 0;
            if (mt >> l & 1ull)
                t = bcd_match(mlen[i], mdist[i]);
            else if (lit >> l & 1ull)
                t = bcd_litlen(byte[i]);
            nb[i] = t.nb;
            bits[i] = t.bits;
        }
        m.scan(nb, off, total);
        BCD_LANES(m, i, l) {
            if (nb[i]) bcd_put(m, sbits + off[i], bits[i], nb[i]);
        }
        sbits += total;
        if (flushed + (sbits + 7u) / 8u - BCD_HEAD >= len + BCD_STORED_EXTRA) {
            fall = true;
            break;
        }
        m.sync();
        if (sbits >= 8u * BCD_FLUSH) {
            m.flush(flushed, BCD_FLUSH / 16u);
            m.sync();
            BCD_LANES(m, i, l) {
                const uint32_t keep = l < BCD_STAGE_WORDS - BCD_FLUSH / 4u ? stg[BCD_FLUSH / 4u + l] : 0u;
                for (uint32_t e = l; e < BCD_STAGE_WORDS; e += 64u) stg[e] = e == l ? keep : 0u;
            }
            m.sync();
            flushed += BCD_FLUSH;
            sbits -= 8u * BCD_FLUSH;
        }
    }
    if (!fall) {
        sbits = (sbits + 7u + 7u) & ~7u;  // end-of-block is seven zero bits; then up to the byte
        fall = flushed + sbits / 8u - BCD_HEAD >= len + BCD_STORED_EXTRA;
    }
    *stored = fall;
    if (!fall) {
        const uint32_t total = flushed + sbits / 8u + BCD_TAIL;
        BCD_LANES(m, i, l) {
            if (l == 0u) bcd_put(m, sbits, crc, 32);
            if (l == 1u) bcd_put(m, sbits + 32u, len, 32);
            if (l == 2u && flushed == 0u) bcd_put(m, 8u * 16u, total - 1u, 16);
        }
        m.sync();
        m.flush(flushed, (sbits / 8u + BCD_TAIL + 15u) / 16u);
        if (flushed != 0u) {
            m.slot_fence();
            BCD_LANES(m, i, l) {
                if (l < 2u) m.slot_byte(16u + l, bcd_header_byte(16u + l, total - 1u));
            }
        }
        return total;
    }
    // the stored block, over whatever the flushes left in the slot
    const uint32_t total = BCD_HEAD + BCD_STORED_EXTRA + len + BCD_TAIL;
    m.slot_fence();
    BCD_LANES(m, i, l) {
        if (l < BCD_HEAD) m.slot_byte(l, bcd_header_byte(l, total - 1u));
        if (l == 18u) m.slot_byte(18, 1);  // BFINAL = 1, BTYPE = 00, padding
        if (l >= 19u && l < 23u) {
            const uint32_t w = (len & 0xFFFFu) | ((~len & 0xFFFFu) << 16);
            m.slot_byte(l, (uint8_t)(w >> (8u * (l - 19u))));
        }
        if (l >= 24u && l < 32u) {
            const uint64_t w = (uint64_t)crc | (uint64_t)len << 32;
            m.slot_byte(BCD_HEAD + BCD_STORED_EXTRA + len + (l - 24u), (uint8_t)(w >> (8u * (l - 24u))));
        }
        for (uint32_t q = l; q < len; q += 64u) m.slot_byte(BCD_HEAD + BCD_STORED_EXTRA + q, (uint8_t)m.load32(q));
    }
    return total;
}

// ---- the host machine ---------------------------------------------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
struct BcdHost {
    static constexpr uint32_t NL = 1, PER = 64;
    const uint8_t* in;
    uint32_t len;
    uint8_t* slot;  // [BCD_SLOT]
    uint16_t table_[1u << BCD_HASH_BITS];
    uint32_t stage_[BCD_STAGE_WORDS], crc_[256];
    uint32_t lane() const { return 0; }
    uint32_t load32(uint32_t p) const {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; ++k)
            if (p + k < len) v |= (uint32_t)in[p + k] << (8 * k);
        return v;
    }
    uint16_t* table() { return table_; }
    uint32_t* stage() { return stage_; }
    uint32_t* crc_table() { return crc_; }
    void sync() {}
    uint64_t mask(const bool (&v)[PER]) const {
        uint64_t r = 0;
        for (uint32_t l = 0; l < 64; ++l) r |= (uint64_t)v[l] << l;
        return r;
    }
    uint32_t get(const uint32_t (&v)[PER], uint32_t j) const { return v[j]; }
    void scan(const uint32_t (&v)[PER], uint32_t (&e)[PER], uint32_t& total) const {
        uint32_t s = 0;
        for (uint32_t l = 0; l < 64; ++l) {
            e[l] = s;
            s += v[l];
        }
        total = s;
    }
    void down(const uint32_t (&v)[PER], uint32_t (&o)[PER], uint32_t d) const {
        for (uint32_t l = 0; l < 64; ++l) o[l] = l + d < 64 ? v[l + d] : 0u;
    }
    void insert(const uint32_t (&h)[PER], const uint32_t (&p)[PER], const bool (&on)[PER]) {
        for (uint32_t l = 0; l < 64; ++l)  // ascending: the highest position remains
            if (on[l]) table_[h[l]] = (uint16_t)p[l];
    }
    void stage_or(uint32_t w, uint32_t bits) { stage_[w] |= bits; }
    void flush(uint32_t dst, uint32_t n16) {
        for (uint32_t i = 0; i < 16u * n16; ++i) slot[dst + i] = (uint8_t)(stage_[i >> 2] >> (8u * (i & 3u)));
    }
    void slot_byte(uint32_t off, uint8_t v) { slot[off] = v; }
    void slot_fence() {}
};

// one block on the host: in[0, len) -> slot[0, size), slot of BCD_SLOT bytes
inline uint32_t bcd_block_host(const uint8_t* in, uint32_t len, uint8_t* slot, bool* stored) {
    BcdHost m;
    m.in = in;
    m.len = len;
    m.slot = slot;
    return bcd_block(m, len, stored);
}
#endif
