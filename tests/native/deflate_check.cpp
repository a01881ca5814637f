// deflate_check.cpp — the BGZF block writer of basecount_amd/csrc/bc_deflate.h on its host machine
// (BcdHost, the schedule the kernel runs, lane by lane), built with AddressSanitizer and UBSan by
// tests/test_deflate_host.py and linked with zlib.  Every case is cut into blocks of 65,280 bytes
// and each block is required to
//   * be at most 65,536 bytes, with the BGZF header, BSIZE = size - 1 and ISIZE = its input length;
//   * inflate to exactly its input with zlib's inflate (raw, -15) AND with the project's own
//     decoder (bc_inflate.h, BczHost);
//   * carry the CRC-32 zlib's crc32 gives for the input.
// Cases: tiny lengths, the block cuts, periodic input, matches of exactly 258 and longer candidates,
// candidates at distance 32,768 (used) and 32,769 (not used), incompressible input (the stored
// fallback, taken early and taken late) and the texts whose .out.gz paths are given as arguments.
// For each text it prints "text <name> <plain> <ours> <zlib level 1 Z_FIXED on the same cuts>".
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bc_deflate.h"

static long long checks = 0;
static const char* g_case = "";

#define REQUIRE(c)                                                                   \
    do {                                                                             \
        ++checks;                                                                    \
        if (!(c)) {                                                                  \
            std::printf("FAILED %s (line %d) in case %s\n", #c, __LINE__, g_case);   \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 24);
}

struct Result {
    size_t total = 0, blocks = 0, stored = 0;
};

static Result check(const char* name, const std::vector<uint8_t>& data) {
    g_case = name;
    Result r;
    const uint64_t nb = bcd_nblocks(data.size());
    REQUIRE(nb == (data.size() + 65279) / 65280);
    std::vector<uint8_t> slot(BCD_SLOT + 64, 0xA5), back(BCD_BLOCK), back2(BCD_BLOCK);
    for (uint64_t k = 0; k < nb; ++k) {
        const uint32_t len = bcd_block_len(data.size(), k);
        const uint8_t* in = data.data() + k * BCD_BLOCK;
        // an exact-size copy, so that a read past the block's input is the sanitizer's to find
        std::vector<uint8_t> own(in, in + len);
        bool stored = false;
        const uint32_t size = bcd_block_host(own.data(), len, slot.data(), &stored);
        for (uint32_t i = 0; i < 64; ++i) REQUIRE(slot[BCD_SLOT + i] == 0xA5);
        REQUIRE(size <= 65536u && size >= 28u);
        static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        REQUIRE(std::memcmp(slot.data(), head, 16) == 0);
        REQUIRE((uint32_t)(slot[16] | slot[17] << 8) == size - 1);
        uint32_t crc, isize;
        std::memcpy(&crc, &slot[size - 8], 4);
        std::memcpy(&isize, &slot[size - 4], 4);
        REQUIRE(isize == len);
        REQUIRE(crc == (uint32_t)crc32(crc32(0, nullptr, 0), own.data(), len));
        const uint32_t clen = size - 26;
        REQUIRE(stored == ((slot[18] & 6) == 0));
        if (stored) REQUIRE(clen == len + 5);
        REQUIRE(clen <= len + 5);
        // zlib
        z_stream z;
        std::memset(&z, 0, sizeof z);
        REQUIRE(inflateInit2(&z, -15) == Z_OK);
        z.next_in = slot.data() + 18;
        z.avail_in = clen;
        z.next_out = back.data();
        z.avail_out = BCD_BLOCK;
        REQUIRE(inflate(&z, Z_FINISH) == Z_STREAM_END);
        REQUIRE(z.total_out == len && z.avail_in == 0);
        inflateEnd(&z);
        REQUIRE(std::memcmp(back.data(), own.data(), len) == 0);
        // the project's decoder, on an exact-size copy of the payload
        std::vector<uint8_t> pay(slot.begin() + 18, slot.begin() + 18 + clen);
        REQUIRE(bcz_inflate_host(pay.data(), clen, back2.data(), len) == BC_Z_OK);
        REQUIRE(std::memcmp(back2.data(), own.data(), len) == 0);
        r.total += size;
        r.blocks += 1;
        r.stored += stored;
    }
    return r;
}

static size_t zlib_fixed(const std::vector<uint8_t>& data) {
    size_t total = 0;
    std::vector<uint8_t> out(BCD_BLOCK * 2);
    for (size_t b = 0; b < data.size(); b += BCD_BLOCK) {
        const size_t len = data.size() - b < BCD_BLOCK ? data.size() - b : BCD_BLOCK;
        z_stream z;
        std::memset(&z, 0, sizeof z);
        if (deflateInit2(&z, 1, Z_DEFLATED, -15, 8, Z_FIXED) != Z_OK) std::exit(2);
        z.next_in = const_cast<uint8_t*>(data.data() + b);
        z.avail_in = (uInt)len;
        z.next_out = out.data();
        z.avail_out = (uInt)out.size();
        if (deflate(&z, Z_FINISH) != Z_STREAM_END) std::exit(2);
        total += z.total_out + 26;
        deflateEnd(&z);
    }
    return total;
}

static std::vector<uint8_t> random_bytes(size_t n, uint32_t lo, uint32_t span) {
    std::vector<uint8_t> v(n);
    for (auto& b : v) b = (uint8_t)(lo + rnd() % span);
    return v;
}

int main(int argc, char** argv) {
    // the EOF block is an empty block of the same framing
    {
        g_case = "eof";
        uint8_t eof[28], out[1];
        for (uint32_t i = 0; i < 28; ++i) eof[i] = bcd_eof_byte(i);
        static const uint8_t want[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        REQUIRE(std::memcmp(eof, want, 28) == 0);
        REQUIRE(bcz_inflate_host(eof + 18, 2, out, 0) == BC_Z_OK);
    }
    // the token codes invert the decoder's tables
    g_case = "codes";
    for (uint32_t len = 3; len <= 258; ++len) {
        const uint32_t i = bcd_len_index(len);
        REQUIRE(i <= 28 && bcz_len_base(i) <= len && len - bcz_len_base(i) < (1u << bcz_len_extra(i)));
        if (len == 258) REQUIRE(i == 28);
    }
    for (uint32_t d = 1; d <= 32768; ++d) {
        const uint32_t i = bcd_dist_index(d);
        REQUIRE(i <= 29 && bcz_dist_base(i) <= d && d - bcz_dist_base(i) < (1u << bcz_dist_extra(i)));
    }
    // tiny lengths
    for (uint32_t n : {0u, 1u, 2u, 3u, 4u, 63u, 64u, 65u, 257u, 258u, 259u, 260u}) {
        std::vector<uint8_t> text(n), same(n, 'a');
        for (uint32_t i = 0; i < n; ++i) text[i] = (uint8_t)("ref\t12\t0\t5\n"[i % 11]);
        const std::string nm = "tiny " + std::to_string(n);
        Result r = check(nm.c_str(), text);
        REQUIRE(r.blocks == (n ? 1u : 0u));
        check(nm.c_str(), same);
        check(nm.c_str(), random_bytes(n, 0, 256));
    }
    // block cuts
    for (uint32_t n : {65279u, 65280u, 65281u}) {
        std::vector<uint8_t> v(n);
        for (uint32_t i = 0; i < n; ++i) v[i] = (uint8_t)('0' + (i / 7) % 10 + (rnd() % 16 == 0));
        const std::string nm = "cut " + std::to_string(n);
        Result r = check(nm.c_str(), v);
        REQUIRE(r.blocks == (n > 65280u ? 2u : 1u));
        REQUIRE(r.total < n);
    }
    // periodic input: distance 1 (matches of 258 that overlap themselves), periods 2, 3 and 7
    for (uint32_t period : {1u, 2u, 3u, 7u}) {
        for (uint32_t n : {1000u, 65280u}) {
            std::vector<uint8_t> v(n);
            for (uint32_t i = 0; i < n; ++i) v[i] = (uint8_t)('A' + i % period);
            const std::string nm = "period " + std::to_string(period);
            Result r = check(nm.c_str(), v);
            REQUIRE(r.stored == 0 && r.total < n / 20 + 200);
        }
    }
    // a match of exactly 258, and candidates of 259 and more
    for (uint32_t mlen : {257u, 258u, 259u, 300u, 516u, 517u}) {
        std::vector<uint8_t> v = random_bytes(600, 32, 96);
        std::vector<uint8_t> w(v);
        w.push_back('#');
        w.insert(w.end(), v.begin(), v.begin() + mlen);
        w.push_back('$');
        const std::string nm = "match " + std::to_string(mlen);
        Result r = check(nm.c_str(), w);
        REQUIRE(r.total < 600 + 26 + 80);  // the copy costs a few tokens, not mlen literals
    }
    // the distance limit: the issue's shape (40,000 random bytes, then a copy of their start at
    // 32,768 / 32,769), and a shape in which the one-entry table still holds the candidate when the
    // copy arrives (the filler between them is one byte repeated, which takes one entry)
    {
        size_t used = 0, unused = 0;
        for (uint32_t dist : {32768u, 32769u}) {
            std::vector<uint8_t> v = random_bytes(40000, 0, 144);
            v.insert(v.end(), v.begin() + (40000 - dist), v.begin() + (40000 - dist) + 1000);
            check(dist == 32768u ? "distance 32768 (random)" : "distance 32769 (random)", v);
            std::vector<uint8_t> w = random_bytes(1000, 0, 144);
            w.resize(dist, 150);
            w.insert(w.end(), w.begin(), w.begin() + 1000);
            Result r = check(dist == 32768u ? "distance 32768" : "distance 32769", w);
            (dist == 32768u ? used : unused) = r.total;
        }
        g_case = "distance limit";
        REQUIRE(used + 900 < unused);  // at 32,768 the copy is a few matches, at 32,769 literals
    }
    // incompressible: the stored fallback, decided early and decided late
    {
        std::vector<uint8_t> v = random_bytes(65280, 144, 112);
        Result r = check("incompressible", v);
        REQUIRE(r.stored == 1 && r.total == 65280u + 5 + 26);
        for (uint32_t i = 0; i < 32640; ++i) v[i] = (uint8_t)("0\t"[i & 1]);
        // 32,640 bytes at 9 bits are 36,720: the first half must save more than 4,080 for fixed codes to win
        r = check("incompressible second half", v);
        REQUIRE(r.stored == 0);
        std::vector<uint8_t> w = random_bytes(65280, 144, 112);
        for (uint32_t i = 0; i < 2000; ++i) w[i] = (uint8_t)("0\t"[i & 1]);
        r = check("incompressible, late decision", w);
        REQUIRE(r.stored == 1 && r.total == 65280u + 5 + 26);
        std::vector<uint8_t> u = random_bytes(1500, 144, 112);  // the fallback before the first flush
        r = check("incompressible, short", u);
        REQUIRE(r.stored == 1 && r.total == 1500u + 5 + 26);
        std::vector<uint8_t> t = random_bytes(5, 144, 112);  // 3 + 45 + 7 bits: 7 bytes < 10
        r = check("incompressible, 5 bytes", t);
        REQUIRE(r.stored == 0);
    }
    // real texts
    for (int a = 1; a < argc; ++a) {
        gzFile f = gzopen(argv[a], "rb");
        if (!f) {
            std::printf("FAILED cannot open %s\n", argv[a]);
            return 1;
        }
        std::vector<uint8_t> text;
        uint8_t buf[65536];
        int got;
        while ((got = gzread(f, buf, sizeof buf)) > 0) text.insert(text.end(), buf, buf + got);
        gzclose(f);
        Result r = check(argv[a], text);
        REQUIRE(r.stored == 0);
        std::printf("text %s %zu %zu %zu\n", argv[a], text.size(), r.total, zlib_fixed(text));
    }
    std::printf("ok %lld\n", checks);
    return 0;
}
