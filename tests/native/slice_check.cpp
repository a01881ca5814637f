// slice_check.cpp — the slot arithmetic of k_pileup's slice instance (basecount_amd/csrc/
// bc_slice.h) enumerated on the host, built with AddressSanitizer and UBSan by
// tests/test_slice_host.py.  For every combination below it restates, from the definitions alone,
// which bases a tile reads of a one-run read and where the slot's 64 bytes come from, and checks
// the header against that:
//   * covered() is true exactly when every base on a tile position lies in [0, 64 B) of the slot,
//     in pieces that were issued;
//   * for a covered read the record's nb leads every tile position to that base's place in the
//     stage, and the two words the window fetch reads (tile_fetch: w0 and w0 + 1) stay inside the
//     stage and its 16-B pads;
//   * no issued piece starts at or beyond the buffer's readable end, or ends beyond it;
//   * a read without a leading clip is always covered, and so is one with a clip of up to 33 bases.
// Swept: pos - t0 in [-320, 64), every seq_nib mod 32 (at the buffer's start and further in), run
// starts and query offsets 0-40, run lengths 1-320, a buffer that ends with the read (its last
// slots cut) and one that does not.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "bc_slice.h"

namespace S = bc_slice;

static long long checks = 0, covered_n = 0, missed_n = 0, cut_n = 0;

#define REQUIRE(c)                                                                                   \
    do {                                                                                             \
        ++checks;                                                                                    \
        if (!(c)) {                                                                                  \
            std::printf("FAILED %s (line %d): rel %d seq_nib %u st %u len %u qd %d buf_end %u\n", #c, __LINE__, rel, \
                        seq_nib, st, len, qd, buf_end);                                              \
            std::exit(1);                                                                            \
        }                                                                                            \
    } while (0)

constexpr int kLimWord = S::kStageBytes / 4;  // the walk's `lim`: the stage's last word index + 1 (the pad's first)

static void one(int32_t rel, uint32_t seq_nib, uint32_t st, uint32_t len, int32_t qd, uint32_t buf_end) {
    const uint32_t en = st + len;
    const uint32_t src = S::source_byte(seq_nib, rel);
    REQUIRE(src % 16 == 0);
    // the slot starts at or below the base at the tile's first covered position of an unclipped read
    const int64_t spec = (int64_t)seq_nib + (rel < 0 ? -rel : 0);
    REQUIRE(2 * (int64_t)src <= spec && spec < 2 * (int64_t)src + 32);
    bool issued[S::kPieces];
    for (int k = 0; k < S::kPieces; ++k) {
        issued[k] = S::piece_issued(src, k, buf_end);
        REQUIRE(issued[k] == ((int64_t)src + 16 * k < (int64_t)buf_end));
        if (issued[k]) REQUIRE((int64_t)src + 16 * k + 16 <= (int64_t)buf_end);
        if (!issued[k]) ++cut_n;
    }
    // the tile's positions are t0 + [0, 64); the run covers reference offsets [st, en) from pos
    const int64_t lo = -(int64_t)rel > (int64_t)st ? -(int64_t)rel : (int64_t)st;
    const int64_t hi = 64 - (int64_t)rel < (int64_t)en ? 64 - (int64_t)rel : (int64_t)en;
    const bool cov = S::covered(seq_nib, rel, st, en, qd, src, buf_end);
    if (hi <= lo) {
        REQUIRE(cov);  // nothing is read of it
        return;
    }
    REQUIRE(S::first_nibble(seq_nib, rel, st, qd) == (uint32_t)((int64_t)seq_nib + qd + lo));
    // absolute nibbles of the first and the last base on the tile (contiguous in between)
    const int64_t a0 = (int64_t)seq_nib + qd + lo, a1 = (int64_t)seq_nib + qd + hi - 1;
    bool inside = a0 >= 2 * (int64_t)src && a1 < 2 * (int64_t)src + 2 * S::kSlotBytes;
    if (inside)
        for (int64_t k = ((a0 >> 1) - src) / 16; k <= ((a1 >> 1) - src) / 16; ++k) inside = inside && issued[k];
    REQUIRE(cov == inside);
    // the slack: a slot starts at most 31 nibbles below the assumed first base and a tile reads at
    // most 64, so a run that begins up to 33 bases later than assumed (a leading clip, qd; a run
    // start past the tile's first position) is covered; an unclipped read always is
    const int64_t shift = (int64_t)qd + lo - (rel < 0 ? -(int64_t)rel : 0);
    if (shift <= 33) REQUIRE(cov);
    if (!cov) {
        ++missed_n;
        return;
    }
    ++covered_n;
    const int slots[3] = {0, 37, S::kSlots - 1};
    for (int slot : slots) {
        const int32_t nb = (int32_t)S::slot_nb(slot, seq_nib, rel, qd, src);
        REQUIRE((nb & 3) == 0);
        const int64_t ends[2] = {lo, hi - 1};
        for (int64_t o : ends) {
            const int64_t tp = (int64_t)rel + o;  // tile position
            REQUIRE(tp >= 0 && tp < 64);
            // the base's nibble relative to the stage, as the walk computes it
            const int64_t sn = (int64_t)(nb >> 2) + tp;
            REQUIRE(sn == 2 * S::kSlotBytes * (int64_t)slot + ((int64_t)seq_nib + qd + o - 2 * (int64_t)src));
            REQUIRE(sn >= 2 * S::kSlotBytes * (int64_t)slot && sn < 2 * S::kSlotBytes * ((int64_t)slot + 1));
            // the window that holds it: tile_fetch reads words w0 and w0 + 1 at bit nb + 32 g
            const int g = (int)(tp >> 3);
            const int b = nb + 32 * g;
            const int w0 = b >> 5;
            REQUIRE(w0 >= -1 && w0 <= kLimWord);      // not clamped away from the base's word
            REQUIRE(w0 + 1 >= 0 && w0 + 1 <= kLimWord + 1);  // the read-ahead word: in the stage or its pad
            REQUIRE((int64_t)w0 * 8 <= sn && sn < ((int64_t)w0 + 2) * 8);
        }
    }
}

int main() {
    const uint32_t lens_a[] = {1, 64, 320};
    const int32_t pairs_b[][2] = {{0, 0}, {0, 1}, {0, 24}, {0, 25}, {0, 40}, {7, 3}};  // {st, qd}
    const uint32_t bases[] = {0, 32 * 1000};
    for (uint32_t nbase : bases)
        for (int32_t rel = -320; rel < 64; ++rel)
            for (uint32_t m = 0; m < 32; ++m) {
                const uint32_t seq_nib = nbase + m;
                auto both_ends = [&](uint32_t st, uint32_t len, int32_t qd) {
                    // a buffer that ends with this read's last base (bc_seq_event_bytes), and a long one
                    const uint64_t seq_bytes = ((uint64_t)seq_nib + (uint32_t)qd + st + len + 1) / 2;  // (query offset = offset + qd)
                    const uint32_t tight = (uint32_t)((seq_bytes + 15) / 16 * 16 + 16);
                    one(rel, seq_nib, st, len, qd, tight);
                    one(rel, seq_nib, st, len, qd, tight + 4096);
                };
                if (nbase == 0 || (rel & 3) == 0)
                    for (uint32_t st = 0; st <= 40; ++st)
                        for (int32_t qd = 0; qd <= 40; ++qd)
                            for (uint32_t len : lens_a) both_ends(st, len, qd);
                for (const auto& p : pairs_b)
                    for (uint32_t len = 1; len <= 320; ++len) both_ends((uint32_t)p[0], len, p[1]);
            }
    // clips far beyond the slack: never covered once the tile reads a base
    for (int32_t rel = -320; rel < 64; ++rel)
        for (int32_t qd : {100, 128, 4000, 65535}) one(rel, 77, 0, 150, qd, 1u << 20);
    if (covered_n < 1000000 || missed_n < 100000 || cut_n < 1000) {
        std::printf("FAILED: the sweep met %lld covered, %lld missed reads, %lld cut pieces\n", covered_n, missed_n, cut_n);
        return 1;
    }
    std::printf("ok %lld checks, %lld covered, %lld missed, %lld cut pieces\n", checks, covered_n, missed_n, cut_n);
    return 0;
}
