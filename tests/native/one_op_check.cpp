// one_op_check.cpp — the one-op chunk setup of k_pileup's slice instance (basecount_amd/csrc/
// bc_tile.h: process_chunk<.., SLICE> when every read of a chunk has one CIGAR op) enumerated on
// the host, built with AddressSanitizer and UBSan by tests/test_one_op_host.py.
//   * bc_slice::covered_one_op equals bc_slice::covered for the run [0, len) at query delta 0 over
//     the three pieces such a chunk issues, and equals a restatement from the definitions: every
//     base on a tile position lies in a piece k < 3 that begins below the buffer's end;
//   * whenever it answers true, every needed nibble lies in [0, 96) of the slot (bytes [0, 48):
//     piece 3 is never read unmasked), and the answer over four pieces would be the same;
//   * decode_one_op (bc_runs.h) gives decode_runs<1>'s table, and with it the lean walk's slow
//     decision, for a single word of every op code and length, at every cmax.
// Swept: every seq_nib mod 32 (at the buffer's start and further in), pos - t0 in [-260, 64), the
// lengths below, the buffer's end at every 16-B boundary from two pieces below the slot to two
// beyond it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define BC_HD inline
#include "bc_runs.h"
#include "bc_slice.h"

namespace S = bc_slice;

static const uint32_t kLens[] = {0, 1, 2, 31, 32, 33, 63, 64, 65, 129, 150, 250, 0x1FFE, 0x1FFF};
static long long checks = 0, true_n = 0, false_n = 0;

#define REQUIRE(c, ...)                                         \
    do {                                                        \
        ++checks;                                               \
        if (!(c)) {                                             \
            std::printf("FAILED %s (line %d): ", #c, __LINE__); \
            std::printf(__VA_ARGS__);                           \
            std::printf("\n");                                  \
            std::exit(1);                                       \
        }                                                       \
    } while (0)

static void slot(int32_t rel, uint32_t seq_nib, uint32_t len, uint32_t src, uint32_t buf_end) {
#define AT "rel %d seq_nib %u len %u src %u buf_end %u", rel, seq_nib, len, src, buf_end
    const bool got = S::covered_one_op(seq_nib, rel, len, src, buf_end);
    REQUIRE(got == S::covered(seq_nib, rel, 0u, len, 0, src, buf_end, S::kOneOpPieces), AT);
    // from the definitions: the tile's positions are t0 + [0, 64), the run covers reference offsets
    // [0, len) from pos, offset o's base is nibble seq_nib + o of the buffer
    const int64_t lo = rel < 0 ? -(int64_t)rel : 0;
    const int64_t hi = 64 - (int64_t)rel < (int64_t)len ? 64 - (int64_t)rel : (int64_t)len;
    bool want = true;
    for (int64_t o = lo; o < hi; ++o) {
        const int64_t nib = (int64_t)seq_nib + o - 2 * (int64_t)src;  // slot-relative
        const int64_t k = nib >= 0 ? (nib >> 1) / S::kPieceBytes : -1;
        want = want && k >= 0 && k < S::kOneOpPieces && (int64_t)src + S::kPieceBytes * k < (int64_t)buf_end;
        if (got) REQUIRE(nib >= 0 && nib < 2 * S::kPieceBytes * S::kOneOpPieces, AT);
    }
    REQUIRE(got == want, AT);
    // the fourth piece changes nothing: a one-op read never needs it
    REQUIRE(got == S::covered(seq_nib, rel, 0u, len, 0, src, buf_end), AT);
    if (hi <= lo) REQUIRE(got, AT);
    ++(got ? true_n : false_n);
#undef AT
}

static void decode(uint32_t op, uint32_t len) {
#define AT "op %u len %u cmax %d", op, len, cmax
    const uint32_t w0 = len << 4 | op;
    const RunTable D = decode_one_op(w0);
    for (int cmax = 1; cmax <= kPre; ++cmax) {
        const uint32_t w[kPre] = {w0, 0, 0, 0, 0, 0, 0, 0};
        const RunTable R = decode_runs<1>(w, 1u, cmax);
        REQUIRE(D.st[0] == R.st[0] && D.en[0] == R.en[0] && D.qd[0] == R.qd[0], AT);
        REQUIRE(D.nrun == R.nrun && D.gap == R.gap && D.complex == R.complex, AT);
        REQUIRE(D.span == R.span && D.qlen == R.qlen, AT);
        for (int i = 1; i < kMaxRuns; ++i) REQUIRE(D.st[i] == 0 && D.en[i] == 0 && D.qd[i] == 0, AT);
        // the lean walk's decision and record: a slow read's record is empty, a fast one's is its run
        const bool slow_d = D.complex || D.gap || D.nrun > 1, slow_r = R.complex || R.gap || R.nrun > 1;
        REQUIRE(slow_d == slow_r, AT);
        // what the issue of this decode states, word for word
        const bool m = (op == 0 || op == 7 || op == 8) && len > 0, d = (op == 2 || op == 3) && len > 0;
        REQUIRE(slow_d == (d || ((m || d) && len >= 0x1FFFu)), AT);
        if (!slow_d) REQUIRE(D.st[0] == 0 && D.qd[0] == 0 && D.en[0] == (m ? len : 0u), AT);
    }
#undef AT
}

int main() {
    const uint32_t bases[] = {0, 32 * 1000};
    for (uint32_t nbase : bases)
        for (uint32_t m = 0; m < 32; ++m)
            for (int32_t rel = -260; rel < 64; ++rel)
                for (uint32_t len : kLens) {
                    const uint32_t seq_nib = nbase + m;
                    const uint32_t src = S::source_byte(seq_nib, rel);
                    // every 16-B boundary around the slot [src, src + 64)
                    for (int64_t end = (int64_t)src - 32; end <= (int64_t)src + 96; end += 16)
                        if (end >= 0) slot(rel, seq_nib, len, src, (uint32_t)end);
                    slot(rel, seq_nib, len, src, 1u << 30);
                }
    for (uint32_t op = 0; op < 16; ++op) {
        for (uint32_t len : kLens) decode(op, len);
        decode(op, 0x2000u);
        decode(op, 0xFFFFFFFu);  // the longest a CIGAR word holds
    }
    if (true_n < 100000 || false_n < 100000) {
        std::printf("FAILED: the sweep met %lld covered and %lld uncovered slots\n", true_n, false_n);
        return 1;
    }
    std::printf("ok %lld checks, %lld covered, %lld uncovered\n", checks, true_n, false_n);
    return 0;
}
