// cohort_check.cpp — the shared decisions of a cohort run (basecount_amd/csrc/bc_cohort.h) on the
// host, under AddressSanitizer + UBSan (tests/test_cohort_host.py).
//
// Each function of the header is compared with a plain-loop restatement that shares no code with
// it: the window clip against a position-by-position membership test, k1 / k2 against a sorted
// vector's middle, the segment lookup against a linear scan, and the rebase kernel's schedule
// (waves of 64 reads, a uniform search for waves inside one segment) against a per-read loop in
// 64-bit arithmetic.  Arrays are heap-allocated at their exact sizes, so a lookup that leaves
// the table or a clip that leaves the segment is an ASan report.
//
//   cohort_check            runs every check, prints "ok <n> checks"
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bc_cohort.h"

static long g_checks = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        ++g_checks;                                                           \
        if (!(c)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

// ---- the window clip: which positions of [0, L) lie in [lo, hi] ----
static void check_clip(int64_t lo, int64_t hi, int64_t L) {
    std::vector<int> seg((size_t)L, 0);  // exact size: reading seg[w.lo + i] out of range is a report
    int64_t first = -1, count = 0;
    for (int64_t p = 0; p < L; ++p)
        if (p >= lo && p <= hi) {
            if (first < 0) first = p;
            ++count;
        }
    const bcc_window w = bcc_clip(lo, hi, L);
    CHECK(bcc_empty(w) == (count == 0));
    if (count == 0) return;
    CHECK(w.lo == first && w.n == count);
    long sum = 0;
    for (int64_t i = 0; i < w.n; ++i) sum += seg[(size_t)(w.lo + i)];
    CHECK(sum == 0);
}

// ---- k1 / k2: the middle element(s) of n sorted values ----
static void check_median(int64_t n) {
    std::vector<double> v((size_t)n);
    for (int64_t i = 0; i < n; ++i) v[(size_t)i] = (double)((i * 7919) % n);  // a permutation when gcd = 1, ties else
    std::sort(v.begin(), v.end());
    const int64_t k1 = bcc_k1(n), k2 = bcc_k2(n);
    CHECK(k1 >= 0 && k2 < n && k1 <= k2 && k2 - k1 == (n % 2 == 0 ? 1 : 0));
    // numpy: odd n takes sorted[n // 2]; even n the mean of sorted[n // 2 - 1] and sorted[n // 2]
    if (n % 2) CHECK(k1 == n / 2 && k2 == n / 2);
    else CHECK(k1 == n / 2 - 1 && k2 == n / 2);
    CHECK(v[(size_t)k1] <= v[(size_t)k2]);
    CHECK(bcc_sorted_path(n) == (n <= 512));
}

// ---- the segment lookup ----
static int seg_linear(const std::vector<int64_t>& rb, int64_t i) {
    int s = 0;
    for (int j = 0; j + 1 < (int)rb.size(); ++j)
        if (rb[(size_t)j] <= i) s = j;  // the LAST segment that starts at or before i
    return s;
}

static std::vector<int64_t> table_of(const std::vector<int64_t>& counts) {
    std::vector<int64_t> rb(counts.size() + 1, 0);
    for (size_t j = 0; j < counts.size(); ++j) rb[j + 1] = rb[j] + counts[j];
    return rb;
}

static void check_lookup(const std::vector<int64_t>& counts) {
    const std::vector<int64_t> rb = table_of(counts);
    const int n_seg = (int)counts.size();
    for (int64_t i = 0; i < rb.back(); ++i) {
        const int s = bcc_seg_of(rb.data(), n_seg, i);
        CHECK(s == seg_linear(rb, i));
        CHECK(rb[(size_t)s] <= i && i < rb[(size_t)s + 1]);  // a segment that holds the read: never an empty one
    }
    // whatever is asked, the answer stays inside the table
    const int64_t outside[] = {-1, rb.back(), rb.back() + 1000};
    for (int64_t i : outside) {
        const int s = bcc_seg_of(rb.data(), n_seg, i);
        CHECK(s >= 0 && s < n_seg);
    }
}

// ---- the rebase kernel's schedule ----
static void rebase_twin(int64_t n, const std::vector<int64_t>& rb, int n_seg, const std::vector<uint64_t>& cig_base,
                        const std::vector<uint64_t>& nib_base, const uint32_t* in_cig, const uint32_t* in_nib,
                        uint32_t* out_cig, uint32_t* out_nib) {
    for (int64_t w0 = 0; w0 < n; w0 += 64) {  // one wave
        const int64_t w1 = w0 + 63 < n ? w0 + 63 : n - 1;
        const int s0 = bcc_seg_of(rb.data(), n_seg, w0), s1 = bcc_seg_of(rb.data(), n_seg, w1);
        for (int lane = 0; lane < 64; ++lane) {
            const int64_t i = w0 + lane;
            int seg = s0;
            if (s0 != s1) seg = bcc_seg_of(rb.data(), n_seg, i < n ? i : n - 1);
            if (i >= n) continue;
            const uint32_t c = in_cig[i], q = in_nib[i];
            out_cig[i] = bcc_rebase(c, cig_base[(size_t)seg]);
            out_nib[i] = bcc_rebase(q, nib_base[(size_t)seg]);
        }
    }
}

static void check_rebase(const std::vector<int64_t>& counts, const std::vector<uint64_t>& file_words,
                         const std::vector<uint64_t>& file_seq_bytes, bool in_place) {
    const std::vector<int64_t> rb = table_of(counts);
    const int n_seg = (int)counts.size();
    const int64_t n = rb.back();
    // one file per segment here: bases are the running sums, the sequence offsets multiples of 16
    std::vector<uint64_t> cig_base((size_t)n_seg), nib_base((size_t)n_seg);
    uint64_t words = 0, bytes = 0;
    for (int s = 0; s < n_seg; ++s) {
        CHECK(file_seq_bytes[(size_t)s] % 16 == 0);
        cig_base[(size_t)s] = words;
        nib_base[(size_t)s] = bcc_nib_base(bytes);
        CHECK(bcc_base_aligned(nib_base[(size_t)s]));
        words += file_words[(size_t)s];
        bytes += file_seq_bytes[(size_t)s];
    }
    CHECK(bcc_fits(words, 2 * bytes));
    std::vector<uint32_t> cig((size_t)n), nib((size_t)n), oc((size_t)n, 0xDEADBEEFu), on((size_t)n, 0xDEADBEEFu);
    uint64_t x = 88172645463325252ull;
    for (int s = 0; s < n_seg; ++s)
        for (int64_t i = rb[(size_t)s]; i < rb[(size_t)s + 1]; ++i) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            const uint64_t fw = file_words[(size_t)s], fn = 2 * file_seq_bytes[(size_t)s];
            // the extremes first: the file's last word / nibble, then its first, then anything
            const int64_t j = i - rb[(size_t)s];
            cig[(size_t)i] = (uint32_t)(j == 0 ? fw - 1 : j == 1 ? 0 : x % fw);
            nib[(size_t)i] = (uint32_t)(j == 0 ? fn - 1 : j == 1 ? 0 : (x >> 20) % fn);
        }
    const std::vector<uint32_t> cig0 = cig, nib0 = nib;
    if (in_place) rebase_twin(n, rb, n_seg, cig_base, nib_base, cig.data(), nib.data(), cig.data(), nib.data());
    else rebase_twin(n, rb, n_seg, cig_base, nib_base, cig.data(), nib.data(), oc.data(), on.data());
    const std::vector<uint32_t>& gc = in_place ? cig : oc;
    const std::vector<uint32_t>& gn = in_place ? nib : on;
    for (int64_t i = 0; i < n; ++i) {
        const int s = seg_linear(rb, i);
        const uint64_t ec = (uint64_t)cig0[(size_t)i] + cig_base[(size_t)s], en = (uint64_t)nib0[(size_t)i] + nib_base[(size_t)s];
        CHECK(ec < words && en < 2 * bytes);                      // inside the shared buffers
        CHECK(ec <= 0xFFFFFFFFull && en <= 0xFFFFFFFFull);        // so the 32-bit sum is the sum
        CHECK(gc[(size_t)i] == ec && gn[(size_t)i] == en);
    }
    if (!in_place) CHECK(cig == cig0 && nib == nib0);
}

int main() {
    // the window clip: lo < 0, hi >= L, lo > hi, a window wholly past L, one position, all of it
    const int64_t Ls[] = {1, 63, 64, 65, 300, 513, 700, 8193};
    const int64_t wins[][2] = {{-5, 3}, {0, 0}, {10, 521}, {10, 522}, {250, 10000}, {9000, 9100}, {5, 4},
                               {0, 8192}, {-10, -1}, {-3, 100000}, {8192, 8192}, {8193, 8193}, {699, 700}};
    for (int64_t L : Ls)
        for (auto& w : wins) check_clip(w[0], w[1], L);
    CHECK(bcc_empty(bcc_clip(0, 10, 0)));  // no segment has L = 0, and still nothing is read
    CHECK(bcc_clip(10, 521, 8193).n == 512 && bcc_clip(10, 522, 8193).n == 513);

    const int64_t ns[] = {1, 2, 3, 4, 511, 512, 513, 8192, 8193};
    for (int64_t n : ns) check_median(n);

    // the lookup across empty segments: first, last, adjacent ones, all but one
    check_lookup({5});
    check_lookup({0, 1, 64, 65, 257});
    check_lookup({0, 0, 3, 0, 0, 0, 130, 0});
    check_lookup({64, 64, 64, 64});
    check_lookup({1, 0, 1, 0, 1, 0, 1});
    check_lookup({0, 0, 0, 200});
    check_lookup({200, 0, 0, 0});

    // the rebase: waves inside a segment and straddling several; small bases, then bases near 2^32
    check_rebase({3, 1, 64, 65, 257}, {100, 7, 900, 1000, 5000}, {64, 16, 480, 4096, 8192}, false);
    check_rebase({3, 1, 64, 65, 257}, {100, 7, 900, 1000, 5000}, {64, 16, 480, 4096, 8192}, true);
    // totals of exactly 2^32 - 1 words and 2^32 - 32 nibbles (the largest multiple of 32 below 2^32)
    check_rebase({2, 64, 130}, {0xFFFF0000ull, 0xFFFFull - 10, 10}, {0x7FFF0000ull, 0xFFE0ull, 16}, false);
    check_rebase({2, 64, 130}, {0xFFFF0000ull, 0xFFFFull - 10, 10}, {0x7FFF0000ull, 0xFFE0ull, 16}, true);

    // the overflow rule: 2^32 - 1 words or nibbles fit, 2^32 do not
    CHECK(bcc_fits(0xFFFFFFFFull, 0xFFFFFFFFull));
    CHECK(!bcc_fits(0x100000000ull, 0) && !bcc_fits(0, 0x100000000ull));
    CHECK(!bcc_fits(0x100000000ull, 0x100000000ull) && bcc_fits(0, 0));
    CHECK(bcc_rebase(0xFFFFFFFEu, 1) == 0xFFFFFFFFu && bcc_rebase(0, 0xFFFFFFFFull) == 0xFFFFFFFFu);
    CHECK(bcc_nib_base(0x7FFFFFF0ull) == 0xFFFFFFE0ull && !bcc_base_aligned(bcc_nib_base(8)));

    std::printf("ok %ld checks\n", g_checks);
    return 0;
}
