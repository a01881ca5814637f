// Host check of the tiled walk's bit-plane counters (bc_planes.h) against scalar counting.
//   g++ -O2 -std=c++17 -I basecount_amd/csrc tests/native/planes_check.cpp && ./a.out [rounds]
// One round is a window of 8 read slots (the 8 lanes that share a window on the device).  Each slot
// adds n <= kPlaneAdds window words with planes_add2, two per step as the walk does; the slots are
// summed with planes_join in the fold's order (xor 1, xor 2, the mirrored half) and planes_counts
// takes each position's four sums.
//   * any of the 16 nibble values per position: every bit sum equals a scalar count of that bit;
//   * the seven event classes the walk produces: with the fix-up nibble counters (fix_n / fix_d,
//     folded before they exceed kFixAdds reads), A = plane0 - N, C = plane1 - N, G = plane2 - DS, T = plane3 - DS,
//     DS and N equal the scalar column counts.
// Depths: every n up to the capacity, the capacity itself with every slot full of one class (all
// bit sums of that class at 8 x 30 = 240), and random ones.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#define BC_HD inline
#include "bc_planes.h"

static const uint32_t kClasses[7] = {0x0, 0x1, 0x2, 0x4, 0x8, 0x3, 0xC};  // none A C G T N DS

struct Slot {
    uint32_t p[kPlanes] = {0, 0, 0, 0, 0};
};

static int fail(const char* what, long round, int k, int b, unsigned got, unsigned want) {
    std::printf("FAIL %s round %ld position %d bit/column %d: got %u, want %u\n", what, round, k, b, got, want);
    return 1;
}

int main(int argc, char** argv) {
    const long rounds = argc > 1 ? std::atol(argv[1]) : 20000;
    std::mt19937_64 g(2024);
    long words = 0;
    for (long r = 0; r < rounds; ++r) {
        const int mode = (int)(r % 4);  // 0: all 16 nibble values, 1: the 7 classes, 2: one class, full, 3: N / DS heavy
        const bool classes = mode != 0;
        int n = mode == 2 ? kPlaneAdds : (r < 4 * (kPlaneAdds + 1) ? (int)(r / 4) : (int)(g() % (kPlaneAdds + 1)));
        n &= ~1;  // two reads per step
        Slot s[8];
        unsigned bit[8][4] = {}, col[8][6] = {};   // scalar: per position, bit sums / column counts
        unsigned fixn[8] = {}, fixd[8] = {};         // folded fix-up counters per position
        const uint32_t one = kClasses[1 + (r / 4) % 6];
        for (int l = 0; l < 8; ++l) {
            uint32_t fn = 0, fd = 0;
            int nf = 0;
            auto fix_fold = [&] {
                for (int k = 0; k < 8; ++k) {
                    fixn[k] += (fn >> (4 * k)) & 15u;
                    fixd[k] += (fd >> (4 * k)) & 15u;
                }
                fn = fd = 0;
                nf = 0;
            };
            for (int i = 0; i < n; i += 2) {
                uint32_t x[2] = {0, 0};
                for (int u = 0; u < 2; ++u)
                    for (int k = 0; k < 8; ++k) {
                        uint32_t v;
                        if (mode == 0) v = (uint32_t)(g() % 16);
                        else if (mode == 1) v = kClasses[g() % 7];
                        else if (mode == 2) v = one;
                        else v = (g() % 4) ? (((l + i + u) & 1) ? 0x3u : 0xCu) : kClasses[g() % 7];
                        x[u] |= v << (4 * k);
                        for (int b = 0; b < 4; ++b) bit[k][b] += (v >> b) & 1u;
                        if (classes) {
                            const int c = v == 1 ? 0 : v == 2 ? 1 : v == 4 ? 2 : v == 8 ? 3 : v == 0xC ? 4 : v == 3 ? 5 : -1;
                            if (c >= 0) col[k][c]++;
                        }
                    }
                planes_add2(s[l].p, x[0], x[1]);
                words += 2;
                if (classes) {
                    fn += fix_n(x[0]) + fix_n(x[1]);
                    fd += fix_d(x[0]) + fix_d(x[1]);
                    nf += 2;
                    if (nf + 2 > kFixAdds) fix_fold();  // the next step would not fit
                }
            }
            fix_fold();
        }
        // the fold: lanes l ^ 1, l ^ 2, 7 - l (every lane of the window ends with the same sums)
        uint32_t s6[8][kPlanes + 1], s7[8][kPlanes + 2], s8[8][kSumPlanes];
        for (int l = 0; l < 8; ++l) planes_join<kPlanes>(s[l].p, s[l ^ 1].p, s6[l]);
        for (int l = 0; l < 8; ++l) planes_join<kPlanes + 1>(s6[l], s6[l ^ 2], s7[l]);
        for (int l = 0; l < 8; ++l) planes_join<kPlanes + 2>(s7[l], s7[7 - l], s8[l]);
        for (int l = 0; l < 8; ++l) {  // lane l takes position l
            const uint32_t by = planes_counts(s8[l], l);
            unsigned pl[4];
            for (int b = 0; b < 4; ++b) {
                pl[b] = (by >> (8 * b)) & 0xFFu;
                if (pl[b] != bit[l][b]) return fail("bit sum", r, l, b, pl[b], bit[l][b]);
            }
            if (classes) {
                const unsigned got[6] = {pl[0] - fixn[l], pl[1] - fixn[l], pl[2] - fixd[l], pl[3] - fixd[l], fixd[l], fixn[l]};
                for (int c = 0; c < 6; ++c)
                    if (got[c] != col[l][c]) return fail("column", r, l, c, got[c], col[l][c]);
            }
        }
        if (mode == 2)  // every slot full of one class: that class's bit sums sit at 8 x 30
            for (int b = 0; b < 4; ++b)
                if (((one >> b) & 1u) && bit[0][b] != 8u * (unsigned)n) return fail("capacity", r, 0, b, bit[0][b], 8u * (unsigned)n);
    }
    std::printf("ok %ld rounds, %ld window words\n", rounds, words);
    return 0;
}
