// Host check of the DEFLATE core (basecount_amd/csrc/bc_inflate.h), the header the device kernel
// compiles too.  Reads vectors (tests/inflate_vectors.py writes them), runs each through
// bcz_inflate_host with 64 guard bytes in front of and behind both the input and the output, each
// in a heap allocation of exactly that size, and writes status, guard verdict and output bytes.
//   g++ -fsanitize=address,undefined -I basecount_amd/csrc tests/native/inflate_check.cpp
//   ./a.out vectors.bin results.bin
// vectors.bin:  u32 n, then n x { u32 clen, u32 isize, clen bytes }
// results.bin:  n x { u8 status, u8 guards_ok, isize bytes }
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bc_inflate.h"

namespace {
constexpr size_t kGuard = 64;
constexpr uint8_t kInGuard = 0xA5, kOutGuard = 0x5A, kOutFill = 0xEE;

bool rd32(FILE* f, uint32_t* v) { return std::fread(v, 4, 1, f) == 1; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return std::fprintf(stderr, "usage: inflate_check vectors.bin results.bin\n"), 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return std::fprintf(stderr, "cannot open files\n"), 2;
    uint32_t n = 0;
    if (!rd32(in, &n)) return 2;
    long ok = 0;
    for (uint32_t v = 0; v < n; ++v) {
        uint32_t clen = 0, isize = 0;
        if (!rd32(in, &clen) || !rd32(in, &isize) || isize > (1u << 20)) return std::fprintf(stderr, "bad vector file\n"), 2;
        uint8_t* ibuf = (uint8_t*)std::malloc(clen + 2 * kGuard);
        uint8_t* obuf = (uint8_t*)std::malloc(isize + 2 * kGuard);
        if (!ibuf || !obuf) return 2;
        std::memset(ibuf, kInGuard, clen + 2 * kGuard);
        std::memset(obuf, kOutGuard, isize + 2 * kGuard);
        std::memset(obuf + kGuard, kOutFill, isize);
        if (clen && std::fread(ibuf + kGuard, 1, clen, in) != clen) return std::fprintf(stderr, "short vector file\n"), 2;
        std::vector<uint8_t> copy(ibuf + kGuard, ibuf + kGuard + clen);
        const int st = bcz_inflate_host(ibuf + kGuard, clen, obuf + kGuard, isize);
        bool guards = clen == 0 || std::memcmp(copy.data(), ibuf + kGuard, clen) == 0;  // the input is read-only
        for (size_t i = 0; i < kGuard; ++i) {
            guards &= ibuf[i] == kInGuard && ibuf[kGuard + clen + i] == kInGuard;
            guards &= obuf[i] == kOutGuard && obuf[kGuard + isize + i] == kOutGuard;
        }
        const uint8_t head[2] = {(uint8_t)st, (uint8_t)(guards ? 1 : 0)};
        std::fwrite(head, 1, 2, out);
        std::fwrite(obuf + kGuard, 1, isize, out);
        ok += st == 0;
        std::free(ibuf);
        std::free(obuf);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("ok %u vectors, %ld accepted\n", n, ok);
    return 0;
}
