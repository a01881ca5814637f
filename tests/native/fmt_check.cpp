// Host check of the row formatter (basecount_amd/csrc/bc_fmt.h), the header the device kernels
// compile too: measure, scan and write as plain loops over the same functions and the kernels'
// schedule (bcf_rows_host).
//   g++ -fsanitize=address,undefined -I basecount_amd/csrc tests/native/fmt_check.cpp -ldl
//   ./a.out cases input.bin results.bin
//     formats each case of the input file, every input and every output in a heap allocation of its
//     own with 64 guard bytes on both sides, the outputs pre-filled with 0xEE
//   ./a.out sweep libbcio.so
//     compares bcf_round's text with bcio_fmt_pyround_float (the library is loaded at run time) for
//     dp 0 .. 4 over: c / cov * 100 for 0 <= c <= cov <= 400; k / 2^j ties and their neighbours one ulp
//     away; decimal ties; 10^6 seeded random values in [0, 100] and in [0, 3]; +-0.0, -1e-4, 1e-300; and
//     checks that NaN, +-inf, 1e300 and a value that reaches 1e15 after scaling are declined
// input.bin:   u32 ncases, then per case { i32 k dp long ncols, i64 n stride n_seg names_bytes text_cap,
//              counts i32[ncols * stride], pc f64[k * stride], ent f64[stride], sec f64[stride],
//              segments (32 bytes each), names }
// results.bin: per case { u32 guards_ok, the 64-byte header, seg_off i64[n_seg + 1], text u8[text_cap] }
#include <dlfcn.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "bc_fmt.h"

namespace {
constexpr size_t kGuard = 64;
constexpr uint8_t kGuardByte = 0x5A, kFill = 0xEE;

struct Guarded {  // `bytes` usable bytes between two guards, its own allocation
    uint8_t* base = nullptr;
    size_t bytes = 0;
    explicit Guarded(size_t n, uint8_t fill = kFill) : bytes(n) {
        base = (uint8_t*)std::malloc(n + 2 * kGuard);
        if (!base) std::abort();
        std::memset(base, kGuardByte, n + 2 * kGuard);
        std::memset(base + kGuard, fill, n);
    }
    Guarded(const Guarded&) = delete;
    ~Guarded() { std::free(base); }
    uint8_t* data() { return base + kGuard; }
    template <class T>
    T* as() { return reinterpret_cast<T*>(base + kGuard); }
    bool intact() const {
        for (size_t i = 0; i < kGuard; ++i)
            if (base[i] != kGuardByte || base[kGuard + bytes + i] != kGuardByte) return false;
        return true;
    }
};

bool rd(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int run_cases(const char* fin, const char* fout) {
    FILE* in = std::fopen(fin, "rb");
    FILE* out = std::fopen(fout, "wb");
    if (!in || !out) return std::fprintf(stderr, "cannot open files\n"), 2;
    uint32_t ncases = 0;
    if (!rd(in, &ncases, 4)) return std::fprintf(stderr, "bad input file\n"), 2;
    for (uint32_t c = 0; c < ncases; ++c) {
        int32_t h4[4];
        int64_t h8[5];
        if (!rd(in, h4, sizeof h4) || !rd(in, h8, sizeof h8)) return std::fprintf(stderr, "bad case header\n"), 2;
        const int32_t k = h4[0], dp = h4[1], lg = h4[2], ncols = h4[3];
        const int64_t n = h8[0], stride = h8[1], n_seg = h8[2], names_bytes = h8[3], text_cap = h8[4];
        if (k < 5 || k > 6 || ncols < k || ncols > 6 || n < 0 || n > (1 << 24) || stride < n || stride > (1 << 24) ||
            n_seg < 1 || n_seg > (1 << 20) || names_bytes < 0 || names_bytes > (1 << 24) || text_cap < 0 ||
            text_cap > (1ll << 30))
            return std::fprintf(stderr, "bad case header\n"), 2;
        const size_t us = (size_t)stride;
        const size_t in_bytes[6] = {4 * us * (size_t)ncols, 8 * us * (size_t)k, 8 * us, 8 * us, 32 * (size_t)n_seg,
                                    (size_t)names_bytes};
        std::vector<std::unique_ptr<Guarded>> iv;
        for (size_t b : in_bytes) {
            iv.emplace_back(new Guarded(b, 0xA5));
            if (!rd(in, iv.back()->data(), b)) return std::fprintf(stderr, "short input file\n"), 2;
        }
        bcf_args a{};
        a.counts = iv[0]->as<int32_t>();
        a.pc = iv[1]->as<double>();
        a.ent = iv[2]->as<double>();
        a.sec = iv[3]->as<double>();
        a.stride = stride;
        a.n = n;
        a.segs = iv[4]->as<bcf_seg>();
        a.n_seg = n_seg;
        a.names = iv[5]->data();
        a.names_bytes = names_bytes;
        a.k = k;
        a.dp = dp;
        a.long_format = lg;
        Guarded work(bcf_work_bytes(n)), hdr(sizeof(bcf_header)), seg_off(8 * ((size_t)n_seg + 1)), text((size_t)text_cap);
        bcf_rows_host(a, work.data(), hdr.as<bcf_header>(), seg_off.as<int64_t>(), text.data(), text_cap);
        bool guards = work.intact() && hdr.intact() && seg_off.intact() && text.intact();
        for (auto& g : iv) guards &= g->intact();
        const uint32_t g32 = guards ? 1 : 0;
        std::fwrite(&g32, 4, 1, out);
        std::fwrite(hdr.data(), sizeof(bcf_header), 1, out);
        std::fwrite(seg_off.data(), 1, seg_off.bytes, out);
        if (text.bytes) std::fwrite(text.data(), 1, text.bytes, out);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("ok %u cases\n", ncases);
    return 0;
}

typedef int (*pyround_fn)(double, int, char*, int);

struct Sweep {
    pyround_fn ref;
    uint64_t checked = 0, bad = 0;
    void one(double x) {
        for (int dp = 0; dp <= BCF_MAX_DP; ++dp) {
            char want[512], got[64];
            const int nw = ref(x, dp, want, (int)sizeof want);
            const bcf_num r = bcf_round(x, dp);
            bcf_writer w;
            w.buf = (uint8_t*)got;
            w.base = 0;
            w.cap = sizeof got;
            w.at = 0;
            bcf_put_num(w, r);
            bcf_counter cn;
            cn.n = 0;
            bcf_put_num(cn, r);
            ++checked;
            if (!r.ok || nw < 0 || (uint32_t)nw != w.at || cn.n != w.at || std::memcmp(want, got, w.at) != 0) {
                if (bad++ < 20)
                    std::fprintf(stderr, "x=%.17g dp=%d: want %.*s got %.*s ok=%u\n", x, dp, nw > 0 ? nw : 0, want,
                                 (int)(w.at < sizeof got ? w.at : sizeof got), got, r.ok);
            }
        }
    }
    void around(double x) {
        one(x);
        one(std::nextafter(x, std::numeric_limits<double>::infinity()));
        one(std::nextafter(x, -std::numeric_limits<double>::infinity()));
        one(-x);
    }
    void declined(double x, int dp) {
        ++checked;
        if (bcf_round(x, dp).ok) {
            ++bad;
            std::fprintf(stderr, "x=%.17g dp=%d is not declined\n", x, dp);
        }
    }
};

int run_sweep(const char* libpath) {
    void* h = dlopen(libpath, RTLD_NOW | RTLD_LOCAL);
    if (!h) return std::fprintf(stderr, "cannot load %s: %s\n", libpath, dlerror()), 2;
    Sweep s;
    s.ref = (pyround_fn)dlsym(h, "bcio_fmt_pyround_float");
    if (!s.ref) return std::fprintf(stderr, "no bcio_fmt_pyround_float\n"), 2;
    for (int cov = 1; cov <= 400; ++cov)
        for (int c = 0; c <= cov; ++c) s.one((double)c / (double)cov * 100.0);
    for (int j = 0; j <= 14; ++j)
        for (int k = 0; k <= 4096; ++k) s.around((double)k / (double)(1 << j));
    for (int d = 1; d <= 5; ++d) {  // decimal ties: (i + 0.5) / 10^d as the nearest double and its neighbours
        double p10 = 1.0;
        for (int i = 0; i < d; ++i) p10 *= 10.0;
        for (int i = 0; i < 3000; ++i) s.around(((double)i + 0.5) / p10);
    }
    std::mt19937_64 rng(20260);
    std::uniform_real_distribution<double> u100(0.0, 100.0), u3(0.0, 3.0);
    for (int i = 0; i < 1000000; ++i) {
        s.one(u100(rng));
        s.one(u3(rng));
    }
    for (double x : {0.0, -0.0, -1e-4, 1e-4, 1e-300, -1e-300, 5e-324, 1e10, 123456789.12345, 9999999999.99994,
                     99999999999.5, 99999999999.99985})
        s.one(x);
    const double inf = std::numeric_limits<double>::infinity();
    for (int dp = 0; dp <= BCF_MAX_DP; ++dp) {
        s.declined(std::nan(""), dp);
        s.declined(inf, dp);
        s.declined(-inf, dp);
        s.declined(1e300, dp);
        s.declined(-1e300, dp);
        s.declined(1e15, dp);
    }
    s.declined(1e11, 4);
    s.declined(-1e12, 3);
    s.declined(999999999999999.5, 0);
    dlclose(h);
    if (s.bad) return std::fprintf(stderr, "%llu of %llu differ\n", (unsigned long long)s.bad, (unsigned long long)s.checked), 1;
    std::printf("ok %llu values\n", (unsigned long long)s.checked);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "cases")) return run_cases(argv[2], argv[3]);
    if (argc == 3 && !std::strcmp(argv[1], "sweep")) return run_sweep(argv[2]);
    return std::fprintf(stderr, "usage: fmt_check cases input.bin results.bin | fmt_check sweep libbcio.so\n"), 2;
}
