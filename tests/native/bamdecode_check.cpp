// Host check of the BAM record decoder (basecount_amd/csrc/bc_bam.h), the header the device kernels
// compile too: speculation, stitch, repair and fill as plain loops over the same functions.
// Decodes one buffer of inflated BAM bytes under several configurations, each input and every
// output array in a heap allocation with 64 guard bytes on both sides, and writes the arrays.
//   g++ -fsanitize=address,undefined -I basecount_amd/csrc tests/native/bamdecode_check.cpp
//   ./a.out input.bin results.bin
// input.bin:   u64 raw_bytes, u64 first, i32 n_refs, u32 ncfg, raw bytes,
//              ncfg x { u32 seg_bytes (0 = default), i64 max_records (< 0 = no limit), u32 trunc
//              (bytes dropped from the buffer's end), u32 final, u32 want_qual }
// results.bin: per configuration { u32 guards_ok, i32 status, u64 err_off, i64 n, u64 cigar_words,
//              u64 seq_bytes, i64 repaired, i64 batches, u64 used } and the arrays of all batches
//              concatenated: tid pos flag mapq l_seq qstart qend rec_err ref_span cig_off[n+1]
//              seq_off[n+1] cigar seq seq_event[seq_bytes] and, with want_qual, qual[2 seq_bytes]
// A configuration with a record limit takes kLimited batches at that limit (the first from the whole
// buffer at `first`, each later one from a copy of the carried bytes at offset 0) and the rest in one.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bc_bam.h"

namespace {
constexpr size_t kGuard = 64;
constexpr uint8_t kGuardByte = 0x5A, kFill = 0xEE;
constexpr int kLimited = 32;
constexpr uint32_t kDefaultSeg = 65536;

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

template <class T>
void append(std::vector<uint8_t>& v, const T* p, size_t n) {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(p);
    v.insert(v.end(), b, b + n * sizeof(T));
}

struct All {
    std::vector<uint8_t> tid, pos, flag, mapq, l_seq, qstart, qend, rec_err, ref_span, cigar, seq, seq_event, qual;
    std::vector<uint64_t> cig_off{0}, seq_off{0};
};

bool rd(FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return std::fprintf(stderr, "usage: bamdecode_check input.bin results.bin\n"), 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return std::fprintf(stderr, "cannot open files\n"), 2;
    uint64_t raw_bytes = 0, first = 0;
    int32_t n_refs = 0;
    uint32_t ncfg = 0;
    if (!rd(in, &raw_bytes, 8) || !rd(in, &first, 8) || !rd(in, &n_refs, 4) || !rd(in, &ncfg, 4) || raw_bytes > (1u << 28))
        return std::fprintf(stderr, "bad input file\n"), 2;
    std::vector<uint8_t> raw(raw_bytes);
    if (raw_bytes && !rd(in, raw.data(), raw_bytes)) return std::fprintf(stderr, "short input file\n"), 2;
    for (uint32_t c = 0; c < ncfg; ++c) {
        uint32_t seg = 0, trunc = 0, final = 0, want_qual = 0;
        int64_t max_records = 0;
        if (!rd(in, &seg, 4) || !rd(in, &max_records, 8) || !rd(in, &trunc, 4) || !rd(in, &final, 4) || !rd(in, &want_qual, 4) ||
            trunc > raw_bytes)
            return std::fprintf(stderr, "bad configuration\n"), 2;
        if (seg == 0) seg = kDefaultSeg;
        const uint64_t N = raw_bytes - trunc;
        All all;
        bool guards = true;
        int32_t status = 0;
        uint64_t err_off = 0, used = first, cig_tot = 0, seq_tot = 0;
        int64_t n_tot = 0, repaired = 0, batches = 0;
        for (uint64_t base = 0, q = first; q <= N;) {
            // the batch's bytes: the whole buffer for the first, then the carried bytes alone
            const uint64_t nb = N - base;
            Guarded buf(nb, 0xA5);
            if (nb) std::memcpy(buf.data(), raw.data() + base, nb);
            const int64_t limit = (max_records < 0 || batches >= kLimited) ? INT64_MAX : max_records;
            const bcb_layout l = bcb_make_layout(nb, seg);
            Guarded work(l.total);
            bcb_index_host(buf.data(), nb, q - base, limit, final != 0, n_refs, seg, work.data());
            const bcb_result res = *work.as<bcb_result>();
            guards &= buf.intact() && work.intact();
            ++batches;
            repaired += res.repaired;
            if (res.status != BCB_ST_OK) {
                status = res.status;
                err_off = base + res.err_off;
                break;
            }
            const size_t n = (size_t)res.n, cw = res.cigar_words, sb = res.seq_bytes;
            Guarded tid(4 * n), pos(4 * n), flag(2 * n), mapq(n), l_seq(4 * n), qstart(4 * n), qend(4 * n), rec_err(4 * n),
                ref_span(8 * n), cig_off(8 * (n + 1)), seq_off(8 * (n + 1)), cigar(4 * cw), seq(sb),
                seq_event(bcb_seq_event_bytes(sb)), qual(2 * sb);
            bcb_arrays o;
            o.tid = tid.as<int32_t>();
            o.pos = pos.as<int32_t>();
            o.flag = flag.as<uint16_t>();
            o.mapq = mapq.data();
            o.l_seq = l_seq.as<int32_t>();
            o.qstart = qstart.as<int32_t>();
            o.qend = qend.as<int32_t>();
            o.rec_err = rec_err.as<uint32_t>();
            o.ref_span = ref_span.as<int64_t>();
            o.cig_off = cig_off.as<uint64_t>();
            o.seq_off = seq_off.as<uint64_t>();
            o.cigar = cigar.as<uint32_t>();
            o.seq = seq.data();
            o.seq_event = seq_event.data();
            o.qual = qual.data();
            o.n_cap = res.n;
            o.cigar_cap = cw;
            o.seq_cap = sb;
            bcb_fill_host(buf.data(), work.data(), o, want_qual != 0);
            for (Guarded* g : {&buf, &work, &tid, &pos, &flag, &mapq, &l_seq, &qstart, &qend, &rec_err, &ref_span, &cig_off,
                               &seq_off, &cigar, &seq, &seq_event, &qual})
                guards &= g->intact();
            for (uint64_t j = sb; j < seq_event.bytes; ++j) guards &= seq_event.data()[j] == 0;  // the zero tail
            if (!want_qual)
                for (uint64_t j = 0; j < qual.bytes; ++j) guards &= qual.data()[j] == kFill;  // not asked for: not written
            append(all.tid, o.tid, n);
            append(all.pos, o.pos, n);
            append(all.flag, o.flag, n);
            append(all.mapq, o.mapq, n);
            append(all.l_seq, o.l_seq, n);
            append(all.qstart, o.qstart, n);
            append(all.qend, o.qend, n);
            append(all.rec_err, o.rec_err, n);
            append(all.ref_span, o.ref_span, n);
            append(all.cigar, o.cigar, cw);
            append(all.seq, o.seq, sb);
            append(all.seq_event, o.seq_event, sb);
            if (want_qual) append(all.qual, o.qual, 2 * sb);
            guards &= o.cig_off[0] == 0 && o.seq_off[0] == 0;
            for (size_t i = 1; i <= n; ++i) {
                all.cig_off.push_back(cig_tot + o.cig_off[i]);
                all.seq_off.push_back(seq_tot + o.seq_off[i]);
            }
            n_tot += res.n;
            cig_tot += cw;
            seq_tot += sb;
            used = base + res.used;
            if (res.n == 0 || used >= N) break;
            base = q = used;
        }
        const uint32_t g = guards ? 1 : 0;
        std::fwrite(&g, 4, 1, out);
        std::fwrite(&status, 4, 1, out);
        std::fwrite(&err_off, 8, 1, out);
        std::fwrite(&n_tot, 8, 1, out);
        std::fwrite(&cig_tot, 8, 1, out);
        std::fwrite(&seq_tot, 8, 1, out);
        std::fwrite(&repaired, 8, 1, out);
        std::fwrite(&batches, 8, 1, out);
        std::fwrite(&used, 8, 1, out);
        for (const std::vector<uint8_t>* v : {&all.tid, &all.pos, &all.flag, &all.mapq, &all.l_seq, &all.qstart, &all.qend,
                                              &all.rec_err, &all.ref_span})
            if (!v->empty()) std::fwrite(v->data(), 1, v->size(), out);
        std::fwrite(all.cig_off.data(), 8, all.cig_off.size(), out);
        std::fwrite(all.seq_off.data(), 8, all.seq_off.size(), out);
        for (const std::vector<uint8_t>* v : {&all.cigar, &all.seq, &all.seq_event, &all.qual})
            if (!v->empty()) std::fwrite(v->data(), 1, v->size(), out);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("ok %u configurations\n", ncfg);
    return 0;
}
