// bc_capi.hip — extern "C" boundary (include/basecount_hip.h).  Host-side glue only: argument
// checks, stream/memory management, launch geometry; every count/stat is computed by the
// kernels in bc_kernels.hip.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "bc_cohort.h"
#include "bc_internal.h"
#include "bc_ops_plan.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& m) {
    g_err = m;
    return code;
}

int hip_fail(hipError_t e, const char* where) {
    return fail(BC_E_HIP, std::string(where) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t _e = (expr);                         \
        if (_e != hipSuccess) return hip_fail(_e, #expr); \
    } while (0)

// hipEvents around one launch when the context's timing is on
struct Timed {
    bc_ctx* c;
    int id;
    hipEvent_t a = nullptr, b = nullptr;
    Timed(bc_ctx* ctx, int kid) : c(ctx), id(kid) {
        if (c->timing && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess)
            (void)hipEventRecord(a, c->stream);
    }
    ~Timed() {
        if (a && b) {
            (void)hipEventRecord(b, c->stream);
            c->ev[id].emplace_back(a, b);
        }
    }
};

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Kernel 1 of the deep / long-span paths (use_rc): the read-chunked k_rc, or under BC_SHAPE_OPS
// the scan-expanded k_ops (timed as BC_K_COUNT), atomics into `counts`
hipError_t launch_chunked(bc_ctx* c, const bc_reads& r, int64_t L, uint32_t mbq, int k, int32_t* counts) {
    if (c->shape == BC_SHAPE_OPS) {
        Timed tm(c, BC_K_COUNT);
        struct bc_ops_plan plan;
        bc::ops_plan(r, L, c->reads_per_block, c->ops_passes, plan);
        return bc::launch_ops(c->stream, r, L, mbq, k, counts, c->d_err, plan);
    }
    Timed tm(c, BC_K_RC);
    return bc::launch_rc(c->stream, r, L, mbq, k, counts, c->d_err);
}

// Reads per kernel-1 workgroup: enough workgroups to fill 256 CUs several times over, and few
// enough reads per chunk that a sorted chunk's positions fit one LDS window.
int choose_rpb(int64_t n, int64_t L, int max_span, int sorted, int forced) {
    if (forced > 0) return std::min(forced, 32768);
    int64_t target = std::min<int64_t>(8192, std::max<int64_t>(32, n / 2048));
    if (!sorted || max_span <= 0 || max_span >= bc::kWinMax || L <= 0) return (int)target;
    const double density = (double)n / (double)L;
    const double fit = (bc::kWinMax - max_span) * density * 0.75;
    if (fit >= 32.0) return (int)std::min<double>((double)target, fit);
    return (int)target;  // sparse: chunks take the global-atomic path
}

bool host_sorted(const int32_t* pos, int64_t n) {
    for (int64_t i = 1; i < n; ++i)
        if (pos[i] < pos[i - 1]) return false;
    return true;
}

// max reference span and max read end (pos + span) of a host batch
std::pair<int, int64_t> host_spans(const bc_reads& r) {
    uint64_t best = 0;
    int64_t end = 0;
    for (int64_t i = 0; i < r.n_reads; ++i) {
        const uint32_t* cg = r.cigar + r.cig_beg[i];
        uint64_t span = 0;
        for (uint32_t k = 0; k < r.cig_n[i]; ++k) {
            uint32_t op = cg[k] & 15u;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += cg[k] >> 4;
        }
        best = std::max(best, span);
        end = std::max<int64_t>(end, (int64_t)r.pos[i] + (int64_t)span);
    }
    return {(int)std::min<uint64_t>(best, 0x7fffffff), end};
}

// BC_INDEX_AUTO resolved for this context: the run records when the read-chunked kernel would
// take the batch, else the tile index when the tiled one would (the sparse sweep uses neither)
int index_what(const bc_ctx* c, const bc_reads& r, int64_t L, int what = BC_INDEX_AUTO) {
    if (!(what & BC_INDEX_AUTO)) return what & (BC_INDEX_RUNS | BC_INDEX_TILES);
    if (!r.sorted || r.n_reads <= 0 || r.seq_layout != BC_SEQ_EVENT) return 0;
    if (c->shape == BC_SHAPE_OPS) return 0;  // k_ops reads no index
    if (bc::use_rc(r, L, c->shape)) return BC_INDEX_RUNS;
    return bc::pileup_is_solo(r, L, c->shape, c->tile_waves) ? 0 : BC_INDEX_TILES;
}

int check_host_reads(const bc_reads* r) {
    if (!r) return fail(BC_E_ARG, "reads is NULL");
    if (r->n_reads < 0) return fail(BC_E_ARG, "n_reads < 0");
    if (r->n_reads == 0) return BC_OK;
    if (!r->pos || !r->cig_beg || !r->cig_n || !r->seq_nib) return fail(BC_E_ARG, "missing per-read array");
    for (int64_t i = 0; i < r->n_reads; ++i) {
        if ((uint64_t)r->cig_beg[i] + r->cig_n[i] > (uint64_t)r->n_cigar_words)
            return fail(BC_E_ARG, "read " + std::to_string(i) + ": CIGAR outside the cigar buffer");
        if (r->pos[i] < 0) return fail(BC_E_ARG, "read " + std::to_string(i) + ": negative start");
        // query consumption must stay inside the packed sequence (and quality) buffers
        uint64_t q = 0;
        const uint32_t* cg = r->cigar + r->cig_beg[i];
        for (uint32_t k = 0; k < r->cig_n[i]; ++k) {
            uint32_t op = cg[k] & 15u;
            if (op == 0 || op == 1 || op == 7 || op == 8) q += cg[k] >> 4;
        }
        if (q && (uint64_t)r->seq_nib[i] + q > 2ull * (uint64_t)r->seq_bytes)
            return fail(BC_E_ARG, "read " + std::to_string(i) + ": CIGAR consumes past the sequence");
        if (q && r->qual && (uint64_t)r->seq_nib[i] + q > (uint64_t)r->qual_bytes)
            return fail(BC_E_ARG, "read " + std::to_string(i) + ": CIGAR consumes past the qualities");
    }
    return BC_OK;
}

// refPos the reference's .at() rejects first for read i (host walk in count.cpp:40-96 order)
int64_t host_bad_pos(const bc_reads& r, int64_t i, int64_t ref_len, uint32_t mbq) {
    static const int col_of[16] = {-1, 0, 1, -1, 2, -1, -1, -1, 3, -1, -1, -1, -1, -1, -1, 5};
    int64_t rp = r.pos[i];
    uint64_t qp = r.seq_nib[i];
    const uint32_t* cg = r.cigar + r.cig_beg[i];
    for (uint32_t k = 0; k < r.cig_n[i]; ++k) {
        uint32_t op = cg[k] & 15u, len = cg[k] >> 4;
        if (op == 0 || op == 7 || op == 8) {
            for (uint32_t j = 0; j < len; ++j, ++rp, ++qp) {
                if (r.qual && r.qual[qp] < mbq) continue;
                if (!r.qual && mbq > 0) continue;
                unsigned b = r.seq[qp >> 1];
                unsigned nib = (qp & 1) ? (b & 15u) : (b >> 4);
                if (col_of[nib] >= 0 && rp >= ref_len) return rp;
            }
        } else if (op == 1) {
            qp += len;
        } else if (op == 2 || op == 3) {
            for (uint32_t j = 0; j < len; ++j, ++rp)
                if (rp >= ref_len) return rp;
        }
    }
    return -1;
}

}  // namespace

namespace bc {
int set_error(int code, const std::string& m) { return fail(code, m); }
}  // namespace bc

extern "C" {

const char* bc_last_error(void) { return g_err.c_str(); }
int bc_abi_version(void) { return BC_ABI_VERSION; }

const char* bc_build_info(void) {
    return "gfx950"
#ifdef BC_DIAG
           " diag=1"
#else
           " diag=0"
#endif
#ifdef BC_PHASE_TRACE
           " phase_trace=1"
#else
           " phase_trace=0"
#endif
        ;
}

int bc_device_count(int* n) {
    if (!n) return fail(BC_E_ARG, "n is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *n = (e == hipSuccess) ? c : 0;
    return BC_OK;
}

int bc_ctx_create(int device, void* stream, bc_ctx** out) {
    if (!out) return fail(BC_E_ARG, "out is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(BC_E_NODEV, "no HIP device visible");
    if (device < 0 || device >= n) return fail(BC_E_ARG, "device index out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(BC_E_NODEV, std::string("built for gfx950, device is ") + prop.gcnArchName);
    DeviceGuard g(device);
    auto* c = new bc_ctx();
    c->device = device;
    if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete c;
            return hip_fail(e, "hipStreamCreate");
        }
        c->own_stream = true;
    }
    hipError_t e = hipMalloc(&c->d_err, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->sig, hipEventDisableTiming);
    if (e == hipSuccess) e = hipHostMalloc(&c->h_err, sizeof(unsigned long long), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemsetAsync(c->d_err, 0xFF, sizeof(unsigned long long), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        bc_ctx_destroy(c);
        return hip_fail(e, "context scratch");
    }
    *out = c;
    return BC_OK;
}

int bc_ctx_destroy(bc_ctx* c) {
    if (!c) return BC_OK;
    DeviceGuard g(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->d_err) (void)hipFree(c->d_err);
    if (c->rc_scratch) (void)hipFree(c->rc_scratch);
    if (c->out_scratch) (void)hipFree(c->out_scratch);
    if (c->sum_scratch) (void)hipFree(c->sum_scratch);
    for (void* p : c->z_buf)
        if (p) (void)hipFree(p);
    for (auto& e : c->z_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->h_err) (void)hipHostFree(c->h_err);
    for (auto& v : c->ev)
        for (auto& pr : v) {
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
    for (auto& e : c->mark)
        if (e) (void)hipEventDestroy(e);
    if (c->sig) (void)hipEventDestroy(c->sig);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return BC_OK;
}

int bc_ctx_release_scratch(bc_ctx* c) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    DeviceGuard g(c->device);
    std::lock_guard<std::mutex> zlock(c->z_mutex);
    if (c->rc_scratch || c->out_scratch || c->sum_scratch || c->z_buf[0] || c->z_buf[1] || c->z_buf[2] || c->z_buf[3])
        HIP_TRY(hipStreamSynchronize(c->stream));
    // one buffer at a time: its pointer and size are cleared whether or not its free succeeded,
    // so no later call frees it twice; the first error is returned after all three
    hipError_t first = hipSuccess;
    const char* where = nullptr;
    auto drop = [&](void*& p, size_t& bytes, const char* what) {
        if (p) {
            const hipError_t e = hipFree(p);
            if (e != hipSuccess && first == hipSuccess) first = e, where = what;
        }
        p = nullptr;
        bytes = 0;
    };
    void* rc = c->rc_scratch;
    drop(rc, c->rc_scratch_bytes, "hipFree(rc_scratch)");
    c->rc_scratch = nullptr;
    drop(c->out_scratch, c->out_scratch_bytes, "hipFree(out_scratch)");
    drop(c->sum_scratch, c->sum_scratch_bytes, "hipFree(sum_scratch)");
    for (int i = 0; i < 4; ++i) drop(c->z_buf[i], c->z_bytes[i], "hipFree(inflate scratch)");
    if (first != hipSuccess) return hip_fail(first, where);
    return BC_OK;
}

// ---- BGZF inflate (bc_inflate.hip) ----
static_assert(sizeof(bc_zblock) == 24, "bc_zblock is 24 bytes (bcio_zblock has the same layout)");

int bc_bgzf_inflate(bc_ctx* c, const uint8_t* d_comp, uint64_t comp_bytes, const bc_zblock* d_blocks, int64_t n,
                    uint8_t* d_out, uint64_t out_bytes, uint8_t* d_status) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail(BC_E_ARG, "bc_bgzf_inflate: n must be 0 .. 2^31 - 1");
    if (!d_comp || !d_blocks || !d_out || !d_status) return fail(BC_E_ARG, "bc_bgzf_inflate: NULL pointer");
    if (n == 0) return BC_OK;
    DeviceGuard g(c->device);
    HIP_TRY(bc::launch_inflate(c->stream, d_comp, comp_bytes, d_blocks, n, d_out, out_bytes, d_status));
    return BC_OK;
}

// grow-only device buffer i of the inflate scratch (the stream is idle between slices)
static int z_reserve(bc_ctx* c, int i, size_t need) {
    if (c->z_bytes[i] >= need) return BC_OK;
    if (c->z_buf[i]) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipFree(c->z_buf[i]));
        c->z_buf[i] = nullptr;
        c->z_bytes[i] = 0;
    }
    const size_t cap = need + need / 4 + 256;
    HIP_TRY(hipMalloc(&c->z_buf[i], cap));
    c->z_bytes[i] = cap;
    return BC_OK;
}

int bc_bgzf_inflate_host(void* ctx, const uint8_t* h_comp, uint64_t comp_bytes, const bc_zblock* h_blocks, int64_t n,
                         uint8_t* h_out, uint64_t out_bytes, uint8_t* h_status) {
    bc_ctx* c = static_cast<bc_ctx*>(ctx);
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (n < 0) return fail(BC_E_ARG, "bc_bgzf_inflate_host: n < 0");
    if (!h_comp || !h_blocks || !h_out || !h_status) return fail(BC_E_ARG, "bc_bgzf_inflate_host: NULL pointer");
    if (n == 0) return BC_OK;
    std::lock_guard<std::mutex> lock(c->z_mutex);
    DeviceGuard g(c->device);
    for (auto& e : c->z_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    // slices of bounded inflated size: a fill may ask for gigabytes.  One wave per block and the
    // kernel is latency-bound per wave, so a slice must hold at least the 8192 blocks (512 MiB) a
    // 256-CU device keeps resident, or the slices' kernels run one after the other part-empty
    constexpr uint64_t kSliceBytes = 512ull << 20;
    constexpr int64_t kSliceBlocks = 1 << 16;
    std::vector<bc_zblock> dev;
    for (int64_t b0 = 0; b0 < n;) {
        // the slice's blocks, those the host can already refuse left out; device offsets: the
        // compressed span [cmin, cmax) as it lies in the file, the output packed densely
        dev.clear();
        uint64_t cmin = UINT64_MAX, cmax = 0, dense = 0;
        int64_t b1 = b0;
        for (; b1 < n && b1 - b0 < kSliceBlocks && dense < kSliceBytes; ++b1) {
            const bc_zblock& z = h_blocks[b1];
            bc_zblock d = z;
            if (z.isize > 65536u || z.coff > comp_bytes || z.clen > comp_bytes - z.coff || z.uoff > out_bytes ||
                z.isize > out_bytes - z.uoff) {
                d.coff = UINT64_MAX;  // refused by the kernel's own check as well (status BC_Z_DESC)
                d.clen = 0;
                d.isize = 0;  // takes no room in the slice
            } else {
                cmin = std::min(cmin, z.coff);
                cmax = std::max(cmax, z.coff + z.clen);
            }
            d.uoff = dense;
            dense += d.isize;
            dev.push_back(d);
        }
        const int64_t m = b1 - b0;
        if (cmin > cmax) cmin = cmax = 0;
        for (auto& d : dev)
            if (d.coff != UINT64_MAX) d.coff -= cmin;
        const uint64_t span = cmax - cmin;
        int rc;
        if ((rc = z_reserve(c, 0, span + 16)) != BC_OK || (rc = z_reserve(c, 1, (size_t)m * sizeof(bc_zblock))) != BC_OK ||
            (rc = z_reserve(c, 2, dense + 16)) != BC_OK || (rc = z_reserve(c, 3, (size_t)m)) != BC_OK)
            return rc;
        uint8_t* d_comp = static_cast<uint8_t*>(c->z_buf[0]);
        bc_zblock* d_blocks = static_cast<bc_zblock*>(c->z_buf[1]);
        uint8_t* d_out = static_cast<uint8_t*>(c->z_buf[2]);
        uint8_t* d_status = static_cast<uint8_t*>(c->z_buf[3]);
        HIP_TRY(hipEventRecord(c->z_ev[0], c->stream));
        if (span) HIP_TRY(hipMemcpyAsync(d_comp, h_comp + cmin, span, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_blocks, dev.data(), (size_t)m * sizeof(bc_zblock), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipEventRecord(c->z_ev[1], c->stream));
        HIP_TRY(bc::launch_inflate(c->stream, d_comp, span, d_blocks, m, d_out, dense, d_status));
        HIP_TRY(hipEventRecord(c->z_ev[2], c->stream));
        HIP_TRY(hipMemcpyAsync(h_status + b0, d_status, (size_t)m, hipMemcpyDeviceToHost, c->stream));
        // each run of blocks that lie back to back in h_out comes down as one copy
        for (int64_t i = 0; i < m;) {
            int64_t j = i;
            uint64_t bytes = 0;
            while (j < m && dev[j].coff != UINT64_MAX &&
                   h_blocks[b0 + j].uoff == h_blocks[b0 + i].uoff + bytes) {
                bytes += dev[j].isize;
                ++j;
            }
            if (bytes)
                HIP_TRY(hipMemcpyAsync(h_out + h_blocks[b0 + i].uoff, d_out + dev[i].uoff, bytes, hipMemcpyDeviceToHost,
                                       c->stream));
            i = j > i ? j : i + 1;
        }
        HIP_TRY(hipEventRecord(c->z_ev[3], c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (int k = 0; k < 3; ++k) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, c->z_ev[k], c->z_ev[k + 1]) == hipSuccess) c->z_ms[k] += ms;
        }
        c->z_blocks += m;
        b0 = b1;
    }
    return BC_OK;
}

int bc_bgzf_inflate_host_times(bc_ctx* c, double* ms, int64_t* blocks) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> lock(c->z_mutex);
    if (ms)
        for (int k = 0; k < 3; ++k) ms[k] = c->z_ms[k];
    if (blocks) *blocks = c->z_blocks;
    return BC_OK;
}

// ---- BAM record decode (bc_bam.hip) ----
static_assert(sizeof(bc_bam_batch) == 80, "bc_bam_batch is bc_bam.h's bcb_result");

static int bam_seg_bytes(uint32_t seg_bytes, uint32_t* out) {
    if (seg_bytes == 0) seg_bytes = BC_BAM_SEG_DEFAULT;
    if (seg_bytes < 64u || seg_bytes > (1u << 24)) return fail(BC_E_ARG, "bc_bam: seg_bytes must be 0 or 64 .. 2^24");
    *out = seg_bytes;
    return BC_OK;
}

int bc_bam_index_bytes(uint64_t raw_bytes, uint32_t seg_bytes, size_t* bytes) {
    if (!bytes) return fail(BC_E_ARG, "bc_bam_index_bytes: bytes is NULL");
    uint32_t seg = 0;
    if (int rc = bam_seg_bytes(seg_bytes, &seg)) return rc;
    // a fill too large for the device is declined by bc_bam_index and needs the header only
    *bytes = raw_bytes > 0x7FFFFFFFull ? 128 : bc::bam_index_bytes(raw_bytes, seg);
    return BC_OK;
}

int bc_bam_index(bc_ctx* c, const uint8_t* d_raw, uint64_t raw_bytes, uint64_t first, int64_t max_records, int final,
                 int32_t n_refs, uint32_t seg_bytes, void* d_work, size_t work_bytes, bc_bam_batch* h_out) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (!d_raw || !d_work || !h_out) return fail(BC_E_ARG, "bc_bam_index: NULL pointer");
    if (first > raw_bytes) return fail(BC_E_ARG, "bc_bam_index: first is past raw_bytes");
    if (max_records < 0) return fail(BC_E_ARG, "bc_bam_index: max_records < 0");
    if (n_refs < 0) return fail(BC_E_ARG, "bc_bam_index: n_refs < 0");
    uint32_t seg = 0;
    if (int rc = bam_seg_bytes(seg_bytes, &seg)) return rc;
    size_t need = 0;
    (void)bc_bam_index_bytes(raw_bytes, seg, &need);
    if (work_bytes < need) return fail(BC_E_ARG, "bc_bam_index: d_work smaller than bc_bam_index_bytes");
    if ((uintptr_t)d_work & 15u) return fail(BC_E_ARG, "bc_bam_index: d_work must be 16-byte aligned");
    if (raw_bytes > 0x7FFFFFFFull) {  // declined without touching the device
        *h_out = bc_bam_batch{};
        h_out->status = BC_BAM_TOO_LARGE;
        h_out->used = h_out->err_off = first;
        h_out->raw_bytes = raw_bytes;
        h_out->seg_bytes = seg;
        return BC_OK;
    }
    DeviceGuard g(c->device);
    HIP_TRY(bc::launch_bam_index(c->stream, d_raw, (uint32_t)raw_bytes, seg, (uint32_t)first, max_records, final != 0,
                                 n_refs, d_work));
    HIP_TRY(hipMemcpyAsync(h_out, d_work, sizeof *h_out, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BC_OK;
}

int bc_bam_fill(bc_ctx* c, const uint8_t* d_raw, const void* d_work, const bc_bam_batch* b, const bc_bam_arrays* o,
                int want_qual) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (!d_raw || !d_work || !b || !o) return fail(BC_E_ARG, "bc_bam_fill: NULL pointer");
    if (b->status != BC_BAM_OK) return fail(BC_E_ARG, "bc_bam_fill: the fill was declined (decode it on the host)");
    if (b->n < 0 || b->raw_bytes > 0x7FFFFFFFull || b->seg_bytes < 64u || b->seg_bytes > (1u << 24))
        return fail(BC_E_ARG, "bc_bam_fill: h_batch is not a bc_bam_index result");
    if (o->n_cap < b->n || o->cigar_cap < b->cigar_words || o->seq_cap < b->seq_bytes)
        return fail(BC_E_ARG, "bc_bam_fill: the arrays are smaller than the batch");
    if (!o->tid || !o->pos || !o->flag || !o->mapq || !o->l_seq || !o->qstart || !o->qend || !o->rec_err ||
        !o->ref_span || !o->cig_off || !o->seq_off || !o->seq_event || (b->cigar_words && !o->cigar))
        return fail(BC_E_ARG, "bc_bam_fill: missing output array");
    if (want_qual && !o->qual) return fail(BC_E_ARG, "bc_bam_fill: want_qual needs a qual array");
    DeviceGuard g(c->device);
    HIP_TRY(bc::launch_bam_fill(c->stream, d_raw, (uint32_t)b->raw_bytes, (uint32_t)b->seg_bytes, d_work, *o,
                                want_qual != 0));
    return BC_OK;
}

// ---- the stream decoder: fills in, batches out, the inflated bytes stay in HBM ----
struct bc_bam_decoder {
    bc_ctx* c = nullptr;
    bool want_qual = false;
    uint32_t seg = 0;
    uint8_t* pend = nullptr;  // inflated bytes; [beg, end) not handed out yet
    uint64_t beg = 0, end = 0;
    void* work = nullptr;
    size_t work_cap = 0;
    hipEvent_t ev[4] = {};
    int64_t repaired = 0, declined = 0;
    double ms[7] = {};
};

namespace {

struct BamHandle {
    bc_bam_arrays arrays{};
    void* slab = nullptr;
    std::vector<uint8_t> meta;  // the per-record arrays on the host
};

constexpr size_t kBamAlign = 256;
size_t bam_up(size_t v) { return (v + kBamAlign - 1) / kBamAlign * kBamAlign; }

// host wall time of one decoder call into ms[slot]
struct BamWall {
    bc_bam_decoder* d;
    int slot;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~BamWall() { d->ms[slot] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

void bam_elapsed(bc_bam_decoder* d, int slot, int a, int b) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, d->ev[a], d->ev[b]) == hipSuccess) d->ms[slot] += t;
}

}  // namespace

int bc_bam_decoder_create(bc_ctx* c, int want_qual, uint32_t seg_bytes, bc_bam_decoder** out) {
    if (!c || !out) return fail(BC_E_ARG, "bc_bam_decoder_create: NULL argument");
    uint32_t seg = 0;
    if (int rc = bam_seg_bytes(seg_bytes, &seg)) return rc;
    DeviceGuard g(c->device);
    auto* d = new bc_bam_decoder();
    d->c = c;
    d->want_qual = want_qual != 0;
    d->seg = seg;
    for (auto& e : d->ev) {
        hipError_t err = hipEventCreate(&e);
        if (err != hipSuccess) {
            (void)bc_bam_decoder_destroy(d);
            return hip_fail(err, "hipEventCreate");
        }
    }
    *out = d;
    return BC_OK;
}

int bc_bam_decoder_destroy(bc_bam_decoder* d) {
    if (!d) return fail(BC_E_ARG, "decoder is NULL");
    DeviceGuard g(d->c->device);
    (void)hipStreamSynchronize(d->c->stream);
    if (d->pend) (void)hipFree(d->pend);
    if (d->work) (void)hipFree(d->work);
    for (auto& e : d->ev)
        if (e) (void)hipEventDestroy(e);
    delete d;
    return BC_OK;
}

int bc_bam_decoder_fill(void* user, int append, const uint8_t* h_carry, uint64_t carry_bytes, const uint8_t* h_comp,
                        uint64_t comp_bytes, const bc_zblock* h_blocks, int64_t n, uint64_t inflated) {
    auto* d = static_cast<bc_bam_decoder*>(user);
    if (!d) return fail(BC_E_ARG, "decoder is NULL");
    if (n < 0 || (n > 0 && (!h_comp || !h_blocks)) || (!append && carry_bytes && !h_carry))
        return fail(BC_E_ARG, "bc_bam_decoder_fill: bad argument");
    bc_ctx* c = d->c;
    BamWall wall{d, 5};
    const uint64_t keep = append ? d->end - d->beg : carry_bytes;
    if (keep + inflated > 0x7FFFFFFFull) return (++d->declined, 1);  // 32-bit offsets on the device
    // the descriptors for the device: the compressed span as it lies in the file, the output behind
    // the kept bytes; one the host can already refuse declines the fill
    std::vector<bc_zblock> dev((size_t)n);
    uint64_t cmin = UINT64_MAX, cmax = 0;
    for (int64_t i = 0; i < n; ++i) {
        const bc_zblock& z = h_blocks[i];
        if (z.isize > 65536u || z.coff > comp_bytes || z.clen > comp_bytes - z.coff || z.uoff > inflated ||
            z.isize > inflated - z.uoff)
            return (++d->declined, 1);
        cmin = std::min(cmin, z.coff);
        cmax = std::max(cmax, z.coff + z.clen);
        dev[(size_t)i] = z;
    }
    if (cmin > cmax) cmin = cmax = 0;
    for (auto& z : dev) {
        z.coff -= cmin;
        z.uoff += keep;
    }
    const uint64_t span = cmax - cmin, total = keep + inflated;
    std::lock_guard<std::mutex> lock(c->z_mutex);
    DeviceGuard g(c->device);
    int rc;
    if ((rc = z_reserve(c, 0, span + 16)) != BC_OK || (rc = z_reserve(c, 1, (size_t)n * sizeof(bc_zblock) + 16)) != BC_OK ||
        (rc = z_reserve(c, 3, (size_t)n + 16)) != BC_OK)
        return rc;
    uint8_t* nb = nullptr;
    HIP_TRY(hipMalloc((void**)&nb, total + 64));
    std::vector<uint8_t> status((size_t)n, 1);
    hipError_t e = hipEventRecord(d->ev[0], c->stream);
    if (e == hipSuccess && keep)
        e = append ? hipMemcpyAsync(nb, d->pend + d->beg, keep, hipMemcpyDeviceToDevice, c->stream)
                   : hipMemcpyAsync(nb, h_carry, keep, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && span) e = hipMemcpyAsync(c->z_buf[0], h_comp + cmin, span, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && n)
        e = hipMemcpyAsync(c->z_buf[1], dev.data(), (size_t)n * sizeof(bc_zblock), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipEventRecord(d->ev[1], c->stream);
    if (e == hipSuccess)
        e = bc::launch_inflate(c->stream, static_cast<uint8_t*>(c->z_buf[0]), span, static_cast<bc_zblock*>(c->z_buf[1]), n,
                               nb, total, static_cast<uint8_t*>(c->z_buf[3]));
    if (e == hipSuccess) e = hipEventRecord(d->ev[2], c->stream);
    if (e == hipSuccess && n) e = hipMemcpyAsync(status.data(), c->z_buf[3], (size_t)n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipEventRecord(d->ev[3], c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipFree(nb);
        return hip_fail(e, "bc_bam_decoder_fill");
    }
    bam_elapsed(d, 0, 0, 1);
    bam_elapsed(d, 1, 1, 2);
    bam_elapsed(d, 4, 2, 3);
    for (uint8_t st : status)
        if (st != 0) {  // a block k_inflate refuses: the host inflates and decodes this fill
            (void)hipFree(nb);
            return (++d->declined, 1);
        }
    if (d->pend) (void)hipFree(d->pend);
    d->pend = nb;
    d->beg = 0;
    d->end = total;
    return BC_OK;
}

int bc_bam_decoder_next(void* user, int64_t max_records, int final, int32_t n_refs, bc_bam_host_batch* out) {
    auto* d = static_cast<bc_bam_decoder*>(user);
    if (!d || !out) return fail(BC_E_ARG, "bc_bam_decoder_next: NULL argument");
    if (max_records < 0 || n_refs < 0) return fail(BC_E_ARG, "bc_bam_decoder_next: negative argument");
    *out = bc_bam_host_batch{};
    bc_ctx* c = d->c;
    BamWall wall{d, 6};
    const uint64_t N = d->end - d->beg;
    if (!d->pend || N == 0) return final ? 0 : 1;
    DeviceGuard g(c->device);
    size_t need = 0;
    if (int rc = bc_bam_index_bytes(N, d->seg, &need)) return rc;
    if (need > d->work_cap) {
        if (d->work) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(hipFree(d->work));
            d->work = nullptr;
            d->work_cap = 0;
        }
        HIP_TRY(hipMalloc(&d->work, need + need / 4));
        d->work_cap = need + need / 4;
    }
    const uint8_t* raw = d->pend + d->beg;
    bc_bam_batch b{};
    HIP_TRY(hipEventRecord(d->ev[0], c->stream));
    if (int rc = bc_bam_index(c, raw, N, 0, max_records, final, n_refs, d->seg, d->work, d->work_cap, &b)) return rc;
    HIP_TRY(hipEventRecord(d->ev[1], c->stream));
    HIP_TRY(hipEventSynchronize(d->ev[1]));
    bam_elapsed(d, 2, 0, 1);
    d->repaired += b.repaired;
    if (b.status != BC_BAM_OK) return (++d->declined, 2);
    out->n = b.n;
    if (!final && b.n < max_records) return 1;  // more bytes first; nothing consumed
    if (b.n == 0) return 0;
    // one allocation: the per-record arrays in front (one download), then the batch's bytes
    const size_t n = (size_t)b.n, cw = (size_t)b.cigar_words, sb = (size_t)b.seq_bytes;
    const size_t sizes[15] = {4 * n, 4 * n, 2 * n, n, 4 * n, 4 * n, 4 * n, 4 * n, 8 * n, 8 * (n + 1), 8 * (n + 1),
                              4 * cw, sb, bc::seq_event_bytes((int64_t)sb), d->want_qual ? 2 * sb : 0};
    size_t off[16] = {0};
    for (int i = 0; i < 15; ++i) off[i + 1] = off[i] + bam_up(sizes[i]);
    auto h = std::make_unique<BamHandle>();
    HIP_TRY(hipMalloc(&h->slab, off[15] + kBamAlign));
    uint8_t* p = static_cast<uint8_t*>(h->slab);
    bc_bam_arrays& a = h->arrays;
    a.tid = (int32_t*)(p + off[0]);
    a.pos = (int32_t*)(p + off[1]);
    a.flag = (uint16_t*)(p + off[2]);
    a.mapq = p + off[3];
    a.l_seq = (int32_t*)(p + off[4]);
    a.qstart = (int32_t*)(p + off[5]);
    a.qend = (int32_t*)(p + off[6]);
    a.rec_err = (uint32_t*)(p + off[7]);
    a.ref_span = (int64_t*)(p + off[8]);
    a.cig_off = (uint64_t*)(p + off[9]);
    a.seq_off = (uint64_t*)(p + off[10]);
    a.cigar = (uint32_t*)(p + off[11]);
    a.seq = p + off[12];
    a.seq_event = p + off[13];
    a.qual = d->want_qual ? p + off[14] : nullptr;
    a.n_cap = b.n;
    a.cigar_cap = b.cigar_words;
    a.seq_cap = b.seq_bytes;
    h->meta.resize(off[11]);
    hipError_t e = hipEventRecord(d->ev[1], c->stream);
    int rc = BC_OK;
    if (e == hipSuccess) rc = bc_bam_fill(c, raw, d->work, &b, &a, d->want_qual ? 1 : 0);
    if (rc == BC_OK && e == hipSuccess) e = hipEventRecord(d->ev[2], c->stream);
    if (rc == BC_OK && e == hipSuccess) e = hipMemcpyAsync(h->meta.data(), p, off[11], hipMemcpyDeviceToHost, c->stream);
    if (rc == BC_OK && e == hipSuccess) e = hipEventRecord(d->ev[3], c->stream);
    if (rc == BC_OK && e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (rc != BC_OK || e != hipSuccess) {
        (void)hipFree(h->slab);
        return rc != BC_OK ? rc : hip_fail(e, "bc_bam_decoder_next");
    }
    bam_elapsed(d, 3, 1, 2);
    bam_elapsed(d, 4, 2, 3);
    const uint8_t* m = h->meta.data();
    out->used = b.used;
    out->cigar_words = b.cigar_words;
    out->seq_bytes = b.seq_bytes;
    out->tid = (const int32_t*)(m + off[0]);
    out->pos = (const int32_t*)(m + off[1]);
    out->flag = (const uint16_t*)(m + off[2]);
    out->mapq = m + off[3];
    out->l_seq = (const int32_t*)(m + off[4]);
    out->qstart = (const int32_t*)(m + off[5]);
    out->qend = (const int32_t*)(m + off[6]);
    out->rec_err = (const uint32_t*)(m + off[7]);
    out->ref_span = (const int64_t*)(m + off[8]);
    out->cig_off = (const uint64_t*)(m + off[9]);
    out->seq_off = (const uint64_t*)(m + off[10]);
    d->beg += b.used;
    out->handle = h.release();
    return 0;
}

int bc_bam_decoder_pending(void* user, uint8_t* h_dst, uint64_t* bytes) {
    auto* d = static_cast<bc_bam_decoder*>(user);
    if (!d || !bytes) return fail(BC_E_ARG, "bc_bam_decoder_pending: NULL argument");
    *bytes = d->end - d->beg;
    if (!h_dst) return BC_OK;
    DeviceGuard g(d->c->device);
    if (*bytes) {
        HIP_TRY(hipMemcpyAsync(h_dst, d->pend + d->beg, *bytes, hipMemcpyDeviceToHost, d->c->stream));
        HIP_TRY(hipStreamSynchronize(d->c->stream));
    }
    if (d->pend) (void)hipFree(d->pend);
    d->pend = nullptr;
    d->beg = d->end = 0;
    return BC_OK;
}

int bc_bam_decoder_drop(bc_bam_decoder* d) {
    if (!d) return fail(BC_E_ARG, "decoder is NULL");
    DeviceGuard g(d->c->device);
    if (d->pend) HIP_TRY(hipFree(d->pend));
    d->pend = nullptr;
    d->beg = d->end = 0;
    return BC_OK;
}

void bc_bam_decoder_release(void* user, void* handle) {
    auto* d = static_cast<bc_bam_decoder*>(user);
    auto* h = static_cast<BamHandle*>(handle);
    if (!h) return;
    if (d) {
        DeviceGuard g(d->c->device);
        if (h->slab) (void)hipFree(h->slab);
    }
    delete h;
}

int bc_bam_batch_arrays(const void* handle, bc_bam_arrays* out) {
    if (!handle || !out) return fail(BC_E_ARG, "bc_bam_batch_arrays: NULL argument");
    *out = static_cast<const BamHandle*>(handle)->arrays;
    return BC_OK;
}

int bc_bam_decoder_stats(bc_bam_decoder* d, int64_t* repaired, int64_t* declined, double* ms) {
    if (!d) return fail(BC_E_ARG, "decoder is NULL");
    if (repaired) *repaired = d->repaired;
    if (declined) *declined = d->declined;
    if (ms)
        for (int k = 0; k < 7; ++k) ms[k] = d->ms[k];
    return BC_OK;
}

// ---- read selection on the device (bc_select.hip) ----
int bc_bam_select_bytes(int64_t n, int64_t n_refs, size_t* bytes) {
    if (!bytes) return fail(BC_E_ARG, "bc_bam_select_bytes: bytes is NULL");
    if (n < 0 || n_refs < 0) return fail(BC_E_ARG, "bc_bam_select_bytes: negative n or n_refs");
    if (n > 0x7FFFFFFFll - 1) return fail(BC_E_ARG, "bc_bam_select_bytes: n must be below 2^31");
    *bytes = bc::select_bytes(n, n_refs);
    return BC_OK;
}

int bc_bam_select(bc_ctx* c, const bc_bam_arrays* r, int64_t n, int64_t min_mapq, const uint8_t* d_ref_sel,
                  const int64_t* d_ref_len, int32_t n_refs, void* d_work, size_t work_bytes, const bc_sel_arrays* o) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (!r || !d_ref_sel || !d_ref_len || !d_work || !o) return fail(BC_E_ARG, "bc_bam_select: NULL pointer");
    if (n < 0 || n_refs < 0) return fail(BC_E_ARG, "bc_bam_select: negative n or n_refs");
    if (n > 0x7FFFFFFFll - 1) return fail(BC_E_ARG, "bc_bam_select: n must be below 2^31");
    if (!r->tid || !r->pos || !r->flag || !r->mapq || !r->qstart || !r->qend || !r->rec_err || !r->ref_span ||
        !r->cig_off || !r->seq_off)
        return fail(BC_E_ARG, "bc_bam_select: NULL pointer among the record arrays");
    if (!o->pos || !o->cig_beg || !o->cig_n || !o->seq_nib || !o->qlen || !o->span || !o->rec || !o->ordinal ||
        !o->ref_beg || !o->max_span || !o->max_end || !o->n_reads || !o->n_complex || !o->sum_ops || !o->err_or ||
        !o->flags || !o->header)
        return fail(BC_E_ARG, "bc_bam_select: NULL pointer among the output arrays");
    if (r->n_cap < n) return fail(BC_E_ARG, "bc_bam_select: the record arrays hold fewer than n records");
    if (o->n_cap < n || o->ref_cap < n_refs) return fail(BC_E_ARG, "bc_bam_select: the output arrays are smaller than n / n_refs");
    if (work_bytes < bc::select_bytes(n, n_refs)) return fail(BC_E_ARG, "bc_bam_select: d_work smaller than bc_bam_select_bytes");
    if ((uintptr_t)d_work & 15u) return fail(BC_E_ARG, "bc_bam_select: d_work must be 16-byte aligned");
    DeviceGuard g(c->device);
    HIP_TRY(bc::launch_select(c->stream, *r, n, min_mapq, d_ref_sel, d_ref_len, n_refs, d_work, *o));
    return BC_OK;
}

// ---- row formatting on the device (bc_fmt.hip) ----
namespace {
const char* fmt_size_error(int64_t n, int64_t n_seg) {
    if (n < 0 || n_seg < 0) return "negative n or n_seg";
    if (n > 0x7FFFFFFFll) return "n must be below 2^31";
    if (n_seg < 1) return "n_seg must be at least 1";
    if (n_seg > 0x7FFFFFFFll) return "n_seg must be below 2^31";
    return nullptr;
}
}  // namespace

int bc_fmt_rows_bytes(int64_t n, int64_t n_seg, size_t* work_bytes, size_t* out_small_bytes) {
    if (!work_bytes || !out_small_bytes) return fail(BC_E_ARG, "bc_fmt_rows_bytes: NULL pointer");
    if (const char* m = fmt_size_error(n, n_seg)) return fail(BC_E_ARG, std::string("bc_fmt_rows_bytes: ") + m);
    *work_bytes = bc::fmt_work_bytes(n);
    *out_small_bytes = 64u + 8u * ((size_t)n_seg + 1u);
    return BC_OK;
}

int bc_fmt_rows(bc_ctx* c, const bc_fmt_args* a, void* d_work, size_t work_bytes, void* d_out, uint8_t* d_text,
                int64_t text_cap) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (!a || !d_work || !d_out || !d_text) return fail(BC_E_ARG, "bc_fmt_rows: NULL pointer");
    if (!a->counts || !a->pc || !a->ent || !a->sec || !a->segs || !a->names)
        return fail(BC_E_ARG, "bc_fmt_rows: NULL pointer among the arguments' arrays");
    if (a->k != 5 && a->k != 6) return fail(BC_E_ARG, "bc_fmt_rows: k must be 5 or 6");
    if (a->dp < 0 || a->dp > 4) return fail(BC_E_ARG, "bc_fmt_rows: dp must lie in [0, 4]");
    if (const char* m = fmt_size_error(a->n, a->n_seg)) return fail(BC_E_ARG, std::string("bc_fmt_rows: ") + m);
    if (a->names_bytes < 0 || text_cap < 0) return fail(BC_E_ARG, "bc_fmt_rows: negative names_bytes or text_cap");
    if (a->stride < a->n) return fail(BC_E_ARG, "bc_fmt_rows: stride must be at least n");
    if (work_bytes < bc::fmt_work_bytes(a->n)) return fail(BC_E_ARG, "bc_fmt_rows: d_work smaller than bc_fmt_rows_bytes");
    if (((uintptr_t)d_work | (uintptr_t)d_out) & 7u) return fail(BC_E_ARG, "bc_fmt_rows: d_work and d_out must be 8-byte aligned");
    DeviceGuard g(c->device);
    HIP_TRY(bc::launch_fmt_rows(c->stream, *a, d_work, d_out, d_text, text_cap));
    return BC_OK;
}

// ---- BGZF deflate on the device (bc_deflate.hip) ----
namespace {
const char* dfl_size_error(int64_t text_cap, int64_t n_spans) {
    if (text_cap < 0 || n_spans < 0) return "negative text_cap or n_spans";
    if (text_cap >= (1ll << 40)) return "text_cap must be below 2^40";
    if (n_spans < 1) return "n_spans must be at least 1";
    if (n_spans > 0x7FFFFFFFll) return "n_spans must be below 2^31";
    return nullptr;
}
}  // namespace

int bc_bgzf_deflate_bytes(int64_t text_cap, int64_t n_spans, size_t* work_bytes, size_t* out_small_bytes) {
    if (!work_bytes || !out_small_bytes) return fail(BC_E_ARG, "bc_bgzf_deflate_bytes: NULL pointer");
    if (const char* m = dfl_size_error(text_cap, n_spans)) return fail(BC_E_ARG, std::string("bc_bgzf_deflate_bytes: ") + m);
    *work_bytes = bc::deflate_work_bytes(text_cap, n_spans);
    *out_small_bytes = 64u + 8u * ((size_t)n_spans + 1u);
    return BC_OK;
}

int bc_bgzf_deflate(bc_ctx* c, const uint8_t* d_text, int64_t text_cap, const int64_t* d_span_off, int64_t n_spans,
                    const int32_t* d_gate, void* d_work, size_t work_bytes, void* d_out_small, uint8_t* d_comp,
                    int64_t comp_cap) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (!d_text || !d_span_off || !d_work || !d_out_small || !d_comp) return fail(BC_E_ARG, "bc_bgzf_deflate: NULL pointer");
    if (const char* m = dfl_size_error(text_cap, n_spans)) return fail(BC_E_ARG, std::string("bc_bgzf_deflate: ") + m);
    if (comp_cap < 0) return fail(BC_E_ARG, "bc_bgzf_deflate: negative comp_cap");
    if (work_bytes < bc::deflate_work_bytes(text_cap, n_spans))
        return fail(BC_E_ARG, "bc_bgzf_deflate: d_work smaller than bc_bgzf_deflate_bytes");
    if ((uintptr_t)d_work & 15u) return fail(BC_E_ARG, "bc_bgzf_deflate: d_work must be 16-byte aligned");
    if (((uintptr_t)d_span_off | (uintptr_t)d_out_small) & 7u)
        return fail(BC_E_ARG, "bc_bgzf_deflate: d_span_off and d_out_small must be 8-byte aligned");
    if ((uintptr_t)d_gate & 3u) return fail(BC_E_ARG, "bc_bgzf_deflate: d_gate must be 4-byte aligned");
    DeviceGuard g(c->device);
    HIP_TRY(bc::launch_deflate(c->stream, d_text, text_cap, d_span_off, n_spans, d_gate, d_work, d_out_small, d_comp, comp_cap));
    return BC_OK;
}

int bc_bgzf_deflate_host(const uint8_t* h_text, const int64_t* h_span_off, int64_t n_spans, uint8_t* h_comp,
                         int64_t comp_cap, int64_t* span_coff, int64_t* total, int nthreads) {
    if (!h_text || !h_span_off || !h_comp || !span_coff || !total) return fail(BC_E_ARG, "bc_bgzf_deflate_host: NULL pointer");
    if (n_spans < 1 || n_spans > 0x7FFFFFFFll || comp_cap < 0) return fail(BC_E_ARG, "bc_bgzf_deflate_host: n_spans < 1 or negative comp_cap");
    return bc::deflate_host(h_text, h_span_off, n_spans, h_comp, comp_cap, span_coff, total, nthreads);
}

int bc_ctx_stream(bc_ctx* c, void** s) {
    if (!c || !s) return fail(BC_E_ARG, "NULL argument");
    *s = (void*)c->stream;
    return BC_OK;
}

int bc_ctx_set_shape(bc_ctx* c, int shape, int tile_waves, int rpb) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (shape < BC_SHAPE_AUTO || shape > BC_SHAPE_OPS) return fail(BC_E_ARG, "unknown BC_SHAPE_* value");
    if (tile_waves != 0 && tile_waves != 1 && tile_waves != 2 && tile_waves != 4 && tile_waves != 8)
        return fail(BC_E_ARG, "tile_waves must be 0, 1, 2, 4 or 8");
    if (rpb < 0 || rpb > 32768) return fail(BC_E_ARG, "reads_per_block must be 0..32768");
    c->shape = shape;
    c->tile_waves = tile_waves;
    c->reads_per_block = rpb;
    return BC_OK;
}

int bc_pileup_plan(const bc_reads* r, int64_t ref_len, int shape, int tile_waves, bc_plan* out) {
    if (!r || !out) return fail(BC_E_ARG, "NULL argument");
    if (r->n_reads < 0 || ref_len < 0) return fail(BC_E_ARG, "bc_pileup_plan: n_reads or ref_len < 0");
    if (shape < BC_SHAPE_AUTO || shape > BC_SHAPE_OPS) return fail(BC_E_ARG, "unknown BC_SHAPE_* value");
    if (tile_waves != 0 && tile_waves != 1 && tile_waves != 2 && tile_waves != 4 && tile_waves != 8)
        return fail(BC_E_ARG, "tile_waves must be 0, 1, 2, 4 or 8");
    bc::pileup_plan(*r, ref_len, shape, tile_waves, *out);
    return BC_OK;
}

int bc_ops_plan(const bc_reads* r, int64_t ref_len, int rpb, int passes, struct bc_ops_plan* out) {
    if (!r || !out) return fail(BC_E_ARG, "NULL argument");
    if (r->n_reads < 0 || ref_len < 0) return fail(BC_E_ARG, "bc_ops_plan: n_reads or ref_len < 0");
    if (rpb < 0) return fail(BC_E_ARG, "reads_per_block must be >= 0");
    if (passes < 0 || passes > BC_OPS_PASSES_MAX) return fail(BC_E_ARG, "passes must be 0..BC_OPS_PASSES_MAX");
    bc::ops_plan(*r, ref_len, rpb, passes, *out);
    return BC_OK;
}

int bc_ctx_set_ops_passes(bc_ctx* c, int passes) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (passes < 0 || passes > BC_OPS_PASSES_MAX) return fail(BC_E_ARG, "passes must be 0..BC_OPS_PASSES_MAX");
    c->ops_passes = passes;
    return BC_OK;
}

int bc_ctx_set_instance(bc_ctx* c, int instance) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (instance != BC_INSTANCE_AUTO && instance != BC_INSTANCE_GENERAL && instance != BC_INSTANCE_LEAN &&
        instance != BC_INSTANCE_SLICE)
        return fail(BC_E_ARG, "unknown BC_INSTANCE_* value");
    c->instance = instance;
    return BC_OK;
}

int bc_pileup_launch_info(const bc_reads* r, int64_t ref_len, int shape, int tile_waves, int instance, uint32_t mbq,
                          int k, bc_launch_info* out) {
    if (!r || !out) return fail(BC_E_ARG, "NULL argument");
    if (r->n_reads < 0 || ref_len < 0) return fail(BC_E_ARG, "bc_pileup_launch_info: n_reads or ref_len < 0");
    if (shape < BC_SHAPE_AUTO || shape > BC_SHAPE_OPS) return fail(BC_E_ARG, "unknown BC_SHAPE_* value");
    if (tile_waves != 0 && tile_waves != 1 && tile_waves != 2 && tile_waves != 4 && tile_waves != 8)
        return fail(BC_E_ARG, "tile_waves must be 0, 1, 2, 4 or 8");
    if (instance != BC_INSTANCE_AUTO && instance != BC_INSTANCE_GENERAL && instance != BC_INSTANCE_LEAN &&
        instance != BC_INSTANCE_SLICE)
        return fail(BC_E_ARG, "unknown BC_INSTANCE_* value");
    if (k != 5 && k != 6) return fail(BC_E_ARG, "k must be 5 or 6");
    bc::pileup_launch_info(*r, ref_len, shape, tile_waves, instance, mbq, k, *out);
    return BC_OK;
}

int bc_sync(bc_ctx* c) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    DeviceGuard g(c->device);
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BC_OK;
}

int bc_malloc(bc_ctx* c, size_t bytes, void** p) {
    if (!c || !p) return fail(BC_E_ARG, "NULL argument");
    DeviceGuard g(c->device);
    *p = nullptr;
    if (bytes == 0) bytes = 16;
    HIP_TRY(hipMalloc(p, bytes));
    return BC_OK;
}

int bc_free(bc_ctx* c, void* p) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (!p) return BC_OK;
    DeviceGuard g(c->device);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipFree(p));
    return BC_OK;
}

int bc_memcpy_h2d(bc_ctx* c, void* d, const void* h, size_t bytes) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (!bytes) return BC_OK;
    DeviceGuard g(c->device);
    HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    return BC_OK;
}

int bc_memcpy_d2h(bc_ctx* c, void* h, const void* d, size_t bytes) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (!bytes) return BC_OK;
    DeviceGuard g(c->device);
    HIP_TRY(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
    return BC_OK;
}

int bc_memset(bc_ctx* c, void* d, int v, size_t bytes) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (!bytes) return BC_OK;
    DeviceGuard g(c->device);
    HIP_TRY(hipMemsetAsync(d, v, bytes, c->stream));
    return BC_OK;
}

int bc_reads_upload(bc_ctx* c, const bc_reads* h, bc_reads* d) {
    if (!c || !d) return fail(BC_E_ARG, "NULL argument");
    int rc = check_host_reads(h);
    if (rc) return rc;
    DeviceGuard g(c->device);
    std::memset(d, 0, sizeof *d);
    d->n_reads = h->n_reads;
    d->n_cigar_words = h->n_cigar_words;
    d->seq_bytes = h->seq_bytes;
    d->qual_bytes = h->qual ? h->qual_bytes : 0;
    // the tiled kernel relies on both properties: always derive them from the data itself
    d->sorted = h->n_reads ? (host_sorted(h->pos, h->n_reads) ? 1 : 0) : 1;
    const auto sp = h->n_reads ? host_spans(*h) : std::pair<int, int64_t>(0, 0);
    d->max_span = sp.first;
    d->max_end = sp.second;
    if (h->seq_layout != BC_SEQ_BAM && h->seq_layout != BC_SEQ_EVENT)
        return fail(BC_E_ARG, "bc_reads_upload: unknown seq_layout");
    // BC_SEQ_EVENT from the host (the decoder's bcio_records.seq_event): a plain copy, no device
    // conversion pass; BC_SEQ_BAM is converted in place by k_seq_event after the copy
    const bool host_event = h->seq_layout == BC_SEQ_EVENT;
    const size_t n = (size_t)h->n_reads;
    // the batch's device index (bc_index.hip), built on the device after the copies: run
    // records + chunk summaries when the read-chunked kernel would take the batch, else the tile
    // index when the tiled one would (nothing for the sparse sweep)
    d->seq_layout = BC_SEQ_EVENT;  // (the device copy's layout, whatever the host's)
    const int what = index_what(c, *d, d->max_end);
    const bc::IndexPlan plan = bc::index_plan(*d, what);
    constexpr int kArr = 8;
    void* p[kArr] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // the sequence buffer is sized for BC_SEQ_EVENT (converted in place after the copy)
    const size_t sz[kArr] = {n * 4, n * 4, n * 4, n * 4, (size_t)h->n_cigar_words * 4,
                             bc::seq_event_bytes(h->seq_bytes), h->qual ? (size_t)h->qual_bytes : 0, plan.total};
    const size_t cp[kArr] = {sz[0], sz[1], sz[2], sz[3], sz[4], (size_t)h->seq_bytes, sz[6], 0};
    const void* src[kArr] = {h->pos, h->cig_beg, h->cig_n, h->seq_nib, h->cigar, h->seq, h->qual, nullptr};
    // ONE slab for the whole batch (arrays 4 KiB-aligned inside it, the slab a multiple of 2 MiB):
    // the kernels' first touches of a batch then miss the GPU TLB on a few large fragments
    // instead of on every small buffer's pages.  The first array present is the slab base
    // (bc_reads_free).
    size_t off[kArr], total = 0;
    for (int i = 0; i < kArr; ++i) {
        off[i] = total;
        total += (sz[i] + 4095) / 4096 * 4096;
    }
    total = (total + (2u << 20) - 1) / (2u << 20) * (2u << 20);
    void* slab = nullptr;
    HIP_TRY(hipMalloc(&slab, total));
    for (int i = 0; i < kArr; ++i) {
        if (!sz[i]) continue;
        p[i] = (uint8_t*)slab + off[i];
        hipError_t e = cp[i] ? hipMemcpyAsync(p[i], src[i], cp[i], hipMemcpyHostToDevice, c->stream) : hipSuccess;
        if (e == hipSuccess && i == 5) {
            if (host_event)  // zero padding past the copied bytes
                e = hipMemsetAsync((uint8_t*)p[5] + cp[5], 0, sz[5] - cp[5], c->stream);
            else
                e = bc::launch_seq_event(c->stream, (const uint8_t*)p[5], h->seq_bytes, (uint8_t*)p[5]);
        }
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(c->stream);
            (void)hipFree(slab);
            return hip_fail(e, "bc_reads_upload");
        }
    }
    d->pos = (const int32_t*)p[0];
    d->cig_beg = (const uint32_t*)p[1];
    d->cig_n = (const uint32_t*)p[2];
    d->seq_nib = (const uint32_t*)p[3];
    d->cigar = (const uint32_t*)p[4];
    d->seq = (const uint8_t*)p[5];
    d->qual = (const uint8_t*)p[6];
    d->seq_layout = BC_SEQ_EVENT;
    if (plan.total) {
        Timed tm(c, BC_K_INDEX);
        hipError_t e = bc::launch_index(c->stream, *d, plan, p[7]);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(c->stream);
            (void)hipFree(slab);
            std::memset(d, 0, sizeof *d);
            return hip_fail(e, "bc_reads_upload: index");
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BC_OK;
}

int bc_reads_index_bytes(bc_ctx* c, const bc_reads* r, int64_t L, int what, size_t* bytes) {
    if (!c || !r || !bytes) return fail(BC_E_ARG, "NULL argument");
    if (what & ~(BC_INDEX_RUNS | BC_INDEX_TILES | BC_INDEX_AUTO)) return fail(BC_E_ARG, "unknown BC_INDEX_* bits");
    *bytes = bc::index_plan(*r, index_what(c, *r, L, what)).total;
    return BC_OK;
}

int bc_reads_index(bc_ctx* c, bc_reads* r, int64_t L, int what, void* d_mem, size_t bytes) {
    if (!c || !r) return fail(BC_E_ARG, "NULL argument");
    if (what & ~(BC_INDEX_RUNS | BC_INDEX_TILES | BC_INDEX_AUTO)) return fail(BC_E_ARG, "unknown BC_INDEX_* bits");
    r->read_runs = nullptr;
    r->run_chunks = 0;
    r->tile_reads = nullptr;
    r->n_tiles = 0;
    r->index_tag = 0;
    const bc::IndexPlan plan = bc::index_plan(*r, index_what(c, *r, L, what));
    if (!plan.total) return BC_OK;
    if (!d_mem || bytes < plan.total) return fail(BC_E_ARG, "bc_reads_index: d_mem smaller than bc_reads_index_bytes");
    if ((uintptr_t)d_mem & 15u) return fail(BC_E_ARG, "bc_reads_index: d_mem must be 16-byte aligned");
    if (!r->pos || !r->cig_beg || !r->cig_n || !r->seq_nib || (r->n_cigar_words > 0 && !r->cigar))
        return fail(BC_E_ARG, "bc_reads_index: missing per-read array");
    DeviceGuard g(c->device);
    Timed tm(c, BC_K_INDEX);
    HIP_TRY(bc::launch_index(c->stream, *r, plan, d_mem));
    return BC_OK;
}

// The sort leaves the sequence in place (sorts the fields + run records only) when the sorted
// batch will take the read-chunked k_rc, which gathers a chunk's scattered reads into LDS itself;
// batches with qualities (a quality threshold: k_rc's variants that stage through registers) and
// the tiled kernels' shallower batches get the sequence copied into start order.
static bool sort_fields_only(const bc_ctx* c, const bc_reads& r) {
    if (r.qual) return false;
    bc_reads v = r;
    v.sorted = 1;
    return bc::use_rc(v, r.max_end, c->shape);
}

int bc_reads_sort_bytes(bc_ctx* c, const bc_reads* r, size_t* bytes) {
    if (!c || !r || !bytes) return fail(BC_E_ARG, "NULL argument");
    *bytes = bc::sort_bytes(*r, sort_fields_only(c, *r));
    return BC_OK;
}

int bc_reads_sort(bc_ctx* c, const bc_reads* r, bc_reads* out, void* d_mem, size_t bytes) {
    if (!c || !r || !out) return fail(BC_E_ARG, "NULL argument");
    if (r->n_reads < 0 || r->max_end < 0) return fail(BC_E_ARG, "bc_reads_sort: negative n_reads / max_end");
    if (r->n_reads >= (int64_t)0xFFFFFFFF) return fail(BC_E_ARG, "bc_reads_sort: more than 2^32 - 1 reads");
    if (r->n_reads == 0) {
        *out = *r;
        out->sorted = 1;
        return BC_OK;
    }
    if (r->seq_layout != BC_SEQ_EVENT) return fail(BC_E_ARG, "bc_reads_sort needs seq_layout == BC_SEQ_EVENT");
    if (!r->pos || !r->cig_beg || !r->cig_n || !r->seq_nib || !r->seq) return fail(BC_E_ARG, "bc_reads_sort: missing array");
    const bool fields = sort_fields_only(c, *r);
    const size_t need = bc::sort_bytes(*r, fields);
    if (!d_mem || bytes < need) return fail(BC_E_ARG, "bc_reads_sort: d_mem smaller than bc_reads_sort_bytes");
    if ((uintptr_t)d_mem & 255u) return fail(BC_E_ARG, "bc_reads_sort: d_mem must be 256-byte aligned");
    if (!bc::sort_fits(*r))
        return fail(BC_E_ARG, "bc_reads_sort: batch too large to sort (seq_bytes + 5 n_reads + 16 > 0x55555550): "
                              "split it");
    DeviceGuard g(c->device);
    bc_reads tmp;
    {
        Timed tm(c, BC_K_SORT);
        HIP_TRY(bc::launch_sort(c->stream, *r, tmp, d_mem, fields));
    }
    *out = tmp;
    return BC_OK;
}

int bc_reads_sort_check(bc_ctx* c, const bc_reads* r, const void* d_mem) {
    if (!c || !r) return fail(BC_E_ARG, "NULL argument");
    if (r->n_reads <= 0) return BC_OK;
    if (!d_mem) return fail(BC_E_ARG, "bc_reads_sort_check: d_mem is NULL");
    DeviceGuard g(c->device);
    HIP_TRY(hipMemcpyAsync(c->h_err, bc::sort_flags_word(*r, d_mem), 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint32_t flags = (uint32_t)(*c->h_err & 0xFFFFFFFFu);
    if (flags & 2u) return fail(BC_E_ARG, "bc_reads_sort: a read starts outside [0, max_end] (max_end not truthful)");
    if (flags & 1u) return fail(BC_E_ARG, "bc_reads_sort: the reads' sequences overlap (sorted copy would not fit)");
    return BC_OK;
}

int bc_reads_free(bc_ctx* c, bc_reads* d) {
    if (!c || !d) return fail(BC_E_ARG, "NULL argument");
    DeviceGuard g(c->device);
    (void)hipStreamSynchronize(c->stream);
    const void* p[9] = {d->pos, d->cig_beg, d->cig_n, d->seq_nib, d->cigar, d->seq, d->qual, d->read_runs, d->tile_reads};
    for (auto q : p)  // the first array present is the base of the batch's slab (bc_reads_upload)
        if (q) {
            (void)hipFree((void*)q);
            break;
        }
    std::memset(d, 0, sizeof *d);
    return BC_OK;
}

int bc_count(bc_ctx* c, const bc_reads* r, int64_t ref_len, uint32_t mbq, int ncols, int32_t* d_hist) {
    if (!c || !r) return fail(BC_E_ARG, "NULL argument");
    if (ncols != 5 && ncols != 6) return fail(BC_E_ARG, "ncols must be 5 or 6");
    if (ref_len < 0) return fail(BC_E_ARG, "ref_len < 0");
    if (r->n_reads == 0) return BC_OK;
    if (!d_hist && ref_len > 0) return fail(BC_E_ARG, "d_hist is NULL");
    if (mbq > 0 && !r->qual) return fail(BC_E_ARG, "min_base_quality > 0 needs qualities");
    DeviceGuard g(c->device);
    const bool event = r->seq_layout == BC_SEQ_EVENT && !((uintptr_t)r->seq & 15u);
    if (c->shape == BC_SHAPE_OPS && r->seq_layout == BC_SEQ_EVENT) {
        // k_ops reads bases one by one: sorted or not, any sequence alignment
        HIP_TRY(launch_chunked(c, *r, ref_len, mbq, ncols, d_hist));
        return BC_OK;
    }
    if (r->sorted && event && bc::use_rc(*r, ref_len, c->shape)) {
        HIP_TRY(launch_chunked(c, *r, ref_len, mbq, ncols, d_hist));
        return BC_OK;
    }
    if (r->sorted && r->max_span <= bc::kTileMaxSpan && event) {
        // sorted batch: the tiled kernel in accumulate mode (plain read-add-write per owned tile)
        Timed tm(c, bc::pileup_is_solo(*r, ref_len, c->shape, c->tile_waves) ? BC_K_SOLO : BC_K_PILEUP);
        HIP_TRY(bc::launch_pileup_tiles(c->stream, *r, ref_len, r->max_end, mbq, ncols, false, true, 0.0, 0.0,
                                        d_hist, nullptr, nullptr, nullptr, nullptr, c->d_err, c->shape,
                                        c->tile_waves, c->instance));
        return BC_OK;
    }
    const int rpb = choose_rpb(r->n_reads, ref_len, r->max_span, r->sorted, c->reads_per_block);
    Timed tm(c, BC_K_COUNT);
    HIP_TRY(bc::launch_count(c->stream, *r, ref_len, mbq, ncols, d_hist, rpb, c->d_err));
    return BC_OK;
}

int bc_pileup(bc_ctx* c, const bc_reads* r, int64_t L, uint32_t mbq, int k, double nf, double nf2, int32_t* d_counts,
              int32_t* d_cov, double* d_pc, double* d_ent, double* d_sec) {
    if (!c || !r) return fail(BC_E_ARG, "NULL argument");
    if (k != 5 && k != 6) return fail(BC_E_ARG, "k must be 5 or 6");
    if (L < 0) return fail(BC_E_ARG, "ref_len < 0");
    if (!r->sorted) return fail(BC_E_ARG, "bc_pileup needs a coordinate-sorted batch (sorted == 1)");
    if (mbq > 0 && r->n_reads > 0 && !r->qual) return fail(BC_E_ARG, "min_base_quality > 0 needs qualities");
    if (r->n_reads > 0 && r->seq_layout != BC_SEQ_EVENT)
        return fail(BC_E_ARG, "bc_pileup needs seq_layout == BC_SEQ_EVENT (see bc_seq_to_event)");
    if (r->n_reads > 0 && ((uintptr_t)r->seq & 15u))
        return fail(BC_E_ARG, "bc_pileup needs a 16-byte aligned sequence buffer");
    if (L > 0 && (!d_counts || !d_cov || !d_ent || !d_sec)) return fail(BC_E_ARG, "NULL output");
    DeviceGuard g(c->device);
    if (bc::use_rc(*r, L, c->shape)) {
        // deep batch: counts by the read-chunked kernel (atomics into the context's zeroed
        // scratch), then kernel 2, which also moves the counts to d_counts and re-zeroes the
        // scratch (no memset launch per call)
        const size_t need = (size_t)k * (size_t)L * 4;
        if (need > c->rc_scratch_bytes) {
            if (c->rc_scratch) {
                HIP_TRY(hipStreamSynchronize(c->stream));
                HIP_TRY(hipFree(c->rc_scratch));
                c->rc_scratch = nullptr;
                c->rc_scratch_bytes = 0;
            }
            HIP_TRY(hipMalloc((void**)&c->rc_scratch, need));
            c->rc_scratch_bytes = need;
            HIP_TRY(hipMemsetAsync(c->rc_scratch, 0, need, c->stream));
        }
        HIP_TRY(launch_chunked(c, *r, L, mbq, k, c->rc_scratch));
        Timed tm(c, BC_K_STATS);
        HIP_TRY(bc::launch_stats(c->stream, c->rc_scratch, L, k, nf, nf2, d_cov, d_pc, d_ent, d_sec, d_counts));
        return BC_OK;
    }
    Timed tm(c, bc::pileup_is_solo(*r, L, c->shape, c->tile_waves) ? BC_K_SOLO : BC_K_PILEUP);
    HIP_TRY(bc::launch_pileup_tiles(c->stream, *r, L, r->max_end, mbq, k, true, false, nf, nf2, d_counts, d_cov,
                                    d_pc, d_ent, d_sec, c->d_err, c->shape, c->tile_waves, c->instance));
    return BC_OK;
}

int bc_segments_layout(const int64_t* ref_lens, int n, int64_t* voff) {
    if (!ref_lens || !voff) return fail(BC_E_ARG, "NULL argument");
    if (n <= 0) return fail(BC_E_ARG, "bc_segments_layout: n must be > 0");
    const int64_t cap = BC_SEGMENTS_MAX_LEN;  // starts are int32
    int64_t off = 0;
    voff[0] = 0;
    for (int i = 0; i < n; ++i) {
        if (ref_lens[i] <= 0) return fail(BC_E_ARG, "bc_segments_layout: segment " + std::to_string(i) + ": length <= 0");
        if (ref_lens[i] > cap - off) return fail(BC_E_ARG, "bc_segments_layout: the virtual reference exceeds 2^31 - 128");
        off += (ref_lens[i] + 63) / 64 * 64;  // (<= 2^31 - 65 here)
        if (off > cap) return fail(BC_E_ARG, "bc_segments_layout: the virtual reference exceeds 2^31 - 128");
        voff[i + 1] = off;
    }
    return BC_OK;
}

int bc_pileup_segments(bc_ctx* c, const bc_reads* r, int n_seg, const int64_t* d_ref_len, const int64_t* d_read_beg,
                       const int64_t* d_voff, int64_t virt_len, int32_t* d_vpos, uint32_t mbq, int k, double nf,
                       double nf2, int32_t* d_counts, int32_t* d_cov, double* d_pc, double* d_ent, double* d_sec,
                       double* d_sum) {
    if (!c || !r) return fail(BC_E_ARG, "NULL argument");
    if (n_seg <= 0) return fail(BC_E_ARG, "bc_pileup_segments: n_seg must be > 0");
    if (!d_ref_len || !d_read_beg || !d_voff) return fail(BC_E_ARG, "bc_pileup_segments: NULL segment table");
    if (virt_len <= 0 || virt_len % 64 || virt_len > BC_SEGMENTS_MAX_LEN)
        return fail(BC_E_ARG, "bc_pileup_segments: virt_len must be bc_segments_layout's voff[n_seg]");
    if (r->n_reads < 0) return fail(BC_E_ARG, "n_reads < 0");
    if (r->n_reads > 0 && (!r->pos || !d_vpos)) return fail(BC_E_ARG, "bc_pileup_segments: NULL pos / d_vpos");
    DeviceGuard g(c->device);
    {
        Timed tm(c, BC_K_INDEX);
        HIP_TRY(bc::launch_seg_vpos(c->stream, r->pos, r->n_reads, d_ref_len, d_read_beg, d_voff, n_seg, d_vpos));
    }
    // the group's reads as one sorted batch on the virtual reference: no index (none was built for
    // these starts), every read ends inside it
    bc_reads v = *r;
    v.pos = d_vpos;
    v.sorted = 1;
    v.max_end = virt_len;
    v.tile_reads = nullptr;
    v.n_tiles = 0;
    v.read_runs = nullptr;
    v.run_chunks = 0;
    v.index_tag = 0;
    const int rc = bc_pileup(c, &v, virt_len, mbq, k, nf, nf2, d_counts, d_cov, d_pc, d_ent, d_sec);
    if (rc != BC_OK || !d_sum) return rc;
    Timed tm(c, BC_K_SUMMARY);
    HIP_TRY(bc::launch_sum_segments(c->stream, n_seg, d_ref_len, d_voff, d_cov, d_ent, d_sum));
    return BC_OK;
}

int bc_segments_rebase(bc_ctx* c, int64_t n_reads, int n_seg, const int64_t* d_read_beg, const uint64_t* d_cig_base,
                       const uint64_t* d_nib_base, uint64_t cig_words_total, uint64_t nib_total,
                       const uint32_t* d_cig_beg, const uint32_t* d_seq_nib, uint32_t* d_cig_beg_out,
                       uint32_t* d_seq_nib_out) {
    if (!c) return fail(BC_E_ARG, "bc_segments_rebase: ctx is NULL");
    if (n_reads < 0 || n_reads > 0x7FFFFFFFll) return fail(BC_E_ARG, "bc_segments_rebase: n_reads must lie in [0, 2^31)");
    if (n_seg < 1) return fail(BC_E_ARG, "bc_segments_rebase: n_seg must be > 0");
    if (!bcc_fits(cig_words_total, nib_total))
        return fail(BC_E_ARG, "bc_segments_rebase: the shared buffers must hold fewer than 2^32 CIGAR words and nibbles");
    if (!d_read_beg || !d_cig_base || !d_nib_base) return fail(BC_E_ARG, "bc_segments_rebase: NULL segment table");
    if (n_reads > 0 && (!d_cig_beg || !d_seq_nib || !d_cig_beg_out || !d_seq_nib_out))
        return fail(BC_E_ARG, "bc_segments_rebase: NULL per-read array");
    DeviceGuard g(c->device);
    Timed tm(c, BC_K_INDEX);
    HIP_TRY(bc::launch_seg_rebase(c->stream, n_reads, d_read_beg, n_seg, d_cig_base, d_nib_base, d_cig_beg, d_seq_nib,
                                  d_cig_beg_out, d_seq_nib_out));
    return BC_OK;
}

int bc_amplicons_segments(bc_ctx* c, const int32_t* d_cov, const double* d_ent, const double* d_sec, int n_seg,
                          const int64_t* d_ref_len, const int64_t* d_voff, const int64_t* d_lo, const int64_t* d_hi,
                          int32_t n_tiles, double* d_out) {
    if (!c) return fail(BC_E_ARG, "bc_amplicons_segments: ctx is NULL");
    if (n_seg < 1) return fail(BC_E_ARG, "bc_amplicons_segments: n_seg must be > 0");
    if (n_tiles < 0) return fail(BC_E_ARG, "bc_amplicons_segments: n_tiles < 0");
    if ((int64_t)n_seg * n_tiles > 0x7FFFFFFFll)
        return fail(BC_E_ARG, "bc_amplicons_segments: n_seg * n_tiles must stay below 2^31");
    if (n_tiles == 0) return BC_OK;
    if (!d_cov || !d_ent || !d_sec || !d_ref_len || !d_voff || !d_lo || !d_hi || !d_out)
        return fail(BC_E_ARG, "bc_amplicons_segments: NULL argument");
    DeviceGuard g(c->device);
    Timed tm(c, BC_K_AMPLICONS);
    HIP_TRY(bc::launch_amplicons_segments(c->stream, d_cov, d_ent, d_sec, n_seg, d_ref_len, d_voff, d_lo, d_hi,
                                          n_tiles, d_out));
    return BC_OK;
}

// grow-only context scratch (a synchronizing allocation when it grows: outside graph capture)
static int out_scratch(bc_ctx* c, size_t need) {
    if (need <= c->out_scratch_bytes) return BC_OK;
    if (c->out_scratch) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipFree(c->out_scratch));
        c->out_scratch = nullptr;
        c->out_scratch_bytes = 0;
    }
    HIP_TRY(hipMalloc(&c->out_scratch, need));
    c->out_scratch_bytes = need;
    return BC_OK;
}

int bc_pileup_partials(bc_ctx* c, const bc_reads* r, int64_t L, uint32_t mbq, int k, double nf, double nf2,
                       int32_t* d_counts, int32_t* d_cov, double* d_pc, double* d_ent, double* d_sec, void* d_work) {
    if (!c || !r || !d_work) return fail(BC_E_ARG, "NULL argument");
    if (L <= 0) return fail(BC_E_ARG, "ref_len must be > 0 (np.mean of an empty list)");
    const bool sparse_path = !bc::use_rc(*r, L, c->shape) && r->n_reads > 0;
    if (!d_counts && !d_cov && !d_pc && !d_ent && !d_sec) {
        // Summary only (main.py:469-499 prints six numbers per reference): the sparse sweep writes
        // no per-position output but the last partial buffer's coverage / entropy (into context
        // scratch); the other paths write their outputs into context scratch.
        if (k != 5 && k != 6) return fail(BC_E_ARG, "k must be 5 or 6");
        DeviceGuard g(c->device);
        // (the sparse sweep k_pileup_solo is the kernel that fuses the partials)
        if (sparse_path && L >= bc::kNpBuf && bc::pileup_is_solo(*r, L, c->shape, c->tile_waves)) {
            if (!r->sorted) return fail(BC_E_ARG, "bc_pileup needs a coordinate-sorted batch (sorted == 1)");
            if (mbq > 0 && !r->qual) return fail(BC_E_ARG, "min_base_quality > 0 needs qualities");
            if (r->seq_layout != BC_SEQ_EVENT) return fail(BC_E_ARG, "bc_pileup needs seq_layout == BC_SEQ_EVENT");
            if ((uintptr_t)r->seq & 15u) return fail(BC_E_ARG, "bc_pileup needs a 16-byte aligned sequence buffer");
            if (int rc = out_scratch(c, (size_t)bc::kNpBuf * 12)) return rc;
            bc::SumParts parts = bc::summary_parts(d_work, L);
            parts.no_store = true;
            parts.ent_tail = (double*)c->out_scratch;
            parts.cov_tail = (int32_t*)((double*)c->out_scratch + bc::kNpBuf);
#ifdef BC_SUM_SWEEP  // A/B builds only: the per-tile sweep k_pileup_solo<STORE = false>
            {
                Timed tm(c, BC_K_SOLO);
                HIP_TRY(bc::launch_pileup_tiles(c->stream, *r, L, r->max_end, mbq, k, true, false, nf, nf2, nullptr,
                                                nullptr, nullptr, nullptr, nullptr, c->d_err, c->shape, c->tile_waves,
                                                c->instance, &parts));
            }
#else
            {
                const size_t need = bc::sum_sparse_bytes(L);
                if (need > c->sum_scratch_bytes) {  // grow-only, zeroed once (the kernels leave it zeroed)
                    if (c->sum_scratch) {
                        HIP_TRY(hipStreamSynchronize(c->stream));
                        HIP_TRY(hipFree(c->sum_scratch));
                        c->sum_scratch = nullptr;
                        c->sum_scratch_bytes = 0;
                    }
                    HIP_TRY(hipMalloc(&c->sum_scratch, need));
                    c->sum_scratch_bytes = need;
                    HIP_TRY(hipMemsetAsync(c->sum_scratch, 0, need, c->stream));
                }
                Timed tm(c, BC_K_SOLO);
                const hipError_t e = bc::launch_sum_sparse(c->stream, *r, L, mbq, k, nf, c->d_err, parts,
                                                           c->sum_scratch, c->sum_scratch_bytes);
                if (e != hipSuccess) {
                    // the leaf arrays may be left partly counted (k_sum_buffers re-zeroes them at the
                    // end of the chain): give them back, so the next call allocates and zeroes afresh
                    (void)hipStreamSynchronize(c->stream);
                    (void)hipFree(c->sum_scratch);
                    c->sum_scratch = nullptr;
                    c->sum_scratch_bytes = 0;
                    return hip_fail(e, "bc::launch_sum_sparse");
                }
            }
#endif
            if (!parts.fused) return fail(BC_E_ARG, "internal: summary-only sweep without fused partials");
            // the fold's last partial buffer reads positions [full_chunks * 8192, L): the tail
            // arrays stand at that offset (only those elements are addressed)
            const int64_t off = parts.full_chunks * bc::kNpBuf;
            const int32_t* cov_base = (const int32_t*)((uintptr_t)parts.cov_tail - (uintptr_t)off * 4u);
            const double* ent_base = (const double*)((uintptr_t)parts.ent_tail - (uintptr_t)off * 8u);
            Timed tm(c, BC_K_SUMMARY);
            // (the read-parallel summary writes whole-buffer partials, the sweep quarter ones)
            HIP_TRY(bc::launch_summary_partials(c->stream, cov_base, ent_base, L, d_work, parts.full_chunks,
                                                !parts.whole_buffers));
            return BC_OK;
        }
        // counts [k][L] int32, cov [L] int32, ent / sec [L] double
        const size_t need = (size_t)L * (4u * (size_t)k + 4u + 16u);
        if (int rc = out_scratch(c, need)) return rc;
        double* ent = (double*)c->out_scratch;
        double* sec = ent + L;
        int32_t* cov = (int32_t*)(sec + L);
        int32_t* counts = cov + L;
        return bc_pileup_partials(c, r, L, mbq, k, nf, nf2, counts, cov, nullptr, ent, sec, d_work);
    }
    if (!sparse_path) {
        int rc = bc_pileup(c, r, L, mbq, k, nf, nf2, d_counts, d_cov, d_pc, d_ent, d_sec);
        if (rc) return rc;
        if (!d_cov || !d_ent) return fail(BC_E_ARG, "NULL coverage / entropy");
        DeviceGuard g(c->device);
        Timed tm(c, BC_K_SUMMARY);
        HIP_TRY(bc::launch_summary_partials(c->stream, d_cov, d_ent, L, d_work, 0));
        return BC_OK;
    }
    // the argument checks of bc_pileup
    if (k != 5 && k != 6) return fail(BC_E_ARG, "k must be 5 or 6");
    if (!r->sorted) return fail(BC_E_ARG, "bc_pileup needs a coordinate-sorted batch (sorted == 1)");
    if (mbq > 0 && !r->qual) return fail(BC_E_ARG, "min_base_quality > 0 needs qualities");
    if (r->seq_layout != BC_SEQ_EVENT) return fail(BC_E_ARG, "bc_pileup needs seq_layout == BC_SEQ_EVENT");
    if ((uintptr_t)r->seq & 15u) return fail(BC_E_ARG, "bc_pileup needs a 16-byte aligned sequence buffer");
    if (!d_counts || !d_cov || !d_ent || !d_sec) return fail(BC_E_ARG, "NULL output");
    DeviceGuard g(c->device);
    bc::SumParts parts = bc::summary_parts(d_work, L);
    {
        Timed tm(c, bc::pileup_is_solo(*r, L, c->shape, c->tile_waves) ? BC_K_SOLO : BC_K_PILEUP);
        HIP_TRY(bc::launch_pileup_tiles(c->stream, *r, L, r->max_end, mbq, k, true, false, nf, nf2, d_counts, d_cov,
                                        d_pc, d_ent, d_sec, c->d_err, c->shape, c->tile_waves, c->instance, &parts));
    }
    const int64_t first = parts.fused ? parts.full_chunks : 0;
    Timed tm(c, BC_K_SUMMARY);  // the last, partial buffer (or all of them), and the header
    HIP_TRY(bc::launch_summary_partials(c->stream, d_cov, d_ent, L, d_work, first));
    return BC_OK;
}

int bc_summary_fold(bc_ctx* c, int n, const int64_t* ref_lens, void* const* d_works, double* const* d_outs) {
    if (!c || n < 0 || (n > 0 && (!ref_lens || !d_works || !d_outs))) return fail(BC_E_ARG, "NULL argument");
    for (int i = 0; i < n; ++i) {
        if (ref_lens[i] <= 0) return fail(BC_E_ARG, "ref_len must be > 0 (np.mean of an empty list)");
        if (!d_works[i] || !d_outs[i]) return fail(BC_E_ARG, "NULL work / output");
    }
    if (n == 0) return BC_OK;
    DeviceGuard g(c->device);
    Timed tm(c, BC_K_SUMMARY);
    HIP_TRY(bc::launch_summary_fold(c->stream, n, ref_lens, d_works, d_outs));
    return BC_OK;
}

int bc_pileup_summary(bc_ctx* c, const bc_reads* r, int64_t L, uint32_t mbq, int k, double nf, double nf2,
                      int32_t* d_counts, int32_t* d_cov, double* d_pc, double* d_ent, double* d_sec, void* d_work,
                      double* d_out) {
    if (!d_out) return fail(BC_E_ARG, "NULL argument");
    if (c && r && d_work && L > 0 && !d_pc && bc::use_rc(*r, L, c->shape) && (k == 5 || k == 6)) {
        // a deep batch: kernel 2 leaves numpy's leaf partials and ONE launch folds them (the fused
        // tail of bc_pileup_summary_amplicons, no windows); summary only: context stand-ins
        if (!d_counts && !d_cov && !d_ent && !d_sec) {
            const size_t need = (size_t)L * (4u * (size_t)k + 4u + 16u);
            DeviceGuard g(c->device);
            if (int rc = out_scratch(c, need)) return rc;
            d_ent = (double*)c->out_scratch;
            d_sec = d_ent + L;
            d_cov = (int32_t*)(d_sec + L);
            d_counts = d_cov + L;
        }
        if (d_counts && d_cov && d_ent && d_sec)
            return bc_pileup_summary_amplicons(c, r, L, mbq, k, nf, nf2, d_counts, d_cov, d_ent, d_sec, d_work, d_out,
                                               nullptr, nullptr, 0, nullptr);
    }
    int rc = bc_pileup_partials(c, r, L, mbq, k, nf, nf2, d_counts, d_cov, d_pc, d_ent, d_sec, d_work);
    if (rc) return rc;
    return bc_summary_fold(c, 1, &L, &d_work, &d_out);
}

int bc_graph_begin(bc_ctx* c) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (!c->stream) return fail(BC_E_ARG, "cannot capture the legacy default stream");
    DeviceGuard g(c->device);
    HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    return BC_OK;
}

int bc_graph_end(bc_ctx* c, bc_graph** out) {
    if (!c || !out) return fail(BC_E_ARG, "NULL argument");
    DeviceGuard g(c->device);
    auto* gr = new bc_graph();
    hipError_t e = hipStreamEndCapture(c->stream, &gr->graph);
    if (e == hipSuccess) e = hipGraphInstantiate(&gr->exec, gr->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        bc_graph_destroy(gr);
        return hip_fail(e, "graph capture");
    }
    *out = gr;
    return BC_OK;
}

int bc_graph_launch(bc_ctx* c, bc_graph* gr) {
    if (!c || !gr) return fail(BC_E_ARG, "NULL argument");
    DeviceGuard g(c->device);
    HIP_TRY(hipGraphLaunch(gr->exec, c->stream));
    return BC_OK;
}

int bc_graph_destroy(bc_graph* gr) {
    if (!gr) return BC_OK;
    if (gr->exec) (void)hipGraphExecDestroy(gr->exec);
    if (gr->graph) (void)hipGraphDestroy(gr->graph);
    delete gr;
    return BC_OK;
}

int bc_timing_enable(bc_ctx* c, int on) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    c->timing = on != 0;
    return BC_OK;
}

int bc_timing_report(bc_ctx* c, int64_t* launches, double* mean_us) {
    if (!c || !launches || !mean_us) return fail(BC_E_ARG, "NULL argument");
    DeviceGuard g(c->device);
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int id = 0; id < BC_KERNEL_IDS; ++id) {
        double tot = 0.0;
        for (auto& pr : c->ev[id]) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) tot += ms;
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
        launches[id] = (int64_t)c->ev[id].size();
        mean_us[id] = c->ev[id].empty() ? 0.0 : tot * 1e3 / (double)c->ev[id].size();
        c->ev[id].clear();
    }
    return BC_OK;
}

int bc_ctx_wait(bc_ctx* c, bc_ctx* other) {
    if (!c || !other) return fail(BC_E_ARG, "NULL argument");
    if (c->device != other->device) return fail(BC_E_ARG, "bc_ctx_wait: contexts on different devices");
    if (c == other || c->stream == other->stream) return BC_OK;
    DeviceGuard g(c->device);
    HIP_TRY(hipEventRecord(other->sig, other->stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, other->sig, 0));
    return BC_OK;
}

int bc_event_record(bc_ctx* c, int slot) {
    if (!c || slot < 0 || slot >= BC_EVENT_SLOTS) return fail(BC_E_ARG, "bad context or event slot");
    DeviceGuard g(c->device);
    if (!c->mark[slot]) HIP_TRY(hipEventCreate(&c->mark[slot]));
    HIP_TRY(hipEventRecord(c->mark[slot], c->stream));
    return BC_OK;
}

int bc_event_elapsed_ms(bc_ctx* c, int s0, int s1, float* ms) {
    if (!c || !ms || s0 < 0 || s1 < 0 || s0 >= BC_EVENT_SLOTS || s1 >= BC_EVENT_SLOTS)
        return fail(BC_E_ARG, "bad context, slot or output");
    if (!c->mark[s0] || !c->mark[s1]) return fail(BC_E_ARG, "event slot never recorded");
    DeviceGuard g(c->device);
    HIP_TRY(hipEventSynchronize(c->mark[s1]));
    HIP_TRY(hipEventElapsedTime(ms, c->mark[s0], c->mark[s1]));
    return BC_OK;
}

int bc_range_error(bc_ctx* c, int64_t* first_bad) {
    if (!c || !first_bad) return fail(BC_E_ARG, "NULL argument");
    DeviceGuard g(c->device);
    HIP_TRY(hipMemcpyAsync(c->h_err, c->d_err, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_err, 0xFF, sizeof(unsigned long long), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *first_bad = (*c->h_err == ~0ull) ? -1 : (int64_t)*c->h_err;
    return BC_OK;
}

int bc_stats(bc_ctx* c, const int32_t* d_hist, int64_t L, int k, double nf, double nf2, int32_t* d_cov,
             double* d_pc, double* d_ent, double* d_sec) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (k != 5 && k != 6) return fail(BC_E_ARG, "k must be 5 or 6");
    if (L < 0) return fail(BC_E_ARG, "ref_len < 0");
    if (L == 0) return BC_OK;
    if (!d_hist) return fail(BC_E_ARG, "d_hist is NULL");
    DeviceGuard g(c->device);
    Timed tm(c, BC_K_STATS);
    HIP_TRY(bc::launch_stats(c->stream, d_hist, L, k, nf, nf2, d_cov, d_pc, d_ent, d_sec));
    return BC_OK;
}

size_t bc_summary_work_bytes(int64_t L) { return bc::summary_work_bytes(L); }

size_t bc_seq_event_bytes(int64_t seq_bytes) { return bc::seq_event_bytes(seq_bytes); }

int bc_seq_to_event(bc_ctx* c, const uint8_t* d_bam, int64_t seq_bytes, uint8_t* d_event) {
    if (!c || !d_event || (seq_bytes > 0 && !d_bam)) return fail(BC_E_ARG, "NULL argument");
    if (seq_bytes < 0) return fail(BC_E_ARG, "seq_bytes < 0");
    DeviceGuard g(c->device);
    HIP_TRY(bc::launch_seq_event(c->stream, d_bam, seq_bytes, d_event));
    return BC_OK;
}

int bc_summary(bc_ctx* c, const int32_t* d_cov, const double* d_ent, int64_t L, void* d_work, double* d_out) {
    if (!c || !d_out || !d_work) return fail(BC_E_ARG, "NULL argument");
    if (L <= 0) return fail(BC_E_ARG, "ref_len must be > 0 (np.mean of an empty list)");
    if (!d_cov || !d_ent) return fail(BC_E_ARG, "NULL coverage / entropy");
    DeviceGuard g(c->device);
    Timed tm(c, BC_K_SUMMARY);
    HIP_TRY(bc::launch_summary(c->stream, d_cov, d_ent, L, d_work, d_out));
    return BC_OK;
}

int bc_amplicons(bc_ctx* c, const int32_t* d_cov, const double* d_ent, const double* d_sec, int64_t L,
                 const int64_t* d_lo, const int64_t* d_hi, int32_t n_tiles, double* d_out) {
    if (!c) return fail(BC_E_ARG, "ctx is NULL");
    if (n_tiles < 0) return fail(BC_E_ARG, "n_tiles < 0");
    if (n_tiles == 0) return BC_OK;
    if (!d_cov || !d_ent || !d_sec || !d_lo || !d_hi || !d_out) return fail(BC_E_ARG, "NULL argument");
    DeviceGuard g(c->device);
    Timed tm(c, BC_K_AMPLICONS);
    HIP_TRY(bc::launch_amplicons(c->stream, d_cov, d_ent, d_sec, L, d_lo, d_hi, n_tiles, d_out));
    return BC_OK;
}

int bc_pileup_summary_amplicons(bc_ctx* c, const bc_reads* r, int64_t L, uint32_t mbq, int k, double nf, double nf2,
                                int32_t* d_counts, int32_t* d_cov, double* d_ent, double* d_sec, void* d_work,
                                double* d_out, const int64_t* d_lo, const int64_t* d_hi, int32_t n_tiles,
                                double* d_amp) {
    if (!c || !r || !d_work || !d_out) return fail(BC_E_ARG, "NULL argument");
    if (L <= 0) return fail(BC_E_ARG, "ref_len must be > 0 (np.mean of an empty list)");
    if (n_tiles < 0) return fail(BC_E_ARG, "n_tiles < 0");
    if (n_tiles > 0 && (!d_lo || !d_hi || !d_amp)) return fail(BC_E_ARG, "NULL window argument");
    if (!d_counts || !d_cov || !d_ent || !d_sec) return fail(BC_E_ARG, "NULL output");
    if (!bc::use_rc(*r, L, c->shape)) {  // shallow batches: the fused sweeps, then the windows
        int rc = bc_pileup_summary(c, r, L, mbq, k, nf, nf2, d_counts, d_cov, nullptr, d_ent, d_sec, d_work, d_out);
        if (rc) return rc;
        return bc_amplicons(c, d_cov, d_ent, d_sec, L, d_lo, d_hi, n_tiles, d_amp);
    }
    // the argument checks of bc_pileup
    if (k != 5 && k != 6) return fail(BC_E_ARG, "k must be 5 or 6");
    if (!r->sorted) return fail(BC_E_ARG, "bc_pileup needs a coordinate-sorted batch (sorted == 1)");
    if (mbq > 0 && r->n_reads > 0 && !r->qual) return fail(BC_E_ARG, "min_base_quality > 0 needs qualities");
    if (r->n_reads > 0 && r->seq_layout != BC_SEQ_EVENT)
        return fail(BC_E_ARG, "bc_pileup needs seq_layout == BC_SEQ_EVENT (see bc_seq_to_event)");
    if (r->n_reads > 0 && ((uintptr_t)r->seq & 15u))
        return fail(BC_E_ARG, "bc_pileup needs a 16-byte aligned sequence buffer");
    DeviceGuard g(c->device);
    const size_t need = (size_t)k * (size_t)L * 4;
    if (need > c->rc_scratch_bytes) {  // as bc_pileup: grow-only, kept zeroed by kernel 2
        if (c->rc_scratch) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(hipFree(c->rc_scratch));
            c->rc_scratch = nullptr;
            c->rc_scratch_bytes = 0;
        }
        HIP_TRY(hipMalloc((void**)&c->rc_scratch, need));
        c->rc_scratch_bytes = need;
        HIP_TRY(hipMemsetAsync(c->rc_scratch, 0, need, c->stream));
    }
    HIP_TRY(launch_chunked(c, *r, L, mbq, k, c->rc_scratch));
    {
        Timed tm(c, BC_K_STATS);
        HIP_TRY(bc::launch_stats_leaves(c->stream, c->rc_scratch, L, k, nf, nf2, d_cov, d_ent, d_sec, d_counts, d_work));
    }
    Timed tm(c, BC_K_AMPLICONS);
    HIP_TRY(bc::launch_tail(c->stream, d_cov, d_ent, d_sec, L, d_work, d_out, d_lo, d_hi, n_tiles, d_amp));
    return BC_OK;
}

int bc_bcount_host(int device, int64_t ref_len, uint32_t mbq, const bc_reads* h, uint32_t* h_out, int64_t* bad_read,
                   int64_t* bad_pos) {
    if (bad_read) *bad_read = -1;
    if (bad_pos) *bad_pos = -1;
    if (ref_len < 0 || ref_len > 0xFFFFFFFFll) return fail(BC_E_ARG, "refLen out of uint32 range");
    if (ref_len > 0 && !h_out) return fail(BC_E_ARG, "h_out is NULL");
    int rc = check_host_reads(h);
    if (rc) return rc;
    if (mbq > 0 && h->n_reads > 0 && !h->qual) return fail(BC_E_ARG, "min_base_quality > 0 needs qualities");
    if (h->seq_layout != BC_SEQ_BAM) return fail(BC_E_ARG, "bc_bcount_host takes BC_SEQ_BAM sequences");
    bc_ctx* c = nullptr;
    rc = bc_ctx_create(device, nullptr, &c);
    if (rc) return rc;
    struct Cleanup {
        bc_ctx* c;
        bc_reads d{};
        int32_t* hist = nullptr;
        ~Cleanup() {
            if (hist) bc_free(c, hist);
            bc_reads_free(c, &d);
            bc_ctx_destroy(c);
        }
    } cl{c};
    rc = bc_reads_upload(c, h, &cl.d);
    if (rc) return rc;
    const size_t hb = (size_t)std::max<int64_t>(ref_len, 1) * 6 * sizeof(int32_t);
    rc = bc_malloc(c, hb, (void**)&cl.hist);
    if (rc) return rc;
    rc = bc_memset(c, cl.hist, 0, hb);
    if (rc) return rc;
    rc = bc_count(c, &cl.d, ref_len, mbq, 6, cl.hist);
    if (rc) return rc;
    int64_t bad = -1;
    rc = bc_range_error(c, &bad);
    if (rc) return rc;
    if (bad >= 0) {
        if (bad_read) *bad_read = bad;
        const int64_t bp = host_bad_pos(*h, bad, ref_len, mbq);
        if (bad_pos) *bad_pos = bp;
        return fail(BC_E_RANGE, "vector::_M_range_check: __n (which is " + std::to_string(bp) +
                                    ") >= this->size() (which is " + std::to_string(ref_len) + ")");
    }
    if (ref_len == 0) return BC_OK;
    std::vector<int32_t> planes((size_t)ref_len * 6);
    rc = bc_memcpy_d2h(c, planes.data(), cl.hist, (size_t)ref_len * 6 * sizeof(int32_t));
    if (rc) return rc;
    rc = bc_sync(c);
    if (rc) return rc;
    for (int64_t p = 0; p < ref_len; ++p)
        for (int col = 0; col < 6; ++col) h_out[p * 6 + col] = (uint32_t)planes[(size_t)col * ref_len + p];
    return BC_OK;
}

}  // extern "C"
