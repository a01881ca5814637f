// bc_fmt.hip — the TSV rows of the per-position outputs, written where the kernels left them.
//
// Three launches over bc_fmt.h's functions (the host check compiles the same ones):
//   k_fmt_measure  a wave per tile of 64 positions: the segment once per tile, each lane the byte
//                  length of its row(s) through the counting sink (kept for k_fmt_write), the
//                  tile's byte count by a wave reduction and its first declined position by ballot
//   k_fmt_scan     one workgroup: every thread a run of consecutive tiles, the run totals scanned
//                  in LDS, the byte counts replaced by byte offsets; then seg_off and the header
//   k_fmt_write    a wave per tile, at once back unless the status is OK: the lane lengths' wave
//                  prefix, each lane its row(s) into the wave's LDS staging area at the
//                  alignment skew of the destination, then 16-byte stores from consecutive lanes
//                  and byte stores at the unaligned head and tail; more text than the area holds
//                  goes through in windows
// A workgroup is one wave, so its barrier orders the staging area's writes and reads at no cost.
// Launch sizes come from n only; nothing here synchronises or allocates.
#include "bc_internal.h"

#include <cstring>

#include "bc_fmt.h"

namespace bc {
namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}

// the lane's text length; 0 past the tile's positions
__device__ __forceinline__ uint32_t lane_len(const bcf_args& a, const bcf_tile& t, uint64_t tile, uint32_t ln, bool* ok) {
    *ok = true;
    if (ln >= t.cnt) return 0u;
    bcf_counter s;
    s.n = 0;
    *ok = bcf_emit_pos(s, a, t, (int64_t)(tile * BCF_TILE + ln), ln);
    return s.n;
}

__global__ __launch_bounds__(64) void k_fmt_measure(bcf_args a, void* work) {
    const uint64_t tile = blockIdx.x;
    if (tile >= bcf_tiles(a.n)) return;
    const uint32_t ln = threadIdx.x;
    const bcf_tile t = bcf_tile_of(a, tile);
    bool ok;
    const uint32_t len = lane_len(a, t, tile, ln, &ok);
    const uint32_t sum = wave_sum(len);
    const uint64_t bad = __ballot(!ok);
    bcf_work_len(work, a.n)[tile * BCF_TILE + ln] = len;
    if (ln == 0) {
        int64_t d = INT64_MAX;
        if (t.name_bad && t.cnt)
            d = (int64_t)(tile * BCF_TILE);
        else if (bad)
            d = (int64_t)(tile * BCF_TILE) + __builtin_ctzll(bad);
        bcf_work_off(work)[tile] = (int64_t)sum;
        bcf_work_decl(work, a.n)[tile] = d;
    }
}

__global__ __launch_bounds__(BCF_SCAN_THREADS) void k_fmt_scan(bcf_args a, void* work, bcf_header* hdr, int64_t* seg_off,
                                                               int64_t text_cap) {
    __shared__ int64_t s_sum[BCF_SCAN_THREADS], s_bad[BCF_SCAN_THREADS];
    const uint64_t nt = bcf_tiles(a.n);
    int64_t* off = bcf_work_off(work);
    const int64_t* decl = bcf_work_decl(work, a.n);
    const uint32_t t = threadIdx.x;
    const uint64_t per = (nt + BCF_SCAN_THREADS - 1u) / BCF_SCAN_THREADS;
    const uint64_t g0 = t * per < nt ? t * per : nt, g1 = g0 + per < nt ? g0 + per : nt;
    int64_t sum = 0, bad = INT64_MAX;
    for (uint64_t g = g0; g < g1; ++g) {
        sum += off[g];
        if (decl[g] < bad) bad = decl[g];
    }
    s_sum[t] = sum;
    s_bad[t] = bad;
    __syncthreads();
    for (uint32_t o = 1; o < BCF_SCAN_THREADS; o <<= 1) {
        const int64_t vs = t >= o ? s_sum[t - o] : 0, vb = t >= o ? s_bad[t - o] : INT64_MAX;
        __syncthreads();
        s_sum[t] += vs;
        if (vb < s_bad[t]) s_bad[t] = vb;
        __syncthreads();
    }
    int64_t e = s_sum[t] - sum;  // exclusive
    for (uint64_t g = g0; g < g1; ++g) {
        const int64_t b = off[g];
        off[g] = e;
        e += b;
    }
    __syncthreads();  // the offsets of every run, for seg_off
    const int64_t total = s_sum[BCF_SCAN_THREADS - 1u];
    for (int64_t i = t; i <= a.n_seg; i += BCF_SCAN_THREADS) seg_off[i] = bcf_seg_off(a, off, total, i);
    if (t == 0) bcf_store_header(hdr, s_bad[BCF_SCAN_THREADS - 1u], total, text_cap);
}

__global__ __launch_bounds__(64) void k_fmt_write(bcf_args a, const void* work, const bcf_header* hdr, uint8_t* text) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[BCF_STAGE];
    if (hdr->status != BCF_ST_OK) return;
    const uint64_t tile = blockIdx.x;
    if (tile >= bcf_tiles(a.n)) return;
    const uint32_t ln = threadIdx.x;
    const bcf_tile t = bcf_tile_of(a, tile);
    if (!t.cnt) return;
    const uint32_t len = ln < t.cnt ? bcf_work_len(const_cast<void*>(work), a.n)[tile * BCF_TILE + ln] : 0u;
    uint32_t incl = len;  // inclusive wave prefix
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, o, 64);
        if (ln >= (uint32_t)o) incl += v;
    }
    const uint32_t beg = incl - len;
    uint64_t tot = (uint32_t)__shfl((int)incl, 63, 64);
    const uint64_t g0 = (uint64_t)bcf_work_off(const_cast<void*>(work))[tile];
    const uint64_t total = (uint64_t)hdr->total_bytes;
    if (g0 >= total) return;
    if (tot > total - g0) tot = total - g0;  // (never: the offsets are the prefix sums of these lengths)
    uint8_t* dst0 = text + g0;
    const uint32_t skew = (uint32_t)((uintptr_t)dst0 & 15u);
    for (uint32_t wb = 0; wb < tot; wb += BCF_WIN) {
        const uint32_t wlen = tot - wb < BCF_WIN ? (uint32_t)(tot - wb) : BCF_WIN;
        if (len && beg < wb + wlen && beg + len > wb) {
            bcf_writer w;
            w.buf = stage + skew;
            w.base = wb;
            w.cap = wlen;
            w.at = beg;
            bcf_emit_pos(w, a, t, (int64_t)(tile * BCF_TILE + ln), ln);
        }
        __syncthreads();
        const bcf_copy c = bcf_copy_plan(skew, wlen);
        uint8_t* dst = dst0 + wb;
        const uint8_t* src = stage + skew;
        if (ln < c.head) dst[ln] = src[ln];
        const uint4* s16 = reinterpret_cast<const uint4*>(src + c.head);  // skew + head is a multiple of 16
        uint4* d16 = reinterpret_cast<uint4*>(dst + c.head);
        for (uint32_t i = ln; i < c.body; i += 64u) d16[i] = s16[i];
        const uint32_t tb = c.head + 16u * c.body;
        if (ln < c.tail) dst[tb + ln] = src[tb + ln];
        __syncthreads();
    }
}

}  // namespace

size_t fmt_work_bytes(int64_t n) { return (size_t)bcf_work_bytes(n); }

hipError_t launch_fmt_rows(hipStream_t s, const bc_fmt_args& args, void* work, void* out, uint8_t* text,
                           int64_t text_cap) {
    static_assert(sizeof(bcf_args) == sizeof(bc_fmt_args), "bc_fmt_args has bcf_args' layout");
    static_assert(sizeof(bcf_seg) == sizeof(bc_fmt_seg) && sizeof(bcf_seg) == 32, "bc_fmt_seg is bcf_seg");
    static_assert(sizeof(bcf_header) == sizeof(bc_fmt_header) && sizeof(bcf_header) == 64, "bc_fmt_header is bcf_header");
    bcf_args a;
    memcpy(&a, &args, sizeof a);
    const uint64_t nt = bcf_tiles(a.n);
    const dim3 tiles((uint32_t)(nt ? nt : 1u)), wave(64);
    bcf_header* hdr = (bcf_header*)out;
    int64_t* seg_off = (int64_t*)((uint8_t*)out + sizeof(bcf_header));
    hipLaunchKernelGGL(k_fmt_measure, tiles, wave, 0, s, a, work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fmt_scan, dim3(1), dim3(BCF_SCAN_THREADS), 0, s, a, work, hdr, seg_off, text_cap);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_fmt_write, tiles, wave, 0, s, a, (const void*)work, (const bcf_header*)hdr, text);
    return hipGetLastError();
}

}  // namespace bc
