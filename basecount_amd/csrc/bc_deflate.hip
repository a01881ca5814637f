// bc_deflate.hip — BGZF blocks written on the device: spans of text into whole compressed blocks.
//
// Four launches over bc_deflate.h's functions (the host twin below runs the same ones):
//   k_dfl_plan   one workgroup: the gate, the offsets' check (non-decreasing, within text_cap: a
//                violation is a status), the spans' block counts scanned, the block table
//   k_dfl_block  one wave per block: bcd_block over the wave machine.  The hash table (8 KiB), the
//                staging area (1,152 B) and the CRC table (1 KiB) are the wave's LDS: 10,368 B, room
//                for 15 waves per CU.  The input is read from global memory (a block's 64 KiB stay in
//                L2), the output leaves 1 KiB at a time as aligned 16-byte stores into the block's own
//                64 KiB slot.  No byte is written outside the slot.
//   k_dfl_scan   one workgroup: block sizes into offsets, span_coff[], the total and the status
//   k_dfl_pack   the slots into d_comp, contiguously: 16-byte stores from consecutive lanes, byte
//                stores at the unaligned head and tail; nothing unless the status is OK
// A workgroup of k_dfl_block is one wave, so its barrier orders the LDS writes and reads at no cost.
// Launch sizes come from text_cap and n_spans only; nothing here synchronises or allocates.
#include "bc_internal.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

#include "bc_deflate.h"

namespace bc {
namespace {

constexpr uint32_t kPlanThreads = 256;
constexpr uint32_t kPackParts = 4;  // workgroups that share one block's copy

// d_work: the header, first[n_spans + 1] (a span's first block), the block table, the block sizes,
// the block offsets, then the slots
struct DflWork {
    int64_t n_blocks;
    int32_t status;  // BC_DFL_OK or _OFFSETS, by k_dfl_plan
    int32_t reserved0;
    int64_t reserved[6];
};
struct DflBlock {
    int64_t uoff;
    uint32_t isize, span;
};
static_assert(sizeof(DflWork) == 64 && sizeof(DflBlock) == 16, "work layout");
constexpr uint32_t kStoredBit = 1u << 31;

struct DflLayout {
    uint64_t max_blocks, first, table, size, coff, slots, bytes;
};
__host__ __device__ inline DflLayout dfl_layout(int64_t text_cap, int64_t n_spans) {
    DflLayout l;
    l.max_blocks = bcd_max_blocks((uint64_t)text_cap, (uint64_t)n_spans);
    l.first = sizeof(DflWork);
    l.table = (l.first + 8u * ((uint64_t)n_spans + 1u) + 15u) & ~15ull;
    l.size = l.table + 16u * l.max_blocks;
    l.coff = (l.size + 4u * l.max_blocks + 7u) & ~7ull;
    l.slots = (l.coff + 8u * l.max_blocks + 255u) & ~255ull;
    l.bytes = l.slots + (uint64_t)BCD_SLOT * l.max_blocks;
    return l;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4), may_alias));

struct __attribute__((aligned(16))) DflLds {
    uint32_t stage[BCD_STAGE_WORDS];
    uint32_t crc[256];
    uint16_t table[1u << BCD_HASH_BITS];
};
static_assert(sizeof(DflLds) <= 10 * 1024 + 128, "per-wave LDS must leave room for 15 waves per CU");

struct BcdWave {
    static constexpr uint32_t NL = 64, PER = 1;
    DflLds* L;
    const uint8_t* src;
    uint32_t len;
    uint8_t* slot;
    uint32_t ln;

    __device__ __forceinline__ uint32_t lane() const { return ln; }
    // the aligned word that holds byte p (p < len), and the next one where it holds a byte of the input
    __device__ __forceinline__ uint32_t load32(uint32_t p) const {
        const uintptr_t a = (uintptr_t)(src + p);
        const uint32_t* w = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
        const uint32_t sh = 8u * (uint32_t)(a & 3u);
        const uint32_t lo = w[0];
        const uint32_t hi = sh != 0 && (uintptr_t)(w + 1) < (uintptr_t)(src + len) ? w[1] : 0u;
        return __builtin_amdgcn_alignbit(hi, lo, sh);  // {hi, lo} >> sh
    }
    __device__ __forceinline__ uint16_t* table() { return L->table; }
    __device__ __forceinline__ uint32_t* stage() { return L->stage; }
    __device__ __forceinline__ uint32_t* crc_table() { return L->crc; }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ uint64_t mask(const bool (&v)[1]) const { return __ballot(v[0]); }
    __device__ __forceinline__ uint32_t get(const uint32_t (&v)[1], uint32_t j) const {
        return (uint32_t)__builtin_amdgcn_readlane((int)v[0], __builtin_amdgcn_readfirstlane((int)j));
    }
    __device__ __forceinline__ void scan(const uint32_t (&v)[1], uint32_t (&e)[1], uint32_t& total) const {
        uint32_t incl = v[0];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = (uint32_t)__shfl_up((int)incl, o, 64);
            if (ln >= (uint32_t)o) incl += u;
        }
        e[0] = incl - v[0];
        total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    __device__ __forceinline__ void down(const uint32_t (&v)[1], uint32_t (&o)[1], uint32_t d) const {
        const uint32_t u = (uint32_t)__shfl_down((int)v[0], d, 64);
        o[0] = ln + d < 64u ? u : 0u;
    }
    // every lane that is on writes; the lanes whose position is above the one that landed write
    // again: the entry only grows and ends at the highest position, whichever write landed first
    __device__ __forceinline__ void insert(const uint32_t (&h)[1], const uint32_t (&p)[1], const bool (&on)[1]) {
        bool act = on[0];
        while (__any(act)) {
            if (act) L->table[h[0]] = (uint16_t)p[0];
            __syncthreads();
            if (act && (uint32_t)L->table[h[0]] >= p[0]) act = false;
            __syncthreads();
        }
    }
    __device__ __forceinline__ void stage_or(uint32_t w, uint32_t bits) { atomicOr(&L->stage[w], bits); }
    __device__ __forceinline__ void flush(uint32_t dst, uint32_t n16) {
        u32x4* d = reinterpret_cast<u32x4*>(slot + dst);  // the slot and dst are multiples of 16
        const u32x4* s = reinterpret_cast<const u32x4*>(L->stage);
        for (uint32_t i = ln; i < n16; i += 64u) d[i] = s[i];
    }
    __device__ __forceinline__ void slot_byte(uint32_t off, uint8_t v) { slot[off] = v; }
    // the flushes' stores are complete before other lanes store to the same bytes
    __device__ __forceinline__ void slot_fence() { __threadfence(); }
};

__global__ __launch_bounds__(kPlanThreads) void k_dfl_plan(const int64_t* span_off, int64_t n_spans, int64_t text_cap,
                                                           const int32_t* gate, uint8_t* work, bc_dfl_header* hdr) {
    __shared__ int64_t s_sum[kPlanThreads];
    const DflLayout lay = dfl_layout(text_cap, n_spans);
    DflWork* wh = reinterpret_cast<DflWork*>(work);
    const uint32_t t = threadIdx.x;
    if (gate != nullptr && *gate != 0) {
        if (t == 0) {  // the header, and nothing else: the other kernels read the gate themselves
            bc_dfl_header h;
            memset(&h, 0, sizeof h);
            h.status = BC_DFL_GATED;
            *hdr = h;
        }
        return;
    }
    int64_t* first = reinterpret_cast<int64_t*>(work + lay.first);
    const uint64_t per = ((uint64_t)n_spans + kPlanThreads - 1u) / kPlanThreads;
    const uint64_t g0 = std::min<uint64_t>(t * per, (uint64_t)n_spans), g1 = std::min<uint64_t>(g0 + per, (uint64_t)n_spans);
    int bad = 0;
    for (uint64_t g = g0; g < g1; ++g) bad |= span_off[g] < 0 || span_off[g] > span_off[g + 1] || span_off[g + 1] > text_cap;
    if (__syncthreads_or(bad)) {
        if (t == 0) {
            wh->n_blocks = 0;
            wh->status = BC_DFL_OFFSETS;
        }
        return;
    }
    int64_t sum = 0;
    for (uint64_t g = g0; g < g1; ++g) sum += (int64_t)bcd_nblocks((uint64_t)(span_off[g + 1] - span_off[g]));
    s_sum[t] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < kPlanThreads; o <<= 1) {
        const int64_t v = t >= o ? s_sum[t - o] : 0;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    int64_t e = s_sum[t] - sum;  // exclusive
    for (uint64_t g = g0; g < g1; ++g) {
        first[g] = e;
        e += (int64_t)bcd_nblocks((uint64_t)(span_off[g + 1] - span_off[g]));
    }
    const int64_t nb = std::min<int64_t>(s_sum[kPlanThreads - 1u], (int64_t)lay.max_blocks);  // (never more: the cut's bound)
    if (t == 0) {
        first[n_spans] = nb;
        wh->n_blocks = nb;
        wh->status = BC_DFL_OK;
    }
    __syncthreads();
    DflBlock* tab = reinterpret_cast<DflBlock*>(work + lay.table);
    for (int64_t b = t; b < nb; b += kPlanThreads) {
        int64_t lo = 0, hi = n_spans;  // the span with first[s] <= b < first[s + 1]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) / 2;
            if (first[mid] <= b)
                lo = mid;
            else
                hi = mid;
        }
        const uint64_t k = (uint64_t)(b - first[lo]), bytes = (uint64_t)(span_off[lo + 1] - span_off[lo]);
        DflBlock d;
        d.uoff = span_off[lo] + (int64_t)(k * BCD_BLOCK);
        d.isize = k < bcd_nblocks(bytes) ? bcd_block_len(bytes, k) : 0u;
        d.span = (uint32_t)lo;
        tab[b] = d;
    }
}

__global__ __launch_bounds__(64) void k_dfl_block(const uint8_t* text, int64_t text_cap, int64_t n_spans,
                                                  const int32_t* gate, uint8_t* work) {
    __shared__ DflLds lds;
    if (gate != nullptr && *gate != 0) return;
    const DflLayout lay = dfl_layout(text_cap, n_spans);
    const DflWork* wh = reinterpret_cast<const DflWork*>(work);
    const int64_t b = blockIdx.x;
    if (b >= wh->n_blocks) return;
    const DflBlock d = reinterpret_cast<const DflBlock*>(work + lay.table)[b];
    uint32_t* size = reinterpret_cast<uint32_t*>(work + lay.size);
    // (the plan wrote only blocks inside the text; a block that is not writes nothing)
    if (d.isize == 0 || d.isize > BCD_BLOCK || d.uoff < 0 || d.uoff > text_cap || (int64_t)d.isize > text_cap - d.uoff) {
        if (threadIdx.x == 0) size[b] = 0;
        return;
    }
    BcdWave m;
    m.L = &lds;
    m.src = text + d.uoff;
    m.len = d.isize;
    m.slot = work + lay.slots + (uint64_t)b * BCD_SLOT;
    m.ln = threadIdx.x;
    bool stored;
    const uint32_t total = bcd_block(m, d.isize, &stored);
    if (threadIdx.x == 0) size[b] = total | (stored ? kStoredBit : 0u);
}

__global__ __launch_bounds__(kPlanThreads) void k_dfl_scan(int64_t n_spans, int64_t text_cap, const int64_t* span_off,
                                                           const int32_t* gate, uint8_t* work, bc_dfl_header* hdr,
                                                           int64_t* span_coff, int64_t comp_cap) {
    __shared__ int64_t s_sum[kPlanThreads];
    __shared__ int32_t s_stored[kPlanThreads];
    const DflLayout lay = dfl_layout(text_cap, n_spans);
    const DflWork* wh = reinterpret_cast<const DflWork*>(work);
    if (gate != nullptr && *gate != 0) return;
    const uint32_t t = threadIdx.x;
    const int64_t nb = wh->n_blocks;
    const uint32_t* size = reinterpret_cast<const uint32_t*>(work + lay.size);
    int64_t* coff = reinterpret_cast<int64_t*>(work + lay.coff);
    const int64_t* first = reinterpret_cast<const int64_t*>(work + lay.first);
    const uint64_t per = ((uint64_t)nb + kPlanThreads - 1u) / kPlanThreads;
    const uint64_t g0 = std::min<uint64_t>(t * per, (uint64_t)nb), g1 = std::min<uint64_t>(g0 + per, (uint64_t)nb);
    int64_t sum = 0;
    int32_t st = 0;
    for (uint64_t g = g0; g < g1; ++g) {
        sum += (int64_t)(size[g] & ~kStoredBit);
        st += (size[g] & kStoredBit) != 0;
    }
    s_sum[t] = sum;
    s_stored[t] = st;
    __syncthreads();
    for (uint32_t o = 1; o < kPlanThreads; o <<= 1) {
        const int64_t v = t >= o ? s_sum[t - o] : 0;
        const int32_t u = t >= o ? s_stored[t - o] : 0;
        __syncthreads();
        s_sum[t] += v;
        s_stored[t] += u;
        __syncthreads();
    }
    int64_t e = s_sum[t] - sum;
    for (uint64_t g = g0; g < g1; ++g) {
        coff[g] = e;
        e += (int64_t)(size[g] & ~kStoredBit);
    }
    __syncthreads();
    const int64_t total = s_sum[kPlanThreads - 1u];
    const bool ok = wh->status == BC_DFL_OK;
    for (int64_t i = t; i <= n_spans; i += kPlanThreads) span_coff[i] = ok && first[i] < nb ? coff[first[i]] : total;
    if (t == 0) {
        bc_dfl_header h;
        memset(&h, 0, sizeof h);
        h.status = !ok ? wh->status : total > comp_cap ? BC_DFL_TOO_SMALL : BC_DFL_OK;
        h.n_stored = s_stored[kPlanThreads - 1u];
        h.n_blocks = nb;
        h.total_bytes = total;
        h.text_bytes = ok ? span_off[n_spans] - span_off[0] : 0;
        *hdr = h;
    }
}

__global__ __launch_bounds__(64) void k_dfl_pack(int64_t text_cap, int64_t n_spans, const uint8_t* work,
                                                 const bc_dfl_header* hdr, uint8_t* comp, int64_t comp_cap) {
    if (hdr->status != BC_DFL_OK) return;
    const DflLayout lay = dfl_layout(text_cap, n_spans);
    const int64_t b = blockIdx.x;
    if (b >= hdr->n_blocks) return;
    const uint32_t size = reinterpret_cast<const uint32_t*>(work + lay.size)[b] & ~kStoredBit;
    const int64_t c = reinterpret_cast<const int64_t*>(work + lay.coff)[b];
    const int64_t lim = hdr->total_bytes < comp_cap ? hdr->total_bytes : comp_cap;
    if (size > BCD_SLOT || c < 0 || c > lim || (int64_t)size > lim - c) return;  // (never: the scan's own sums)
    const uint8_t* slot = work + lay.slots + (uint64_t)b * BCD_SLOT;
    uint8_t* dst = comp + c;
    const uint32_t ln = threadIdx.x, part = blockIdx.y;
    uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);
    if (head > size) head = size;
    const uint32_t body = (size - head) / 16u, tb = head + 16u * body, tail = size - tb;
    if (part == 0) {
        if (ln < head) dst[ln] = slot[ln];
        if (ln < tail) dst[tb + ln] = slot[tb + ln];
    }
    // piece i is the slot's bytes [head + 16 i, + 16): five aligned words, shifted by head's low bits
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(slot) + (head >> 2);
    const uint32_t sh = 8u * (head & 3u);
    u32x4* d16 = reinterpret_cast<u32x4*>(dst + head);
    for (uint32_t i = part * 64u + ln; i < body; i += kPackParts * 64u) {
        const uint32_t* w = sw + 4u * i;
        const uint32_t a0 = w[0], a1 = w[1], a2 = w[2], a3 = w[3];
        const uint32_t a4 = sh ? w[4] : 0u;  // (below the slot's end: size <= 65,311)
        u32x4 v;
        v.x = __builtin_amdgcn_alignbit(a1, a0, sh);  // {a1, a0} >> sh
        v.y = __builtin_amdgcn_alignbit(a2, a1, sh);
        v.z = __builtin_amdgcn_alignbit(a3, a2, sh);
        v.w = __builtin_amdgcn_alignbit(a4, a3, sh);
        d16[i] = v;
    }
}

}  // namespace

size_t deflate_work_bytes(int64_t text_cap, int64_t n_spans) { return (size_t)dfl_layout(text_cap, n_spans).bytes; }

hipError_t launch_deflate(hipStream_t s, const uint8_t* text, int64_t text_cap, const int64_t* span_off, int64_t n_spans,
                          const int32_t* gate, void* work, void* out_small, uint8_t* comp, int64_t comp_cap) {
    static_assert(sizeof(bc_dfl_header) == 64, "bc_dfl_header is 64 bytes");
    const DflLayout lay = dfl_layout(text_cap, n_spans);
    const uint32_t nb = (uint32_t)std::max<uint64_t>(lay.max_blocks, 1u);
    bc_dfl_header* hdr = (bc_dfl_header*)out_small;
    int64_t* span_coff = (int64_t*)((uint8_t*)out_small + sizeof(bc_dfl_header));
    hipLaunchKernelGGL(k_dfl_plan, dim3(1), dim3(kPlanThreads), 0, s, span_off, n_spans, text_cap, gate, (uint8_t*)work, hdr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_dfl_block, dim3(nb), dim3(64), 0, s, text, text_cap, n_spans, gate, (uint8_t*)work);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_dfl_scan, dim3(1), dim3(kPlanThreads), 0, s, n_spans, text_cap, span_off, gate,
                       (uint8_t*)work, hdr, span_coff, comp_cap);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_dfl_pack, dim3(nb, kPackParts), dim3(64), 0, s, text_cap, n_spans, (const uint8_t*)work,
                       (const bc_dfl_header*)hdr, comp, comp_cap);
    return hipGetLastError();
}

// the host twin: the same cut, the same blocks (BcdHost), blocks in parallel over host threads
int deflate_host(const uint8_t* text, const int64_t* span_off, int64_t n_spans, uint8_t* comp, int64_t comp_cap,
                 int64_t* span_coff, int64_t* total, int nthreads) {
    for (int64_t i = 0; i < n_spans; ++i)
        if (span_off[i] < 0 || span_off[i] > span_off[i + 1]) {
            for (int64_t j = 0; j <= n_spans; ++j) span_coff[j] = 0;
            *total = 0;
            return BC_DFL_OFFSETS;
        }
    std::vector<int64_t> first((size_t)n_spans + 1);
    int64_t nb = 0;
    for (int64_t i = 0; i < n_spans; ++i) {
        first[(size_t)i] = nb;
        nb += (int64_t)bcd_nblocks((uint64_t)(span_off[i + 1] - span_off[i]));
    }
    first[(size_t)n_spans] = nb;
    std::vector<DflBlock> tab((size_t)nb);
    for (int64_t i = 0; i < n_spans; ++i) {
        const uint64_t bytes = (uint64_t)(span_off[i + 1] - span_off[i]);
        for (int64_t b = first[(size_t)i]; b < first[(size_t)i + 1]; ++b) {
            const uint64_t k = (uint64_t)(b - first[(size_t)i]);
            tab[(size_t)b] = DflBlock{span_off[i] + (int64_t)(k * BCD_BLOCK), bcd_block_len(bytes, k), (uint32_t)i};
        }
    }
    std::vector<std::vector<uint8_t>> done((size_t)nb);
    std::atomic<int64_t> next{0};
    auto worker = [&]() {
        std::vector<uint8_t> slot(BCD_SLOT);
        for (;;) {
            const int64_t b = next.fetch_add(1);
            if (b >= nb) return;
            bool stored = false;
            uint32_t size = 0;
#if !defined(__HIP_DEVICE_COMPILE__)  // (the host machine exists in the host pass only)
            size = bcd_block_host(text + tab[(size_t)b].uoff, tab[(size_t)b].isize, slot.data(), &stored);
#endif
            (void)stored;
            done[(size_t)b].assign(slot.begin(), slot.begin() + size);
        }
    };
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(nthreads, 16), nb));
    std::vector<std::thread> pool;
    for (int i = 1; i < nt; ++i) pool.emplace_back(worker);
    worker();
    for (auto& th : pool) th.join();
    std::vector<int64_t> coff((size_t)nb + 1);
    int64_t sum = 0;
    for (int64_t b = 0; b < nb; ++b) {
        coff[(size_t)b] = sum;
        sum += (int64_t)done[(size_t)b].size();
    }
    coff[(size_t)nb] = sum;
    for (int64_t i = 0; i <= n_spans; ++i) span_coff[i] = coff[(size_t)first[(size_t)i]];
    *total = sum;
    if (sum > comp_cap) return BC_DFL_TOO_SMALL;
    for (int64_t b = 0; b < nb; ++b) memcpy(comp + coff[(size_t)b], done[(size_t)b].data(), done[(size_t)b].size());
    return BC_DFL_OK;
}

}  // namespace bc
