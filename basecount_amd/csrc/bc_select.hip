// bc_select.hip — the read selection of a device-decoded batch: bcio_select on the arrays that
// bc_bam_fill left in HBM.
//
// Five launches over bc_select.h's functions (the host check compiles the same ones):
//   k_sel_count    a workgroup per run of BCS_RUN records: accepted and selected records by ballot,
//                  the first accepted record that is not wanted
//   k_sel_scan     one workgroup: exclusive prefix sums of the two int64 columns (at most 2^14
//                  entries for a batch of 2^24 records), the first keyerror record, the header
//   k_sel_scatter  rank = workgroup base + the waves before + the steps before + mbcnt of the ballot,
//                  so consecutive selected reads are stored by consecutive lanes; the eight per-read
//                  arrays, the compacted tid and rec_err; the keyerror record's lane writes its ordinal
//   k_sel_refs     a thread per reference: ref_beg[t] = lower bound of t in the compacted tid
//                  (log2(m) steps, no walk over read-free references), n_reads, the facts' neutral values
//   k_sel_facts    a thread per selected read: the order tests against its predecessor in the
//                  compacted order and the per-reference facts; a wave whose lanes share one tid
//                  reduces in the wave and issues one atomic per fact, a wave that straddles
//                  references issues them per lane
// Launch sizes come from n and n_refs only; nothing here synchronises or allocates.
#include "bc_internal.h"

#include <cstring>

#include "bc_select.h"

namespace bc {
namespace {

__device__ __forceinline__ uint32_t lanes_before(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(BCS_THREADS) void k_sel_count(bcb_arrays r, int64_t n, int64_t min_mapq,
                                                           const uint8_t* ref_sel, int32_t n_refs, void* work) {
    __shared__ int64_t s_acc[BCS_WAVES], s_sel[BCS_WAVES], s_ke[BCS_WAVES];
    const bcs_work w = bcs_bind(work, bcs_make_layout(n, n_refs));
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t ln = threadIdx.x & 63u;
    const int64_t base = (int64_t)blockIdx.x * BCS_RUN + (int64_t)wave * BCS_WAVE_RUN;
    int64_t acc = 0, sel = 0, ke = -1;
#pragma unroll
    for (uint32_t s = 0; s < BCS_STEPS; ++s) {
        const int64_t i = base + s * 64u + ln;
        const uint32_t c = i < n ? bcs_classify(r, i, min_mapq, n_refs, ref_sel) : 0u;
        const uint64_t mk = __ballot(c == 1u);
        acc += __popcll(__ballot(c & 1u));
        sel += __popcll(__ballot(c >> 1));
        if (mk && ke < 0) ke = base + s * 64u + (uint32_t)__builtin_ctzll(mk);
    }
    if (ln == 0) {
        s_acc[wave] = acc;
        s_sel[wave] = sel;
        s_ke[wave] = ke;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        acc = sel = 0;
        ke = -1;
        for (uint32_t k = 0; k < BCS_WAVES; ++k) {
            acc += s_acc[k];
            sel += s_sel[k];
            if (ke < 0) ke = s_ke[k];
        }
        w.acc[blockIdx.x] = acc;
        w.sel[blockIdx.x] = sel;
        w.ke[blockIdx.x] = ke;
    }
}

__global__ __launch_bounds__(BCS_THREADS) void k_sel_scan(bcb_arrays r, int64_t n, int32_t n_refs, void* work,
                                                          bcs_header* hdr) {
    __shared__ int64_t s_a[BCS_THREADS], s_s[BCS_THREADS], s_k[BCS_THREADS];
    const bcs_work w = bcs_bind(work, bcs_make_layout(n, n_refs));
    const uint32_t t = threadIdx.x;
    const uint32_t per = (w.nwg + BCS_THREADS - 1u) / BCS_THREADS;
    const uint32_t g0 = t * per, g1 = g0 + per < w.nwg ? g0 + per : w.nwg;
    int64_t a = 0, s = 0, k = INT64_MAX;
    for (uint32_t g = g0; g < g1; ++g) {
        a += w.acc[g];
        s += w.sel[g];
        if (k == INT64_MAX && w.ke[g] >= 0) k = w.ke[g];
    }
    s_a[t] = a;
    s_s[t] = s;
    s_k[t] = k;
    __syncthreads();
    for (uint32_t off = 1; off < BCS_THREADS; off <<= 1) {
        const int64_t va = t >= off ? s_a[t - off] : 0, vs = t >= off ? s_s[t - off] : 0;
        const int64_t vk = t >= off ? s_k[t - off] : INT64_MAX;
        __syncthreads();
        s_a[t] += va;
        s_s[t] += vs;
        if (vk < s_k[t]) s_k[t] = vk;
        __syncthreads();
    }
    int64_t ea = s_a[t] - a, es = s_s[t] - s;  // exclusive
    for (uint32_t g = g0; g < g1; ++g) {
        const int64_t ca = w.acc[g], cs = w.sel[g];
        w.acc[g] = ea;
        w.sel[g] = es;
        ea += ca;
        es += cs;
    }
    if (t == BCS_THREADS - 1u) {
        bcs_header h;
        h.status = bcs_too_large(r.cig_off[n], r.seq_off[n]) ? BCS_ST_TOO_LARGE : BCS_ST_OK;
        h.err_or = 0;
        h.n_accepted = s_a[t];
        h.n_selected = s_s[t];
        h.keyerror_rec = s_k[t] == INT64_MAX ? -1 : s_k[t];
        h.keyerror_ordinal = -1;
        h.reserved[0] = h.reserved[1] = h.reserved[2] = 0;
        *hdr = h;
    }
}

__global__ __launch_bounds__(BCS_THREADS) void k_sel_scatter(bcb_arrays r, int64_t n, int64_t min_mapq,
                                                             const uint8_t* ref_sel, int32_t n_refs, void* work,
                                                             bcs_arrays o) {
    __shared__ uint32_t s_acc[BCS_WAVES], s_sel[BCS_WAVES];
    const bcs_work w = bcs_bind(work, bcs_make_layout(n, n_refs));
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t ln = threadIdx.x & 63u;
    const int64_t base = (int64_t)blockIdx.x * BCS_RUN + (int64_t)wave * BCS_WAVE_RUN;
    uint32_t c[BCS_STEPS];
    uint64_t ma[BCS_STEPS], ms[BCS_STEPS];
    uint32_t acc = 0, sel = 0;
#pragma unroll
    for (uint32_t s = 0; s < BCS_STEPS; ++s) {
        const int64_t i = base + s * 64u + ln;
        c[s] = i < n ? bcs_classify(r, i, min_mapq, n_refs, ref_sel) : 0u;
        ma[s] = __ballot(c[s] & 1u);
        ms[s] = __ballot(c[s] >> 1);
        acc += (uint32_t)__popcll(ma[s]);
        sel += (uint32_t)__popcll(ms[s]);
    }
    if (ln == 0) {
        s_acc[wave] = acc;
        s_sel[wave] = sel;
    }
    __syncthreads();
    int64_t ord0 = w.acc[blockIdx.x], j0 = w.sel[blockIdx.x];
    for (uint32_t k = 0; k < wave; ++k) {
        ord0 += s_acc[k];
        j0 += s_sel[k];
    }
    const int64_t ke = o.header->keyerror_rec;
#pragma unroll
    for (uint32_t s = 0; s < BCS_STEPS; ++s) {
        const int64_t i = base + s * 64u + ln;
        if (c[s] & 1u) {
            const int64_t ord = ord0 + lanes_before(ma[s]);
            if (c[s] == 3u) {
                const int64_t j = j0 + lanes_before(ms[s]);
                if (j < o.n_cap) bcs_store_read(r, i, j, ord, o, w);  // (always: the counts bound the ranks)
            } else if (i == ke) {
                o.header->keyerror_ordinal = ord;
            }
        }
        ord0 += __popcll(ma[s]);
        j0 += __popcll(ms[s]);
    }
}

__global__ __launch_bounds__(BCS_THREADS) void k_sel_refs(int64_t n, int32_t n_refs, void* work, bcs_arrays o) {
    const bcs_work w = bcs_bind(work, bcs_make_layout(n, n_refs));
    const int64_t t = (int64_t)blockIdx.x * BCS_THREADS + threadIdx.x;
    if (t > n_refs) return;
    int64_t m = o.header->n_selected;
    if (m > n) m = n;
    bcs_ref_init((int32_t)t, n_refs, m, o, w);
}

template <class T, class F>
__device__ __forceinline__ T wave_reduce(T v, F f) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = f(v, (T)__shfl_xor(v, off, 64));
    return v;
}

__global__ __launch_bounds__(BCS_THREADS) void k_sel_facts(int64_t n, int32_t n_refs, const int64_t* ref_len, void* work,
                                                           bcs_arrays o) {
    const bcs_work w = bcs_bind(work, bcs_make_layout(n, n_refs));
    const int64_t j = (int64_t)blockIdx.x * BCS_THREADS + threadIdx.x;
    int64_t m = o.header->n_selected;
    if (m > n) m = n;
    const bool active = j < m;
    if (!__ballot(active)) return;  // wave-uniform
    bcs_fact f;
    f.tid = -1;
    f.span = 0;
    f.end = INT64_MIN;
    f.ops = f.complex = f.err = f.clear = f.ungrouped = 0;
    if (active) f = bcs_read_fact(j, o, w, ref_len);
    const uint32_t ln = threadIdx.x & 63u;
    const uint32_t err = wave_reduce(f.err, [](uint32_t a, uint32_t b) { return a | b; });
    const bool ungrouped = __ballot(f.ungrouped != 0u) != 0;
    if (ln == 0) {
        if (ungrouped) atomicMax(&o.header->status, (int32_t)BCS_ST_UNGROUPED);
        if (err) atomicOr(&o.header->err_or, err);
    }
    const int32_t t0 = __builtin_amdgcn_readfirstlane(f.tid);  // lane 0 is active: it has the wave's first j
    if (__ballot(active && f.tid != t0) == 0) {
        // the common case: the wave's reads share one reference; one atomic per fact
        const int64_t span = wave_reduce((long long)f.span, [](long long a, long long b) { return a > b ? a : b; });
        const int64_t end = wave_reduce((long long)f.end, [](long long a, long long b) { return a > b ? a : b; });
        const unsigned long long ops =
            wave_reduce((unsigned long long)f.ops, [](unsigned long long a, unsigned long long b) { return a + b; });
        const uint32_t clear = wave_reduce(f.clear, [](uint32_t a, uint32_t b) { return a | b; });
        const uint32_t cx = (uint32_t)__popcll(__ballot(f.complex != 0u));
        if (ln == 0) {
            if (span > 0) atomicMax((long long*)&o.max_span[t0], (long long)span);
            atomicMax((long long*)&o.max_end[t0], (long long)end);
            if (cx) atomicAdd((unsigned long long*)&o.n_complex[t0], (unsigned long long)cx);
            if (ops) atomicAdd((unsigned long long*)&o.sum_ops[t0], ops);
            if (err) atomicOr(&o.err_or[t0], err);
            if (clear) atomicAnd(&o.flags[t0], ~clear);
        }
    } else if (active) {
        const int32_t t = f.tid;
        if (f.span > 0) atomicMax((long long*)&o.max_span[t], (long long)f.span);
        atomicMax((long long*)&o.max_end[t], (long long)f.end);
        if (f.complex) atomicAdd((unsigned long long*)&o.n_complex[t], 1ull);
        if (f.ops) atomicAdd((unsigned long long*)&o.sum_ops[t], (unsigned long long)f.ops);
        if (f.err) atomicOr(&o.err_or[t], f.err);
        if (f.clear) atomicAnd(&o.flags[t], ~f.clear);
    }
}

}  // namespace

size_t select_bytes(int64_t n, int64_t n_refs) { return (size_t)bcs_make_layout(n, n_refs).total; }

hipError_t launch_select(hipStream_t s, const bc_bam_arrays& rec, int64_t n, int64_t min_mapq, const uint8_t* ref_sel,
                         const int64_t* ref_len, int32_t n_refs, void* work, const bc_sel_arrays& out) {
    static_assert(sizeof(bcb_arrays) == sizeof(bc_bam_arrays), "bc_bam_arrays has bcb_arrays' layout");
    static_assert(sizeof(bcs_arrays) == sizeof(bc_sel_arrays), "bc_sel_arrays has bcs_arrays' layout");
    static_assert(sizeof(bcs_header) == sizeof(bc_sel_header) && sizeof(bcs_header) == 64, "bc_sel_header is bcs_header");
    bcb_arrays r;
    bcs_arrays o;
    memcpy(&r, &rec, sizeof r);
    memcpy(&o, &out, sizeof o);
    const bcs_layout l = bcs_make_layout(n, n_refs);
    const dim3 block(BCS_THREADS), runs(l.nwg);
    hipLaunchKernelGGL(k_sel_count, runs, block, 0, s, r, n, min_mapq, ref_sel, n_refs, work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sel_scan, dim3(1), block, 0, s, r, n, n_refs, work, o.header);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_sel_scatter, runs, block, 0, s, r, n, min_mapq, ref_sel, n_refs, work, o);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const dim3 refs((uint32_t)(((int64_t)n_refs + 1 + BCS_THREADS - 1) / BCS_THREADS));
    hipLaunchKernelGGL(k_sel_refs, refs, block, 0, s, n, n_refs, work, o);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const dim3 reads((uint32_t)((n + BCS_THREADS - 1) / BCS_THREADS > 0 ? (n + BCS_THREADS - 1) / BCS_THREADS : 1));
    hipLaunchKernelGGL(k_sel_facts, reads, block, 0, s, n, n_refs, ref_len, work, o);
    return hipGetLastError();
}

}  // namespace bc
