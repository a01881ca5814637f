// bc_ops.hip — kernel 1 for batches of many-op reads (nanopore-like input: an indel every 10-20
// bases, tens to thousands of CIGAR ops per read; count.cpp:22-97).
//
// The short-read kernels (k_pileup, k_rc) decode at most 8 ops / 4 runs per read and walk every
// other read with a wave-uniform op loop restarted per 64-event step (rc_complex, walk_complex):
// O(span / 64 x n_ops) per read.  Here a wave owns a read and expands its CIGAR by scans:
//
//   1. 64 CIGAR words per load, one per lane (coalesced).  Each lane classifies its op (M/=/X
//      consume reference and query, D/N reference, I query; S/H/P/B nothing: seq_nib already
//      skips the leading clip) and a wave prefix sum (DPP row scans + the rows' totals) gives
//      every op its exclusive (reference offset, query offset); the totals carry to the next 64.
//   2. the reference events of those ops are emitted 64 consecutive positions per step.  An op
//      lane whose op starts inside the step (or covers the step's first position) writes its lane
//      number at that offset of a 64-entry LDS row; a prefix max over the event lanes gives each
//      its op, whose (start, query offset, kind) it fetches by ds_bpermute.  No per-op loop: a
//      read costs O(n_ops / 64 + span / 64) wave steps.
//   3. a block takes a run of consecutive reads and owns an LDS window of packed 16-bit column
//      pairs (k_count's `win`) that starts at its first read's start: events inside it are LDS
//      atomics on 64 consecutive addresses, events past it (the far part of long reads) one
//      coalesced 64-lane global atomic per step; the window's non-zero entries are flushed once
//      at the end.  An unsorted batch has no window.
//
// Event semantics are walk_read's / rc_complex's: bases by absolute nibble index seq_nib + q
// (BC_SEQ_EVENT), class 0000 counts nowhere, qual[index] >= mbq when mbq > 0, D/N count DS with
// no quality test, column N only with 6 columns, a counted event outside [0, L) records the read
// (smallest index wins) and counts nothing.  No scratch memory, no pre-pass: stream-ordered and
// capturable.
#include "bc_internal.h"

namespace bc {
namespace {

// CIGAR op classes (count.cpp:40-96): M/=/X consume reference and query, D/N the reference only
__device__ __forceinline__ bool mlike(uint32_t op) { return op == 0 || op == 7 || op == 8; }
__device__ __forceinline__ bool dlike(uint32_t op) { return op == 2 || op == 3; }

constexpr int kOpsThreads = 256;
constexpr int kOpsWaves = kOpsThreads / 64;
constexpr unsigned long long kOpsCol = 0x6666666366625106ull;  // event class -> column, 6 = none

struct OpsArgs {
    const int32_t* pos;
    const uint32_t* cig_beg;
    const uint32_t* cig_n;
    const uint32_t* seq_nib;
    const uint32_t* cigar;
    const uint8_t* seq;
    const uint8_t* qual;
    int64_t n;
    int64_t L;
    uint32_t mbq;
    int rpb;       // consecutive reads per block (<= 32768: a 16-bit half cannot overflow)
    int window;    // sorted batch: the block's LDS window from its first read's start
    int max_span;  // upper bound of a read's span (bounds the window's flush; need not hold)
    int32_t* counts;  // [NC][L], accumulated into
    unsigned long long* err;
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t lane_of(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }

// Inclusive wave prefix (sum, or max of values >= 0; identity 0): a prefix within each 16-lane
// row by DPP (row_shr 1, 2, 4, 8; lanes shifted in from outside the row read the identity), then
// the earlier rows' totals from their last lanes.  Must be called by the whole wave.
template <bool MAX>
__device__ __forceinline__ uint32_t wave_prefix(uint32_t v, int lane) {
    auto op = [](uint32_t a, uint32_t b) { return MAX ? (a > b ? a : b) : a + b; };
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false));
    const uint32_t t0 = lane_of(v, 15), t1 = lane_of(v, 31), t2 = lane_of(v, 47);
    const uint32_t t01 = op(t0, t1), t012 = op(t01, t2);
    const int row = lane >> 4;
    const uint32_t before = row == 0 ? 0u : (row == 1 ? t0 : (row == 2 ? t01 : t012));
    return op(v, before);
}

template <bool QUAL, int NC>
__global__ __launch_bounds__(kOpsThreads, 3) void k_ops(OpsArgs A) {
    __shared__ uint32_t win[3 * kWinMax];       // planes {A|C, G|T, DS|N}, 16-bit halves
    __shared__ uint32_t mark[kOpsWaves][64];    // per wave: the op lane (+1) starting at each step offset
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = (int)uni((uint32_t)(tid >> 6));
    const int64_t L = A.L;
    const int64_t r0 = (int64_t)blockIdx.x * A.rpb;
    const int64_t r1 = r0 + A.rpb < A.n ? r0 + A.rpb : A.n;
    if (r0 >= r1) return;

    // the window: positions [wbase, wbase + wlen) below L
    int64_t wbase = 0;
    int wlen = 0;
    if (A.window) {
        wbase = A.pos[r0];
        int64_t wl = (int64_t)A.pos[r1 - 1] - wbase + (A.max_span > 0 ? A.max_span : kWinMax);
        wl = wl > kWinMax ? kWinMax : wl;
        wl = wl > L - wbase ? L - wbase : wl;
        wlen = wl > 0 ? (int)wl : 0;
        for (int t = tid; t < wlen; t += kOpsThreads) {
            win[t] = 0;
            win[kWinMax + t] = 0;
            win[2 * kWinMax + t] = 0;
        }
        __syncthreads();
    }

    volatile uint32_t* const mk = mark[wave];
    int64_t first_bad = -1;  // (uniform) this wave's first read with an event outside [0, L)
    for (int64_t i = r0 + wave; i < r1; i += kOpsWaves) {
        const int64_t p0 = (int32_t)uni((uint32_t)A.pos[i]);
        const uint32_t* cg = A.cigar + uni(A.cig_beg[i]);
        const uint32_t cn = uni(A.cig_n[i]), sn = uni(A.seq_nib[i]);
        uint64_t R = 0;   // (uniform) reference offset of the op batch's first op
        uint32_t Q = 0;   // (uniform) its query offset (mod 2^32, as walk_read's)
        bool bad = false;
        for (uint32_t k0 = 0; k0 < cn; k0 += 64) {
            // ---- 1. 64 ops, their exclusive (reference, query) prefixes
            const uint32_t wd = k0 + (uint32_t)lane < cn ? cg[k0 + lane] : 0u;
            const uint32_t opc = wd & 15u, len = wd >> 4;
            const bool mref = mlike(opc), dref = dlike(opc);
            const uint32_t rl = (mref || dref) ? len : 0u;
            const uint32_t ql = (mref || opc == 1u) ? len : 0u;
            // (64 ops of < 2^28 positions: the reference prefix needs more than 32 bits, summed
            // as two 16-bit digits)
            const uint32_t rlo = wave_prefix<false>(rl & 0xFFFFu, lane);
            const uint32_t rhi = wave_prefix<false>(rl >> 16, lane);
            const uint32_t qinc = wave_prefix<false>(ql, lane);
            const uint64_t rinc = (uint64_t)rlo + ((uint64_t)rhi << 16);
            const uint64_t rtot = (uint64_t)lane_of(rlo, 63) + ((uint64_t)lane_of(rhi, 63) << 16);
            const uint32_t qtot = lane_of(qinc, 63);
            const uint64_t rs = R + rinc - rl;     // this op's first reference offset
            const uint32_t qs = Q + qinc - ql;     // and query offset
            const uint32_t kind = rl == 0u ? 0u : (mref ? 1u : 2u);
            const uint64_t Rend = R + rtot;
            // ---- 2. the ops' reference events, 64 consecutive offsets per step
            for (uint64_t e0 = R; e0 < Rend; e0 += 64) {
                const int64_t rel = (int64_t)(rs - e0);  // the op's start relative to the step
                mk[lane] = 0u;
                if (rl != 0u && rel < 64 && rel + (int64_t)rl > 0) mk[rel > 0 ? (int)rel : 0] = (uint32_t)lane + 1u;
                __builtin_amdgcn_wave_barrier();
                // the op covering offset e0 + lane: the last one starting at or before it (every
                // offset below Rend is covered: the batch's reference-consuming ops are contiguous)
                const uint32_t own = wave_prefix<true>(mk[lane], lane);
                __builtin_amdgcn_wave_barrier();
                const int src = (int)((own - 1u) & 63u);
                const int pk = __shfl((int)(((uint32_t)(int32_t)rel << 2) | kind), src);
                const uint32_t oq = (uint32_t)__shfl((int)qs, src);
                if (own != 0u && e0 + (uint64_t)lane < Rend) {
                    const uint32_t d = (uint32_t)(lane - (pk >> 2));  // offset inside the op
                    unsigned col = 4;  // D / N: DS, no quality test (count.cpp:80-90)
                    bool counted = true;
                    if ((pk & 3) == 1) {
                        const uint32_t ni = sn + oq + d;
                        col = (unsigned)(kOpsCol >> (((A.seq[ni >> 1] >> ((ni & 1u) * 4)) & 15u) * 4)) & 0xFu;
                        counted = col != 6u;
                        if (QUAL) counted = counted && (uint32_t)A.qual[ni] >= A.mbq;  // count.cpp:56
                    }
                    const int64_t p = p0 + (int64_t)(e0 + (uint64_t)lane);
                    if (counted && (p >= L || p < 0)) {
                        bad = true;  // .at() would throw (count.cpp:60-65,85)
                    } else if (counted && (int)col < NC) {
                        const int64_t idx = p - wbase;
                        if (idx >= 0 && idx < wlen)
                            atomicAdd(&win[(col >> 1) * kWinMax + (int)idx], 1u << ((col & 1u) * 16));
                        else
                            atomicAdd(&A.counts[(int64_t)col * L + p], 1);
                    }
                }
            }
            R = Rend;
            Q += qtot;
        }
        if (__any(bad) && first_bad < 0) first_bad = i;  // (reads in increasing order)
    }
    if (first_bad >= 0 && lane == 0) atomicMin(A.err, (unsigned long long)first_bad);

    if (wlen > 0) {
        __syncthreads();
        // flush: one global atomic per non-zero (position, column), neighbouring positions from
        // neighbouring lanes
        for (int t = tid; t < wlen; t += kOpsThreads) {
            const int64_t p = wbase + t;
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                const uint32_t v = win[pl * kWinMax + t];
                const uint32_t lo = v & 0xFFFFu, hi = v >> 16;
                if (lo) atomicAdd(&A.counts[(int64_t)(2 * pl) * L + p], (int32_t)lo);
                if (hi && 2 * pl + 1 < NC) atomicAdd(&A.counts[(int64_t)(2 * pl + 1) * L + p], (int32_t)hi);
            }
        }
    }
}

}  // namespace

// Consecutive reads per block.  Enough blocks to fill the device several times over; for a sorted
// batch few enough that the block's reads start within the window with room for a typical read
// (its length from the batch's sequence bytes: max_span is one outlier's), so that most events
// meet in LDS.  At most 32768 (the window's 16-bit halves).
int ops_reads_per_block(const bc_reads& r, int64_t L, int forced) {
    if (forced > 0) return forced < 32768 ? forced : 32768;
    const int64_t n = r.n_reads;
    int64_t target = n / 2048;
    target = target < 32 ? 32 : (target > 8192 ? 8192 : target);
    if (!r.sorted || L <= 0) return (int)target;
    const int64_t reach = r.max_end > L ? r.max_end : L;
    const double density = (double)n / (double)reach;
    double len = n > 0 ? 2.0 * (double)r.seq_bytes / (double)n : 0.0;
    if (r.max_span > 0 && len > (double)r.max_span) len = (double)r.max_span;
    if (len > kWinMax / 2) len = kWinMax / 2;
    const double fit = ((double)kWinMax - len) * density * 0.75;
    if (fit < (double)target) target = fit < 16.0 ? 16 : (int64_t)fit;
    return (int)target;
}

hipError_t launch_ops(hipStream_t s, const bc_reads& r, int64_t L, uint32_t mbq, int ncols, int32_t* counts,
                      unsigned long long* d_err, int reads_per_block) {
    if (r.n_reads <= 0) return hipSuccess;
    OpsArgs A;
    A.pos = r.pos;
    A.cig_beg = r.cig_beg;
    A.cig_n = r.cig_n;
    A.seq_nib = r.seq_nib;
    A.cigar = r.cigar;
    A.seq = r.seq;
    A.qual = r.qual;
    A.n = r.n_reads;
    A.L = L;
    A.mbq = mbq;
    A.rpb = ops_reads_per_block(r, L, reads_per_block);
    A.window = r.sorted ? 1 : 0;
    A.max_span = r.max_span;
    A.counts = counts;
    A.err = d_err;
    const int64_t nblk = (r.n_reads + A.rpb - 1) / A.rpb;
    const dim3 grid((unsigned)nblk), block(kOpsThreads);
    if (mbq > 0) {
        if (ncols == 6) hipLaunchKernelGGL((k_ops<true, 6>), grid, block, 0, s, A);
        else hipLaunchKernelGGL((k_ops<true, 5>), grid, block, 0, s, A);
    } else {
        if (ncols == 6) hipLaunchKernelGGL((k_ops<false, 6>), grid, block, 0, s, A);
        else hipLaunchKernelGGL((k_ops<false, 5>), grid, block, 0, s, A);
    }
    return hipGetLastError();
}

}  // namespace bc
