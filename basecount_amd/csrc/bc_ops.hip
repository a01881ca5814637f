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
//   4. reads longer than half a window (bc_ops_plan.h): k_ops_passes runs the block's reads over
//      consecutive windows, pass p owning [first start + p x 4096, + 4096): every event is
//      examined in exactly the pass that owns its position and meets in LDS up to the pass cap;
//      the passes end when no read of the block reaches further.
//
// Event semantics are walk_read's / rc_complex's: bases by absolute nibble index seq_nib + q
// (BC_SEQ_EVENT), class 0000 counts nowhere, qual[index] >= mbq when mbq > 0, D/N count DS with
// no quality test, column N only with 6 columns, a counted event outside [0, L) records the read
// (smallest index wins) and counts nothing.  No scratch memory, no pre-pass: stream-ordered and
// capturable.
#include "bc_internal.h"
#include "bc_ops_plan.h"

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
    int passes;    // k_ops_passes: the window passes a block runs at most (>= 2)
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

// 64 ops of a read from op k0 on, one per lane: this lane's op (first reference offset rs, length
// rl on the reference, query offset qs, kind 0 none / 1 M-like / 2 D-like) and the batch's end.
struct OpBatch {
    uint64_t rs, Rend;
    uint32_t rl, qs, kind, qtot;
};

// R, Q: the (uniform) reference and query (mod 2^32, as walk_read's) offsets of op k0.  Three
// wave prefix sums; must be called by the whole wave.
__device__ __forceinline__ OpBatch op_batch(const uint32_t* cg, uint32_t cn, uint32_t k0, int lane, uint64_t R,
                                            uint32_t Q) {
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
    OpBatch b;
    b.rl = rl;
    b.rs = R + rinc - rl;     // this op's first reference offset
    b.qs = Q + qinc - ql;     // and query offset
    b.kind = rl == 0u ? 0u : (mref ? 1u : 2u);
    b.Rend = R + rtot;
    b.qtot = lane_of(qinc, 63);
    return b;
}

// One 64-event step of an op batch: the events at reference offsets e0 + lane (below Rend) of the
// ops (rs, rl, qs, kind) the lanes hold.  With OWN only events at the `owned` positions from the
// window's start on are examined (wrel: that start as a reference offset of the read).  Must be
// called by the whole wave; true in the lanes whose counted event lies outside [0, L).
template <bool QUAL, int NC, bool OWN>
__device__ __forceinline__ bool ops_step(const OpsArgs& A, volatile uint32_t* mk, uint32_t* win, int lane, uint64_t e0,
                                         uint64_t Rend, uint64_t rs, uint32_t rl, uint32_t qs, uint32_t kind, uint32_t sn,
                                         int64_t p0, int64_t L, int64_t wrel, int wlen, int64_t owned) {
    bool bad = false;
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
    const int64_t p = p0 + (int64_t)(e0 + (uint64_t)lane);
    const int64_t idx = (int64_t)(e0 + (uint64_t)lane) - wrel;  // wrel: the window's start, from p0
    if (own != 0u && e0 + (uint64_t)lane < Rend && (!OWN || (idx >= 0 && idx < owned))) {
        const uint32_t d = (uint32_t)(lane - (pk >> 2));  // offset inside the op
        unsigned col = 4;  // D / N: DS, no quality test (count.cpp:80-90)
        bool counted = true;
        if ((pk & 3) == 1) {
            const uint32_t ni = sn + oq + d;
            col = (unsigned)(kOpsCol >> (((A.seq[ni >> 1] >> ((ni & 1u) * 4)) & 15u) * 4)) & 0xFu;
            counted = col != 6u;
            if (QUAL) counted = counted && (uint32_t)A.qual[ni] >= A.mbq;  // count.cpp:56
        }
        if (counted && (p >= L || p < 0)) {
            bad = true;  // .at() would throw (count.cpp:60-65,85)
        } else if (counted && (int)col < NC) {
            if (idx >= 0 && idx < wlen)
                atomicAdd(&win[(col >> 1) * kWinMax + (int)idx], 1u << ((col & 1u) * 16));
            else
                atomicAdd(&A.counts[(int64_t)col * L + p], 1);
        }
    }
    return bad;
}

// The window's non-zero entries: one global atomic per (position, column), neighbouring positions
// from neighbouring lanes
template <int NC>
__device__ __forceinline__ void ops_flush(const OpsArgs& A, const uint32_t* win, int tid, int64_t L, int64_t wbase,
                                          int wlen) {
    for (int t = tid; t < wlen; t += kOpsThreads) {
        int32_t* c = A.counts + (wbase + t);  // the position's column 0; the next column L further
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            const uint32_t v = win[pl * kWinMax + t];
            const uint32_t lo = v & 0xFFFFu, hi = v >> 16;
            if (lo) atomicAdd(c, (int32_t)lo);
            c += L;
            if (hi && 2 * pl + 1 < NC) atomicAdd(c, (int32_t)hi);
            c += L;
        }
    }
}

// The single window (and the unsorted batch's none): every event examined once, those past the
// window as global atomics.
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
            const OpBatch b = op_batch(cg, cn, k0, lane, R, Q);
            // ---- 2. the ops' reference events, 64 consecutive offsets per step
            for (uint64_t e0 = R; e0 < b.Rend; e0 += 64)
                bad |= ops_step<QUAL, NC, false>(A, mk, win, lane, e0, b.Rend, b.rs, b.rl, b.qs, b.kind, sn, p0, L,
                                                 wbase - p0, wlen, 0);
            R = b.Rend;
            Q += b.qtot;
        }
        if (__any(bad) && first_bad < 0) first_bad = i;  // (reads in increasing order)
    }
    if (first_bad >= 0 && lane == 0) atomicMin(A.err, (unsigned long long)first_bad);

    if (wlen > 0) {
        __syncthreads();
        ops_flush<NC>(A, win, tid, L, wbase, wlen);
    }
}

// Window passes over a sorted batch (A.passes >= 2): pass p owns the positions [wb, we) =
// pos[r0] + [p, p + 1) x kWinMax, the last pass everything from its wb on.  Per pass: clear the
// reachable part of the window, barrier, walk, barrier, flush.  An event is examined in exactly the
// pass that owns its position (a step straddling a window end is split per lane); what the last
// pass owns past its window goes to HBM as in the single window.  Nothing is kept between passes
// but each wave's first read that reaches on: a pass recomputes the op prefixes of the reads it
// visits (three wave_prefix per 64 ops), starts a batch's event loop at the first step that
// overlaps the pass, leaves a read at the first step at or beyond the pass's end, and stops at
// the first read that starts there (sorted order).  The passes end when no wave saw a read reach
// on: a block-wide flag, one word per pass parity (zeroed during the other parity's walk).
template <bool QUAL, int NC>
__global__ __launch_bounds__(kOpsThreads, 3) void k_ops_passes(OpsArgs A) {
    __shared__ uint32_t win[3 * kWinMax];
    __shared__ uint32_t mark[kOpsWaves][64];
    __shared__ int more[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = (int)uni((uint32_t)(tid >> 6));
    const int64_t L = A.L;
    const int64_t r0 = (int64_t)blockIdx.x * A.rpb;
    const int64_t r1 = r0 + A.rpb < A.n ? r0 + A.rpb : A.n;
    if (r0 >= r1) return;

    const int nr = (int)(r1 - r0);
    const int32_t wbase0 = A.pos[r0];
    // what the block's reads can reach from wbase0 (when max_span holds; else the events past it
    // take the global path), at most the passes' windows
    const int64_t cover = (int64_t)A.passes * kWinMax;
    const int64_t span = A.max_span > 0 ? (int64_t)A.pos[r1 - 1] - wbase0 + A.max_span : cover;
    const int reach = (int)(span < cover ? span : cover);
    volatile uint32_t* const mk = mark[wave];
    int j_first = wave;   // (uniform) this wave's first read (from r0) that can reach the pass
    if (tid == 0) more[0] = 0;
    for (int pass = 0;; ++pass) {
        const int64_t wb = (int64_t)wbase0 + (int64_t)pass * kWinMax;
        // the positions the pass owns from wb on: the last pass all of them (no event offset reaches 2^62)
        const int64_t own = pass == A.passes - 1 ? INT64_MAX >> 1 : (int64_t)kWinMax;
        int64_t wl = reach - pass * kWinMax;
        wl = wl > kWinMax ? kWinMax : wl;
        wl = wl > L - wb ? L - wb : wl;
        const int wlen = wl > 0 ? (int)wl : 0;
        for (int t = tid; t < wlen; t += kOpsThreads) {  // (the thread that flushed these entries)
            win[t] = 0;
            win[kWinMax + t] = 0;
            win[2 * kWinMax + t] = 0;
        }
        __syncthreads();
        if (tid == 0) more[(pass + 1) & 1] = 0;

        int j_next = -1;  // (uniform) the first read of this wave with events at or beyond we
        for (int j = j_first; j < nr; j += kOpsWaves) {
            const int64_t i = r0 + j;
            const int64_t p0 = (int32_t)uni((uint32_t)A.pos[i]);
            const int64_t lo = wb - p0, hi = lo + own;  // the pass in the read's reference offsets
            if (hi <= 0) {  // starts at or beyond the pass's end, and so does every later read
                if (j_next < 0) j_next = j;
                break;
            }
            const uint32_t* cg = A.cigar + uni(A.cig_beg[i]);
            const uint32_t cn = uni(A.cig_n[i]), sn = uni(A.seq_nib[i]);
            uint64_t R = 0;
            uint32_t Q = 0;
            bool bad = false, on = false;
            for (uint32_t k0 = 0; k0 < cn && !on; k0 += 64) {
                const OpBatch b = op_batch(cg, cn, k0, lane, R, Q);
                uint64_t e0 = R;
                if (lo > (int64_t)R) e0 += (uint64_t)(lo - (int64_t)R) & ~(uint64_t)63;  // steps below the pass
                for (; e0 < b.Rend && (int64_t)e0 < hi; e0 += 64)
                    bad |= ops_step<QUAL, NC, true>(A, mk, win, lane, e0, b.Rend, b.rs, b.rl, b.qs, b.kind, sn, p0, L, lo,
                                                    wlen, own);
                on = (int64_t)b.Rend > hi;  // (later batches lie further still)
                R = b.Rend;
                Q += b.qtot;
            }
            if (on && j_next < 0) j_next = j;
            // (atomicMin leaves the batch's smallest read, whatever pass or block saw it)
            if (__any(bad) && lane == 0) atomicMin(A.err, (unsigned long long)i);
        }
        if (j_next >= 0 && lane == 0) more[pass & 1] = 1;
        j_first = j_next >= 0 ? j_next : nr;
        __syncthreads();
        const bool go = more[pass & 1] != 0;
        ops_flush<NC>(A, win, tid, L, wb, wlen);
        if (!go) break;
    }
}

}  // namespace

// The launch bc_ops_plan describes (bc_ops_plan.h): the single-pass kernel for passes_max 1 and
// for every unsorted batch, else the window passes.
hipError_t launch_ops(hipStream_t s, const bc_reads& r, int64_t L, uint32_t mbq, int ncols, int32_t* counts,
                      unsigned long long* d_err, const struct bc_ops_plan& plan) {
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
    A.rpb = plan.reads_per_block;
    A.window = plan.window ? 1 : 0;
    A.passes = plan.passes_max;
    A.max_span = r.max_span;
    A.counts = counts;
    A.err = d_err;
    const dim3 grid((unsigned)plan.blocks), block(kOpsThreads);
    if (A.window && A.passes > 1) {
        if (mbq > 0) {
            if (ncols == 6) hipLaunchKernelGGL((k_ops_passes<true, 6>), grid, block, 0, s, A);
            else hipLaunchKernelGGL((k_ops_passes<true, 5>), grid, block, 0, s, A);
        } else {
            if (ncols == 6) hipLaunchKernelGGL((k_ops_passes<false, 6>), grid, block, 0, s, A);
            else hipLaunchKernelGGL((k_ops_passes<false, 5>), grid, block, 0, s, A);
        }
    } else if (mbq > 0) {
        if (ncols == 6) hipLaunchKernelGGL((k_ops<true, 6>), grid, block, 0, s, A);
        else hipLaunchKernelGGL((k_ops<true, 5>), grid, block, 0, s, A);
    } else {
        if (ncols == 6) hipLaunchKernelGGL((k_ops<false, 6>), grid, block, 0, s, A);
        else hipLaunchKernelGGL((k_ops<false, 5>), grid, block, 0, s, A);
    }
    return hipGetLastError();
}

}  // namespace bc
