// bc_pileup.hip — the fused, position-tiled pileup kernel (kernel 1 + kernel 2 in ONE launch).
//
// Layout: the reference is cut into 64-position tiles; a tile is owned by a group of S waves.
// Reads are coordinate-sorted, so the reads overlapping a tile form one contiguous index range,
// read from the batch's tile index (bc_reads.tile_reads) or found by a 64-ary search over pos[].  They are processed in chunks of 64: each lane
// loads one read and decodes its CIGAR into a run table (count.cpp:40-96 semantics), the chunk's
// packed sequence is staged into LDS, and then the chunk is walked with
//     lane = (window g = lane >> 3, read slot s = lane & 7):
// the lane assembles the 8 event classes its read has in reference window [t0+8g, t0+8g+8) as
// ONE 32-bit word (a funnel shift of the BC_SEQ_EVENT sequence per CIGAR run, deletions as class
// 1100) and counts all 8 positions x 6 columns with bit-plane counters (bc_planes.h; without a
// quality threshold at 32-bit indices) or SWAR nibble counters: ~22 / ~30 VALU per 8 bases.
// No atomics and no histogram memset: the 8 read slots are reduced with DPP, the S waves of a
// group through LDS atomics, and the per-position statistics of main.py:29-53 are computed in the
// same launch (kernel 2 fused: tile_tail, every wave of the group finishing and storing its own
// positions, counts included: count.cpp's baseCounts).  Reads with more than 8 CIGAR ops / 4 runs
// take a per-position walk.
//
// Positions >= L (the last, partial tile and "edge" tiles past the reference end, up to the
// furthest read end) do not count: a counted event there is the reference's std::out_of_range
// (count.cpp:60-65,85) and is recorded as the first offending read index.
#include "bc_tile.h"

namespace bc {
namespace {

// LDS seen as LDS: the tail's reads must be ds_read, not flat loads of a generic pointer.
typedef __attribute__((address_space(3))) const uint32_t lds_u32;
typedef __attribute__((address_space(3))) const double lds_f64;
struct LdsLog2Tab {  // log2d::kTab copied to LDS, indexable as tab[i][j] (glibc_log2_t)
    lds_f64* p;
    __device__ __forceinline__ lds_f64* operator[](int i) const { return p + 4 * i; }
};

// The value of the lane N places up in the same 16-lane row (DPP row_shl: no LDS traffic).  Run
// it with every lane active: an inactive source lane reads as 0.
template <int N>
__device__ __forceinline__ double row_up(double v) {
    if (N == 0) return v;
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, 0x100 + N, 0xF, 0xF, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), 0x100 + N, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// Column j's percentage and terms (oct_terms) with the log2 table in LDS.  Kept out of line:
// inlined, the log2 constants are hoisted out of the tile loop into registers the read walk
// needs.  It touches no global memory, so the call's entry and return wait for nothing.
struct ColTerms {
    double pct, t, u;
};
__device__ __attribute__((noinline)) ColTerms col_terms(OctPos o, uint32_t cj, int j, bool col, lds_f64* tab) {
    ColTerms r;
    oct_terms(o, cj, j, col, true, LdsLog2Tab{tab}, r.pct, r.t, r.u);
    return r;
}

// The first lane of each position adds its NS columns' terms (oct_sums).
template <int K, int NS>
__device__ __forceinline__ void tail_sums(const uint32_t (&c)[K], const OctPos& o, double t, double u, double nf,
                                          double nf2, double& h, double& h2) {
    double ts[K], us[K];
#pragma unroll
    for (int i = 0; i < K; ++i) ts[i] = us[i] = 0.0;
    ts[0] = t, us[0] = u;
    ts[1] = row_up<1>(t), us[1] = row_up<1>(u);
    ts[2] = row_up<2>(t), us[2] = row_up<2>(u);
    ts[3] = row_up<3>(t), us[3] = row_up<3>(u);
    if (NS > 4) ts[4] = row_up<4>(t), us[4] = row_up<4>(u);
    if (NS > 5) ts[5] = row_up<5>(t), us[5] = row_up<5>(u);
    oct_sums<K, NS>(c, o, ts, us, nf, nf2, h, h2);
}

// Fused kernel 2: the statistics of a tile from its reduced counts f[K][kTile] in LDS (bc_stats.h:
// lane j of a position's lanes owns column j; the position's first lane adds the terms).  The
// tile's four 16-position groups `first`, `first + step`, ... are this wave's.  A group whose
// columns 4.. (deletions, N) are zero at all 16 positions (wave-uniform; every group of an all-M
// batch) takes ONE pass with four lanes per position: the lanes own A, C, G, T, the sums run over
// those four columns, and the zero columns' counts and percentages (0.0, or -1.0 at zero
// coverage: oct_terms at a zero count) are stored as constants.  Any other group takes two passes
// of 8 positions with eight lanes each.  The two layouts share one body (the lane's shift is
// uniform): col_terms per column, the columns added in the same order (a zero count adds no
// term), so they give the same bits.  Nothing is read from global memory (the log2 table is in
// LDS), and a pass stores its counts, percentages, coverage and entropies last: the stores wait
// for nothing, and nothing but the wave's next pass or tile waits for them.
template <int K, typename ARGS>
__device__ __forceinline__ void tile_tail(const ARGS& A, lds_u32* f, lds_f64* tab, int first, int step, int64_t t0,
                                          int64_t L, int lane) {
    // (the tail's lane-derived indices and addresses are computed here, not hoisted out of the
    // tile loop and kept in registers through the read walk)
    asm volatile("" : "+v"(lane));
    for (int gq = first; gq < kTile / 16; gq += step) {
        uint32_t rare = 0;
#pragma unroll
        for (int i = 4; i < K; ++i) rare |= f[i * kTile + 16 * gq + (lane & 15)];
        const bool four = !__any(rare != 0);  // (uniform) four lanes per position, one pass
        const int sh = four ? 2 : 3;
        const int j = lane & ((1 << sh) - 1);
        for (int q = 0; q < (four ? 1 : 2); ++q) {
            const int p = 16 * gq + 8 * q + (lane >> sh);
            const int64_t P = t0 + p;
            const bool col = j < K && P < L;
            uint32_t c[K];
#pragma unroll
            for (int i = 0; i < K; ++i) c[i] = f[i * kTile + p];
            const uint32_t cj = f[(j < K ? j : 0) * kTile + p];
            const OctPos o = oct_pos<K>(c);
            const ColTerms r = col_terms(o, cj, j, col, tab);
            double h, h2;
            if (four) tail_sums<K, 4>(c, o, r.t, r.u, A.nf, A.nf2, h, h2);
            else tail_sums<K, K>(c, o, r.t, r.u, A.nf, A.nf2, h, h2);
            if (col) {
                A.counts[(int64_t)j * L + P] = (int32_t)cj;
                if (A.pc) A.pc[(int64_t)j * L + P] = r.pct;
            }
            // the zero columns, which no lane owns.  K = 6: lane j stores column 4 + j; K = 5: the
            // first lane stores the one column with its own outputs (either form for both K costs
            // one of the quality variants a spilled VGPR: scripts/resources.py)
            if (K > 5 && four && j + 4 < K && P < L) {
                A.counts[(int64_t)(j + 4) * L + P] = 0;
                if (A.pc) A.pc[(int64_t)(j + 4) * L + P] = o.cov != 0 ? 0.0 : -1.0;
            }
            if (j == 0 && P < L) {
                A.cov[P] = (int32_t)o.cov;
                A.ent[P] = h;
                A.sec[P] = h2;
                if (K == 5 && four) {
                    A.counts[(int64_t)4 * L + P] = 0;
                    if (A.pc) A.pc[(int64_t)4 * L + P] = o.cov != 0 ? 0.0 : -1.0;
                }
            }
        }
    }
}

// LEAN: the register- and LDS-lean instance (process_chunk: the one-run window walk, every other
// read alone in walk_complex) at five waves per SIMD instead of four; exact on any batch, ahead
// while slow reads are few (launch_pileup_tiles routes).
// SLICE (with LEAN): the lean walk over per-read slices (process_chunk, bc_slice.h): 4 KiB of
// stage per wave whatever the read length, and six waves per SIMD.
template <bool QUAL, int K, bool STATS, typename IT, bool LEAN = false, bool SLICE = false>
__global__ __launch_bounds__(512, SLICE ? 6 : LEAN ? 5 : 4) void k_pileup(TileArgs A) {
    static_assert(!SLICE || (LEAN && !QUAL && sizeof(IT) == 4), "slice instances: lean, no threshold, 32-bit indices");
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    __shared__ IT rng[8][2];  // per group: the tile's read range
    if (BC_ABL(A) & 64) return;
    trace_stamp(A, 0);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    const int S = A.S;
    const int g = wave / S, ws = wave - g * S;
    const int groups = nw / S;
    constexpr int rec_bytes = LEAN ? kLeanRecBytes : kRecBytes;
    constexpr int stage_region = SLICE ? kSliceStageRegion : LEAN ? kLeanStageRegion : kStageRegion;
    uint4* rec_all = (uint4*)dyn;
    uint8_t* stage_all = dyn + (size_t)nw * rec_bytes;
    uint32_t(*fin)[6][kTile] = (uint32_t(*)[6][kTile])(stage_all + (size_t)nw * stage_region);
    double2* tab = (double2*)((uint8_t*)fin + (size_t)groups * kFinBytes);  // log2d::kTab for the tail
    // IT: the index type of reads, tiles and positions (int32_t when they fit: scalar math)
    const IT n_tiles = (IT)A.n_tiles;
    const IT nblk_tiles = (n_tiles + groups - 1) / groups;
    const IT L = (IT)A.L;
    const int s8 = lane & 7;
    const bool qual_vec = ((uintptr_t)A.qual & 15u) == 0;
    constexpr bool PLANES = !QUAL && sizeof(IT) == 4;  // bit-plane counters (bc_walk.h: WalkCounters)
    if (STATS && S == 1) {  // no barrier per tile: the table is copied once
        if (threadIdx.x < 128) tab[threadIdx.x] = ((const double2*)log2d::kTab)[threadIdx.x];
        __syncthreads();
    }

    // XCD-aware: workgroups are dispatched round-robin over the 8 XCDs; give each XCD a
    // contiguous run of tiles so neighbouring tiles (which share ~2/3 of their reads) hit the
    // same L2 instead of fetching the reads' CIGAR / sequence from HBM once per tile
    const IT G = gridDim.x;
    const IT lb = (G % 8 == 0) ? (IT)(blockIdx.x % 8) * (G / 8) + (IT)(blockIdx.x / 8) : (IT)blockIdx.x;
    for (IT bt = lb; bt < nblk_tiles; bt += G) {
        const IT t = bt * groups + g;
        const IT t0 = t * kTile;
        const IT P = t0 + lane;
        const int gb = (int)t0 + 8 * (lane >> 3);  // this lane's window [gb, gb + 8)
        uint32_t cnt[6] = {0, 0, 0, 0, 0, 0};
        int64_t bad = INT64_MAX;
        // the tile's reads [lo, hi): searched by the group's first wave (the S waves would all
        // find the same range), handed to the others through LDS
        IT lo = 0, hi = 0;
        // the log2 table's way to LDS shares the range's memory round trip (S > 1: written again
        // for every tile, which costs one L2 hit and keeps four registers out of the tile loop)
        double2 tabv = {0.0, 0.0};
        if (STATS && S > 1 && threadIdx.x < 128) tabv = ((const double2*)log2d::kTab)[threadIdx.x];
        if (ws == 0 && t < n_tiles && !(BC_ABL(A) & 2)) {
#ifdef BC_PHASE_TRACE
            if (A.trace) {  // diagnostic: latency of one dependent global load from here
                const int32_t probe = A.pos[(lane * 1543) % (int)A.n];
                if (probe == 0x7FFFFFFF) A.trace[0] = 1;
                trace_stamp(A, 8);
                const int32_t probe2 = A.pos[(lane * 977 + 5 + (probe & 1)) % (int)A.n];
                if (probe2 == 0x7FFFFFFF) A.trace[0] = 1;
                trace_stamp(A, 10);
                const int32_t probe3 = A.cigar[(lane * 977 + 11 + (probe2 & 1)) % (int)A.n];
                if (probe3 == 0x7FFFFFFF) A.trace[0] = 1;
                trace_stamp(A, 11);
            }
#endif
            if (t < A.n_trange) {  // the upload's tile index: one load instead of a search
                const int2 rg = A.trange[t];
                lo = rg.x;
                hi = rg.y;
            } else {
                int64_t l64, h64;
                int sl = lane;
                // (SLICE: the search's lane-derived operands are computed here, not hoisted out of
                // the tile loop into registers the six-wave budget does not have)
                if constexpr (SLICE) asm volatile("" : "+v"(sl));
                lower_bound_pair(A.pos, A.n, (int64_t)t0 - A.max_span + 1, (int64_t)t0 + kTile, sl, l64, h64);
                lo = (IT)l64;
                hi = (IT)h64;
            }
            trace_stamp(A, 9);
        }
        if (S > 1) {
            if (ws == 0 && lane == 0) rng[g][0] = lo, rng[g][1] = hi;
            if (ws == 0) {  // the S waves add their counts here after the walk
#pragma unroll
                for (int c = 0; c < K; ++c) fin[g][c][lane] = 0u;
            }
            if (STATS && threadIdx.x < 128) tab[threadIdx.x] = tabv;
            __syncthreads();
            trace_stamp(A, 1);
            lo = rng[g][0];
            hi = rng[g][1];
        }
        if (t < n_tiles) {
            if (BC_ABL(A) & 1) hi = lo;
            const bool edge = t0 + kTile > L;  // uniform
            const bool beyond = P >= L;
            uint32_t bmask = 0;                // window nibbles at positions >= L
            if (edge) {
                int64_t kL = L - gb;
                kL = kL < 0 ? 0 : (kL > 8 ? 8 : kL);
                bmask = ~(lo32_bit(4 * (int)kL) - 1u);
            }
            unsigned long long acc = 0;
            int pending = 0;
            typename WalkCounters<PLANES>::type W;
            counters_zero(W);
            uint4* myrec = rec_all + wave * (rec_bytes / 16);
            uint8_t* mystage = stage_all + (size_t)wave * stage_region + 16;
            auto chunk_nr = [&](IT b) { return b < hi ? (int)((hi - b) < 64 ? (hi - b) : 64) : 0; };
            IT base = lo + (IT)ws * 64;
            ReadFields F = load_fields(A, base, chunk_nr(base), lane);
#ifdef BC_PHASE_TRACE
            int nch = 0;
#endif
            for (; base < hi; base += (IT)S * 64) {
                const IT nb = base + (IT)S * 64;
                process_chunk<QUAL, K, PLANES, LEAN, SLICE>(A, base, chunk_nr(base), F, nb, chunk_nr(nb), lane, s8, gb, t0, P,
                                                     edge, beyond, bmask, myrec, mystage, qual_vec, W, cnt, acc,
                                                     pending, bad);
                __builtin_amdgcn_wave_barrier();
#ifdef BC_PHASE_TRACE
                if (nch < 2) trace_stamp(A, 2 + nch);
                ++nch;
#endif
            }
            flush_acc(acc, cnt);
            counters_finish<K>(W, cnt, s8);
            if (edge) {  // first offending read of this tile (std::out_of_range in the reference)
                for (int o = 32; o > 0; o >>= 1) {
                    const int64_t b2 = __shfl_down(bad, o);
                    bad = b2 < bad ? b2 : bad;
                }
                if (lane == 0 && bad != INT64_MAX) atomicMin(A.err, (unsigned long long)bad);
            }
        }
        // ---- reduce the S waves of the group: LDS atomics into fin (zeroed before the range
        // barrier), so every wave reads the totals after one barrier.  S == 1: the wave's own
        // counts, handed to its own tail through LDS (no other wave touches fin[g]).
        const bool more = bt + G < nblk_tiles;  // (uniform over the block) another tile follows
        if (S > 1) {
#pragma unroll
            for (int c = 0; c < K; ++c) atomicAdd(&fin[g][c][lane], cnt[c]);
            __syncthreads();
            trace_stamp(A, 4);
            if (!STATS && ws == 0) {
#pragma unroll
                for (int c = 0; c < K; ++c) cnt[c] = fin[g][c][lane];
            }
        } else if (STATS) {
#pragma unroll
            for (int c = 0; c < K; ++c) fin[g][c][lane] = cnt[c];
            __builtin_amdgcn_wave_barrier();
        }
        const bool own = t < n_tiles && t0 < L && !(BC_ABL(A) & 16);  // tile holds real positions
        if (!STATS) {
            if (ws == 0 && own && P < L) {
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    int32_t* dst = A.counts + (int64_t)c * L + P;
                    if (A.accumulate) cnt[c] += (uint32_t)*dst;
                    *dst = (int32_t)cnt[c];
                }
            }
        } else {
            trace_stamp(A, 5);
            // ---- fused kernel 2: every wave finishes its share of the tile's positions and
            // stores them, counts included
            if (own && !(BC_ABL(A) & 8))
                tile_tail<K>(A, (lds_u32*)&fin[g][0][0], (lds_f64*)tab, ws, S, (int64_t)t0, (int64_t)L, lane);
            trace_stamp(A, 6);
        }
        // fin and rng are written again for the block's next tile: not before every wave has read
        // them.  The last tile (every tile of a one-round grid) ends without a barrier.
        if (S > 1 && more) __syncthreads();
        trace_stamp(A, 7);
    }
}

// ---- sparse batches (at most ~48 reads per tile): one wave per tile, tiles swept in order ----

// Kernel 2 for one position from its counts (bc_stats.h: the bits of k_pileup's tail), written
// by the position's lane.
template <int K>
__device__ __forceinline__ double pos_stats(const PileArgs& A, const uint32_t* c, int64_t P) {
    return position_stats<K>(c, A.L, P, A.nf, A.nf2, A.cov, A.pc, A.ent, A.sec);
}

// Move a read cursor forward to the first index >= cur whose pos >= key (pos is sorted and the
// keys of successive tiles increase).  `win` holds pos[wbase + lane]: the 64 reads after the
// cursor are looked at with one ballot, refilled only when the cursor leaves them.
// IT: the index type of reads and positions (int32_t when both fit, so the cursor arithmetic
// stays on the scalar unit; int64_t otherwise).
template <typename IT>
__device__ __forceinline__ void advance_cursor(const int32_t* pos, IT n, IT& cur, IT key, int32_t& win, IT& wbase,
                                               int lane) {
    for (;;) {
        if (cur >= n) return;
        if (cur >= wbase + 64) {
            wbase = cur;
            const IT i = wbase + lane;
            win = i < n ? pos[i] : INT32_MAX;
        }
        const int below = __popcll(__ballot((IT)win < key));  // a prefix of the window
        IT end = wbase + below;
        end = end < n ? end : n;
        if (end > cur) cur = end;
        if (below < 64 || cur >= n) return;
        cur = wbase + 64;
    }
}

// Sparse batches: every wave owns a contiguous run of tiles and sweeps it with two read cursors
// (no per-tile search), walks the few reads of each tile alone, and computes the statistics of
// its own positions in registers: no block barriers at all.  Empty tiles only store.
// STORE = false (with STATS and SUMP; bc_pileup_partials with no outputs, the summary of
// main.py:469-499): no per-position output at all but the last partial buffer's coverage and
// entropy; the summary partials alone are written, and a quarter buffer with no reads is one
// constant store (its 16 leaves are 128.0 each: 2048.0, exactly).
// per wave: a quarter's 16 leaves, then the 64-double transposition scratch (80 doubles: four
// 4-wave workgroups with their records and stages fit a CU's 160 KiB of LDS)
constexpr int kLeafDoubles = 16 + 64;
static_assert(4 * (4 * (kRecBytes + kStageRegion) + 4 * kLeafDoubles * 8) <= 160 * 1024, "4 workgroups per CU");
template <bool QUAL, int K, bool STATS, bool SUMP, typename IT, bool STORE = true>
__global__ __launch_bounds__(256, 4) void k_pileup_solo(PileArgs A) {
    static_assert(STORE || (STATS && SUMP), "the summary-only sweep computes the summary partials");
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    uint4* myrec = (uint4*)dyn + wave * kTile * 3;
    uint8_t* mystage = dyn + (size_t)nw * kRecBytes + (size_t)wave * kStageRegion + 16;
    const IT L = (IT)A.L, n = (IT)A.n;
    const int s8 = lane & 7;
    const bool qual_vec = ((uintptr_t)A.qual & 15u) == 0;
    const IT G = gridDim.x;
    const IT lb = (G % 8 == 0) ? (IT)(blockIdx.x % 8) * (G / 8) + (IT)(blockIdx.x / 8) : (IT)blockIdx.x;
    const IT tpw = (IT)A.tiles_per_wave;
    const IT t_begin = (lb * nw + wave) * tpw;
    const IT t_end = t_begin + tpw < (IT)A.n_tiles ? t_begin + tpw : (IT)A.n_tiles;
    if (t_begin >= t_end) return;  // no barriers in this kernel
    IT lo, hi;
    {
        int64_t l64, h64;
        lower_bound_pair(A.pos, A.n, (int64_t)t_begin * kTile - A.max_span + 1, (int64_t)t_begin * kTile + kTile, lane,
                         l64, h64);
        lo = (IT)l64;
        hi = (IT)h64;
    }
    IT wlo_base = lo, whi_base = hi;
    int32_t wlo = lo + lane < n ? A.pos[lo + lane] : INT32_MAX;
    int32_t whi = hi + lane < n ? A.pos[hi + lane] : INT32_MAX;
    const IT max_span = (IT)A.max_span;
    // SUMP: the wave's tiles start on a quarter-buffer boundary (tiles_per_wave is a multiple of
    // 32), so it sees whole 2048-position quarters, each a subtree of numpy's pairwise tree over
    // an 8192 buffer (split evenly down to 128-element leaves): leaves of two tiles wait in LDS (16
    // per quarter) and are added pairwise across the lanes once the quarter is complete; the fold
    // kernel joins the 4 quarters of a buffer
    double e_prev = 0.0;
    bool prev_empty = false;
    double* myleaves = (double*)(dyn + (size_t)nw * (kRecBytes + kStageRegion)) + kLeafDoubles * wave;
    double* mytr = myleaves + 16;  // transposition scratch of the leaf sums (64 doubles)
    long long sum_cov = 0, sum_nz = 0;
    // SUMP: tile t's share of numpy's pairwise leaves (h: its entropies; an empty tile's are 1.0)
    auto leaf_step = [&](IT t, bool empty, double h) {
        if (t & 1) {
            const double lf = (prev_empty && empty) ? 128.0
                              : empty                 ? leaf_finish_ones(prev_empty ? 8.0 : e_prev, lane, mytr)
                                                      : leaf_finish(prev_empty ? 8.0 : e_prev, h, lane, mytr);
            const int leaf = (int)((t >> 1) & 15);
            if (lane == 0) myleaves[leaf] = lf;
            if (leaf == 15) {  // the quarter is complete: its 16 leaves, pairwise
                __builtin_amdgcn_wave_barrier();
                double v = myleaves[lane & 15];
#pragma unroll
                for (int l = 1; l < 16; l <<= 1) {  // left (lower lanes) + right
                    const double w = __shfl_down(v, l);
                    if ((lane & (2 * l - 1)) == 0) v = v + w;
                }
                const long long cs = wave_sum_i64(sum_cov), nz = wave_sum_i64(sum_nz);
                if (lane == 0) {
                    const int64_t q = t >> 5;
                    A.sub_ent[q] = v;
                    A.sub_cov[q] = cs;
                    A.sub_nz[q] = nz;
                }
                sum_cov = sum_nz = 0;
            }
        } else {
            prev_empty = empty;  // an empty first tile's half is 8.0 (leaf_finish_ones)
            if (!empty) e_prev = leaf_half(h, lane, mytr);  // its half of the chains
        }
    };
    for (IT t = t_begin; t < t_end; ++t) {
        const IT t0 = t * kTile;
        const IT P = t0 + lane;
        const int gb = (int)t0 + 8 * (lane >> 3);
        if (t > t_begin) {
            advance_cursor<IT>(A.pos, n, lo, t0 - max_span + 1, wlo, wlo_base, lane);
            advance_cursor<IT>(A.pos, n, hi, t0 + kTile, whi, whi_base, lane);
        }
        if (STATS && lo >= hi && !A.accumulate && !(BC_ABL(A) & 16)) {
            // No read overlaps this tile, nor any tile before the next read's start tile: write
            // that run of full tiles' constant outputs (main.py:29-53 at zero coverage) without
            // per-tile cursor work.  The next tile with reads resumes the normal path.
            IT nxt = t_end;
            if (hi < n) {
                const IT d = hi - whi_base;  // in [0, 64]: the window holds pos[whi_base ..]
                const int32_t ph = d < 64 ? (int32_t)__builtin_amdgcn_readlane(whi, (int)d) : A.pos[hi];
                nxt = (IT)(ph >> 6);
            }
            IT stop = nxt < t_end ? nxt : t_end;
            const IT full = L / kTile;  // tiles entirely below L
            stop = stop < full ? stop : full;
            if (stop > t + 1) {
                for (; t < stop; ++t) {
                    const IT tz = t * kTile;
                    const bool whole = SUMP && (int64_t)(tz >> 13) < A.full_chunks;  // in a whole buffer
                    if (STORE) {
#pragma unroll
                        for (int c = 0; c < K; ++c) (A.counts + ((int64_t)c * L + tz))[lane] = 0;
                        (A.cov + tz)[lane] = 0;
                        if (A.pc) {
#pragma unroll
                            for (int j = 0; j < K; ++j) (A.pc + ((int64_t)j * L + tz))[lane] = -1.0;
                        }
                        (A.ent + tz)[lane] = 1.0;
                        (A.sec + tz)[lane] = 1.0;
                    } else if (!whole) {  // the last partial buffer: coverage 0, entropy 1
                        const int64_t i = (int64_t)tz - A.full_chunks * kNpBuf + lane;
                        A.cov_tail[i] = 0;
                        A.ent_tail[i] = 1.0;
                        continue;
                    } else if ((t & 31) == 0 && t + 32 <= stop) {
                        // a whole quarter without reads (32 tiles, one subtree of numpy's tree;
                        // the quarters before it left the coverage sums at 0)
                        if (lane == 0) {
                            const int64_t q = (int64_t)(t >> 5);
                            A.sub_ent[q] = 2048.0;
                            A.sub_cov[q] = 0;
                            A.sub_nz[q] = 0;
                        }
                        t += 31;
                        continue;
                    }
                    if (whole) leaf_step(t, true, 1.0);
                }
                --t;  // the loop's increment moves to `stop`
                continue;
            }
        }
        uint32_t cnt[6] = {0, 0, 0, 0, 0, 0};
        if (hi > lo) {
            int64_t bad = INT64_MAX;
            const bool edge = t0 + kTile > L;
            const bool beyond = P >= L;
            uint32_t bmask = 0;
            if (edge) {
                int64_t kL = L - gb;
                kL = kL < 0 ? 0 : (kL > 8 ? 8 : kL);
                bmask = ~(lo32_bit(4 * (int)kL) - 1u);
            }
            unsigned long long acc = 0;
            int pending = 0;
            SwarCnt W;
            counters_zero(W);
            auto chunk_nr = [&](int64_t b) { return b < hi ? (int)((hi - b) < 64 ? (hi - b) : 64) : 0; };
            ReadFields F = load_fields(A, lo, chunk_nr(lo), lane);
            for (int64_t base = lo; base < (int64_t)hi; base += 64) {
                process_chunk<QUAL, K, false>(A, base, chunk_nr(base), F, base + 64, chunk_nr(base + 64), lane, s8, gb, t0, P,
                                       edge, beyond, bmask, myrec, mystage, qual_vec, W, cnt, acc, pending, bad);
                __builtin_amdgcn_wave_barrier();
            }
            flush_acc(acc, cnt);
            counters_finish<K>(W, cnt, s8);
            if (edge) {
                for (int o = 32; o > 0; o >>= 1) {
                    const int64_t b2 = __shfl_down(bad, o);
                    bad = b2 < bad ? b2 : bad;
                }
                if (lane == 0 && bad != INT64_MAX) atomicMin(A.err, (unsigned long long)bad);
            }
        }
        const bool empty = hi <= lo;  // (uniform) no read overlaps the tile: all counts zero
        if (!STORE && t0 < L && P < L) {  // summary only: coverage and entropy, no stores
            uint32_t cov;
            const double h = position_entropy<K>(cnt, A.nf, cov);
            if ((int64_t)(t0 >> 13) < A.full_chunks) {
                if (!empty) {
                    sum_cov += cov;
                    sum_nz += cov != 0;
                }
                leaf_step(t, empty, h);
            } else {
                const int64_t i = (int64_t)P - A.full_chunks * kNpBuf;
                A.cov_tail[i] = (int32_t)cov;
                A.ent_tail[i] = h;
            }
        } else if (STORE && t0 < L && P < L && !(BC_ABL(A) & 16)) {
#pragma unroll
            for (int c = 0; c < K; ++c) {
                int32_t* cb = A.counts + ((int64_t)c * L + t0);  // (uniform)
                if (A.accumulate) cnt[c] += (uint32_t)cb[lane];
                cb[lane] = (int32_t)cnt[c];
            }
            if (STATS) {
                // (an explicit zero-coverage branch here costs registers: the kernel spills)
                const double h = pos_stats<K>(A, cnt, P);
                if (SUMP) {
                    static_assert(kNpBuf == 8192 && kNpBuf == 128 * kTile, "buffers of 128 tiles");
                    const int64_t ch = t0 >> 13;  // 8192-position buffer
                    if (ch < A.full_chunks) {
                        if (!empty) {
                            const uint32_t cov = cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[4] + (K == 6 ? cnt[5] : 0u);
                            sum_cov += cov;
                            sum_nz += cov != 0;
                        }
                        leaf_step(t, empty, h);
                    }
                }
            }
        }
    }
}

}  // namespace


int pileup_waves(const bc_reads& r, int64_t L, int64_t max_end, int tile_waves) {
    if (tile_waves == 1 || tile_waves == 2 || tile_waves == 4 || tile_waves == 8) return tile_waves;
    // waves per tile from the mean number of reads a tile walks: up to 48 one wave (the sparse
    // sweep), else the smallest S in {4, 8} with per_tile <= 512 S.  Sized for batches in flight:
    // a wave holds its slot for the workgroup's whole life, so it is the resident waves that set
    // the rate of a stream of batches.  Four 4-wave workgroups fill a CU (16 waves, 4 x 40 KiB
    // of LDS) where two 8-wave ones wait on each other's barriers; two waves per tile (three
    // 4-wave workgroups of two tiles per CU) were behind four at every depth measured, eight
    // behind four up to the switch to k_rc ("What bounds C2").  One batch
    // alone finishes sooner with tile_waves = 8.
    const double per_tile = pileup_reads_per_tile(r, L, max_end);
    if (per_tile <= kSoloMaxReadsPerTile) return 1;
    return per_tile <= kTileReadsPerWave * 4 ? 4 : 8;
}

double pileup_reads_per_tile(const bc_reads& r, int64_t L, int64_t max_end) {
    // reads overlapping a tile ~ density * (span + 63)
    const int64_t reach = max_end > L ? max_end : L;
    return reach > 0 ? (double)r.n_reads * (double)(r.max_span + kTile - 1) / (double)reach : 0.0;
}

namespace {

// k_pileup's launch shape for n_tiles tiles at S waves per tile
struct TileShape {
    int nw, groups;  // waves and tiles per workgroup
    int64_t blocks;
    size_t lds;      // dynamic
};
TileShape tile_shape(int64_t n_tiles, int S, int inst = kInstGeneral) {
    TileShape t;
    t.nw = S >= 4 ? S : 4;
    t.groups = t.nw / S;
    t.blocks = (n_tiles + t.groups - 1) / t.groups;
    const int64_t cap = 256 * 64;
    if (t.blocks > cap) t.blocks = cap;
    t.blocks = (t.blocks + 7) / 8 * 8;  // a multiple of the XCD count (see the kernel's tile mapping)
    t.lds = pileup_lds_bytes(t.nw, t.groups, inst);
    return t;
}

// ---- k_pileup's instances ----
// The lean instance is built where it holds five waves per SIMD (at most 96 VGPRs, nothing
// spilled: scripts/resources.py); every other combination has the
// general instance alone.
// The slice instance is built where the LDS-DMA staging runs and the planes walk is taken: no
// quality threshold, 32-bit indices (four kernels: k = 5, 6 with and without statistics), each at
// six waves per SIMD (at most 80 VGPRs, nothing spilled: round 11).
constexpr bool lean_built(bool qual, bool i32) { return !qual || i32; }
constexpr bool slice_built(bool qual, bool i32) { return !qual && i32; }
typedef void (*TileKernel)(TileArgs);
template <bool Q, int KK, bool ST, typename IT>
TileKernel tile_kernel_of(int inst) {
    if constexpr (slice_built(Q, sizeof(IT) == 4)) {
        if (inst == kInstSlice) return k_pileup<Q, KK, ST, IT, true, true>;
    }
    if constexpr (lean_built(Q, sizeof(IT) == 4)) {
        if (inst == kInstLean) return k_pileup<Q, KK, ST, IT, true>;
    }
    return k_pileup<Q, KK, ST, IT, false>;
}
template <bool Q, int KK>
TileKernel tile_kernel_qk(bool stats, bool i32, int inst) {
    if (stats) return i32 ? tile_kernel_of<Q, KK, true, int32_t>(inst) : tile_kernel_of<Q, KK, true, int64_t>(inst);
    return i32 ? tile_kernel_of<Q, KK, false, int32_t>(inst) : tile_kernel_of<Q, KK, false, int64_t>(inst);
}
TileKernel tile_kernel(bool qual, int k, bool stats, bool i32, int inst) {
    if (qual) return k == 5 ? tile_kernel_qk<true, 5>(stats, i32, inst) : tile_kernel_qk<true, 6>(stats, i32, inst);
    return k == 5 ? tile_kernel_qk<false, 5>(stats, i32, inst) : tile_kernel_qk<false, 6>(stats, i32, inst);
}
// > 64 KiB of dynamic LDS must be allowed per kernel (160 KiB per CU on gfx950), once
void allow_lds(TileKernel fn) {
    static TileKernel done[64];
    static int n_done = 0;
    for (int i = 0; i < n_done; ++i)
        if (done[i] == fn) return;
    (void)hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024);
    if (n_done < 64) done[n_done++] = fn;
}

// Both instances are exact; the lean one is ahead while the reads walk_complex takes alone are
// few.  A read of more than one run has at least three CIGAR ops (an op between the runs), so
// such reads <= (CIGAR words - reads) / 2; a one-run read that begins or ends with a deletion is
// slow with two ops and is not expected in numbers.  n_cigar_words counts the buffer: for a slice that shares a larger batch's CIGAR
// buffer the bound is the larger batch's (never too small), and such a slice takes the general
// instance unless every read of the buffer has one op (kLeanMaxSlowShare is zero: measured).
bool tile_lean(const bc_reads& r, bool qual, bool i32, int instance) {
    if (!lean_built(qual, i32) || instance == BC_INSTANCE_GENERAL) return false;
    if (instance == BC_INSTANCE_LEAN || instance == BC_INSTANCE_SLICE) return true;
    const int64_t extra = r.n_cigar_words - r.n_reads;
    const double slow_max = extra > 0 ? (double)extra / 2.0 : 0.0;
    return slow_max <= kLeanMaxSlowShare * (double)r.n_reads;
}
// The instance launched (TileInstance).  The slice instance is the lean walk at six workgroups per
// CU instead of five, and it stages a read's 64-B slice once per tile where the lean instance
// stages the whole read: BC_INSTANCE_AUTO takes it wherever it takes the lean walk, a slice
// instance is built, and a read can be longer than a tile (max_span > kTile: only then is a slice
// less than the read).  Forced where none is built it falls back as a forced lean instance does.
int tile_instance(const bc_reads& r, bool qual, bool i32, int instance) {
    if (!tile_lean(r, qual, i32, instance)) return kInstGeneral;
    if (!slice_built(qual, i32) || instance == BC_INSTANCE_LEAN) return kInstLean;
    return (instance == BC_INSTANCE_SLICE || r.max_span > kTile) ? kInstSlice : kInstLean;
}

// the sparse sweep's: tiles per wave and workgroups of kSoloWaves waves (sump: whole quarter
// buffers per wave)
constexpr int kSoloWaves = 4;
int64_t solo_tiles_per_wave(int64_t n_tiles, bool sump) {
    // ~8 rounds of resident waves (256 CUs x 16): shorter runs shorten the last round's tail
    // (C5: 31.6 ms at 2 rounds, 30.2-30.6 at 4-8, 30.4-30.8 at 16-32)
    const int64_t target_waves = 256 * 16 * 8;
    int64_t tpw = (n_tiles + target_waves - 1) / target_waves;
    if (tpw < 1) tpw = 1;
    if (sump) tpw = (tpw + 31) / 32 * 32;
    return tpw;
}
int64_t solo_blocks(int64_t n_tiles, int64_t tpw) {
    const int64_t waves = (n_tiles + tpw - 1) / tpw;
    const int64_t blocks = (waves + kSoloWaves - 1) / kSoloWaves;
    return (blocks + 7) / 8 * 8;  // a multiple of the XCD count (see the kernel's tile mapping)
}

// 32-bit reads, tiles and positions when they fit
bool tiles_fit_i32(int64_t n, int64_t n_tiles, int max_span) {
    return n < (int64_t)0x7FFFFF00 && n_tiles * kTile + max_span + 2 * kTile < (int64_t)0x7FFFFF00;
}

}  // namespace

void pileup_plan(const bc_reads& r, int64_t L, int shape, int tile_waves, bc_plan& p) {
    p = bc_plan{};
    p.blocks_per_cu = -1;
    p.reads_per_tile = pileup_reads_per_tile(r, L, r.max_end);
    if (use_rc(r, L, shape)) {
        p.kernel = BC_PLAN_RC;
        return;
    }
    const int S = pileup_waves(r, L, r.max_end, tile_waves);
    const int64_t reach = r.max_end > L ? r.max_end : L;
    const int64_t n_tiles = (reach + kTile - 1) / kTile;
    const bool i32 = tiles_fit_i32(r.n_reads, n_tiles, r.max_span);
    const void* fn;
    size_t dyn;
    p.waves_per_tile = S;
    if (S == 1 && shape != BC_SHAPE_TILE_NO_SOLO) {
        p.kernel = BC_PLAN_SOLO;
        p.block_threads = 64 * kSoloWaves;
        p.tiles_per_wave = (int32_t)solo_tiles_per_wave(n_tiles, false);
        p.blocks = solo_blocks(n_tiles, p.tiles_per_wave);
        dyn = (size_t)kSoloWaves * (kRecBytes + kStageRegion);
        p.lds_bytes = (int32_t)dyn;
        fn = i32 ? (const void*)k_pileup_solo<false, 5, true, false, int32_t>
                 : (const void*)k_pileup_solo<false, 5, true, false, int64_t>;
    } else {
        const TileShape t = tile_shape(n_tiles, S);
        p.kernel = BC_PLAN_TILES;
        p.block_threads = 64 * t.nw;
        p.blocks = t.blocks;
        dyn = t.lds;
        p.lds_bytes = (int32_t)(dyn + 8 * 2 * (i32 ? 4 : 8));  // + rng, the static range hand-off
        fn = i32 ? (const void*)k_pileup<false, 5, true, int32_t> : (const void*)k_pileup<false, 5, true, int64_t>;
    }
    if (n_tiles == 0) p.blocks = 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return;
    }
    // (more than 64 KiB of dynamic LDS must be allowed per kernel before the runtime counts with it)
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024);
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, p.block_threads, dyn) == hipSuccess) p.blocks_per_cu = nb;
    else (void)hipGetLastError();
}

void pileup_launch_info(const bc_reads& r, int64_t L, int shape, int tile_waves, int instance, uint32_t mbq, int k,
                        bc_launch_info& o) {
    o = bc_launch_info{};
    o.blocks_per_cu = -1;
    bc_plan p;
    pileup_plan(r, L, shape, tile_waves, p);  // the kernel, and everything of the general instance
    o.kernel = p.kernel;
    o.waves_per_tile = p.waves_per_tile;
    o.block_threads = p.block_threads;
    o.lds_bytes = p.lds_bytes;
    o.blocks = p.blocks;
    if (p.kernel != BC_PLAN_TILES) {
        o.blocks_per_cu = p.blocks_per_cu;  // (the sparse sweep's mbq = 0, k = 5 variant)
        return;
    }
    const int64_t reach = r.max_end > L ? r.max_end : L;
    const int64_t n_tiles = (reach + kTile - 1) / kTile;
    const bool i32 = tiles_fit_i32(r.n_reads, n_tiles, r.max_span);
    const int inst = tile_instance(r, mbq > 0, i32, instance);
    const TileShape t = tile_shape(n_tiles, p.waves_per_tile, inst);
    o.lean = inst != kInstGeneral ? 1 : 0;
    o.lds_bytes = (int32_t)(t.lds + 8 * 2 * (i32 ? 4 : 8));  // + rng, the static range hand-off
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return;
    }
    const TileKernel fn = tile_kernel(mbq > 0, k, true, i32, inst);
    allow_lds(fn);
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)fn, o.block_threads, t.lds) == hipSuccess)
        o.blocks_per_cu = nb;
    else (void)hipGetLastError();
}

hipError_t launch_pileup_tiles(hipStream_t s, const bc_reads& r, int64_t L, int64_t max_end, uint32_t mbq, int k,
                               bool stats, bool accumulate, double nf, double nf2, int32_t* counts, int32_t* cov,
                               double* pc, double* ent, double* sec, unsigned long long* d_err, int shape,
                               int tile_waves, int instance, SumParts* parts) {
    PileArgs A = make_args(r, L, mbq);
    const int64_t reach = max_end > L ? max_end : L;  // edge tiles up to the furthest read end
    A.n_tiles = (reach + kTile - 1) / kTile;
    if (A.n_tiles == 0) return hipSuccess;
    A.accumulate = accumulate ? 1 : 0;
    A.nf = nf;
    A.nf2 = nf2;
    A.counts = counts;
    A.cov = cov;
    A.pc = pc;
    A.ent = ent;
    A.sec = sec;
    A.err = d_err;
#ifdef BC_DIAG
    if (const char* ab = std::getenv("BC_ABLATE")) A.ablate = std::atoi(ab);
#endif
    const int S = pileup_waves(r, L, max_end, tile_waves);
    A.S = S;
    if (parts) parts->fused = false;
    if (S == 1 && shape != BC_SHAPE_TILE_NO_SOLO) {
        // sparse: waves sweep contiguous tile runs
        const int nw = kSoloWaves;
        const bool sump = parts && stats && L >= kNpBuf;
        const bool nostore = sump && parts->no_store;
        A.tiles_per_wave = solo_tiles_per_wave(A.n_tiles, sump);
        if (sump) {  // whole quarter buffers per wave: the summary partials come for free
            A.sub_ent = parts->sub_ent;
            A.sub_cov = parts->sub_cov;
            A.sub_nz = parts->sub_nz;
            A.full_chunks = L / kNpBuf;
            parts->fused = true;
            parts->full_chunks = A.full_chunks;
            A.cov_tail = parts->cov_tail;
            A.ent_tail = parts->ent_tail;
        }
        const int64_t blocks = solo_blocks(A.n_tiles, A.tiles_per_wave);
        const dim3 grid((unsigned)blocks), block(64 * nw);
        const size_t lds = (size_t)nw * (kRecBytes + kStageRegion) + (sump ? (size_t)nw * kLeafDoubles * 8 : 0);
        // 32-bit reads and positions when they fit (the cursor loop then stays on the scalar unit)
        const bool i32 = tiles_fit_i32(A.n, A.n_tiles, A.max_span);
#define BC_SOLO(Q, KK, ST)                                                                                       \
    do {                                                                                                         \
        if (nostore && i32)                                                                                      \
            hipLaunchKernelGGL((k_pileup_solo<Q, KK, true, true, int32_t, false>), grid, block, lds, s, A);      \
        else if (nostore) hipLaunchKernelGGL((k_pileup_solo<Q, KK, true, true, int64_t, false>), grid, block, lds, s, A); \
        else if (sump && i32) hipLaunchKernelGGL((k_pileup_solo<Q, KK, true, true, int32_t>), grid, block, lds, s, A); \
        else if (sump) hipLaunchKernelGGL((k_pileup_solo<Q, KK, true, true, int64_t>), grid, block, lds, s, A);   \
        else if (i32) hipLaunchKernelGGL((k_pileup_solo<Q, KK, ST, false, int32_t>), grid, block, lds, s, A);     \
        else hipLaunchKernelGGL((k_pileup_solo<Q, KK, ST, false, int64_t>), grid, block, lds, s, A);              \
    } while (0)
        if (mbq > 0) {
            if (k == 5) {
                if (stats) BC_SOLO(true, 5, true); else BC_SOLO(true, 5, false);
            } else {
                if (stats) BC_SOLO(true, 6, true); else BC_SOLO(true, 6, false);
            }
        } else {
            if (k == 5) {
                if (stats) BC_SOLO(false, 5, true); else BC_SOLO(false, 5, false);
            } else {
                if (stats) BC_SOLO(false, 6, true); else BC_SOLO(false, 6, false);
            }
        }
#undef BC_SOLO
        return hipGetLastError();
    }
    const bool i32 = tiles_fit_i32(A.n, A.n_tiles, A.max_span);
    const int inst = tile_instance(r, mbq > 0, i32, instance);
    const TileShape ts = tile_shape(A.n_tiles, S, inst);
    const int nw = ts.nw;
    const int64_t blocks = ts.blocks;
    const dim3 grid((unsigned)blocks), block(64 * nw);
    const size_t lds = ts.lds;
    if (stats && accumulate) return hipErrorInvalidValue;  // no caller: the fused tail only stores
    // diagnostic only: BC_TRACE=<file> dumps the per-wave phase stamps of the 20th launch
    static unsigned long long* tbuf = nullptr;
    static int tcalls = 0;
#ifdef BC_PHASE_TRACE
    const char* tpath = std::getenv("BC_TRACE");
#else
    const char* tpath = nullptr;
#endif
    const size_t tn = (size_t)blocks * nw * kTracePhases;
    if (tpath) {
        if (!tbuf && hipMallocManaged((void**)&tbuf, 8 * (size_t)256 * 64 * 16 * kTracePhases) != hipSuccess) tbuf = nullptr;
        if (tn <= (size_t)256 * 64 * 16 * kTracePhases) A.trace = tbuf;
    }
    const TileArgs T = A;  // k_pileup takes the walk's fields only
    const TileKernel fn = tile_kernel(mbq > 0, k, stats, i32, inst);
    allow_lds(fn);
    hipLaunchKernelGGL(fn, grid, block, lds, s, T);
    if (A.trace && ++tcalls == 20) {
        (void)hipStreamSynchronize(s);
        if (FILE* f = std::fopen(tpath, "wb")) {
            std::fwrite(A.trace, 8, tn, f);
            std::fclose(f);
        }
    }
    return hipGetLastError();
}

}  // namespace bc
