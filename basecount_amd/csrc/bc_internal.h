// bc_internal.h — shared between the kernel file and the C-ABI file.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "basecount_hip.h"

struct bc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    unsigned long long* d_err = nullptr;  // first out-of-range read index (atomicMin), ~0 = none
    unsigned long long* h_err = nullptr;  // pinned mirror
    bool timing = false;                  // bc_timing_enable: hipEvents around every launch
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[BC_KERNEL_IDS];
    hipEvent_t mark[BC_EVENT_SLOTS] = {};   // bc_event_record slots (created on first use)
    hipEvent_t sig = nullptr;               // bc_ctx_wait: "everything enqueued so far"
    int32_t* rc_scratch = nullptr;         // bc_pileup's k_rc accumulation buffer, kept zeroed
    size_t rc_scratch_bytes = 0;
    void* out_scratch = nullptr;           // bc_pileup_partials without outputs: their stand-ins
    size_t out_scratch_bytes = 0;
    void* sum_scratch = nullptr;           // the read-parallel summary's leaf arrays, kept zeroed
    size_t sum_scratch_bytes = 0;
    // bc_bgzf_inflate_host: device buffers of one slice, its event pairs and the times so far
    std::mutex z_mutex;
    void* z_buf[4] = {};  // compressed bytes, descriptors, inflated bytes, statuses
    size_t z_bytes[4] = {};
    hipEvent_t z_ev[4] = {};
    double z_ms[3] = {};
    int64_t z_blocks = 0;
    // kernel-shape overrides (bc_ctx_set_shape); 0 = chosen from the batch
    int shape = BC_SHAPE_AUTO;
    int tile_waves = 0;
    int reads_per_block = 0;
    int instance = BC_INSTANCE_AUTO;  // k_pileup's instance (bc_ctx_set_instance)
    int ops_passes = 0;               // k_ops' window passes (bc_ctx_set_ops_passes); 0 = from the batch
};

// Diagnostic work-skipping switches (BC_ABLATE) exist only in -DBC_DIAG builds
// (scripts/ablate.sh); the shipped library compiles them out.
#ifdef BC_DIAG
#define BC_ABL(A) ((A).ablate)
#else
#define BC_ABL(A) 0
#endif

struct bc_graph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

namespace bc {

// Kernel-1 geometry.  One 256-thread workgroup (4 waves) per chunk of consecutive reads.
constexpr int kCountThreads = 256;
// LDS window: counts of one chunk's reads, packed two 16-bit columns per 32-bit word
// (planes {A|C, G|T, DS|N}); a chunk holds < 65536 reads so a 16-bit half never overflows.
constexpr int kWinMax = 4096;  // positions per window -> 3 * 4096 * 4 B = 48 KiB
constexpr int kNpBuf = 8192;   // numpy's default ufunc buffer size (reduction chunk)

// launchers (bc_kernels.hip); all async on `s`, return hipError_t
hipError_t launch_count(hipStream_t s, const bc_reads& r, int64_t ref_len, uint32_t mbq, int ncols,
                        int32_t* hist, int reads_per_block, unsigned long long* d_err);
size_t seq_event_bytes(int64_t seq_bytes);
hipError_t launch_seq_event(hipStream_t s, const uint8_t* src, int64_t nbytes, uint8_t* dst);
hipError_t launch_span(hipStream_t s, const bc_reads& r, int* d_max_span);
// scratch_counts_out != nullptr: hist is the context's zeroed accumulation scratch; its counts go
// to scratch_counts_out and it is zeroed again (k_stats)
hipError_t launch_stats(hipStream_t s, const int32_t* hist, int64_t L, int k, double nf, double nf2,
                        int32_t* cov, double* pc, double* ent, double* sec, int32_t* scratch_counts_out = nullptr);
// Summary partials (the per-8192-buffer sums bc_summary starts from): when the sparse sweep
// runs with `parts`, it writes those of the whole buffers [0, full_chunks) itself (fused = true).
struct SumParts {
    int32_t* hdr;  // the work buffer's header: [0] = buffers whose partials are the quarters'
    double* ent;  // per buffer
    long long* cov;
    long long* nz;
    double* sub_ent;  // per quarter buffer (2048 positions), written by the sparse sweep
    long long* sub_cov;
    long long* sub_nz;
    bool fused;
    int64_t full_chunks;  // buffers whose partials are in the quarter arrays (fused)
    // summary only (in): the sweep writes no per-position output except the coverage and entropy
    // of the positions past the whole buffers, into cov_tail / ent_tail (index P - full_chunks *
    // 8192; at most 8192 positions) for the fold's last partial buffer.  Honoured only when the
    // sweep fuses the partials (out: fused); otherwise the caller must give full outputs.
    bool no_store = false;
    bool whole_buffers = false;  // (out) the partials of [0, full_chunks) are per buffer, not per quarter
    int32_t* cov_tail = nullptr;
    double* ent_tail = nullptr;
};
// shape: BC_SHAPE_*; tile_waves: 0 = from the depth, else 1/2/4/8 waves per tile
hipError_t launch_pileup_tiles(hipStream_t s, const bc_reads& r, int64_t L, int64_t max_end, uint32_t mbq, int k,
                               bool stats, bool accumulate, double nf, double nf2, int32_t* counts, int32_t* cov,
                               double* pc, double* ent, double* sec, unsigned long long* d_err, int shape = 0,
                               int tile_waves = 0, int instance = 0, SumParts* parts = nullptr);
// instance: BC_INSTANCE_*; AUTO takes k_pileup's lean instance while the bound on the batch's
// multi-run reads, (n_cigar_words - n_reads) / 2, is at most this share of its reads.  Measured
// (scripts/lean_fraction.py): the lean instance is 10 % ahead with
// no slow read and already 4 % behind with one read in 64 carrying an indel, so the share is zero:
// only a batch whose reads all have ONE CIGAR op takes it.
constexpr double kLeanMaxSlowShare = 0.0;
// bc_pileup_launch_info: the instance launch_pileup_tiles launches (no pointer of r is read)
void pileup_launch_info(const bc_reads& r, int64_t L, int shape, int tile_waves, int instance, uint32_t mbq, int k,
                        bc_launch_info& out);
// Summary only (main.py:469-499) for a sparse sorted batch: the read-parallel summary (counted
// positions per 128-position leaf, exact walks of the leaves two reads share; k_sum_buffers adds
// each 8192-position buffer's 64 leaves in numpy's tree order) into WHOLE-buffer partials
// (parts.ent / cov / nz, parts.whole_buffers set: the fold is told so through a header value of
// 0) and the tail arrays; `scratch` (>= sum_sparse_bytes(L) bytes, laid out by its capacity)
// zeroed when allocated, left zeroed (on a launch error the caller drops it).  Needs L >= kNpBuf.
size_t sum_sparse_bytes(int64_t L);
hipError_t launch_sum_sparse(hipStream_t s, const bc_reads& r, int64_t L, uint32_t mbq, int k, double nf,
                             unsigned long long* d_err, SumParts& parts, void* scratch, size_t scratch_bytes);
hipError_t launch_rc(hipStream_t s, const bc_reads& r, int64_t L, uint32_t mbq, int ncols, int32_t* counts,
                     unsigned long long* d_err);
// k_ops (bc_ops.hip, BC_SHAPE_OPS): launch_rc's contract for batches of many-op reads, sorted or
// not; plan: ops_plan's (bc_ops_plan.h) for the batch, ref_len and the context's overrides
hipError_t launch_ops(hipStream_t s, const bc_reads& r, int64_t L, uint32_t mbq, int ncols, int32_t* counts,
                      unsigned long long* d_err, const struct bc_ops_plan& plan);
// bc_pileup / bc_count choose the read-chunked k_rc over the tiled k_pileup when a tile would
// walk at least this many reads (deep batches; bc_ctx_set_shape overrides)
constexpr double kRcMinReadsPerTile = 2048.0;
bool use_rc(const bc_reads& r, int64_t L, int shape);
constexpr int kTileMaxSpan = 4096;  // beyond this span the tiled kernel's look-back gets too long
// the tiled kernels: waves per 64-position tile from the depth (1 = the sparse sweep k_pileup_solo)
// (with per_tile the mean reads a tile walks: one wave up to kSoloMaxReadsPerTile, else the
// smallest S in {4, 8} with per_tile <= kTileReadsPerWave x S)
constexpr double kSoloMaxReadsPerTile = 48.0;
constexpr double kTileReadsPerWave = 512.0;
double pileup_reads_per_tile(const bc_reads& r, int64_t L, int64_t max_end);
int pileup_waves(const bc_reads& r, int64_t L, int64_t max_end, int tile_waves);
// bc_pileup_plan: what bc_pileup launches for the batch's header (no pointer of r is read)
void pileup_plan(const bc_reads& r, int64_t L, int shape, int tile_waves, bc_plan& p);
inline bool pileup_is_solo(const bc_reads& r, int64_t L, int shape, int tile_waves) {
    return shape != BC_SHAPE_TILE_NO_SOLO && pileup_waves(r, L, r.max_end, tile_waves) == 1;
}

// ---- the coordinate-sorted copy of an unsorted batch (bc_sort.hip) ----
// fields: sort only the per-read fields (+ run records) and leave the sequence where it is (k_rc
// stages a chunk's scattered reads by LDS-DMA gathers); else copy the sequence (and qualities)
// into start order as well
size_t sort_bytes(const bc_reads& r, bool fields);
// enqueues the sort into mem (sort_bytes(r, fields) bytes; stream-ordered, no host round trip)
// and fills `out` (sorted; no index, or with fields the run records); needs sort_fits(r)
hipError_t launch_sort(hipStream_t s, const bc_reads& r, bc_reads& out, void* mem, bool fields);
bool sort_fits(const bc_reads& r);
// device word of caller errors (read after a sync): bit 0 the reads' sequences overlap (the copy
// did not fit), bit 1 a start outside [0, max_end]
const uint32_t* sort_flags_word(const bc_reads& r, const void* mem);

// ---- the device index of a sorted batch (bc_index.hip) ----
// bc_reads.index_tag: the batch identity an index was built for (never 0)
inline uint64_t index_tag(const bc_reads& r) {
    uint64_t h = 0x243F6A8885A308D3ull;
    auto mix = [&h](uint64_t v) { h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2); };
    mix((uint64_t)r.n_reads);
    mix((uint64_t)(uint32_t)r.sorted);
    mix((uint64_t)(uint32_t)r.max_span);
    mix((uint64_t)r.max_end);
    mix((uint64_t)(uintptr_t)r.pos);
    mix((uint64_t)(uintptr_t)r.cig_beg);
    return h | 1u;
}
inline bool index_valid(const bc_reads& r) { return r.index_tag != 0 && r.index_tag == index_tag(r); }
struct IndexPlan {
    size_t runs_bytes = 0, sums_bytes = 0, tiles_bytes = 0, total = 0;
    int64_t n_chunks = 0, n_tiles = 0;
};
// what = BC_INDEX_RUNS | BC_INDEX_TILES (AUTO resolved by the caller)
IndexPlan index_plan(const bc_reads& r, int what);
// builds the planned parts into mem (plan.total bytes) and sets r's index fields and tag
hipError_t launch_index(hipStream_t s, bc_reads& r, const IndexPlan& plan, void* mem);
size_t summary_work_bytes(int64_t L);
hipError_t launch_summary(hipStream_t s, const int32_t* cov, const double* ent, int64_t L, void* work,
                          double* out, int64_t first_chunk = 0);
// (quarters: the buffers before first_chunk come as quarter partials, else as whole-buffer ones)
hipError_t launch_summary_partials(hipStream_t s, const int32_t* cov, const double* ent, int64_t L, void* work,
                                   int64_t first_chunk, bool quarters = true);
// (the work buffers' headers say which leading buffers come as quarters)
hipError_t launch_summary_fold(hipStream_t s, int n, const int64_t* L, void* const* work, double* const* out);
// the partial arrays inside a summary work buffer
SumParts summary_parts(void* work, int64_t L);
hipError_t launch_amplicons(hipStream_t s, const int32_t* cov, const double* ent, const double* sec,
                            int64_t L, const int64_t* lo, const int64_t* hi, int n_tiles, double* out);
// The fused --summarise-with-bed tail (bc_pileup_summary_amplicons): kernel 2 that also writes
// numpy's 128-position leaf partials into the summary work buffer, then ONE launch for the
// summary (out: mean coverage, mean entropy, non-zero positions, coverage sum) and every
// amplicon window (amp: 6 doubles per window)
hipError_t launch_stats_leaves(hipStream_t s, int32_t* hist, int64_t L, int k, double nf, double nf2, int32_t* cov,
                               double* ent, double* sec, int32_t* counts_out, void* work);
hipError_t launch_tail(hipStream_t s, const int32_t* cov, const double* ent, const double* sec, int64_t L, void* work,
                       double* out, const int64_t* lo, const int64_t* hi, int n_tiles, double* amp);

// ---- several references as one virtual reference (bc_segments.hip, bc_pileup_segments) ----
// vpos[i] = voff[segment of read i] + pos[i], the segment found in read_beg[0..n_seg]
hipError_t launch_seg_vpos(hipStream_t s, const int32_t* pos, int64_t n, const int64_t* ref_len,
                           const int64_t* read_beg, const int64_t* voff, int n_seg, int32_t* vpos);
// bc_summary's 4 doubles of every segment's slice [voff[i], voff[i] + ref_len[i]) into out[i][4]
hipError_t launch_sum_segments(hipStream_t s, int n_seg, const int64_t* ref_len, const int64_t* voff,
                               const int32_t* cov, const double* ent, double* out);
// ---- a cohort's files as segments (bc_cohort.h: bc_segments_rebase, bc_amplicons_segments) ----
// out_cig[i] = in_cig[i] + cig_base[segment of read i], out_nib[i] = in_nib[i] + nib_base[segment]
// (uint32; in place when in == out)
hipError_t launch_seg_rebase(hipStream_t s, int64_t n, const int64_t* read_beg, int n_seg, const uint64_t* cig_base,
                             const uint64_t* nib_base, const uint32_t* in_cig, const uint32_t* in_nib,
                             uint32_t* out_cig, uint32_t* out_nib);
// bc_amplicons' 6 doubles of window t clipped to segment seg's slice into out[seg][t][6]
hipError_t launch_amplicons_segments(hipStream_t s, const int32_t* cov, const double* ent, const double* sec,
                                     int n_seg, const int64_t* ref_len, const int64_t* voff, const int64_t* lo,
                                     const int64_t* hi, int n_tiles, double* out);

// ---- BGZF inflate (bc_inflate.hip): one wave per block, every descriptor checked on the device ----
hipError_t launch_inflate(hipStream_t s, const uint8_t* comp, uint64_t comp_bytes, const bc_zblock* blocks, int64_t n,
                          uint8_t* out, uint64_t out_bytes, uint8_t* status);

// ---- BAM record decode (bc_bam.hip over bc_bam.h): raw_bytes < 2^31 is the caller's check ----
size_t bam_index_bytes(uint64_t raw_bytes, uint64_t seg_bytes);
hipError_t launch_bam_index(hipStream_t s, const uint8_t* raw, uint32_t N, uint32_t seg_bytes, uint32_t first,
                            int64_t max_records, bool final, int32_t n_refs, void* work);
hipError_t launch_bam_fill(hipStream_t s, const uint8_t* raw, uint32_t N, uint32_t seg_bytes, const void* work,
                           const bc_bam_arrays& out, bool want_qual);

// ---- read selection (bc_select.hip over bc_select.h): 0 <= n < 2^31 is the caller's check ----
size_t select_bytes(int64_t n, int64_t n_refs);
hipError_t launch_select(hipStream_t s, const bc_bam_arrays& rec, int64_t n, int64_t min_mapq, const uint8_t* ref_sel,
                         const int64_t* ref_len, int32_t n_refs, void* work, const bc_sel_arrays& out);

// ---- BGZF deflate (bc_deflate.hip over bc_deflate.h): the argument limits are the caller's check ----
size_t deflate_work_bytes(int64_t text_cap, int64_t n_spans);
hipError_t launch_deflate(hipStream_t s, const uint8_t* text, int64_t text_cap, const int64_t* span_off, int64_t n_spans,
                          const int32_t* gate, void* work, void* out_small, uint8_t* comp, int64_t comp_cap);
int deflate_host(const uint8_t* text, const int64_t* span_off, int64_t n_spans, uint8_t* comp, int64_t comp_cap,
                 int64_t* span_coff, int64_t* total, int nthreads);

// ---- row formatting (bc_fmt.hip over bc_fmt.h): the argument limits are the caller's check ----
size_t fmt_work_bytes(int64_t n);
hipError_t launch_fmt_rows(hipStream_t s, const bc_fmt_args& args, void* work, void* out, uint8_t* text,
                           int64_t text_cap);

}  // namespace bc
