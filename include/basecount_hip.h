/*
 * basecount_hip.h — C-ABI of the MI355X (gfx950) pileup counter.
 *
 * This is the drop-in boundary for the reference's only native operator:
 *
 *     count.bcount(refLen, minBaseQuality, reads, qualities, starts, ctuples)
 *         -> list[list[int]]   (refLen x 6: A, C, G, T, DS, N)
 *
 *   defined at /root/reference/basecount/count.cpp:7-99, exported at count.cpp:102-105,
 *   built as the top-level module `count` by /root/reference/setup.py:5 and called from
 *   /root/reference/basecount/main.py:146-153 and :179-186,
 *
 * plus the per-position statistics the reference computes in Python right after it
 * (get_stats / get_entropy, /root/reference/basecount/main.py:10-79) and the summary /
 * amplicon reductions of main.py:469-595.
 *
 * Conventions
 *   - Every function returns BC_OK (0) or a negative BC_E_* status; bc_last_error() gives the
 *     message of the calling thread's last failure.
 *   - Pointers named d_* are device (HBM) pointers, h_* are host pointers.  Device buffers passed
 *     in are caller-owned; buffers created by bc_reads_upload()/bc_malloc() are library-owned and
 *     released with bc_reads_free()/bc_free().
 *   - Compute calls are stream-ordered and asynchronous on the context's stream; bc_sync() blocks.
 *     No compute call allocates or synchronises, so a sequence of them can be captured into a
 *     hipGraph (bc_graph_* below).
 *   - Nothing here falls back to the CPU: without a gfx950 device, bc_ctx_create() fails.
 */
#ifndef BASECOUNT_HIP_H
#define BASECOUNT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BC_OK 0
#define BC_E_ARG (-1)   /* invalid argument (mirrors pybind11's TypeError on bad bcount args)   */
#define BC_E_HIP (-2)   /* HIP runtime error                                                     */
#define BC_E_RANGE (-3) /* a counted event fell outside [0, refLen) (count.cpp:60-65,85 .at())   */
#define BC_E_NODEV (-4) /* no usable gfx950 device                                               */
#define BC_E_COMM (-5)  /* RCCL error in a multi-GPU call                                        */

#define BC_ABI_VERSION 8

/* Layouts of bc_reads.seq.
 *   BC_SEQ_BAM   BAM packing: "=ACMGRSVTWYHKDBN" codes, two per byte, high nibble first
 *                (what the host decoder produces; bc_reads_upload/bc_bcount_host inputs).
 *   BC_SEQ_EVENT the device layout of the tiled kernel: one nibble per base in LINEAR order
 *                (base i at bits 4*(i%8) of little-endian 32-bit word i/8), pre-classified to
 *                event classes  A 0001, C 0010, G 0100, T 1000, N 0011, not counted 0000
 *                (count.cpp:58-65 through pysam's decode: '=' and IUPAC codes count nowhere).
 *                The buffer must hold bc_seq_event_bytes(seq_bytes) bytes (zero padding).
 * bc_reads_upload produces BC_SEQ_EVENT; bc_seq_to_event converts a device buffer in place. */
#define BC_SEQ_BAM 0
#define BC_SEQ_EVENT 1

/* A batch of pre-decoded, accepted reads of ONE reference, struct-of-arrays.
 * For read i (all fields as the reference's bcount sees them, count.cpp:22-38):
 *   starts[i]  = pos[i]                              (0-based reference_start)
 *   ctuples[i] = cigar[cig_beg[i] .. cig_beg[i]+cig_n[i])   BAM words: len << 4 | op
 *   reads[i][j]     = SEQ nibble at index seq_nib[i] + j    (layout: seq_layout, BC_SEQ_*)
 *   qualities[i][j] = qual[seq_nib[i] + j]                  (qual is indexed by nibble index)
 * i.e. seq_nib already includes the query_alignment_start (soft-clip) offset.
 * The same struct describes host arrays (bc_reads_upload input, bc_bcount_host) and device
 * arrays (bc_count input).                                                                     */
typedef struct bc_reads {
    int64_t n_reads;
    const int32_t* pos;
    const uint32_t* cig_beg;
    const uint32_t* cig_n;
    const uint32_t* seq_nib;
    const uint32_t* cigar;
    int64_t n_cigar_words;
    const uint8_t* seq;
    int64_t seq_bytes;
    const uint8_t* qual;      /* may be NULL; then minBaseQuality must be 0                    */
    int64_t qual_bytes;       /* >= 2*seq_bytes when qual != NULL                              */
    int32_t sorted;           /* 1 if pos[] is non-decreasing (enables the tiled kernel)       */
    int32_t max_span;         /* upper bound of every read's reference span (M/D/N/=/X bases)  */
    int64_t max_end;          /* upper bound of pos[i] + span[i] over the batch                */
    int32_t seq_layout;       /* BC_SEQ_BAM or BC_SEQ_EVENT                                    */
    int32_t run_chunks;       /* chunk summaries after the run records (see read_runs), or 0   */
    /* Optional device index of a sorted batch (NULL / 0: the tiled kernel searches pos[]).  For
     * the 64-position tile t < n_tiles, tile_reads[2t] and tile_reads[2t+1] are the reads
     * [lo, hi) that can overlap it: lo = first i with pos[i] > 64t - max_span, hi = first i with
     * pos[i] >= 64t + 64 (so valid for this max_span only).  Built on the device by
     * bc_reads_upload / bc_reads_index (k_index_tiles) for dense batches (fewer tiles than
     * reads/16, fewer than 2^31 reads); host inputs ignore it.                                  */
    const int32_t* tile_reads;
    int64_t n_tiles;
    /* Optional device run records of a sorted batch (NULL: the kernels decode the CIGARs): 4
     * words per read, the first two aligned runs of its CIGAR as the read-chunked kernel needs
     * them (layout in basecount_amd/csrc/bc_runs.h).  Built on the device by bc_reads_upload /
     * bc_reads_index (k_index_runs: the same decode the kernels run) for sorted batches that
     * take the read-chunked kernel; host inputs ignore it.
     * When run_chunks > 0, read_runs[4 n_reads ..] then holds run_chunks summaries of 8 words,
     * one per 256 consecutive reads (the read-chunked kernel's chunk): min start, max end,
     * first / last-plus-one byte of their aligned sequence, max span, a run-shape code and a
     * deletion flag over the reads with simple CIGARs (bc_runs.h: chunk_summary).              */
    const uint32_t* read_runs;
    /* Identity of the batch the index above was built for (bc_reads_upload / bc_reads_index):
     * a hash of n_reads, sorted, max_span, max_end and the pos / cig_beg pointers.  The kernels
     * use tile_reads / read_runs only while it matches, so a copied struct that was sliced (pos
     * offset, n_reads shrunk) or given another max_span falls back to searching / decoding
     * instead of reading another batch's index.  0 = no index.
     * The tag detects slicing, not new CONTENT in the same buffers: a caller that refills the
     * arrays of a struct in place (same pointers, same counts and bounds) must set index_tag = 0
     * or rebuild the index (bc_reads_index) before the next launch.                          */
    uint64_t index_tag;
} bc_reads;

typedef struct bc_ctx bc_ctx;

const char* bc_last_error(void);
int bc_abi_version(void);
/* Build description, e.g. "gfx950 diag=0 phase_trace=0": diag=1 marks a diagnostic build whose
 * kernels can skip work on request (BC_ABLATE); bench.py refuses to report numbers from one.    */
const char* bc_build_info(void);
int bc_device_count(int* n);

/* Create a context on `device`.  `stream` is a hipStream_t (NULL: the library creates and owns
 * a non-blocking stream).  The context holds only small scratch state (the range-error word).   */
int bc_ctx_create(int device, void* stream, bc_ctx** out);
int bc_ctx_destroy(bc_ctx* ctx);
int bc_ctx_stream(bc_ctx* ctx, void** stream);
/* Give back the context's grow-only device scratch (bc_pileup's k_rc accumulation buffer,
 * bc_pileup_partials' stand-in outputs and the read-parallel summary's leaf arrays) after
 * finishing the work enqueued on its stream; the next call that needs one allocates it again
 * (outside any graph capture).  The context stays usable.                                      */
int bc_ctx_release_scratch(bc_ctx* ctx);

/* Kernel-shape selection for bc_count / bc_pileup on this context (parity tests and tuning; no
 * shape skips work, every one computes the same counts).  The default, BC_SHAPE_AUTO, picks
 * from the batch's depth:
 *   BC_SHAPE_TILE         tiled k_pileup, or its sparse sweep k_pileup_solo (read-chunked k_rc
 *                         only for spans > 4096)
 *   BC_SHAPE_RC           read-chunked k_rc (+ k_stats) for every sorted batch
 *   BC_SHAPE_TILE_NO_SOLO tiled k_pileup, never the sparse sweep
 *   BC_SHAPE_OPS          scan-expanded k_ops (+ k_stats) in k_rc's place, for batches of many-op
 *                         reads (nanopore-like: tens to thousands of CIGAR ops per read).  Never
 *                         picked by BC_SHAPE_AUTO.  bc_count under it also takes unsorted
 *                         BC_SEQ_EVENT batches (any sequence alignment); BC_SEQ_BAM batches keep
 *                         k_count.  Reads no index: BC_INDEX_AUTO builds none, reads_per_block
 *                         (0 = from the batch) is the reads per k_ops workgroup.  Reads longer
 *                         than its LDS window are counted over window passes (bc_ops_plan
 *                         below).  Timed under BC_K_COUNT.
 * tile_waves: 0 = from the depth, else 1, 2, 4 or 8 waves per 64-position tile (BC_E_ARG
 * otherwise).  reads_per_block: 0 = automatic, else 1..32768 reads per k_count workgroup
 * (unsorted batches).                                                                          */
#define BC_SHAPE_AUTO 0
#define BC_SHAPE_TILE 1
#define BC_SHAPE_RC 2
#define BC_SHAPE_TILE_NO_SOLO 3
#define BC_SHAPE_OPS 4
int bc_ctx_set_shape(bc_ctx* ctx, int shape, int tile_waves, int reads_per_block);

/* k_ops' launch for a batch (BC_SHAPE_OPS), from the batch's header alone: n_reads, sorted,
 * max_span, max_end and seq_bytes are read, no pointer is dereferenced, nothing is enqueued and
 * no context is needed.  A workgroup takes reads_per_block consecutive reads.  For a sorted batch
 * it counts into an LDS window of `window` = 4,096 positions and runs up to passes_max passes:
 * pass p owns the positions [first read's start + p x window, + (p + 1) x window), every counted
 * event is examined in exactly the pass that owns its position (events at or beyond the end of
 * the last pass's window in the last pass, as global atomics), the window is cleared before and
 * flushed after every pass, and the passes end as soon as no read of the workgroup reaches
 * further.  The counts are those of the single window, bit for bit.
 *   typical read = min(2 x seq_bytes / n_reads, max_span) <= 2,048, or an unsorted batch:
 *       reads_per_block as the single-window rule gives it (DESIGN.md section 3 "k_ops"),
 *       passes_max 1: the single-pass kernel; an unsorted batch has window 0
 *   longer reads: reads_per_block the reads that start within one window, 4,096 x n_reads /
 *       max(ref_len, max_end), at least 4 (a read per wave) and at most n_reads / 2,048 clamped to
 *       [32, 8,192]; passes_max what the workgroup's reads can reach, (reads_per_block x
 *       max(ref_len, max_end) / n_reads + max_span) / 4,096 + 1, at least 2 and at most
 *       BC_OPS_PASSES_MAX (that cap when max_span is 0)
 * reads_per_block: 0 = from the batch, else forced (at most 32,768: a 16-bit half of the window
 * counts one workgroup's reads at one position).  passes: 0 = from the batch, 1 = the single
 * window and its own reads_per_block, 2..BC_OPS_PASSES_MAX = that many at most, for any sorted
 * batch, with the reads_per_block of passes = 0.  `blocks` is the launch's workgroups.
 * bc_ctx_set_ops_passes sets `passes` for the context's launches (A/B runs and tests, as
 * bc_ctx_set_instance; BC_E_ARG outside 0..BC_OPS_PASSES_MAX); reads_per_block is
 * bc_ctx_set_shape's.  Measured in DESIGN.md section 3 "k_ops".                                */
#define BC_OPS_PASSES_MAX 16
struct bc_ops_plan { /* (the call has the tag's name, as stat has: no typedef) */
    int32_t reads_per_block, window, passes_max;
    int32_t reserved;
    int64_t blocks;
};
int bc_ops_plan(const bc_reads* reads, int64_t ref_len, int reads_per_block, int passes, struct bc_ops_plan* out);
int bc_ctx_set_ops_passes(bc_ctx* ctx, int passes);

/* What bc_pileup launches for a coordinate-sorted BC_SEQ_EVENT batch on a reference of ref_len
 * positions under (shape, tile_waves), from the batch's header alone: n_reads, max_span and
 * max_end are read, no pointer is dereferenced, nothing is enqueued and no context is needed.
 * With reads_per_tile = n_reads x (max_span + 63) / max(ref_len, max_end), BC_SHAPE_AUTO takes
 *   reads_per_tile <= 48      the sparse sweep k_pileup_solo, one wave per 64-position tile;
 *   below 2,048               the tiled k_pileup with FOUR waves per tile: sized for batches in
 *                             flight (four such workgroups are resident per CU; a stream of
 *                             C2-sized batches runs ~20 % faster than with eight per tile);
 *   from 2,048 on             the read-chunked k_rc (+ k_stats).
 * BC_SHAPE_TILE / _NO_SOLO keep the tiled kernel beyond 2,048, with eight waves per tile there.
 * tile_waves = 8 remains for a caller that wants ONE batch's latency: a single C2-sized launch
 * takes ~15.8 us with eight waves per tile and ~18.5 us with four.
 *   kernel          BC_PLAN_RC (the fields below are then 0), BC_PLAN_SOLO or BC_PLAN_TILES
 *   waves_per_tile  1, 2, 4 or 8
 *   block_threads   threads per workgroup
 *   lds_bytes       LDS per workgroup, dynamic + static (bc_pileup's launch; the sparse sweep
 *                   with summary partials asks for 2,560 B more)
 *   blocks          workgroups of the launch
 *   blocks_per_cu   workgroups resident per CU as the HIP runtime counts them for the mbq = 0,
 *                   k = 5 variant (hipOccupancyMaxActiveBlocksPerMultiprocessor); -1 when no
 *                   device is visible
 *   tiles_per_wave  BC_PLAN_SOLO: the consecutive tiles one wave of bc_pileup's (and bc_count's)
 *                   sweep takes, 1 up to 2^21 positions and ceil(tiles / 32,768) beyond; the
 *                   fused-summary calls (bc_pileup_summary / bc_pileup_partials on a reference
 *                   of 8,192 positions or more) round it up to a multiple of 32, a whole
 *                   quarter of a summary buffer.  0 for the other kernels
 *   reads_per_tile  the figure above                                                          */
#define BC_PLAN_RC 0
#define BC_PLAN_SOLO 1
#define BC_PLAN_TILES 2
typedef struct bc_plan {
    int32_t kernel;
    int32_t waves_per_tile;
    int32_t block_threads;
    int32_t lds_bytes;
    int64_t blocks;
    int32_t blocks_per_cu;
    int32_t tiles_per_wave;
    double reads_per_tile;
} bc_plan;
int bc_pileup_plan(const bc_reads* reads, int64_t ref_len, int shape, int tile_waves, bc_plan* out);

/* The tiled k_pileup has three instances, all exact on every batch:
 *   general  the one bc_pileup_plan describes (run tables of up to four runs, deletions, unstaged
 *            chunks; four four-wave workgroups per CU);
 *   lean     only the one-run, ungapped window walk, with every other read (an indel, a skip,
 *            more than 8 ops) walked alone per position; fewer registers and less LDS, so FIVE
 *            four-wave workgroups per CU.  10 % ahead on a batch without such reads, behind
 *            from one such read in 64 on.  A chunk's stage holds
 *            its 64 reads' whole sequence (up to 94 B per read; longer reads are walked per
 *            position).
 *   slice    the lean walk with a stage of 64 slots of 64 B, one per read, each holding only the
 *            bytes the TILE reads of it: 4 KiB per wave whatever the read length, SIX four-wave
 *            workgroups per CU.  A read whose leading insertion pushes
 *            its bases out of its slot is walked per position like the other slow reads.  Built
 *            without a quality threshold at 32-bit indices.
 * BC_INSTANCE_AUTO therefore takes the lean instance only when (n_cigar_words - n_reads) / 2, an
 * upper bound of the reads with more than one run, is zero (every read has ONE CIGAR op: an
 * ungapped, unclipped batch), and where a lean instance is built (no quality threshold, or 32-bit
 * indices).  n_cigar_words is the CIGAR buffer's count: a bc_reads that is a slice of a larger
 * batch and shares its buffer is judged by the larger batch's count, never by another slice's
 * alone, and keeps the general instance unless every read of the buffer has one op (the bound
 * can be too large for a slice, never too small).  Where it takes the lean walk it takes the slice
 * instance when one is built (min_base_quality 0, 32-bit indices) and max_span > 64, a read longer
 * than a tile: only then is a slice less than the read.  bc_ctx_set_instance forces one for A/B
 * runs and tests (BC_INSTANCE_LEAN where none is built keeps the general one; BC_INSTANCE_SLICE
 * where none is built is BC_INSTANCE_LEAN).
 * bc_pileup_plan keeps describing the GENERAL tiled instance whatever bc_pileup launches;
 * bc_pileup_launch_info reports the instance a bc_pileup(ctx, reads, ref_len, mbq, k, ...) call
 * launches on a context set to (shape, tile_waves, instance); like bc_pileup_plan it needs no
 * context, reads no pointer of reads and enqueues nothing:
 *   kernel, waves_per_tile, block_threads, blocks   as in bc_plan
 *   lean           1 the lean or the slice instance, 0 the general one (0 for the other kernels);
 *                  the slice instance is the one with lds_bytes ==
 *                  BC_SLICE_LDS_BYTES(block_threads / 64, waves_per_tile)
 *   lds_bytes      LDS per workgroup, dynamic + static, of that instance
 *   blocks_per_cu  hipOccupancyMaxActiveBlocksPerMultiprocessor's answer for that very kernel
 *                  (mbq, k and the index width included); -1 when no device is visible          */
#define BC_INSTANCE_AUTO 0
#define BC_INSTANCE_GENERAL 1
#define BC_INSTANCE_LEAN 2
#define BC_INSTANCE_SLICE 4 /* (3 is not a value) */
#define BC_SLICE_LDS_BYTES(waves, waves_per_tile) \
    ((waves) * (1024 + 4096 + 32) + ((waves) / (waves_per_tile)) * 1536 + 2048 + 64)
int bc_ctx_set_instance(bc_ctx* ctx, int instance);
typedef struct bc_launch_info {
    int32_t kernel;
    int32_t lean;
    int32_t waves_per_tile;
    int32_t block_threads;
    int32_t lds_bytes;
    int32_t blocks_per_cu;
    int64_t blocks;
} bc_launch_info;
int bc_pileup_launch_info(const bc_reads* reads, int64_t ref_len, int shape, int tile_waves, int instance,
                          uint32_t min_base_quality, int k, bc_launch_info* out);
int bc_sync(bc_ctx* ctx);

/* Library-owned device memory helpers (for hosts without another allocator). */
int bc_malloc(bc_ctx* ctx, size_t bytes, void** d_ptr);
int bc_free(bc_ctx* ctx, void* d_ptr);
int bc_memcpy_h2d(bc_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);  /* async */
int bc_memcpy_d2h(bc_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);  /* async */
int bc_memset(bc_ctx* ctx, void* d_dst, int value, size_t bytes);              /* async */

/* Bytes a BC_SEQ_EVENT buffer needs for seq_bytes bytes of packed sequence. */
size_t bc_seq_event_bytes(int64_t seq_bytes);
/* Convert BAM-packed sequence (device) to BC_SEQ_EVENT: d_event (bc_seq_event_bytes bytes) may
 * alias d_bam.  Async on the context's stream.                                                */
int bc_seq_to_event(bc_ctx* ctx, const uint8_t* d_bam, int64_t seq_bytes, uint8_t* d_event);

/* Copy a host batch to HBM (library-owned, BC_SEQ_EVENT on the device).  A BC_SEQ_EVENT host
 * batch (the layout the host decoder already emits, bcio_records.seq_event) is copied as is; a
 * BC_SEQ_BAM one is converted on the device after the copy (k_seq_event).  `sorted`,
 * `max_span` and `max_end` of the device batch are derived from the data (the host's values
 * are ignored).  For batches assembled directly in
 * device memory the caller must set both truthfully: the tiled kernel trusts them.           */
int bc_reads_upload(bc_ctx* ctx, const bc_reads* h_reads, bc_reads* d_reads);
int bc_reads_free(bc_ctx* ctx, bc_reads* d_reads);

/* The device index of a sorted batch assembled in device memory by the caller (e.g. one
 * reference's slice of a file-wide upload), built ON THE DEVICE into caller-owned memory:
 *   BC_INDEX_RUNS   run records + k_rc chunk summaries (read_runs, run_chunks)
 *   BC_INDEX_TILES  the tile index (tile_reads, n_tiles; dense batches only)
 *   BC_INDEX_AUTO   what this context's kernels would use for a reference of length ref_len
 *                   (records for the read-chunked shape, tiles for the tiled one, nothing for
 *                   the sparse sweep)
 * bc_reads_index_bytes gives the bytes d_mem must hold (0: nothing to build); bc_reads_index
 * launches the build on the context's stream (async, no allocation: capturable) and sets the
 * index fields and index_tag of *d_reads.  d_reads->sorted / max_span / max_end must be
 * truthful.  bc_reads_upload builds BC_INDEX_AUTO for ref_len = max_end into its own slab.    */
/* A coordinate-sorted copy of an unsorted device batch, built on the device (bc_sort.hip):
 * the reads bucketed by start (per-block LDS histograms, one block per bucket ordering it), their
 * per-read arrays written in start order and each read's aligned sequence (and qualities) copied
 * so that consecutive reads have consecutive sequence again.  The copy shares d_reads' CIGAR
 * buffer; everything else lives in d_mem (bc_reads_sort_bytes bytes, 256-byte aligned), which
 * must outlive its use -- with one exception, the FIELDS-ONLY view: a batch without qualities
 * (d_reads->qual == NULL) that, once sorted, this context's shape would give to the read-chunked
 * k_rc on a reference of max_end positions (shape "rc" / "ops"; under any shape a max_span
 * above 4,096; under "auto" n_reads * (max_span + 63) / max_end >= 2,048) and that the bucketed
 * sort takes (max_end + 2 <= 2^24) has only its four per-read arrays sorted.  Then d_sorted->seq
 * == d_reads->seq and seq_nib still indexes it: d_reads' SEQUENCE buffer, like its CIGAR buffer,
 * must outlive *d_sorted (compare the two pointers to tell; a batch with qualities and the
 * counting sort of a longer reference always copy).  The decision uses max_end and the shape in
 * force at the call, not the reference length or shape of the later kernels: every kernel takes
 * either kind of view.  *d_sorted is then a sorted batch (sorted = 1, same max_span / max_end,
 * no index: build one with bc_reads_index) that every kernel takes, with the same counts as the
 * input (count.cpp's sums do not depend on the read order).  Needs seq_layout == BC_SEQ_EVENT
 * and seq_bytes + 5 n_reads + 16 <= 0x55555550 (BC_E_ARG otherwise: split the batch).
 * Stream-ordered and capturable (round 6): the call only enqueues four kernels; every layout
 * decision is taken on the device, so there is no host round trip and no fallback path.
 * Caller errors that only the device can see -- a read starting outside [0, max_end], reads whose
 * aligned sequences overlap so that the copy would not fit -- leave a flag in d_mem (the sorted
 * copy stays safe to count: such reads start at 0 / carry no CIGAR): bc_reads_sort_check waits
 * for the stream and returns BC_E_ARG with the reason if a flag is set, BC_OK otherwise.      */
int bc_reads_sort_bytes(bc_ctx* ctx, const bc_reads* d_reads, size_t* bytes);
int bc_reads_sort(bc_ctx* ctx, const bc_reads* d_reads, bc_reads* d_sorted, void* d_mem, size_t bytes);
int bc_reads_sort_check(bc_ctx* ctx, const bc_reads* d_reads, const void* d_mem);

#define BC_INDEX_RUNS 1
#define BC_INDEX_TILES 2
#define BC_INDEX_AUTO 4
int bc_reads_index_bytes(bc_ctx* ctx, const bc_reads* d_reads, int64_t ref_len, int what, size_t* bytes);
int bc_reads_index(bc_ctx* ctx, bc_reads* d_reads, int64_t ref_len, int what, void* d_mem, size_t bytes);

/* Kernel 1 — CIGAR-expand + scatter-add (count.cpp:22-97).
 * Accumulates into d_hist, an int32 histogram of `ncols` planes of `ref_len` positions
 * (plane-major: d_hist[c * ref_len + p]).  ncols = 6 gives the reference's full layout
 * (A,C,G,T,DS,N); ncols = 5 drops N (main.py:19-31 never uses it unless show_n_bases).
 * M/=/X bases with qual >= min_base_quality count A/C/G/T/N; other letters count nowhere;
 * I advances the read; D/N-skip count DS with no quality test; S/H/P/B are no-ops.
 * A counted event at position >= ref_len is recorded (first offending read index kept);
 * read it with bc_range_error().  Async; does not zero d_hist.                               */
int bc_count(bc_ctx* ctx, const bc_reads* d_reads, int64_t ref_len, uint32_t min_base_quality,
             int ncols, int32_t* d_hist);

/* Fused kernel 1 + kernel 2 — the hot path in ONE launch.  For a coordinate-sorted batch
 * (d_reads->sorted == 1, max_span / max_end truthful) the reference is cut into
 * 64-position tiles; each tile finds its reads by a search over pos[], walks them with lanes
 * owning 8-position windows and SWAR register counters (no atomics, no histogram memset;
 * needs seq_layout == BC_SEQ_EVENT), and writes
 *   d_counts [k][L] int32 (the reference's baseCounts columns, N only when k == 6),
 *   d_cov, d_pc (may be NULL), d_ent, d_sec  exactly as bc_stats defines them.
 * Deep batches (many reads per tile) and spans > 4096 instead run the read-chunked kernel 1
 * (each read decoded once, per-block LDS event image / histograms, atomic flush into a
 * context-owned scratch kept zeroed) followed by kernel 2, which moves the counts to d_counts
 * and re-zeroes the scratch: two stream-ordered launches, same results.  The scratch grows on
 * first use for a larger k * ref_len (a synchronizing allocation: make that first call outside
 * a graph capture).
 * Out-of-range counted events are recorded for bc_range_error() as with bc_count.
 * Overwrites its outputs; async; capturable.                                                   */
int bc_pileup(bc_ctx* ctx, const bc_reads* d_reads, int64_t ref_len, uint32_t min_base_quality, int k,
              double nf, double nf2, int32_t* d_counts, int32_t* d_cov, double* d_pc, double* d_ent,
              double* d_sec);

/* Several small references of one file in ONE launch (a transcriptome, a plasmid panel, the short
 * contigs of an assembly): the segmented pileup.
 * A coordinate-sorted file orders reads by (refID, pos).  Reference i of a group of n consecutive
 * references is placed at virtual offset voff[i] = sum_{j<i} round_up(ref_len[j], 64); with
 * voff[i] added to its reads' starts, the group's reads are one sorted batch on one virtual
 * reference of voff[n] positions, and every 64-position tile belongs to exactly one reference.
 * The pileup kernels run on that batch as they are; segment i's results are the slices
 * [voff[i], voff[i] + ref_len[i]) of the outputs (pad positions have coverage 0 and mean nothing).
 *
 * bc_segments_layout: host arithmetic only.  voff[0..n] from ref_lens[0..n); BC_E_ARG for n <= 0,
 * a length <= 0, or voff[n] > BC_SEGMENTS_MAX_LEN (starts are int32).
 *
 * bc_pileup_segments enqueues, on the context's stream:
 *   1. k_seg_vpos: d_vpos[i] = d_reads->pos[i] + voff[segment of read i] (the segment found in
 *      d_read_beg; d_vpos: int32 [n_reads], caller-owned);
 *   2. bc_pileup on a copy of *d_reads with pos = d_vpos, sorted = 1, max_end = virt_len and no
 *      index, for a reference of virt_len positions: the kernel shape is chosen as for any batch
 *      (bc_ctx_set_shape honoured); outputs as bc_pileup's, at virtual size (d_counts [k][virt_len],
 *      d_cov, d_pc or NULL, d_ent, d_sec);
 *   3. when d_sum != NULL, k_sum_segments: d_sum[i][0..4) = bc_summary's four doubles of segment
 *      i's slice, bit for bit (one workgroup per segment, one launch).
 * d_reads: the group's reads in file order with their ORIGINAL starts (max_span truthful; sorted,
 * max_end and the index fields are ignored); n_reads may be 0 (every segment empty).
 * The segment table is three device arrays the caller uploaded: d_ref_len [n_seg], d_read_beg
 * [n_seg + 1] (segment i's reads are [read_beg[i], read_beg[i + 1]) of d_reads; read_beg[0] = 0,
 * read_beg[n_seg] = n_reads; empty segments allowed), d_voff [n_seg + 1] as bc_segments_layout
 * gives it, virt_len = voff[n_seg].
 * Contract: every read lies inside its segment, 0 <= pos and pos + span <= ref_len, and each
 * segment's starts are non-decreasing.  No range error can then occur (bc_range_error stays -1).  A
 * caller that breaks this gets counts in a pad or in a neighbouring segment, never an access
 * outside the buffers: starts are clamped into [0, ref_len] of their segment, and everything past
 * that is the kernels' own edge logic on [0, virt_len).
 * Stream-ordered and capturable like bc_pileup: no synchronisation, and no allocation except the
 * k_rc scratch growing on first use (make that first call outside a graph capture).
 * Timed as BC_K_INDEX (k_seg_vpos), the pileup's own ids, and BC_K_SUMMARY (k_sum_segments).  */
#define BC_SEGMENTS_MAX_LEN 2147483520 /* 2^31 - 128 */
int bc_segments_layout(const int64_t* ref_lens, int n, int64_t* voff /* [n + 1] */);
int bc_pileup_segments(bc_ctx* ctx, const bc_reads* d_reads, int n_seg, const int64_t* d_ref_len,
                       const int64_t* d_read_beg, const int64_t* d_voff, int64_t virt_len, int32_t* d_vpos,
                       uint32_t min_base_quality, int k, double nf, double nf2, int32_t* d_counts, int32_t* d_cov,
                       double* d_pc, double* d_ent, double* d_sec, double* d_sum /* [n_seg][4] or NULL */);

/* Several FILES in one launch (a cohort: thousands of amplicon samples of one small genome).  The
 * selected reads of the files lie side by side in shared device buffers and every (file, reference)
 * pair is one segment of bc_pileup_segments.  Two calls complete that picture; both are
 * stream-ordered, allocate nothing, never synchronise and can be captured in a graph, and both
 * check their arguments (BC_E_ARG) before any device is touched.
 *
 * bc_segments_rebase.  File f's CIGAR words were copied to word offset cig_base of the shared
 * CIGAR buffer, its BC_SEQ_EVENT bytes (and its qualities, indexed by nibble) to a byte offset that
 * is a multiple of 16, nib_base = 2 x that offset.  Its reads' cig_beg / seq_nib still count from
 * the file's own arrays.  One launch (k_seg_rebase, one lane per read) finds each read's segment in
 * d_read_beg [n_seg + 1] (as bc_pileup_segments takes it) and writes
 *     d_cig_beg_out[i] = d_cig_beg[i] + d_cig_base[seg],  d_seq_nib_out[i] = d_seq_nib[i] + d_nib_base[seg]
 * in uint32; d_cig_base / d_nib_base: uint64 [n_seg], one entry per SEGMENT (a file's segments
 * repeat the file's bases).  In place when the output pointers equal the input pointers; any
 * other overlap of the four arrays is a caller error.  No CIGAR or sequence byte is read.
 * cig_words_total / nib_total: the shared buffers' sizes in CIGAR words and in nibbles (2 x the
 * sequence bytes); BC_E_ARG when either reaches 2^32, for then a sum could wrap.  The caller
 * guarantees value + base < total for every read.  BC_E_ARG also for n_reads outside [0, 2^31),
 * n_seg < 1 and NULL arrays (the per-read arrays may be NULL when n_reads == 0).
 * Timed as BC_K_INDEX.
 *
 * bc_amplicons_segments.  The windows [d_lo[t], d_hi[t]] (inclusive, t < n_tiles) applied to every
 * segment of a virtual reference laid out by bc_segments_layout (d_ref_len [n_seg], d_voff
 * [n_seg + 1] or longer): d_out[seg][t][0..6) = mean_cov, median_cov, mean_ent, median_ent,
 * mean_sec, median_sec, bit for bit what bc_amplicons gives on segment seg's slice
 * [voff[seg], voff[seg] + ref_len[seg]) with ref_len[seg] as its L: the window is clipped to the
 * segment's own [0, ref_len - 1], an empty window gives -1.0 six times, and no pad or neighbouring
 * segment is ever read.  One launch (k_amplicon_segments) of n_seg x n_tiles workgroups with
 * k_amplicon's arithmetic.  n_tiles == 0 does nothing.  BC_E_ARG for n_seg < 1, n_tiles < 0,
 * n_seg x n_tiles >= 2^31 and NULL arrays.  Timed as BC_K_AMPLICONS.                             */
int bc_segments_rebase(bc_ctx* ctx, int64_t n_reads, int n_seg, const int64_t* d_read_beg,
                       const uint64_t* d_cig_base, const uint64_t* d_nib_base, uint64_t cig_words_total,
                       uint64_t nib_total, const uint32_t* d_cig_beg, const uint32_t* d_seq_nib,
                       uint32_t* d_cig_beg_out, uint32_t* d_seq_nib_out);
int bc_amplicons_segments(bc_ctx* ctx, const int32_t* d_cov, const double* d_ent, const double* d_sec, int n_seg,
                          const int64_t* d_ref_len, const int64_t* d_voff, const int64_t* d_lo,
                          const int64_t* d_hi, int32_t n_tiles, double* d_out /* [n_seg][n_tiles][6] */);

/* hipGraph capture of a sequence of compute calls on the context's stream (the context must own
 * its stream or have been given a non-default one).  bc_graph_end instantiates the graph;
 * bc_graph_launch replays it on the context's stream.                                         */
typedef struct bc_graph bc_graph;
int bc_graph_begin(bc_ctx* ctx);
int bc_graph_end(bc_ctx* ctx, bc_graph** out);
int bc_graph_launch(bc_ctx* ctx, bc_graph* g);
int bc_graph_destroy(bc_graph* g);

/* Stream order between two contexts of one device: ctx's later work waits for everything enqueued
 * on other's stream so far (an event, no host wait).  Independent references can then run on
 * several contexts' streams at once, e.g. inside a capture begun on `main`: fork with
 * bc_ctx_wait(side, main), enqueue on each, join with bc_ctx_wait(main, side).                */
int bc_ctx_wait(bc_ctx* ctx, bc_ctx* other);

/* Per-kernel timing (SURVEY §5 tracing): when enabled, every launch made through the context is
 * bracketed by hipEvents on its stream.  bc_timing_report() synchronises and returns, per kernel
 * id (BC_K_*), the number of timed launches and their mean duration in microseconds, then clears
 * the record.  Do not enable while capturing a graph.                                          */
#define BC_K_COUNT 0      /* event-parallel kernel 1 (unsorted / long-span batches) */
#define BC_K_STATS 1      /* kernel 2                                              */
#define BC_K_RC 2         /* read-chunked kernel 1 (deep sorted batches)           */
#define BC_K_PILEUP 3     /* fused tiled kernel 1 + 2                              */
#define BC_K_SUMMARY 4
#define BC_K_AMPLICONS 5
#define BC_K_INDEX 6      /* the device index build (bc_reads_index / bc_reads_upload)  */
#define BC_K_SOLO 7       /* the sparse sweep k_pileup_solo (fused kernel 1 + 2)     */
#define BC_K_SORT 8       /* the device sort of an unsorted batch (bc_reads_sort)     */
#define BC_KERNEL_IDS 9
int bc_timing_enable(bc_ctx* ctx, int on);
int bc_timing_report(bc_ctx* ctx, int64_t* launches /* [BC_KERNEL_IDS] */, double* mean_us /* [..] */);

/* Region timing: bc_event_record(ctx, slot) records hipEvent `slot` (0 .. BC_EVENT_SLOTS-1) on the
 * context's stream; bc_event_elapsed_ms synchronises on the later one and returns the time
 * between two recorded slots.  Measures a whole sequence of launches (e.g. K steps) on-device. */
#define BC_EVENT_SLOTS 4
int bc_event_record(bc_ctx* ctx, int slot);
int bc_event_elapsed_ms(bc_ctx* ctx, int slot0, int slot1, float* ms);

/* Blocking: returns the smallest read index that produced an out-of-range counted event since
 * the last call (or -1) and clears the record.                                                 */
int bc_range_error(bc_ctx* ctx, int64_t* first_bad_read);

/* Kernel 2 — per-position statistics (main.py:14-79), fp64, same operation order as CPython:
 *   cov = sum(c);  pc_j = 100 * (c_j / cov);  H = nf * sum_j -(p_j*log2(p_j)) [p_j != 0];
 *   H2 = nf2 * (same over the counts with the first argmax removed, over cov - max).
 * k = 5 (A,C,G,T,DS) or 6 (+N, show_n_bases); planes 0..k-1 of d_hist are used.
 * Outputs (device, caller-owned; any of d_pc / d_ent / d_sec may be NULL to skip):
 *   d_cov [L] int32, d_pc [k][L] f64, d_ent [L] f64, d_sec [L] f64.
 * Where cov == 0 the reference emits ints (-1 / 1 / 1): here pc = -1.0, H = H2 = 1.0.
 * Where cov2 == 0 the reference emits int 1 for H2: here 1.0.                                 */
int bc_stats(bc_ctx* ctx, const int32_t* d_hist, int64_t ref_len, int k, double nf, double nf2,
             int32_t* d_cov, double* d_pc, double* d_ent, double* d_sec);

/* Summary reductions of one reference (main.py:469-495), bit-identical to numpy:
 *   out[0] = np.mean(coverages)     out[1] = np.mean(entropies)
 *   out[2] = number of positions with coverage != 0 (as double, exact)
 *   out[3] = sum of coverages (exact, as double when < 2^53)
 * numpy's float64 add.reduce is emulated exactly: 8192-element buffer chunks added left to right,
 * each chunk summed by numpy's pairwise_sum (8-way unrolled leaves of <= 128).  d_out: 4 doubles,
 * device memory.  d_work must hold bc_summary_work_bytes(ref_len) bytes.                     */
size_t bc_summary_work_bytes(int64_t ref_len);
int bc_summary(bc_ctx* ctx, const int32_t* d_cov, const double* d_ent, int64_t ref_len,
               void* d_work, double* d_out);

/* Fused pileup + summary (main.py:469-499's numbers for one reference, as bc_pileup followed by
 * bc_summary, bit-identical): for sparse batches the pileup sweep computes numpy's per-buffer
 * partial sums while the statistics are still in registers, so the per-position coverage and
 * entropies are not read back; other batches run bc_pileup + bc_summary.  Arguments as bc_pileup
 * (all per-position outputs written) plus d_work (bc_summary_work_bytes(ref_len)) and d_out (4
 * doubles, as bc_summary).  ref_len must be > 0.                                              */
int bc_pileup_summary(bc_ctx* ctx, const bc_reads* d_reads, int64_t ref_len, uint32_t min_base_quality, int k,
                      double nf, double nf2, int32_t* d_counts, int32_t* d_cov, double* d_pc, double* d_ent,
                      double* d_sec, void* d_work, double* d_out);
/* The same in two parts, for several references: bc_pileup_partials leaves numpy's per-buffer
 * partial sums of one reference in d_work; bc_summary_fold then folds n references' partials
 * (one workgroup each, side by side: the fold is one dependent add per 8192 positions, the only
 * sequential step of the summary) and writes each reference's 4 doubles to d_outs[i].
 * ref_lens / d_works / d_outs are host arrays of n entries (device pointers).
 * Summary only: with d_counts, d_cov, d_pc, d_ent and d_sec ALL NULL, bc_pileup_partials (and
 * bc_pileup_summary) write no per-position output (the CLI's --summarise prints six numbers per
 * reference): a sparse batch's sweep writes only the summary partials (and the coverage /
 * entropy of the last partial 8192-position buffer, into context scratch); other batches write
 * their outputs into context scratch.  Same numbers, bit for bit.  The scratch grows on first use
 * (a synchronizing allocation: make that call outside a graph capture).                        */
int bc_pileup_partials(bc_ctx* ctx, const bc_reads* d_reads, int64_t ref_len, uint32_t min_base_quality, int k,
                       double nf, double nf2, int32_t* d_counts, int32_t* d_cov, double* d_pc, double* d_ent,
                       double* d_sec, void* d_work);
int bc_summary_fold(bc_ctx* ctx, int n, const int64_t* ref_lens, void* const* d_works, double* const* d_outs);

/* Amplicon vectors (main.py:501-551): for each tile t with inclusive window
 * [lo[t], hi[t]] (already clipped to [0, ref_len-1]; lo > hi = empty), np.mean and np.median of
 * coverage, entropy and secondary entropy over the window.  d_out: [n_tiles][6] f64 device
 * (mean_cov, median_cov, mean_ent, median_ent, mean_sec, median_sec); empty tiles give -1.0. */
int bc_amplicons(bc_ctx* ctx, const int32_t* d_cov, const double* d_ent, const double* d_sec,
                 int64_t ref_len, const int64_t* d_lo, const int64_t* d_hi, int32_t n_tiles,
                 double* d_out);

/* --summarise-with-bed for one reference (main.py:469-551): bc_pileup_summary and bc_amplicons
 * in one call, same numbers bit for bit.  For a deep batch (the read-chunked k_rc) the tail after
 * kernel 1 is two launches: kernel 2 that also leaves numpy's 128-position leaf partials in
 * d_work, and ONE launch for the summary fold and every window's means and medians (instead of
 * kernel 2, the summary's chunk sums, its fold and the amplicon kernel); other batches run
 * bc_pileup_summary + bc_amplicons.  Arguments as those two (d_counts, d_cov, d_ent and d_sec all
 * non-NULL: the windows read them; no percentages), n_tiles >= 0.                             */
int bc_pileup_summary_amplicons(bc_ctx* ctx, const bc_reads* d_reads, int64_t ref_len, uint32_t min_base_quality,
                                int k, double nf, double nf2, int32_t* d_counts, int32_t* d_cov, double* d_ent,
                                double* d_sec, void* d_work, double* d_out, const int64_t* d_lo,
                                const int64_t* d_hi, int32_t n_tiles, double* d_amp);

/* ---- BGZF inflate on the device (opt-in; DESIGN.md §3 "Device inflate") ----------------------
 * One descriptor per BGZF block: its raw-DEFLATE bytes are comp[coff, coff + clen) and inflate to
 * exactly isize bytes (<= 65536) at out[uoff, uoff + isize).  Offsets have any byte alignment.  */
typedef struct bc_zblock {
    uint64_t coff;
    uint32_t clen;
    uint32_t isize;
    uint64_t uoff;
} bc_zblock; /* 24 bytes */

/* k_inflate, one wave per block, stream-ordered (no host synchronisation).  All pointers are device
 * memory; d_status gets one byte per block: 0 = inflated, else the reason (BC_Z_* of
 * basecount_amd/csrc/bc_inflate.h: 1 descriptor outside its buffers or too large, 2..13 what
 * zlib's inflate would refuse too).  Validity is zlib's: a block it refuses is refused here, and an
 * accepted block holds the same bytes.  The kernel checks every descriptor itself against
 * comp_bytes / out_bytes; a failing block is skipped, its own output bytes are unspecified and no
 * byte outside out[uoff, uoff + isize) is written.  isize == 0 is fine and writes nothing.
 * BC_E_ARG (before any device is touched): NULL pointer, n < 0 or n >= 2^31.                    */
int bc_bgzf_inflate(bc_ctx* ctx, const uint8_t* d_comp, uint64_t comp_bytes, const bc_zblock* d_blocks, int64_t n,
                    uint8_t* d_out, uint64_t out_bytes, uint8_t* d_status);
/* The same from and to host memory, blocking: uploads the compressed span the blocks cover, runs
 * k_inflate, downloads each block's bytes to h_out + uoff (bytes of h_out outside the blocks are
 * not touched) and the statuses.  Works in slices of bounded inflated size; the device buffers are
 * context scratch (grow-only, given back by bc_ctx_release_scratch).  Calls on one context are
 * serialised.  `ctx` is a bc_ctx*: it is void* so that the symbol has the type of bcio.h's
 * bcio_inflate_fn and can be handed to bcio_stream_set_inflater unchanged.                      */
int bc_bgzf_inflate_host(void* ctx, const uint8_t* h_comp, uint64_t comp_bytes, const bc_zblock* h_blocks, int64_t n,
                         uint8_t* h_out, uint64_t out_bytes, uint8_t* h_status);
/* Device time of this context's bc_bgzf_inflate_host calls so far (hipEvent pairs on its stream),
 * cumulative: ms[0] upload, ms[1] kernel, ms[2] download; *blocks the blocks handed in.  Either
 * output may be NULL.                                                                           */
int bc_bgzf_inflate_host_times(bc_ctx* ctx, double* ms /* [3] */, int64_t* blocks);

/* ---- BAM record decode on the device (DESIGN.md §3 "Device record decode") --------------------
 * d_raw[0, raw_bytes) holds inflated BAM bytes (bc_bgzf_inflate's output); `first` is the offset of
 * a record start in it.  bc_bam_index finds the record chain (segments of seg_bytes speculated in
 * parallel, then verified from `first` by the record rules alone), bc_bam_fill writes the arrays of
 * bcio.h's bcio_records, byte for byte what the host decoder produces from the same bytes.
 * A fill the device cannot take is DECLINED, not failed: the call returns BC_OK, status says why and
 * err_off where; the caller decodes that fill on the host, so every error is the host's own.    */
#define BC_BAM_OK 0
#define BC_BAM_PARTIAL_LEN 1 /* final, fewer than 4 bytes left at err_off                           */
#define BC_BAM_PARTIAL 2     /* final, the record at err_off ends past the buffer                   */
#define BC_BAM_SHORT 3       /* block_size < 32                                                     */
#define BC_BAM_NEG_LSEQ 4    /* l_seq < 0                                                           */
#define BC_BAM_FIELDS 5      /* the record is shorter than its fields                               */
#define BC_BAM_TOO_LARGE 6   /* raw_bytes >= 2^31: offsets are 32-bit on the device                 */
#define BC_BAM_REPAIRS 7     /* more wrongly speculated segments than 16 + segments / 4             */
#define BC_BAM_INTERNAL 8
#define BC_BAM_SEG_DEFAULT 65536u

typedef struct bc_bam_batch {
    int64_t n;            /* records taken: at most max_records, complete ones only                */
    uint64_t used;        /* offset after the last record taken (the next fill's first byte)       */
    uint64_t cigar_words; /* sizes of the arrays bc_bam_fill writes                                */
    uint64_t seq_bytes;
    int32_t status;       /* BC_BAM_*; non-zero: declined, n and the sizes are not to be used      */
    int32_t reserved;
    uint64_t err_off;
    int64_t segments;     /* segments of the fill                                                  */
    int64_t repaired;     /* segments whose speculated entry was wrong and that were hopped again  */
    uint64_t raw_bytes;   /* the arguments the work buffer was laid out for (bc_bam_fill reads them) */
    uint64_t seg_bytes;
} bc_bam_batch;

/* Device pointers of the output arrays (bcio_records' fields).  seq may be NULL (the kernels read
 * seq_event only); qual is written only with want_qual and may be NULL without.                 */
typedef struct bc_bam_arrays {
    int32_t* tid;        /* [n] */
    int32_t* pos;
    uint16_t* flag;
    uint8_t* mapq;
    int32_t* l_seq;
    int32_t* qstart;
    int32_t* qend;
    uint32_t* rec_err;
    int64_t* ref_span;
    uint64_t* cig_off;   /* [n + 1] */
    uint64_t* seq_off;   /* [n + 1] */
    uint32_t* cigar;     /* [cigar_words] */
    uint8_t* seq;        /* [seq_bytes] BAM packing */
    uint8_t* seq_event;  /* [bc_seq_event_bytes(seq_bytes)] BC_SEQ_EVENT, tail zeroed */
    uint8_t* qual;       /* [2 * seq_bytes] by nibble index */
    int64_t n_cap;       /* what the arrays hold; a batch that needs more is refused (BC_E_ARG) */
    uint64_t cigar_cap;
    uint64_t seq_cap;
} bc_bam_arrays;

/* Bytes of bc_bam_index's work buffer.  seg_bytes 0 = BC_BAM_SEG_DEFAULT, else 64 .. 2^24. */
int bc_bam_index_bytes(uint64_t raw_bytes, uint32_t seg_bytes, size_t* bytes);
/* Blocking (it returns the counts that size the arrays).  first <= raw_bytes, max_records >= 0
 * (bcio_stream_next's contract: at most that many), final != 0: no bytes follow, so an incomplete
 * last record declines the fill; n_refs bounds the reference ids the speculation believes.
 * d_work: 16-byte aligned, work_bytes >= bc_bam_index_bytes.  BC_E_ARG before any device is touched:
 * NULL pointer, first > raw_bytes, negative max_records / n_refs, seg_bytes out of range, small or
 * misaligned work buffer.                                                                        */
int bc_bam_index(bc_ctx* ctx, const uint8_t* d_raw, uint64_t raw_bytes, uint64_t first, int64_t max_records, int final,
                 int32_t n_refs, uint32_t seg_bytes, void* d_work, size_t work_bytes, bc_bam_batch* h_out);
/* Stream-ordered, no allocation, capturable: fills the arrays for the batch bc_bam_index left in
 * d_work (h_batch: its result; status must be BC_BAM_OK).                                        */
int bc_bam_fill(bc_ctx* ctx, const uint8_t* d_raw, const void* d_work, const bc_bam_batch* h_batch,
                const bc_bam_arrays* d_out, int want_qual);

/* A stream's record decoder (bcio.h: bcio_stream_set_decoder) on the device: the fills' compressed
 * bytes are uploaded, inflated by k_inflate and decoded by the two calls above; the inflated bytes
 * never leave HBM, the bytes behind a batch are carried device to device, and only the per-record
 * arrays come back to the host.  The four callbacks have the types of bcio.h's bcio_decoder
 * (user = the bc_bam_decoder*; bc_bam_host_batch has bcio_dev_batch's layout), so the stream calls
 * them with no Python in between.  A fill with a block k_inflate refuses, a fill of 2 GiB or more
 * and every fill bc_bam_index declines are declined: the host decodes them.
 * A batch's handle owns one device allocation with its arrays (bc_bam_batch_arrays: the pointers;
 * seq and, without want_qual, qual included or NULL as bc_bam_fill takes them); release frees it.
 * Calls on one decoder are serial and blocking (each ends with its download).                   */
typedef struct bc_bam_decoder bc_bam_decoder;
typedef struct bc_bam_host_batch {
    int64_t n;
    uint64_t used;
    uint64_t cigar_words, seq_bytes;
    const int32_t* tid;
    const int32_t* pos;
    const uint16_t* flag;
    const uint8_t* mapq;
    const int32_t* l_seq;
    const int32_t* qstart;
    const int32_t* qend;
    const uint32_t* rec_err;
    const int64_t* ref_span;
    const uint64_t* cig_off;
    const uint64_t* seq_off;
    void* handle;
} bc_bam_host_batch;
int bc_bam_decoder_create(bc_ctx* ctx, int want_qual, uint32_t seg_bytes, bc_bam_decoder** out);
int bc_bam_decoder_destroy(bc_bam_decoder* d);
int bc_bam_decoder_fill(void* user, int append, const uint8_t* h_carry, uint64_t carry_bytes, const uint8_t* h_comp,
                        uint64_t comp_bytes, const bc_zblock* h_blocks, int64_t n, uint64_t inflated_bytes);
int bc_bam_decoder_next(void* user, int64_t max_records, int final, int32_t n_refs, bc_bam_host_batch* out);
int bc_bam_decoder_pending(void* user, uint8_t* h_dst, uint64_t* bytes);
void bc_bam_decoder_release(void* user, void* handle);
int bc_bam_batch_arrays(const void* handle, bc_bam_arrays* out);
/* Cumulative: segments repaired, fills / batches declined, device time (hipEvent pairs) of
 * ms[0] uploads, ms[1] k_inflate, ms[2] index kernels, ms[3] fill kernel, ms[4] downloads, and the
 * host's wall time inside ms[5] the fill calls and ms[6] the next calls (allocations and
 * synchronisation included).  Any output may be NULL.                                            */
int bc_bam_decoder_stats(bc_bam_decoder* d, int64_t* repaired, int64_t* declined, double* ms /* [7] */);
/* The pending bytes are let go (a stream that is closed before its end leaves some). */
int bc_bam_decoder_drop(bc_bam_decoder* d);

/* ---- Read selection on the device (bc_select.hip over bc_select.h) -----------------------------
 * bcio_select (bcio.h) on the record arrays bc_bam_fill left in HBM, bit for bit: a record is
 * accepted when !(flag & 4) && mapq >= min_mapq, wanted when 0 <= tid < n_refs && d_ref_sel[tid],
 * selected when both.  The selected reads come out by reference, file order within a reference:
 *   pos, cig_beg = (uint32)cig_off[i], cig_n = (uint32)(cig_off[i+1] - cig_off[i]),
 *   seq_nib = (uint32)(2 seq_off[i] + max(0, qstart[i])), qlen = (uint32)max(0, qend[i] - qstart[i]),
 *   span = ref_span[i], rec = i, ordinal = accepted records before i (wanted or not);
 * ref_beg[n_refs + 1] slices them.  Per reference, so that the host reads no per-read array:
 *   max_span (0 without reads), max_end = max(pos + span) (0 without reads), n_reads,
 *   n_complex = reads with cig_n > 8, sum_ops = sum of cig_n, err_or = OR of the reads' rec_err,
 *   flags: BC_SEL_SORTED pos is non-decreasing within the reference, BC_SEL_INSIDE every read has
 *   0 <= pos and pos + span <= d_ref_len[tid] (64-bit).
 * The header: n_accepted, n_selected, the first accepted record that is not wanted and its ordinal
 * (-1 / -1 without one), the OR of rec_err over the selected reads, and a status.
 * Declined, never failed: the device handles the batches whose selected reads have non-decreasing
 * tid (a coordinate-sorted or reference-grouped file; unselected records in between do not matter);
 * any other has status BC_SEL_UNGROUPED, and a batch whose cig_off[n] or 2 * seq_off[n] is above
 * 2^32 - 1 has BC_SEL_TOO_LARGE (it wins when both hold).  The call still returns BC_OK; with a
 * non-zero status only the header's status is to be trusted: run bcio_select on the host.       */
#define BC_SEL_OK 0
#define BC_SEL_UNGROUPED 1
#define BC_SEL_TOO_LARGE 2
#define BC_SEL_SORTED 1u
#define BC_SEL_INSIDE 2u

typedef struct bc_sel_header {
    int32_t status;   /* BC_SEL_* */
    uint32_t err_or;
    int64_t n_accepted;
    int64_t n_selected;
    int64_t keyerror_rec;
    int64_t keyerror_ordinal;
    int64_t reserved[3];
} bc_sel_header;

/* Device pointers of the outputs and what they hold: n_cap reads, ref_cap references
 * (ref_beg: ref_cap + 1 entries).                                                             */
typedef struct bc_sel_arrays {
    int32_t* pos;
    uint32_t* cig_beg;
    uint32_t* cig_n;
    uint32_t* seq_nib;
    uint32_t* qlen;
    int64_t* span;
    int64_t* rec;
    int64_t* ordinal;
    int64_t n_cap;
    int64_t* ref_beg;
    int64_t* max_span;
    int64_t* max_end;
    int64_t* n_reads;
    int64_t* n_complex;
    uint64_t* sum_ops;
    uint32_t* err_or;
    uint32_t* flags;     /* BC_SEL_SORTED | BC_SEL_INSIDE */
    int64_t ref_cap;
    bc_sel_header* header;
} bc_sel_arrays;

/* Bytes of bc_bam_select's work buffer for n records (0 <= n < 2^31, n_refs >= 0). */
int bc_bam_select_bytes(int64_t n, int64_t n_refs, size_t* bytes);
/* Stream-ordered, no allocation, no synchronisation: capturable.  d_rec: the arrays of n records
 * (tid, pos, flag, mapq, qstart, qend, rec_err, ref_span, cig_off[n + 1], seq_off[n + 1] are read);
 * d_ref_sel: n_refs bytes, d_ref_len: n_refs int64; d_work: 16-byte aligned, work_bytes >=
 * bc_bam_select_bytes.  BC_E_ARG before any device is touched: NULL pointer, negative n or n_refs,
 * n >= 2^31, small or misaligned work buffer, n_cap < n or ref_cap < n_refs.                    */
int bc_bam_select(bc_ctx* ctx, const bc_bam_arrays* d_rec, int64_t n, int64_t min_mapq, const uint8_t* d_ref_sel,
                  const int64_t* d_ref_len, int32_t n_refs, void* d_work, size_t work_bytes, const bc_sel_arrays* d_out);

/* ---- Row formatting on the device (bc_fmt.hip over bc_fmt.h) ------------------------------------
 * The TSV rows bcio_fmt_rows (bcio.h) writes, byte for byte, from the arrays the kernels left in
 * HBM: counts int32 [k][.] and pc f64 [k][.] as planes of `stride` elements, ent and sec f64, n
 * array positions.  A table of n_seg >= 1 segments, sorted by beg, says what prints: segment i is
 * the array positions [beg, beg + len) with beg a multiple of 64, printed as positions pos0 + 1 ..
 * under the name names[name_off, name_off + name_len); array positions outside every segment (the
 * pads of bc_segments_layout) print nothing.  One reference is n_seg = 1 with beg = 0; a slice of a
 * large reference passes pos0 > 0 and pointers offset to the slice.
 * d_out receives a 64-byte bc_fmt_header followed by seg_off[n_seg + 1] (int64): segment i's text is
 * the bytes [seg_off[i], seg_off[i + 1]) of d_text.
 * Declined, never failed.  BC_FMT_VALUE: a printed value is not finite or reaches 1e15 after scaling
 * by 10^dp, or a name is longer than 255 bytes or leaves the names array; declined_pos is the first
 * such array position.  BC_FMT_TOO_SMALL: total_bytes > text_cap; total_bytes and seg_off are
 * exact, so the call can be repeated with a buffer of that size.  BC_FMT_VALUE wins when both hold.
 * The call returns BC_OK in either case and no text byte is to be trusted.  Whatever the arrays and
 * the table hold, nothing is read past n positions or the names array, nothing is written at or
 * past min(total_bytes, text_cap).                                                               */
#define BC_FMT_OK 0
#define BC_FMT_TOO_SMALL 1
#define BC_FMT_VALUE 2

typedef struct bc_fmt_header {
    int32_t status;        /* BC_FMT_* */
    int32_t reserved0;
    int64_t total_bytes;
    int64_t declined_pos;  /* -1 without one */
    int64_t reserved[5];
} bc_fmt_header;

typedef struct bc_fmt_seg {
    int64_t beg, len, pos0;
    int32_t name_off, name_len;
} bc_fmt_seg;

typedef struct bc_fmt_args {
    const int32_t* counts;   /* device pointers */
    const double* pc;
    const double* ent;
    const double* sec;
    int64_t stride;          /* elements between the planes of counts and of pc, >= n */
    int64_t n;               /* array positions, 0 <= n < 2^31 */
    const bc_fmt_seg* segs;  /* device, n_seg entries */
    int64_t n_seg;
    const uint8_t* names;    /* device, names_bytes bytes */
    int64_t names_bytes;
    int32_t k;               /* 5 or 6 columns printed */
    int32_t dp;              /* decimal places, 0 .. 4 */
    int32_t long_format;
    int32_t reserved;
} bc_fmt_args;

/* Host arithmetic: the bytes of d_work and of d_out (the header and seg_off) for n positions and
 * n_seg segments.                                                                                */
int bc_fmt_rows_bytes(int64_t n, int64_t n_seg, size_t* work_bytes, size_t* out_small_bytes);
/* Stream-ordered, no allocation, no synchronisation: capturable.  d_work and d_out: 8-byte aligned.
 * BC_E_ARG before any device is touched: NULL pointer, k not 5 or 6, dp outside [0, 4], negative
 * sizes, n >= 2^31, n_seg < 1, stride < n, a work buffer smaller than bc_fmt_rows_bytes.         */
int bc_fmt_rows(bc_ctx* ctx, const bc_fmt_args* args, void* d_work, size_t work_bytes, void* d_out, uint8_t* d_text,
                int64_t text_cap);

/* ---- BGZF deflate on the device (bc_deflate.hip over bc_deflate.h) -------------------------------
 * Spans of text into whole BGZF blocks: span i is the bytes [span_off[i], span_off[i + 1]) of the
 * text and becomes ceil(bytes / 65280) blocks of 65,280 input bytes (the last one shorter; an empty
 * span becomes none), each one DEFLATE block with the fixed Huffman codes, or a stored block where
 * those would take at least len + 5 bytes.  The compressed bytes are a pure function of the text
 * and the cut: bc_bgzf_deflate_host writes the same bytes.  No EOF block is appended.
 * d_out_small receives a 64-byte bc_dfl_header followed by span_coff[n_spans + 1] (int64): span i's
 * blocks are the bytes [span_coff[i], span_coff[i + 1]) of d_comp.
 * Declined, never failed (the device call returns BC_OK in every case below).  BC_DFL_TOO_SMALL:
 * total_bytes > comp_cap; total_bytes and span_coff are exact, nothing was written to d_comp, and
 * the call can be repeated with a buffer of that size.  BC_DFL_GATED: *d_gate != 0 (d_gate may be
 * NULL): every kernel returned at once and nothing but the header was written.  Pointing d_span_off
 * at bc_fmt_rows' seg_off and d_gate at its header's status puts the call behind the formatter with
 * no host round trip.  BC_DFL_OFFSETS: the offsets decrease, are negative or pass text_cap.
 * Whatever the offsets hold, nothing is read outside the text's aligned 32-bit words, nothing is
 * written at or past min(total_bytes, comp_cap).                                                  */
#define BC_DFL_OK 0
#define BC_DFL_TOO_SMALL 1
#define BC_DFL_GATED 2
#define BC_DFL_OFFSETS 3

typedef struct bc_dfl_header {
    int32_t status;      /* BC_DFL_* */
    int32_t n_stored;    /* blocks written by the stored fallback */
    int64_t n_blocks;
    int64_t total_bytes; /* compressed */
    int64_t text_bytes;  /* span_off[n_spans] - span_off[0] */
    int64_t reserved[4];
} bc_dfl_header;

/* Host arithmetic: the bytes of d_work (a 64 KiB slot per possible block: text_cap / 65280 + n_spans
 * of them) and of d_out_small, monotone in both arguments.                                         */
int bc_bgzf_deflate_bytes(int64_t text_cap, int64_t n_spans, size_t* work_bytes, size_t* out_small_bytes);
/* Stream-ordered, no allocation, no synchronisation: capturable.  Launch sizes depend on text_cap and
 * n_spans only.  d_work: 16-byte aligned; d_span_off and d_out_small: 8-byte aligned.  BC_E_ARG
 * before any device is touched: NULL pointer (d_gate excepted), negative sizes, n_spans < 1,
 * text_cap >= 2^40, a misaligned buffer, a work buffer smaller than bc_bgzf_deflate_bytes.          */
int bc_bgzf_deflate(bc_ctx* ctx, const uint8_t* d_text, int64_t text_cap,
                    const int64_t* d_span_off /* [n_spans + 1], device, any byte alignment of the values */,
                    int64_t n_spans, const int32_t* d_gate /* may be NULL */, void* d_work, size_t work_bytes,
                    void* d_out_small, uint8_t* d_comp, int64_t comp_cap);
/* The twin over host threads (at most nthreads, capped at 16); touches no device.  Returns a
 * BC_DFL_* status (>= 0) or BC_E_ARG; span_coff and *total are exact under BC_DFL_TOO_SMALL.       */
int bc_bgzf_deflate_host(const uint8_t* h_text, const int64_t* h_span_off, int64_t n_spans, uint8_t* h_comp,
                         int64_t comp_cap, int64_t* span_coff /* [n_spans + 1] */, int64_t* total, int nthreads);

/* ---- Multi-GPU: one process per GPU, RCCL over xGMI---------------------------
 * Counting needs no exchange: references are independent, so each rank owns whole references
 * and runs the single-GPU path on them.  What crosses GPUs is small: the per-reference results
 * the reference prints (main.py:469-595) gathered to rank 0, the reference order rank 0 chose
 * (main.py:92 iterates a set, whose order is per process), and every reference's first
 * out-of-range read (so all ranks raise the reference's first error).  The reference itself has
 * no collective: this replaces nothing in it, it is what lets its per-reference loop
 * (main.py:130-205) run on N GPUs.
 * Rendezvous: rank 0 calls bc_comm_unique_id and hands the BC_COMM_ID_BYTES bytes to the other
 * ranks out of band (basecount_amd/dist.py: a TCP socket next to MASTER_ADDR:MASTER_PORT); then
 * every rank calls bc_comm_init with its own context (one GPU per rank).  Every call below but
 * bc_gather_layout is collective: all ranks make it, in the same order.  Collectives run on the
 * context's stream; the bc_*_bytes / _i64 / barrier calls are blocking, bc_gather_dev is
 * stream-ordered and asynchronous.                                                            */
#define BC_COMM_ID_BYTES 128
typedef struct bc_comm bc_comm;
int bc_comm_unique_id(uint8_t* id /* [BC_COMM_ID_BYTES] */);
int bc_comm_init(bc_ctx* ctx, const uint8_t* id, int rank, int world, bc_comm** out);
int bc_comm_destroy(bc_comm* comm);
int bc_comm_rank(const bc_comm* comm, int* rank, int* world);
int bc_comm_barrier(bc_comm* comm);
/* h_recv[r * n + i] = rank r's h_send[i] (n is the same on every rank). */
int bc_allgather_i64(bc_comm* comm, const int64_t* h_send, int64_t n, int64_t* h_recv);
/* root's n bytes to every rank (n the same on every rank). */
int bc_broadcast_bytes(bc_comm* comm, void* h_buf, int64_t n, int root);
/* Ragged gather layout (host arithmetic, no GPU): offsets[r] = sum of sizes[0..r),
 * offsets[world] = total.  BC_E_ARG on a negative size or an overflowing total.             */
int bc_gather_layout(const int64_t* sizes, int world, int64_t* offsets /* [world + 1] */);
/* Ragged gather to `root`: rank r sends n_r bytes; sizes[0..world) holds every n_r on every rank
 * (exchange them first with bc_allgather_i64).  On root the payloads land concatenated in rank
 * order at bc_gather_layout's offsets; other ranks' receive pointers are ignored.
 *   bc_gather_bytes: host buffers, blocking (h_recv: offsets[world] bytes on root).
 *   bc_gather_dev:   device buffers, stream-ordered on the context's stream, capturable.       */
int bc_gather_bytes(bc_comm* comm, const void* h_send, int64_t n, void* h_recv, const int64_t* sizes, int root);
int bc_gather_dev(bc_comm* comm, const void* d_send, int64_t n, void* d_recv, const int64_t* sizes, int root);
/* One reference's reads split over the ranks (a single contig on N GPUs): every
 * rank's int32 histogram [n] summed into root's d_recv (may alias d_send; ignored off the root).
 * Device buffers, stream-ordered on the context's stream, capturable (RCCL reduce over xGMI). */
int bc_reduce_i32_dev(bc_comm* comm, const int32_t* d_send, int32_t* d_recv, int64_t n, int root);

/* Drop-in for count.bcount with host buffers: uploads, counts all 6 columns, downloads.
 * h_out: refLen x 6 uint32, ROW-major like the reference's vector<vector<unsigned>>
 * (h_out[p*6 + c]).  On BC_E_RANGE, *bad_read / *bad_pos give the first offending read (in
 * read order) and the refPos the reference's .at() would have rejected (count.cpp:60-65,85). */
int bc_bcount_host(int device, int64_t ref_len, uint32_t min_base_quality, const bc_reads* h_reads,
                   uint32_t* h_out, int64_t* bad_read, int64_t* bad_pos);

#ifdef __cplusplus
}
#endif
#endif
