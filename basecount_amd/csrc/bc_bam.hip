// bc_bam.hip — BAM record decode on the device: inflated bytes to the arrays of a read batch.
//
// Three launches over bc_bam.h's functions (the host check compiles the same ones):
//   k_bam_speculate  one wave per segment of seg_bytes: its lanes test consecutive offsets with
//                    bcb_plausible, the first that passes is the segment's entry, and one lane hops
//                    from there to the segment's end (bcb_hop), storing starts and running counts
//   k_bam_stitch     one lane walks the chain from the known first offset (bcb_stitch): a segment
//                    counts only if its entry is the chain's offset, else it is hopped again from
//                    there; prefix sums, the cut at max_records and the fill's status
//   k_bam_fill       one wave per accepted segment: a lane per record for the scalars (64 records a
//                    step), then each record's CIGAR words, SEQ and QUAL bytes strided over the wave
// Nothing here synchronises or allocates; bc_bam_index's download of the result is the only
// blocking step (bc_capi.hip).
#include "bc_internal.h"

#include <cstring>

#include "bc_bam.h"

namespace bc {
namespace {

constexpr int kBamWaves = 4;
constexpr int kBamThreads = 64 * kBamWaves;

__global__ __launch_bounds__(kBamThreads) void k_bam_speculate(const uint8_t* raw, uint32_t N, uint32_t seg_bytes,
                                                               uint32_t first, int32_t n_refs, void* work) {
    const bcb_work w = bcb_bind(work, bcb_make_layout(N, seg_bytes));
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t ln = threadIdx.x & 63u;
    const uint32_t s = blockIdx.x * kBamWaves + wave;
    if (s >= w.nseg) return;
    const uint32_t beg = s * seg_bytes, end = bcb_seg_end(s, seg_bytes, N);
    uint32_t entry = BCB_NO_ENTRY;
    if (first >= beg && first < end) {
        entry = first;
    } else {
        for (uint32_t base = beg; base < end; base += 64u) {  // wave-uniform loop
            const uint32_t q = base + ln;
            const uint64_t m = __ballot(q < end && bcb_plausible(raw, N, q, n_refs));
            if (m) {
                entry = base + (uint32_t)__builtin_ctzll(m);
                break;
            }
        }
    }
    if (ln == 0) bcb_speculate_from(raw, N, s, seg_bytes, entry, w);
}

__global__ __launch_bounds__(64) void k_bam_stitch(const uint8_t* raw, uint32_t N, uint32_t seg_bytes, uint32_t first,
                                                   int64_t max_records, int final, void* work) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bcb_work w = bcb_bind(work, bcb_make_layout(N, seg_bytes));
    bcb_stitch(raw, N, seg_bytes, first, max_records, final != 0, w);
}

__global__ __launch_bounds__(kBamThreads) void k_bam_fill(const uint8_t* raw, uint32_t N, uint32_t seg_bytes,
                                                          const void* work, bcb_arrays o, int want_qual) {
    const bcb_work w = bcb_bind(const_cast<void*>(work), bcb_make_layout(N, seg_bytes));
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t ln = threadIdx.x & 63u;
    const uint32_t s = blockIdx.x * kBamWaves + wave;
    if (s >= w.nseg) return;
    const bcb_result* res = w.res;
    // a result the arrays were not sized for, or a declined fill, writes nothing
    if (res->status != BCB_ST_OK || res->raw_bytes != N || res->seg_bytes != seg_bytes || res->n > o.n_cap ||
        res->cigar_words > o.cigar_cap || res->seq_bytes > o.seq_cap)
        return;
    if (s == 0) bcb_fill_tail(res, o, ln, 64u);
    const bcb_seg sg = w.segs[s];
    const uint64_t slot = (uint64_t)s * (w.cap + 1u);
    for (uint32_t j0 = 0; j0 < sg.take; j0 += 64u) {
        const uint32_t j = j0 + ln;
        if (j < sg.take)
            bcb_fill_meta(raw, w.starts[slot + j], (uint64_t)sg.rec_base + j, (uint64_t)sg.cig_base + w.cigx[slot + j],
                          (uint64_t)sg.seq_base + w.seqx[slot + j], o);
    }
    for (uint32_t j = 0; j < sg.take; ++j)
        bcb_fill_bytes(raw, w.starts[slot + j], (uint64_t)sg.cig_base + w.cigx[slot + j],
                       (uint64_t)sg.seq_base + w.seqx[slot + j], o, want_qual != 0, ln, 64u);
}

}  // namespace

size_t bam_index_bytes(uint64_t raw_bytes, uint64_t seg_bytes) { return (size_t)bcb_make_layout(raw_bytes, seg_bytes).total; }

hipError_t launch_bam_index(hipStream_t s, const uint8_t* raw, uint32_t N, uint32_t seg_bytes, uint32_t first,
                            int64_t max_records, bool final, int32_t n_refs, void* work) {
    const bcb_layout l = bcb_make_layout(N, seg_bytes);
    const dim3 grid((l.nseg + kBamWaves - 1) / kBamWaves), block(kBamThreads);
    hipLaunchKernelGGL(k_bam_speculate, grid, block, 0, s, raw, N, seg_bytes, first, n_refs, work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bam_stitch, dim3(1), dim3(64), 0, s, raw, N, seg_bytes, first, max_records, final ? 1 : 0, work);
    return hipGetLastError();
}

hipError_t launch_bam_fill(hipStream_t s, const uint8_t* raw, uint32_t N, uint32_t seg_bytes, const void* work,
                           const bc_bam_arrays& out, bool want_qual) {
    static_assert(sizeof(bcb_arrays) == sizeof(bc_bam_arrays), "bc_bam_arrays has bcb_arrays' layout");
    bcb_arrays o;
    memcpy(&o, &out, sizeof o);
    const bcb_layout l = bcb_make_layout(N, seg_bytes);
    const dim3 grid((l.nseg + kBamWaves - 1) / kBamWaves), block(kBamThreads);
    hipLaunchKernelGGL(k_bam_fill, grid, block, 0, s, raw, N, seg_bytes, work, o, want_qual ? 1 : 0);
    return hipGetLastError();
}

}  // namespace bc
