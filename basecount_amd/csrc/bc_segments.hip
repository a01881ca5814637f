// bc_segments.hip — several small references counted as ONE virtual reference (bc_pileup_segments).
//
// A coordinate-sorted file orders reads by (refID, pos).  Reference i of a group sits at virtual
// offset voff[i] = sum_{j<i} round_up(L_j, 64): its reads' starts moved by voff[i], the group's
// reads are one sorted batch on a reference of voff[n] positions, every 64-position tile of which
// belongs to one reference only.  The pileup kernels then run on that batch unchanged; what this
// file adds is the start shift before them and the per-reference summary after them:
//   k_seg_vpos      one lane per read: its segment (a search of read_beg[]), vpos = voff + pos;
//   k_sum_segments  one workgroup per segment: bc_summary's four doubles over the segment's slice
//                   of the coverage and entropy, by the numpy-exact routines of bc_npsum.h.
#include "bc_cohort.h"
#include "bc_internal.h"
#include "bc_npsum.h"

namespace bc {
namespace {

// The segment of read i: the last s with read_beg[s] <= i (empty segments, read_beg[s] ==
// read_beg[s + 1], are stepped over).  Stays inside [0, n_seg) whatever the table holds.
__device__ __forceinline__ int seg_of(const int64_t* __restrict__ read_beg, int n_seg, int64_t i) {
    int lo = 0, hi = n_seg;  // read_beg[lo] <= i < read_beg[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (read_beg[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// Most waves' 64 reads lie in one segment: the wave then searches once, with uniform addresses
// (scalar loads), for its first and its last read; only a wave that straddles segments searches
// per lane.  A start outside [0, ref_len] is a caller error (the header's contract); it is
// clamped into the segment so that the batch stays sorted and inside the virtual reference.
__global__ __launch_bounds__(256) void k_seg_vpos(const int32_t* __restrict__ pos, int64_t n,
                                                  const int64_t* __restrict__ ref_len,
                                                  const int64_t* __restrict__ read_beg,
                                                  const int64_t* __restrict__ voff, int n_seg,
                                                  int32_t* __restrict__ vpos) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t w0 = (int64_t)blockIdx.x * 256 + 64 * wave;
    if (w0 >= n) return;  // (uniform; no barriers in this kernel)
    const int64_t w1 = w0 + 63 < n ? w0 + 63 : n - 1;
    const int64_t i = w0 + (threadIdx.x & 63);
    const int s0 = seg_of(read_beg, n_seg, w0), s1 = seg_of(read_beg, n_seg, w1);
    int seg = s0;
    if (s0 != s1) seg = seg_of(read_beg, n_seg, i < n ? i : n - 1);
    if (i >= n) return;
    const int64_t L = ref_len[seg];
    int64_t p = pos[i];
    p = p < 0 ? 0 : (p > L ? L : p);
    vpos[i] = (int32_t)(voff[seg] + p);
}

// bc_summary per segment (main.py:469-495): numpy takes the slice's entropies in 8192-element
// buffers, s = 0; s += pairwise_sum(buffer), and the pairwise tree of a buffer depends on its
// element count only, so the slice's own buffers [c0, c0 + 8192) are summed from wherever the
// slice starts (pw_full8192 / pw_block read element by element: no alignment is assumed).  The
// coverage sum and the non-zero count are exact integers, as in k_sum_chunks / k_sum_final.
__global__ __launch_bounds__(256) void k_sum_segments(const int64_t* __restrict__ ref_len,
                                                      const int64_t* __restrict__ voff,
                                                      const int32_t* __restrict__ cov,
                                                      const double* __restrict__ ent, double* __restrict__ out) {
    __shared__ double s_wave[4];
    __shared__ long long s_red[8];
    __shared__ int s_off[(2 << kLv) - 1], s_len[(2 << kLv) - 1];
    __shared__ double s_val[2 << kLv];
    const int seg = blockIdx.x, t = threadIdx.x;
    const int64_t L = ref_len[seg];
    if (L <= 0) {  // (uniform) not a segment bc_segments_layout accepts
        if (t < 4) out[4 * (int64_t)seg + t] = 0.0;
        return;
    }
    const int32_t* c = cov + voff[seg];
    const double* e = ent + voff[seg];
    double s = 0.0;
    for (int64_t c0 = 0; c0 < L; c0 += kNpBuf) {  // numpy's buffers, in order
        const int m = (int)(L - c0 < kNpBuf ? L - c0 : kNpBuf);
        const double v = m == kNpBuf ? pw_full8192([&](int i) { return e[c0 + i]; }, s_wave)
                                     : pw_block(e + c0, m, s_off, s_len, s_val);
        if (t == 0) s += v;
    }
    long long cs = 0, nz = 0;
    for (int64_t i = t; i < L; i += 256) {
        const long long v = c[i];
        cs += v;
        nz += v != 0;
    }
    for (int o = 32; o > 0; o >>= 1) {
        cs += __shfl_down(cs, o);
        nz += __shfl_down(nz, o);
    }
    if ((t & 63) == 0) {
        s_red[t >> 6] = cs;
        s_red[4 + (t >> 6)] = nz;
    }
    __syncthreads();
    if (t == 0) {
        cs = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
        nz = (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]);
        const double n = (double)L;
        double* o = out + 4 * (int64_t)seg;
        o[0] = (double)cs / n;  // the integer sum is exact in float64: np.mean == sum / n
        o[1] = s / n;
        o[2] = (double)nz;
        o[3] = (double)cs;
    }
}

// A cohort batch (bc_cohort.h): read i indexes the arrays of the file its segment belongs to; in
// the shared buffers its CIGAR words and its nibbles lie one base further on.  k_seg_vpos's
// schedule: a wave inside one segment searches twice with uniform addresses, a wave that straddles
// segments once per lane.  No CIGAR or sequence byte is read.  in == out is in place: every lane
// reads its own two words before it writes them.
__global__ __launch_bounds__(256) void k_seg_rebase(int64_t n, const int64_t* __restrict__ read_beg, int n_seg,
                                                    const uint64_t* __restrict__ cig_base,
                                                    const uint64_t* __restrict__ nib_base, const uint32_t* in_cig,
                                                    const uint32_t* in_nib, uint32_t* out_cig, uint32_t* out_nib) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t w0 = (int64_t)blockIdx.x * 256 + 64 * wave;
    if (w0 >= n) return;  // (uniform; no barriers in this kernel)
    const int64_t w1 = w0 + 63 < n ? w0 + 63 : n - 1;
    const int64_t i = w0 + (threadIdx.x & 63);
    const int s0 = bcc_seg_of(read_beg, n_seg, w0), s1 = bcc_seg_of(read_beg, n_seg, w1);
    int seg = s0;
    if (s0 != s1) seg = bcc_seg_of(read_beg, n_seg, i < n ? i : n - 1);
    if (i >= n) return;
    const uint32_t c = in_cig[i], q = in_nib[i];
    out_cig[i] = bcc_rebase(c, cig_base[seg]);
    out_nib[i] = bcc_rebase(q, nib_base[seg]);
}

}  // namespace

hipError_t launch_seg_rebase(hipStream_t s, int64_t n, const int64_t* read_beg, int n_seg, const uint64_t* cig_base,
                             const uint64_t* nib_base, const uint32_t* in_cig, const uint32_t* in_nib,
                             uint32_t* out_cig, uint32_t* out_nib) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_seg_rebase, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, read_beg, n_seg, cig_base,
                       nib_base, in_cig, in_nib, out_cig, out_nib);
    return hipGetLastError();
}

hipError_t launch_seg_vpos(hipStream_t s, const int32_t* pos, int64_t n, const int64_t* ref_len,
                           const int64_t* read_beg, const int64_t* voff, int n_seg, int32_t* vpos) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_seg_vpos, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pos, n, ref_len, read_beg, voff,
                       n_seg, vpos);
    return hipGetLastError();
}

hipError_t launch_sum_segments(hipStream_t s, int n_seg, const int64_t* ref_len, const int64_t* voff,
                               const int32_t* cov, const double* ent, double* out) {
    if (n_seg <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sum_segments, dim3((unsigned)n_seg), dim3(256), 0, s, ref_len, voff, cov, ent, out);
    return hipGetLastError();
}

}  // namespace bc
