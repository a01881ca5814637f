// bc_cohort.h — the decisions a cohort run (several files' reads side by side in shared device
// buffers, basecount_amd/cohort.py) shares between its two kernels and the host.
//
//   k_seg_rebase        (bc_segments.hip, bc_segments_rebase): one lane per read; the read's segment
//                       (bcc_seg_of over read_beg[]) says which file's arrays it indexes, and its
//                       cig_beg / seq_nib move by that file's base (bcc_rebase);
//   k_amplicon_segments (bc_kernels.hip, bc_amplicons_segments): one workgroup per (segment,
//                       window); the window is clipped to ITS segment (bcc_clip), so no pad and no
//                       neighbour is ever read, and the medians take the elements bcc_k1 / bcc_k2.
//
// Every function is plain integer arithmetic, compiled for the device and for the host alike;
// tests/native/cohort_check.cpp runs them as plain loops under AddressSanitizer + UBSan.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BCC_HD __host__ __device__ __forceinline__
#else
#define BCC_HD inline
#endif

#define BCC_SORT_MAX 512 /* positions of a window whose medians one wave sorts; beyond: radix select */

// ---- amplicon windows ----
// main.py:519-551 slices list[max(lo, 0) : min(hi, L - 1) + 1]: the window [lo, hi] (inclusive)
// clipped to the segment's own [0, L - 1].  n <= 0: empty, every vector entry is -1.
struct bcc_window {
    int64_t lo, n;
};

BCC_HD bcc_window bcc_clip(int64_t lo, int64_t hi, int64_t L) {
    bcc_window w;
    w.lo = lo < 0 ? 0 : lo;
    const int64_t h = hi > L - 1 ? L - 1 : hi;
    w.n = h >= w.lo ? h - w.lo + 1 : 0;  // (lo > hi, a window wholly past L, L <= 0: empty)
    return w;
}
BCC_HD bool bcc_empty(const bcc_window& w) { return w.n <= 0; }

// np.median of n >= 1 values: the mean of the sorted elements k1 and k2 (equal for odd n)
BCC_HD int64_t bcc_k1(int64_t n) { return (n - 1) / 2; }
BCC_HD int64_t bcc_k2(int64_t n) { return n / 2; }
BCC_HD bool bcc_sorted_path(int64_t n) { return n <= BCC_SORT_MAX; }

// ---- the segment of a read ----
// The last s in [0, n_seg) with read_beg[s] <= i: empty segments (read_beg[s] == read_beg[s + 1])
// are stepped over.  Stays inside [0, n_seg) whatever the table holds; n_seg >= 1.
BCC_HD int bcc_seg_of(const int64_t* read_beg, int n_seg, int64_t i) {
    int lo = 0, hi = n_seg;  // read_beg[lo] <= i < read_beg[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (read_beg[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- the rebase ----
// File f's CIGAR words start at word cig_base[f] of the shared buffer and its sequence at a byte
// offset that is a multiple of 16, nib_base[f] = 2 x that offset (qualities are indexed by nibble).
// A read's cig_beg / seq_nib count from its file's arrays; in the shared buffers they are value +
// base, kept in 32 bits.  The host never builds a group whose buffers reach 2^32 words or nibbles
// (bcc_fits), so value + base <= total - 1 < 2^32 and the sum cannot wrap.
#define BCC_INDEX_LIMIT 0x100000000ull /* 2^32: a shared buffer holds fewer words / nibbles */

BCC_HD bool bcc_fits(uint64_t cig_words_total, uint64_t nib_total) {
    return cig_words_total < BCC_INDEX_LIMIT && nib_total < BCC_INDEX_LIMIT;
}
BCC_HD uint32_t bcc_rebase(uint32_t value, uint64_t base) { return (uint32_t)((uint64_t)value + base); }
// padded sequence bytes of one file in the shared buffer: its BC_SEQ_EVENT size is a multiple of 16
BCC_HD uint64_t bcc_nib_base(uint64_t seq_byte_offset) { return 2u * seq_byte_offset; }
BCC_HD bool bcc_base_aligned(uint64_t nib_base) { return (nib_base & 31u) == 0; }
