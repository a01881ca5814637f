// bc_npsum.h — numpy's float64 add.reduce on the device: the pairwise-sum routines shared by the
// summary kernels (bc_kernels.hip) and the segmented summary (bc_segments.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace bc {
namespace {

constexpr int kLv = 7;  // 8192 -> 4096 -> ... -> 128: six splits; one spare level
__device__ __forceinline__ void pw_node(int m, int level, int idx, int& off, int& len) {
    // node idx of the given level (level 0: the root) of numpy's recursion over m elements
    // (branch-free: an unsplit node is its own left child, n2 = len, and an empty right one)
    off = 0;
    len = m;
    for (int l = 0; l < level; ++l) {
        const int bit = (idx >> (level - 1 - l)) & 1;
        const int n2 = len > 128 ? (len >> 1) & ~7 : len;  // numpy: n/2 less its remainder mod 8
        off += bit ? n2 : 0;
        len = bit ? len - n2 : n2;
    }
}

// ------------------------------------------------------------------------------ numpy sums
// numpy float64 add.reduce (numpy 2.2, verified against np.add.reduce / np.mean in
// test_summary_matches_numpy in tests/test_gpu_parity.py): the input is consumed in 8192-element buffers, s = 0; s += pw(buffer),
// where pw is numpy's pairwise_sum: n < 8 -> sequential from 0.0; n <= 128 -> eight strided
// accumulators combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) then the tail sequentially;
// else split at n2 = n/2 - (n/2)%8 and add the halves.

__device__ double pw_leaf(const double* a, int n) {
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

// Generic pairwise sum of a[0..m), m <= 8192, by one workgroup (any blockDim >= 128).  numpy's
// recursion (split at n2 = n/2 - (n/2)%8 down to leaves of <= 128) is laid out level by level in
// LDS, in parallel: node i of level l has children 2i, 2i+1 of level l+1; a leaf passes itself
// down as its left child (and an empty right one), so level kLv holds every leaf in order.  The
// leaves are summed in parallel, then every level adds its children bottom-up: the same sums in
// the same order as the recursion, with no per-thread stack (a private array there lives in
// scratch memory, one slow round trip per push).  Returns the value in thread 0 only.
__device__ double pw_block(const double* a, int m, int* s_off, int* s_len, double* s_val) {
    // s_off / s_len: (2^(kLv+1) - 1) nodes; s_val: 2 x 2^kLv values (ping-pong)
    const int t = threadIdx.x;
    if (t == 0) {
        s_off[0] = 0;
        s_len[0] = m;
    }
    __syncthreads();
    for (int l = 0; l < kLv; ++l) {  // top-down: split the nodes of level l
        const int base = (1 << l) - 1, nb = (1 << (l + 1)) - 1;
        for (int i = t; i < (1 << l); i += blockDim.x) {
            const int o = s_off[base + i], n = s_len[base + i];
            int n2 = n;
            if (n > 128) {
                n2 = n / 2;
                n2 -= n2 % 8;
            }
            s_off[nb + 2 * i] = o;
            s_len[nb + 2 * i] = n2;
            s_off[nb + 2 * i + 1] = o + n2;
            s_len[nb + 2 * i + 1] = n - n2;
        }
        __syncthreads();
    }
    const int leaves = 1 << kLv, lbase = leaves - 1;
    double* cur = s_val;
    double* nxt = s_val + leaves;
    for (int i = t; i < leaves; i += blockDim.x) {
        const int n = s_len[lbase + i];
        cur[i] = n > 0 ? pw_leaf(a + s_off[lbase + i], n) : 0.0;
    }
    __syncthreads();
    for (int l = kLv - 1; l >= 0; --l) {  // bottom-up: a split node adds its children, left + right
        const int base = (1 << l) - 1;
        for (int i = t; i < (1 << l); i += blockDim.x)
            nxt[i] = s_len[base + i] > 128 ? cur[2 * i] + cur[2 * i + 1] : cur[2 * i];
        __syncthreads();
        double* tmp = cur;
        cur = nxt;
        nxt = tmp;
    }
    const double r = t == 0 ? cur[0] : 0.0;
    __syncthreads();
    return r;
}

// The same sum, pw_block's tree, without its 14 barriers and one-thread leaves: every leaf slot
// (LV levels of numpy's split: a leaf passes itself down as the left child, an empty right one)
// is found by descending its bit path, its eight strided accumulators are eight threads'
// (every load issued together, unguarded: clamped, and the extra ones selected to -0.0, which
// adds exactly nothing to any double), combined by shuffles in numpy's order; then one wave adds
// the slots up the tree: node i of level d sits in lane i << (LV - 1 - d), its right child
// 2^(LV-2-d) lanes up (a shuffle down), and each lane's descent recorded which of its ancestors
// split.  LV = kLv covers m <= 8192; LV = 4 covers m <= 512 (checked against numpy for every
// such m) with 128 tasks, two waves, instead of 1024.  a: m doubles (LDS or global); s_leaf:
// 2^LV doubles of LDS; NT threads, all calling.  Returns the value in thread 0 only.
template <int NT, int LV = kLv>
__device__ __forceinline__ double pw_fast(const double* a, int m, double* s_leaf) {
    constexpr int kSlots = 1 << LV, kTasks = 8 * kSlots, R = kTasks >= NT ? kTasks / NT : 1;
    static_assert(kTasks % 64 == 0 && (kTasks < NT || R * NT == kTasks), "tasks: whole waves");
    const int t = threadIdx.x, j = t & 7;  // (NT is a multiple of 8: every task of a thread has accumulator j)
    if (kTasks >= NT || t < kTasks) {  // (wave-uniform)
        int len[R], full[R];
        double v[R][16], rem[R][7];
#pragma unroll
        for (int q = 0; q < R; ++q) {  // every task's loads issued first
            int off;
            pw_node(m, LV, (t + NT * q) >> 3, off, len[q]);
            full[q] = len[q] & ~7;
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int i = j + 8 * u;
                v[q][u] = a[off + (i < full[q] ? i : 0)];
            }
#pragma unroll
            for (int u = 0; u < 7; ++u) {  // the leaf's last len % 8 (or, below 8, all) elements
                const int i = full[q] + u;
                rem[q][u] = a[off + (i < len[q] ? i : 0)];
            }
        }
#pragma unroll
        for (int q = 0; q < R; ++q) {
            double x = v[q][0];
#pragma unroll
            for (int u = 1; u < 16; ++u) x = x + (j + 8 * u < full[q] ? v[q][u] : -0.0);
            x = x + __shfl_down(x, 1);  // (r0+r1), (r2+r3), ...
            x = x + __shfl_down(x, 2);
            x = x + __shfl_down(x, 4);  // ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7))
            if (len[q] < 8) x = 0.0;    // numpy: n < 8 sums from 0, in order
#pragma unroll
            for (int u = 0; u < 7; ++u) x = x + (full[q] + u < len[q] ? rem[q][u] : -0.0);
            if (((t + NT * q) & 7) == 0) s_leaf[(t + NT * q) >> 3] = x;
        }
    }
    __syncthreads();
    double res = 0.0;
    if (t < 64) {
        // lane tt's descent to node tt of level LV - 1, recording which ancestors split
        const int tt = t < (1 << (LV - 1)) ? t : 0;
        int n = m;
        unsigned split = 0;
#pragma unroll
        for (int l = 0; l < LV - 1; ++l) {
            split |= (unsigned)(n > 128) << l;
            const int n2 = n > 128 ? (n >> 1) & ~7 : n;
            n = ((tt >> (LV - 2 - l)) & 1) ? n - n2 : n2;
        }
        const double v0 = s_leaf[2 * tt], v1 = s_leaf[2 * tt + 1];
        double val = n > 128 ? v0 + v1 : v0;
#pragma unroll
        for (int d = LV - 2; d >= 0; --d) {
            const double c1 = __shfl_down(val, 1 << (LV - 2 - d));
            val = ((split >> d) & 1) ? val + c1 : val;
        }
        res = val;
    }
    __syncthreads();  // s_leaf reusable
    return res;
}

// Full 8192-element buffer with the fixed tree: 64 leaves of 128; 256 threads, thread t owns
// accumulators {2(t&3), 2(t&3)+1} of leaf t>>2.  Value valid in thread 0.
template <class F>
__device__ double pw_full8192(F&& val, double* s_wave) {
    const int t = threadIdx.x;
    const int leaf = t >> 2, s = t & 3;
    const int base = leaf * 128 + 2 * s;
    double ra = val(base), rb = val(base + 1);
#pragma unroll
    for (int i = 1; i < 16; ++i) {
        ra += val(base + 8 * i);
        rb += val(base + 8 * i + 1);
    }
    double v = ra + rb;              // (r0+r1), (r2+r3), (r4+r5), (r6+r7)
    v = v + __shfl_down(v, 1);       // lanes s=0: (r0+r1)+(r2+r3); s=2: (r4+r5)+(r6+r7)
    v = v + __shfl_down(v, 2);       // s=0: leaf value
    v = v + __shfl_down(v, 4);       // pairs of leaves
    v = v + __shfl_down(v, 8);
    v = v + __shfl_down(v, 16);
    v = v + __shfl_down(v, 32);      // lane 0: 16 leaves = pw(2048)
    if ((t & 63) == 0) s_wave[t >> 6] = v;
    __syncthreads();
    double r = 0.0;
    if (t == 0) r = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
    __syncthreads();
    return r;
}

}  // namespace
}  // namespace bc
