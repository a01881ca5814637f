// bc_planes.h — bit-plane (vertical) counters of the position-tiled walk, on the device and on the
// host (plain integer functions: tests/native/planes_check.cpp compiles them with g++).
//
// A window word x holds the event classes of 8 positions, one nibble each (bc_walk.h).  A, C, G
// and T are one-hot (0001, 0010, 0100, 1000), so x already is four bit planes of 8 positions: bit
// 4k + b says "class bit b at window position k".  The walk therefore counts the 32 BITS of x, not
// the columns: p[j] holds bit j of the 32 running sums, and two reads' words are added with one
// full adder into p[0] and a carry rippling up (9 bitwise operations for two reads).
//
// The two classes that are not one-hot are put right afterwards: N (0011) counts in planes 0 and 1,
// a deletion / ref-skip (1100) in planes 2 and 3.  The walk counts them separately in nibble
// counters (fix_n / fix_d below) and the fold computes
//     A = plane0 - N,  C = plane1 - N,  G = plane2 - DS,  T = plane3 - DS,  column 4 = DS,  5 = N.
//
// Capacities (tests/test_gpu_plane_counters.py sits on each):
//   kPlanes = 5 planes: a lane (read slot) holds sums <= kPlaneAdds = 31.  A chunk of 64 reads
//     adds at most kChunkAdds = 8 reads to a lane, and the walk folds BEFORE a chunk that might
//     not fit (bc_walk.h: counters_reserve), not inside its loop: in practice after every third
//     chunk, at 24 reads per lane.
//   The fold adds the 8 read slots of a window plane by plane (planes_join: 5 -> 6 -> 7 -> 8
//     planes), so a position's sum is <= 8 x 31 = 248 <= 255 and planes_counts' byte fields hold it.
//   The fix-up nibbles hold kFixAdds = 15 reads: folded before every chunk but the first after a
//     fold (8 reads per lane); their 8 slots add up to <= 120 in a byte.
#pragma once
#include <cstdint>

#ifndef BC_HD
#define BC_HD __host__ __device__ __forceinline__
#endif

constexpr uint32_t kM1 = 0x11111111u;  // bit 0 of every nibble
constexpr int kPlanes = 5;
constexpr int kPlaneAdds = 31;  // reads a lane's planes hold
constexpr int kFixAdds = 15;    // reads a lane's fix-up nibbles hold
constexpr int kChunkAdds = 8;   // reads a chunk (64 reads, 8 read slots) adds to a lane at most
constexpr int kSumPlanes = kPlanes + 3;  // planes of the sum over a window's 8 read slots

// bitwise a ^ b ^ c and majority(a, b, c): one v_bitop3_b32 each on the device (spelled out, the
// compiler reassociates the adders below into half as many again)
BC_HD uint32_t bit_xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}
BC_HD uint32_t bit_maj(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
#else
    return (a & b) | (c & (a | b));
#endif
}

// p += x0 + x1, bit by bit: a full adder at weight 1, then the carry ripples up.  The caller keeps
// the number of reads added at or below kPlaneAdds, so nothing is carried out of the last plane.
BC_HD void planes_add2(uint32_t (&p)[kPlanes], uint32_t x0, uint32_t x1) {
    uint32_t c = bit_maj(p[0], x0, x1);
    p[0] = bit_xor3(p[0], x0, x1);
#pragma unroll
    for (int j = 1; j < kPlanes; ++j) {
        const uint32_t t = p[j] & c;
        p[j] ^= c;
        c = t;
    }
}

// s = a + b for two NP-plane counters (NP + 1 planes: no overflow)
template <int NP>
BC_HD void planes_join(const uint32_t (&a)[NP], const uint32_t (&b)[NP], uint32_t (&s)[NP + 1]) {
    uint32_t c = a[0] & b[0];
    s[0] = a[0] ^ b[0];
#pragma unroll
    for (int j = 1; j < NP; ++j) {
        s[j] = bit_xor3(a[j], b[j], c);
        c = bit_maj(a[j], b[j], c);
    }
    s[NP] = c;
}

// plane word s -> bit b of window position k's nibble in bit 0 of byte b
BC_HD uint32_t plane_spread(uint32_t s, int k) { return (((s >> (4 * k)) & 15u) * 0x00204081u) & 0x01010101u; }

// The four sums of window position k (0..7) as bytes: byte b = the sum of class bit b.  Each sum
// is below 256 (see the capacities above), so the Horner steps never carry between the bytes.
BC_HD uint32_t planes_counts(const uint32_t (&s)[kSumPlanes], int k) {
    uint32_t acc = 0;
#pragma unroll
    for (int j = kSumPlanes - 1; j >= 0; --j) {
        acc = (acc << 1) + plane_spread(s[j], k);
    }
    return acc;
}

// Fix-up flags of a window word: bit 0 of a nibble that holds N (0011) / a deletion (1100).
BC_HD uint32_t fix_n(uint32_t x) { return x & (x >> 1) & kM1; }
BC_HD uint32_t fix_d(uint32_t x) { return (x >> 2) & (x >> 3) & kM1; }
