// bc_slice.h — slot arithmetic of k_pileup's slice instance (bc_tile.h: process_chunk<.., SLICE>),
// in plain integers so that a host program can enumerate it (tests/native/slice_check.cpp).
//
// The slice instance stages, per read of a chunk, only the bytes one 64-position tile can read of
// it.  A wave's stage is 64 slots of 64 B, slot r for read r of the chunk, filled by LDS-DMA in
// four 16-B pieces.  A slot holds bytes [src, src + 64) of the BC_SEQ_EVENT buffer (two bases per
// byte), where src is the 16-B-aligned byte at or below the base the read has at the tile's first
// covered position, max(t0, pos + st).  The slices are issued BEFORE the read's CIGAR is decoded,
// assuming one run that starts at query offset 0 and reference offset 0 (st = 0, qd = 0); after
// the decode `covered` says whether every base the tile needs of the read lies in its slot.
//
//   rel      pos - t0, the read's start relative to the tile's first position (may be negative)
//   st, en   the run's reference offsets [st, en) from the read's start
//   qd       the run's query delta (query offset = reference offset + qd: a leading insertion's length)
//   seq_nib  nibble index of the read's first query base in the buffer
//   buf_end  readable bytes of the buffer, a multiple of 16 (bc_seq_event_bytes)
// Nibble indices are 32 bits and modular, as everywhere in the walk (buffers below 2^31 bytes).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define BC_SLICE_HD __host__ __device__ inline
#else
#define BC_SLICE_HD inline
#endif

namespace bc_slice {

constexpr int kTile = 64;        // positions per tile
constexpr int kSlots = 64;       // reads per chunk
constexpr int kSlotBytes = 64;
constexpr int kPieceBytes = 16;  // one lane's LDS-DMA
constexpr int kPieces = kSlotBytes / kPieceBytes;
constexpr int kStageBytes = kSlots * kSlotBytes;  // 4,096 B per wave (+ one 16-B pad on each side)

// Nibble index of the base at the tile's first covered position, max(t0, pos + st).
BC_SLICE_HD uint32_t first_nibble(uint32_t seq_nib, int32_t rel, uint32_t st, int32_t qd) {
    const int32_t nrel = (int32_t)(0u - (uint32_t)rel);
    const int32_t o = nrel > (int32_t)st ? nrel : (int32_t)st;  // its reference offset from the read's start
    return seq_nib + (uint32_t)qd + (uint32_t)o;
}

// The slot's first source byte, from the fields alone (st = 0, qd = 0 assumed).
BC_SLICE_HD uint32_t source_byte(uint32_t seq_nib, int32_t rel) {
    return (first_nibble(seq_nib, rel, 0u, 0) >> 1) & ~(uint32_t)(kPieceBytes - 1);
}

// Piece k of a slot is copied only when it begins below the buffer's readable end.
BC_SLICE_HD bool piece_issued(uint32_t src, int k, uint32_t buf_end) {
    return (uint64_t)src + (uint32_t)(kPieceBytes * k) < buf_end;
}

// The walk record's `nb` (bc_walk.h, tile-relative records): 4 x the nibble index, relative to the
// stage, of the base the run has at the tile's FIRST position t0 (below the slot when the read
// starts inside the tile: such windows are masked).
BC_SLICE_HD uint32_t slot_nb(int slot, uint32_t seq_nib, int32_t rel, int32_t qd, uint32_t src) {
    return ((uint32_t)(2 * kSlotBytes * slot) + seq_nib + (uint32_t)qd - (uint32_t)rel - 2u * src) * 4u;
}

// Slot-relative nibble of the first base the tile needs, and how many it needs ([lo, hi) of the
// run's reference offsets lie on the tile).  count <= 0: the tile reads nothing of the read.
BC_SLICE_HD int32_t needed(uint32_t seq_nib, int32_t rel, uint32_t st, uint32_t en, int32_t qd, uint32_t src,
                           int32_t& first) {
    const int32_t nrel = (int32_t)(0u - (uint32_t)rel), trel = (int32_t)((uint32_t)kTile - (uint32_t)rel);
    const int32_t lo = nrel > (int32_t)st ? nrel : (int32_t)st;
    const int32_t hi = trel < (int32_t)en ? trel : (int32_t)en;
    first = (int32_t)(seq_nib + (uint32_t)qd + (uint32_t)lo - 2u * src);
    return hi - lo;
}

// Every base the tile needs of the read lies in [0, 64 B) of its slot, in pieces that were issued.
BC_SLICE_HD bool covered(uint32_t seq_nib, int32_t rel, uint32_t st, uint32_t en, int32_t qd, uint32_t src,
                         uint32_t buf_end) {
    int32_t first;
    const int32_t n = needed(seq_nib, rel, st, en, qd, src, first);
    if (n <= 0) return true;
    const uint32_t f = (uint32_t)first;  // (n <= 64)
    if (f >= (uint32_t)(2 * kSlotBytes) || f + (uint32_t)n > (uint32_t)(2 * kSlotBytes)) return false;
    return piece_issued(src, (int)(((f + (uint32_t)n - 1u) >> 1) / kPieceBytes), buf_end);  // (the pieces below it begin lower)
}

}  // namespace bc_slice
