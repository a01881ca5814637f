// bc_slice.h — slot arithmetic of k_pileup's slice instance (bc_tile.h: process_chunk<.., SLICE>),
// in plain integers so that a host program can enumerate it (tests/native/slice_check.cpp).
//
// The slice instance stages, per read of a chunk, only the bytes one 64-position tile can read of
// it.  A wave's stage is 64 slots of 64 B, slot r for read r of the chunk, filled by LDS-DMA in
// 16-B pieces: piece k holds bytes [src + 16 k, src + 16 k + 16) of the BC_SEQ_EVENT buffer (two
// bases per byte) when it was issued, and whatever the slot held before when it was not (a piece
// that begins at or beyond the buffer's readable end, and piece 3 of a one-op chunk: below).  src
// is the 16-B-aligned byte at or below the base the read has at the tile's first covered position,
// max(t0, pos + st).  The slices are issued BEFORE the read's CIGAR is decoded, assuming one run
// that starts at query offset 0 and reference offset 0 (st = 0, qd = 0); after the decode `covered`
// says whether every base the tile needs of the read lies in issued pieces of its slot.
//
// One-op chunks (every read of the chunk has ONE CIGAR op, known from the fields before the slices
// are issued): no read has a leading insertion, so st = 0 and qd = 0 hold, the first needed base
// lies in the slot's first 16 bytes and the last of the tile's <= 64 bases at byte <= 47: pieces
// 0-2 (kOneOpPieces) are issued and piece 3 is not; `covered_one_op` is `covered` for such a read.
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
constexpr int kOneOpPieces = 3;  // pieces issued per slot of a one-op chunk
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

// Every base the tile needs of the read lies in [0, 64 B) of its slot, in pieces that were issued
// (`pieces`: how many of the slot's pieces the chunk issues at all).
BC_SLICE_HD bool covered(uint32_t seq_nib, int32_t rel, uint32_t st, uint32_t en, int32_t qd, uint32_t src,
                         uint32_t buf_end, int pieces = kPieces) {
    int32_t first;
    const int32_t n = needed(seq_nib, rel, st, en, qd, src, first);
    if (n <= 0) return true;
    const uint32_t f = (uint32_t)first;  // (n <= 64)
    const uint32_t lim = (uint32_t)(2 * kPieceBytes * pieces);
    if (f >= lim || f + (uint32_t)n > lim) return false;
    return piece_issued(src, (int)(((f + (uint32_t)n - 1u) >> 1) / kPieceBytes), buf_end);  // (the pieces below it begin lower)
}

// `covered` for a read of a one-op chunk: one run [0, len) at query delta 0 (len = 0: the op
// aligns no base) over the kOneOpPieces pieces issued.  With src = source_byte(seq_nib, rel) the
// first needed base is below nibble 32 of the slot and the last below nibble 96, so only the
// buffer's end is left to test: the piece that holds the last needed base was issued.
BC_SLICE_HD bool covered_one_op(uint32_t seq_nib, int32_t rel, uint32_t len, uint32_t src, uint32_t buf_end) {
    const int32_t nrel = (int32_t)(0u - (uint32_t)rel), trel = (int32_t)((uint32_t)kTile - (uint32_t)rel);
    const int32_t lo = nrel > 0 ? nrel : 0;
    const int32_t hi = trel < (int32_t)len ? trel : (int32_t)len;
    if (hi <= lo) return true;
    const uint32_t last = seq_nib + (uint32_t)hi - 1u - 2u * src;  // slot-relative nibble, < 96
    return (uint64_t)src + ((last >> 1) & ~(uint32_t)(kPieceBytes - 1)) < buf_end;
}

}  // namespace bc_slice
