// bc_inflate.hip — k_inflate: BGZF blocks inflated on the device, one wave per block.
//
// The decoder is bc_inflate.h's bcz_inflate (the same template the host check compiles) over the
// wave machine below.  Four waves per workgroup, each with its own LDS slice and no block barrier:
// a wave that finishes its block early just ends.  The symbol loop is wave-uniform (the bit
// buffer, table entries and positions are moved to scalars), so it is bound by the latency of one
// dependent LDS read per symbol; throughput comes from the resident waves: the LDS slice is
// 4.8 KiB, which leaves room for more than 16 waves per CU.
//   input    the block's bytes come into LDS 1 KiB at a time, one aligned 16-byte load per lane
//            (pieces that hold no byte of the block are not loaded and read as zero)
//   tables   built by all lanes (bcz_build: ballots for counts and ranks, every lane fills the
//            entries of its symbols)
//   literals collect in a 64-byte wave buffer (one byte per lane, in a register) and leave as one
//            coalesced store
//   matches  are copied by all lanes, 64 bytes a step, from the block's own earlier output in
//            global memory (read-back; DESIGN.md §3 says why not an LDS window)
#include "bc_internal.h"

#include "bc_inflate.h"

namespace bc {
namespace {

constexpr int kInfWaves = 4;
constexpr int kInfThreads = 64 * kInfWaves;
constexpr uint32_t kInWords = 256;  // the input piece in LDS: 64 lanes x 16 bytes

typedef uint32_t u32x4 __attribute__((ext_vector_type(4), may_alias));

struct __attribute__((aligned(16))) WaveLds {
    uint32_t in[kInWords];
    uint16_t lit_table[1 << BCZ_LIT_ROOT];
    uint16_t dist_table[1 << BCZ_DIST_ROOT];
    uint16_t lit_sorted[288];
    uint16_t dist_sorted[32];
    uint16_t lit_count[16];
    uint16_t dist_count[16];
    uint8_t lens[BCZ_MAXLENS];
    uint8_t stage[BCZ_MAXLENS];
};
static_assert(sizeof(WaveLds) <= 5 * 1024, "per-wave LDS must leave room for 16 waves per CU and more");

// the lanes of one wave see each other's LDS writes in program order (one wave's LDS instructions
// execute in order); the fence keeps the compiler from moving accesses across
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct BczWave {
    WaveLds* L;
    const uint8_t* src;   // the block's first compressed byte
    const uint8_t* base;  // src rounded down to 16 bytes: word 0 of the padded span
    uint32_t clen;
    uint8_t* out;  // the block's first output byte
    int ln;
    uint32_t hi;     // LDS holds the words [hi - kInWords, hi)
    uint32_t nbuf;   // literals buffered (lane i holds the i-th)
    uint32_t obase;  // output bytes stored so far
    uint32_t clean;  // output bytes whose stores are known complete (the last vmcnt(0))
    uint32_t lit;

    __device__ __forceinline__ int lane() const { return ln; }
    __device__ __forceinline__ int nlanes() const { return 64; }
    __device__ __forceinline__ uint64_t ballot(bool p) const { return __ballot(p); }
    __device__ __forceinline__ uint64_t lt_mask() const { return (1ull << ln) - 1ull; }
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ __forceinline__ void sync() { wave_sync(); }

    // words [h, h + kInWords) of the padded span into LDS: lane i takes the 16-byte piece i
    __device__ __forceinline__ void load(uint32_t h) {
        const uint8_t* g = base + (uint64_t)h * 4u + (uint32_t)ln * 16u;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (clen != 0 && g + 16 > src && g < src + clen) v = *reinterpret_cast<const u32x4*>(g);
        wave_sync();
        *reinterpret_cast<u32x4*>(&L->in[ln * 4]) = v;
        wave_sync();
        hi = h + kInWords;
    }
    __device__ __forceinline__ void seek(uint32_t w) { load(w & ~(kInWords - 1u)); }
    __device__ __forceinline__ uint32_t fetch32(uint32_t w) {
        if (w >= hi) load(hi);  // the reader moves forward word by word: w == hi here
        return uni(L->in[w & (kInWords - 1u)]);
    }

    __device__ __forceinline__ uint8_t* lens() { return L->lens; }
    __device__ __forceinline__ uint8_t* lens_stage() { return L->stage; }
    __device__ __forceinline__ uint16_t* lit_table() { return L->lit_table; }
    __device__ __forceinline__ uint16_t* dist_table() { return L->dist_table; }
    __device__ __forceinline__ uint16_t* lit_sorted() { return L->lit_sorted; }
    __device__ __forceinline__ uint16_t* dist_sorted() { return L->dist_sorted; }
    __device__ __forceinline__ uint16_t* lit_count() { return L->lit_count; }
    __device__ __forceinline__ uint16_t* dist_count() { return L->dist_count; }

    __device__ __forceinline__ void flush() {
        if ((uint32_t)ln < nbuf) out[obase + (uint32_t)ln] = (uint8_t)lit;
        obase += nbuf;
        nbuf = 0;
    }
    __device__ __forceinline__ void literal(uint32_t at, uint8_t v) {
        if ((uint32_t)ln == nbuf) lit = v;
        if (++nbuf == 64) {  // a full buffer: every lane stores, no lane mask
            out[obase + (uint32_t)ln] = (uint8_t)lit;
            obase += 64;
            nbuf = 0;
        }
    }
    // The sources are this wave's own earlier stores, read back from global memory.  Stores and
    // loads of one wave reach the CU's vector cache in program order and that cache is coherent
    // for one CU's own accesses, but a load may overtake a store that has not completed: where the
    // source range reaches into bytes stored since the last wait, the wave waits for its stores
    // (vmcnt(0)) first; the fence orders the compiler's view of the other lanes' stores.
    __device__ __forceinline__ void match(uint32_t at, uint32_t len, uint32_t dist) {
        flush();
        if (at - dist + (len < dist ? len : dist) > clean) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0); expcnt and lgkmcnt not waited for
            clean = at;
        }
        uint8_t v[5];  // len <= 258: at most five 64-byte steps, every source below `at`
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) {
            const uint32_t i = k * 64u + (uint32_t)ln;
            if (i < len) v[k] = out[bcz_match_src(at, dist, len, i)];
        }
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) {
            const uint32_t i = k * 64u + (uint32_t)ln;
            if (i < len) out[at + i] = v[k];
        }
        obase += len;
    }
    __device__ __forceinline__ void stored(uint32_t at, uint32_t from, uint32_t len) {
        for (uint32_t i = (uint32_t)ln; i < len; i += 64u) out[at + i] = src[from + i];
        obase += len;
    }
};

__global__ __launch_bounds__(kInfThreads) void k_inflate(const uint8_t* comp, uint64_t comp_bytes,
                                                         const bc_zblock* blocks, int64_t n, uint8_t* out,
                                                         uint64_t out_bytes, uint8_t* status) {
    __shared__ WaveLds lds[kInfWaves];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int ln = (int)(threadIdx.x & 63u);
    const int64_t blk = (int64_t)blockIdx.x * kInfWaves + wave;
    if (blk >= n) return;
    const bc_zblock zb = blocks[blk];
    int st = BC_Z_DESC;
    if (bcz_desc_ok(zb.coff, zb.clen, zb.isize, zb.uoff, comp_bytes, out_bytes)) {
        BczWave m;
        m.L = &lds[wave];
        m.src = comp + zb.coff;
        const uint32_t head = (uint32_t)((uintptr_t)m.src & 15u);
        m.base = m.src - head;
        m.clen = zb.clen;
        m.out = out + zb.uoff;
        m.ln = ln;
        m.hi = 0;
        m.nbuf = 0;
        m.obase = 0;
        m.clean = 0;
        m.lit = 0;
        st = bcz_inflate(m, head, zb.clen, zb.isize);
    }
    if (ln == 0) status[blk] = (uint8_t)st;
}

}  // namespace

hipError_t launch_inflate(hipStream_t s, const uint8_t* comp, uint64_t comp_bytes, const bc_zblock* blocks, int64_t n,
                          uint8_t* out, uint64_t out_bytes, uint8_t* status) {
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n + kInfWaves - 1) / kInfWaves)), block(kInfThreads);
    hipLaunchKernelGGL(k_inflate, grid, block, 0, s, comp, comp_bytes, blocks, n, out, out_bytes, status);
    return hipGetLastError();
}

}  // namespace bc
