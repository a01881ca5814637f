// bc_ops_plan.h — k_ops' launch plan from a batch's header (host only, pure): the consecutive
// reads one workgroup takes and the window passes it may run.  Shared by launch_ops (bc_ops.hip)
// and bc_ops_plan (bc_capi.hip); reads n_reads, sorted, max_span, max_end and seq_bytes, never a
// pointer.
#pragma once
#include <cstdint>

#include "basecount_hip.h"

namespace bc {

constexpr int kOpsWin = 4096;         // positions per LDS window (= kWinMax)
constexpr int kOpsPassesCap = BC_OPS_PASSES_MAX;  // what lies beyond is the global far path
constexpr int kOpsMaxReadsPerBlock = 32768;       // a 16-bit half counts one block's reads

// The typical read's reference length: twice the sequence bytes per read, at most max_span
inline double ops_typical_len(const bc_reads& r) {
    double len = r.n_reads > 0 ? 2.0 * (double)r.seq_bytes / (double)r.n_reads : 0.0;
    if (r.max_span > 0 && len > (double)r.max_span) len = (double)r.max_span;
    return len;
}

// The single-window rule: enough blocks to fill the device several times over; for a sorted batch
// few enough that the block's reads start within the window with room for a typical read (clamped
// to half a window), so that most events meet in LDS.
inline int ops_reads_per_block(const bc_reads& r, int64_t L, int forced) {
    if (forced > 0) return forced < kOpsMaxReadsPerBlock ? forced : kOpsMaxReadsPerBlock;
    const int64_t n = r.n_reads;
    int64_t target = n / 2048;
    target = target < 32 ? 32 : (target > 8192 ? 8192 : target);
    if (!r.sorted || L <= 0) return (int)target;
    const int64_t reach = r.max_end > L ? r.max_end : L;
    const double density = (double)n / (double)reach;
    double len = ops_typical_len(r);
    if (len > kOpsWin / 2) len = kOpsWin / 2;
    const double fit = ((double)kOpsWin - len) * density * 0.75;
    if (fit < (double)target) target = fit < 16.0 ? 16 : (int64_t)fit;
    return (int)target;
}

// forced_rpb: 0 = from the batch, else 1..32768.  forced_passes: 0 = from the batch, 1 = the
// single window with its own reads per block, 2..kOpsPassesCap = that many passes at most.
inline void ops_plan(const bc_reads& r, int64_t L, int forced_rpb, int forced_passes, struct bc_ops_plan& p) {
    p.reserved = 0;
    p.window = r.sorted ? kOpsWin : 0;
    p.passes_max = 1;
    p.reads_per_block = ops_reads_per_block(r, L, forced_rpb);
    const bool longer = r.sorted && L > 0 && r.n_reads > 0 && ops_typical_len(r) > kOpsWin / 2;
    if (r.sorted && forced_passes != 1 && (longer || forced_passes > 1)) {
        const int64_t reach = r.max_end > L ? r.max_end : L;
        const double density = (double)(r.n_reads > 0 ? r.n_reads : 1) / (double)(reach > 0 ? reach : 1);
        if (longer && forced_rpb <= 0) {
            // Reads longer than half a window: the reads that start within one window (at least
            // one per wave, at most the device-filling target).  Measured: more reads per block
            // leave too few blocks and too many passes each, fewer only cost blocks.
            int64_t target = r.n_reads / 2048;
            target = target < 32 ? 32 : (target > 8192 ? 8192 : target);
            const double starts = (double)kOpsWin * density;
            p.reads_per_block = starts < 4.0 ? 4 : (starts < (double)target ? (int)starts : (int)target);
        }
        // The block's reads start over reads_per_block / density positions and reach max_span
        // further (when the batch gives one): as many passes as that takes.  The kernel ends
        // earlier when no read of the block reaches on.
        int passes = kOpsPassesCap;
        if (r.max_span > 0) {
            const double need = ((double)p.reads_per_block / density + (double)r.max_span) / (double)kOpsWin + 1.0;
            passes = need < (double)kOpsPassesCap ? (int)need : kOpsPassesCap;
        }
        if (forced_passes > 1) passes = forced_passes < kOpsPassesCap ? forced_passes : kOpsPassesCap;
        p.passes_max = passes < 2 ? 2 : passes;
    }
    p.blocks = r.n_reads > 0 ? (r.n_reads + p.reads_per_block - 1) / p.reads_per_block : 0;
}

}  // namespace bc
