// The resident transaction witness: one device allocation of eleven 256-byte-aligned segments, 8-byte fields first.  Stated once for
// cstark_tx_witness_upload (capi.hip), cstark_ledger_apply (ledger.hip) and the host planner (ledger_plan.h).  Host only, no HIP.
#pragma once
#include <stddef.h>

namespace cs {

enum WitnessSegment {
    WIT_INITIAL_ROOTS = 0, WIT_S_OLD, WIT_R_OLD, WIT_S_IDX, WIT_R_IDX, WIT_S_PATHS, WIT_R_PATHS, WIT_DELTAS, WIT_SIG_RX, WIT_H_LIMBS, WIT_SIG_S,
    WIT_NUM_SEGMENTS
};

// sz[i]: bytes of segment i for n transfers on a tree of depth d; off[i]: its byte offset; off[WIT_NUM_SEGMENTS]: the whole allocation
inline void witness_segments(size_t n, size_t d, size_t sz[WIT_NUM_SEGMENTS], size_t off[WIT_NUM_SEGMENTS + 1]) {
    const size_t s[WIT_NUM_SEGMENTS] = {n * 7 * 8, n * 14 * 8, n * 14 * 8, n * 8, n * 8, n * (d + 1) * 7 * 8, n * (d + 1) * 7 * 8, n * 8, n * 6 * 8, n * 4 * 8, n * 32};
    off[0] = 0;
    for (int i = 0; i < WIT_NUM_SEGMENTS; i++) {
        sz[i] = s[i];
        off[i + 1] = off[i] + ((s[i] + 255) & ~(size_t)255);
    }
}

} // namespace cs
