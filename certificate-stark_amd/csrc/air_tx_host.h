// Host-side description of the composite TransactionAir that the engine would obtain through the Air trait:
// periodic (mask) columns, constraint degrees and degree adjustments.  Restates
//   periodic_columns()          /root/reference/src/air.rs:194-380
//     merkle masks              src/merkle/update/air.rs:182-212
//     schnorr masks             src/schnorr/air.rs:335-391
//     round constants           src/utils/rescue.rs:306-320
//   TransactionAir::new degrees src/air.rs:76-108
// It runs once per (depth, trace length); the resulting table is kernel input (K7).
#pragma once
#include "../../include/cstark_conventions.h"
#include <stdint.h>
#include <vector>
#include "air_groups.h" // AirShape / air_shape: the standalone sub-AIRs, host-only
#include "constants_gen.h"
#include "constraints.h"
#include "hostfield.h"

namespace cs {
namespace host {

constexpr int TX_NUM_PERIODIC = 48, TX_CYCLE = 1024;

// 48 columns x 1024 rows, column-major.  The length-8 columns of the reference (HASH_INPUT mask and the 28
// round-constant columns) are written out over the full 1024-row cycle: same periodic polynomial.
inline bool tx_periodic_columns(unsigned depth, std::vector<uint64_t> &out) {
    const unsigned hash_len = 8 * depth + 7; // TRANSACTION_HASH_LENGTH, src/merkle/constants.rs:27
    if (depth == 0 || hash_len > 511) return false;
    out.assign((size_t)TX_NUM_PERIODIC * TX_CYCLE, 0);
    auto col = [&](int c) { return out.data() + (size_t)c * TX_CYCLE; };
    const unsigned S = 512; // Schnorr half starts here (MERKLE_UPDATE_LENGTH)
    col(0)[0] = ONE;                                                     // SETUP
    for (unsigned i = 0; i < hash_len; i++) {
        col(1)[i] = ONE;                                                 // MERKLE (hashing in progress)
        col(4)[i] = (i % 8) != 7 ? ONE : 0;                              // HASH (round steps)
    }
    col(3)[hash_len - 1] = ONE;                                          // FINISH
    for (unsigned i = 0; i < TX_CYCLE; i++) col(2)[i] = (i % 8) == 7 ? ONE : 0; // HASH_INPUT (period 8)
    for (unsigned i = 0; i < 511; i++) col(5)[S + i] = ONE;              // SCHNORR global mask (SCALAR_MUL_LENGTH + 1)
    for (unsigned i = 0; i < 510; i++) {
        col(6)[S + i] = ONE;                                             // SCALAR_MULT
        col(7)[S + i] = (i % 2 == 0) ? ONE : 0;                          // DOUBLING
    }
    const unsigned lo[4] = {0, 126, 254, 382}, hi[4] = {126, 254, 382, 510};
    for (int k = 0; k < 4; k++)
        for (unsigned i = lo[k]; i < hi[k]; i++) col(8 + k)[S + i] = ONE; // h-limb selectors
    for (unsigned i = 0; i < 40; i++) col(12)[S + i] = (i % 8) != 7 ? ONE : 0; // SCHNORR_HASH
    for (int k = 0; k < 4; k++) col(13 + k)[S + 8 * (k + 1) - 1] = ONE;  // message-chunk insertion steps
    for (unsigned i = 0; i < 64; i++) col(17)[S + i] = ONE;              // RANGE_STEP
    col(18)[S + 63] = ONE;                                               // RANGE_FINISH
    for (unsigned i = 1; i < S + 64; i++) col(19)[i] = ONE;              // VALUE_COPY
    for (int j = 0; j < 28; j++)
        for (unsigned i = 0; i < TX_CYCLE; i++) col(20 + j)[i] = CS_ARK_MONT[(i % 8) * 28 + j];
    return true;
}

// evaluation degree of degree group g for trace length n (TransitionConstraintDegree [UPSTREAM-RECALL])
inline uint64_t tx_group_eval_degree(int g, uint64_t n) { return TX_GROUP_BASE[g] * (n - 1) + TX_GROUP_CYCLES[g] * (n / TX_CYCLE) * (TX_CYCLE - 1); }
// adjustment so that every merged constraint reaches degree (ce_size - 1) + (n - 1) before division
inline uint64_t tx_group_adjustment(int g, uint64_t n, uint64_t ce_size) { return CSTARK_CONV_TRANSITION_ADJUSTMENT(ce_size, n, tx_group_eval_degree(g, n)); }
inline uint64_t tx_boundary_adjustment(uint64_t n, uint64_t ce_size) { return CSTARK_CONV_BOUNDARY_ADJUSTMENT(ce_size, n, 1); }
static_assert(CSTARK_CONV_TRANSITION_EXEMPTIONS == 1, "the evaluators divide by (x^n - 1) / (x - w^(n-1)): one exempted step");

// ---- standalone sub-AIRs ------------------------------------------------------------
// MerkleAir periodic columns (src/merkle/update/air.rs:182-212): setup, hash, hash_input (period 8), finish,
// hash_mask, 28 round constants; 33 columns x 512 rows
inline bool merkle_periodic_columns(unsigned depth, std::vector<uint64_t> &out) {
    const unsigned hash_len = 8 * depth + 7;
    if (depth == 0 || hash_len > 511) return false;
    out.assign((size_t)33 * 512, 0);
    auto col = [&](int c) { return out.data() + (size_t)c * 512; };
    col(0)[0] = ONE;
    for (unsigned i = 0; i < hash_len; i++) { col(1)[i] = ONE; col(4)[i] = (i % 8) != 7 ? ONE : 0; }
    for (unsigned i = 0; i < 512; i++) col(2)[i] = (i % 8) == 7 ? ONE : 0;
    col(3)[hash_len - 1] = ONE;
    for (int j = 0; j < 28; j++)
        for (unsigned i = 0; i < 512; i++) col(5 + j)[i] = CS_ARK_MONT[(i % 8) * 28 + j];
    return true;
}

// SchnorrAir input-independent periodic columns (src/schnorr/air.rs:335-391): global mask, scalar-mult, doubling, four
// h-limb selectors, hash flag, then the 28 round constants; 36 columns x 512 rows
inline void schnorr_mask_columns(std::vector<uint64_t> &out) {
    out.assign((size_t)36 * 512, 0);
    auto col = [&](int c) { return out.data() + (size_t)c * 512; };
    for (unsigned i = 0; i < 511; i++) col(0)[i] = ONE;
    for (unsigned i = 0; i < 510; i++) { col(1)[i] = ONE; col(2)[i] = (i % 2 == 0) ? ONE : 0; }
    const unsigned lo[4] = {0, 126, 254, 382}, hi[4] = {126, 254, 382, 510};
    for (int k = 0; k < 4; k++)
        for (unsigned i = lo[k]; i < hi[k]; i++) col(3 + k)[i] = ONE;
    for (unsigned i = 0; i < 40; i++) col(7)[i] = (i % 8) != 7 ? ONE : 0;
    for (int j = 0; j < 28; j++)
        for (unsigned i = 0; i < 512; i++) col(8 + j)[i] = CS_ARK_MONT[(i % 8) * 28 + j];
}

// RescueAir periodic columns (benches/rescue.rs:133-142, :245-249): the cycle mask (seven ones, one zero), then the 28 round constants;
// 29 columns x 8 rows
inline void rescue_chain_periodic_columns(std::vector<uint64_t> &out) {
    out.assign((size_t)29 * 8, 0);
    for (unsigned i = 0; i < 7; i++) out[i] = ONE;
    for (int j = 0; j < 28; j++)
        for (unsigned i = 0; i < 8; i++) out[(size_t)(1 + j) * 8 + i] = CS_ARK_MONT[i * 28 + j];
}

} // namespace host
} // namespace cs
