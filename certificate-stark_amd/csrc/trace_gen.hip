// K1 -- execution-trace generation for the state-transition AIR on gfx950.
//
// Replaces TransactionProver::build_trace (/root/reference/src/prover.rs:37-98): the reference fills
// one 1024-row fragment per transaction with a sequential init/update loop (src/trace.rs:28-142).
// Here the 94 registers are split by the chain that produces them, because each chain is an
// independent, latency-bound recurrence:
//   k_trace_merkle        regs 0..64, rows 0..511 (+ root copy rows 512..1023): four Rescue states,
//                         one lane per state element      (src/merkle/update/trace.rs:19-136)
//   k_trace_schnorr_hash  regs 42..55, rows 512..1023: the 5-permutation message hash, also yields h
//                         (src/schnorr/trace.rs:47-67, src/schnorr/mod.rs:247-288)
//   k_trace_schnorr_ec    regs 0..17 and 19..36, rows 512..1023: the two double-and-add ladders,
//                         one lane per F_p6 product       (src/schnorr/trace.rs:69-121, src/utils/ecc.rs)
//   k_trace_aux           every register that is a closed form of the witness (bit registers, limb and
//                         range accumulators, key/delta/sigma/nonce copies; src/trace.rs:43-53,
//                         src/range/prover.rs:65-84, src/utils/field.rs:16-22)
// Rows are staged in LDS 64 at a time and written column-wise, so every global store is a
// contiguous 512-byte line of one column (the trace is column-major, 94 x N).
#include <stdlib.h>
#include "trace_gen.h"
#include "rescue_lane.cuh"
#include "tower.cuh"

namespace cs {

namespace {

constexpr int TXC = 1024;       // TRANSACTION_CYCLE_LENGTH, src/constants.rs:83
constexpr int MERKLE_LEN = 512; // src/merkle/constants.rs:29
constexpr unsigned LADDER_LDS_PAD = 0;
#ifndef CS_RECUR_TILE_ROWS
#define CS_RECUR_TILE_ROWS 16 // staging rows of the Merkle / message-hash recurrences in the overlapped path
#endif
#ifndef CS_RECUR_PRIO
#define CS_RECUR_PRIO 3 // wave priority of the latency-bound recurrences (0..3)
#endif
constexpr int SCALAR_MUL_LEN = 510; // src/schnorr/constants.rs:30

template <int NCOLS, int LD>
__device__ __forceinline__ void flush_tile(const fp (*tile)[LD], fp *__restrict__ trace, size_t n, size_t row0, int c0, int lane,
                                           int skip_at = -1) {
    // tile column c -> trace column c0 + c (+1 past skip_at); lane = row within the 64-row tile
    for (int c = 0; c < NCOLS; c++) {
        int tc = c0 + c + ((skip_at >= 0 && c >= skip_at) ? 1 : 0);
        trace[(size_t)tc * n + row0 + lane] = tile[lane][c];
    }
}

// TR-row staging tile (TR | 64): lane = (row, column group); one wave
template <int NCOLS, int LD, int TR>
__device__ __forceinline__ void flush_rows(const fp (*tile)[LD], fp *__restrict__ trace, size_t n, size_t row0, int c0, int lane) {
    for (int c = lane / TR; c < NCOLS; c += 64 / TR) trace[(size_t)(c0 + c) * n + row0 + (lane & (TR - 1))] = tile[lane & (TR - 1)][c];
}

// ---------------------------------------------------------------------------------------------------
// STANDALONE: the 65-register, 512-rows-per-transaction trace of MerkleProver (src/merkle/update/prover.rs:28-80)
// TR = rows of the staging tile: 64 alone; 16 when the recurrence runs beside the transforms (prove.hip), whose workgroups need the
// LDS (a 64-row tile is 33 KB: four resident recurrences per CU leave no room for a 75 KB transform workgroup)
template <bool STANDALONE, int TR>
__global__ __launch_bounds__(64) void k_trace_merkle(TxWitnessDev w, fp *__restrict__ trace, size_t n) {
    __builtin_amdgcn_s_setprio(CS_RECUR_PRIO); // latency-bound recurrence: issue ahead of the chip-filling kernels it runs beside
    __shared__ fp tile[TR][65];
    __shared__ fp st[4][14];
    const int t = blockIdx.x, lane = threadIdx.x;
    const int hash_len = 8 * (int)w.depth + 7; // TRANSACTION_HASH_LENGTH
    const bool is_state = lane < 56;
    const int s = is_state ? lane / 14 : 0, e = is_state ? lane % 14 : 0;
    // lanes 0..55: state elements; lane 56: both index-bit registers; lanes 57..63: previous-root registers 58..64
    const int col = is_state ? (s == 0 ? 0 : s == 1 ? 15 : s == 2 ? 29 : 44) + e : (lane == 56 ? 14 : lane + 1);
    fp mrow[14];
#pragma unroll
    for (int j = 0; j < 14; j++) mrow[j] = c_mds[e * 14 + j];

    const fp *sv = w.s_old + 14 * (size_t)t, *rv = w.r_old + 14 * (size_t)t;
    const fp delta = w.deltas[t];
    const uint64_t s_index = w.s_idx[t], r_index = w.r_idx[t];
    const fp *s_branch = w.s_paths + (size_t)7 * (w.depth + 1) * t, *r_branch = w.r_paths + (size_t)7 * (w.depth + 1) * t;

    // row 0: init_merkle_update_state, src/merkle/update/trace.rs:19-48
    fp v = 0, v2 = 0;
    if (is_state) {
        v = (s < 2 ? sv : rv)[e];
        if (s == 1 && e == 12) v = fp_sub(v, delta);
        if (s == 1 && e == 13) v = fp_add(v, FP_ONE);
        if (s == 3 && e == 12) v = fp_add(v, delta);
    } else if (lane >= 57) {
        v = w.initial_roots[7 * (size_t)t + lane - 57];
    }
    tile[0][col] = v;
    if (lane == 56) tile[0][43] = 0;

    const size_t gbase = (size_t)t * (STANDALONE ? MERKLE_LEN : TXC);
    for (int step = 0; step < MERKLE_LEN - 1; step++) {
        if (step < hash_len) {
            const int cyc = step & 7, lvl = step >> 3;
            if (cyc < 7) {
                v = rescue_round_lane(v, st[s], mrow, e, cyc, is_state);
            } else {
                // sibling insertion, src/merkle/update/trace.rs:112-135
                if (is_state) st[s][e] = v;
                __syncthreads();
                if (is_state) {
                    const fp *node = (s < 2 ? s_branch : r_branch) + 7 * (lvl + 1);
                    const int bit = (int)(((s < 2 ? s_index : r_index) >> lvl) & 1);
                    if (!bit) { if (e >= 7) v = node[e - 7]; }
                    else v = e >= 7 ? st[s][e - 7] : node[e];
                } else if (lane == 56) {
                    v = ((s_index >> lvl) & 1) ? FP_ONE : 0;
                    v2 = ((r_index >> lvl) & 1) ? FP_ONE : 0;
                }
                __syncthreads();
            }
            if (step == hash_len - 1) { // root copy, src/merkle/update/trace.rs:87-93
                if (is_state) st[s][e] = v;
                __syncthreads();
                if (lane >= 57) v = st[3][lane - 57];
                __syncthreads();
            }
        }
        const int r = (step + 1) & (TR - 1);
        tile[r][col] = v;
        if (lane == 56) tile[r][43] = v2;
        if (r == TR - 1) {
            __syncthreads();
            flush_rows<65, 65, TR>(tile, trace, n, gbase + (step + 1 - (TR - 1)), 0, lane);
            __syncthreads();
        }
    }
    if (STANDALONE) {
        // index-bit poke at global row 1 (src/merkle/update/prover.rs:72-77); after this workgroup's own flushes
        if (t == 0 && lane == 0) { trace[(size_t)14 * n + 1] = FP_ONE; trace[(size_t)43 * n + 1] = FP_ONE; }
        return;
    }
    // registers 58..64 keep the new root through the Schnorr half (rows 512..1023)
    if (lane >= 57) st[0][lane - 57] = v;
    __syncthreads();
    for (int k = 0; k < 8; k++)
        for (int c = 58; c < 65; c++) trace[(size_t)c * n + gbase + MERKLE_LEN + 64 * k + lane] = st[0][c - 58];
}

// ---------------------------------------------------------------------------------------------------
template <bool STANDALONE, int TR>
__global__ __launch_bounds__(64) void k_trace_schnorr_hash(TxWitnessDev w, fp *__restrict__ trace, size_t n) {
    __builtin_amdgcn_s_setprio(CS_RECUR_PRIO); // latency-bound recurrence: issue ahead of the chip-filling kernels it runs beside
    __shared__ fp tile[TR][15];
    __shared__ fp st[14];
    const int t = blockIdx.x, lane = threadIdx.x;
    const bool active = lane < 14;
    const int e = active ? lane : 0;
    fp mrow[14];
#pragma unroll
    for (int j = 0; j < 14; j++) mrow[j] = c_mds[e * 14 + j];
    const fp *sv = w.s_old + 14 * (size_t)t, *rv = w.r_old + 14 * (size_t)t;

    // row 512: init_sig_verification_state, src/schnorr/trace.rs:18-30
    fp v = (active && e < 6) ? w.sig_rx[6 * (size_t)t + e] : 0;
    if (active) tile[0][e] = v;
    const size_t gbase = STANDALONE ? (size_t)t * MERKLE_LEN : (size_t)t * TXC + MERKLE_LEN;
    for (int step = 0; step < MERKLE_LEN - 1; step++) {
        if (step < 40) { // TOTAL_HASH_LENGTH
            const int cyc = step & 7;
            if (cyc < 7) {
                v = rescue_round_lane(v, st, mrow, e, cyc, active);
            } else if (step < 32) { // message chunk, src/lib.rs:467-481 layout
                if (active && e >= 7) {
                    int m = 7 * (step >> 3) + e - 7;
                    v = m < 12 ? sv[m] : m < 24 ? rv[m - 12] : m == 24 ? w.deltas[t] : m == 25 ? sv[13] : (STANDALONE ? w.msg_tail[2 * (size_t)t + m - 26] : 0);
                }
            } else {
                if (active && e >= 7) v = 0;
            }
            if (step == 38 && active && e < 4) w.h_limbs[4 * (size_t)t + e] = fp_to_u64(v); // build_sig_info h_bytes
        }
        const int r = (step + 1) & (TR - 1);
        if (active) tile[r][e] = v;
        if (r == TR - 1) {
            __syncthreads();
            flush_rows<14, 15, TR>(tile, trace, n, gbase + (step + 1 - (TR - 1)), 42, lane);
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Curve ladders.  A point operation is a short program of F_p6 products whose operands are small
// integer combinations of LDS-resident F_p6 "slots"; each product is done by six lanes.
struct Term { int8_t slot, coef; };
struct Instr { int8_t out; Term a[4]; Term b; }; // out < 0: no-op; product: a[0] * b; linear: a[0] + a[1] + a[2] + a[3]

// slots 6..26 are scratch of the programs; QX..QZ: the second point of the complete addition (k_trace_schnorr_final);
// SW, SK, SK2: the ladders' fourth coordinate W = b3*Z and the per-ladder constants b3*qx, b3*qy
enum { SX = 0, SY = 1, SZ = 2, SB3 = 3, SPX = 4, SPY = 5, QX = 27, QY = 28, QZ = 29, SW = 30, SK = 31, SK2 = 32, NSLOT = 33 };
enum { OP_DOUBLE = 0, OP_ADD_MIXED = 1 };
enum { LPHASE = 4, LROLE = 10 }; // the two ladder programs: product, linear, product, linear; up to ten products per phase
enum { FPHASE = 6, FROLE = 6 };  // the complete addition of the final row: three product phases of up to six products
#define NOP {-1, {{0, 0}, {0, 0}, {0, 0}, {0, 0}}, {0, 0}}
#define P(out, sa, ca, sb, cb) {out, {{sa, ca}, {0, 0}, {0, 0}, {0, 0}}, {sb, cb}}
#define L2(out, s, c, s2, c2) {out, {{s, c}, {s2, c2}, {0, 0}, {0, 0}}, {0, 0}}
#define L3(out, s, c, s2, c2, s3, c3) {out, {{s, c}, {s2, c2}, {s3, c3}, {0, 0}}, {0, 0}}
#define L4(out, s, c, s2, c2, s3, c3, s4, c4) {out, {{s, c}, {s2, c2}, {s3, c3}, {s4, c4}}, {0, 0}}
// Product phases take single-slot operands (optionally doubled); every other operand is materialised by a preceding linear
// phase, so that no lane recomputes a combination another lane also needs.  A phase costs the same whether 6 or 60 lanes work
// in it, so the ladder programs carry W = b3*Z as a fourth coordinate: every product by the constant b3 of the reference's
// formulas (b3*Z^2, b3*2XZ; b3*(qx*Z + X), and b3*Z' for the next W) becomes a product by W, or by K = b3*qx, K2 = b3*qy,
// beside the others, and an operation is two product phases instead of three.  The values are the reference's by
// distributivity (the arithmetic is exact and every slot holds a reduced element).  Multiples are written as repeated unit
// terms or doubled operands: a linear phase whose coefficients are all 0, +1, -1 has no multiplication (lincomb2).
// (the tables exist twice: in constant memory for the kernels, and as constexpr twins from which the linear phases take their
// compile-time shape -- how many terms a phase uses and which of them only carry coefficients 0, +1, -1)
#define CS_LADDER_PROG { \
    /* OP_DOUBLE (complete doubling, ecc.rs:177-242): 6..14 = X^2 Y^2 Z^2 XY 2XZ YZ WZ 2XW YW; */ \
    /* a = Y^2-2XZ-WZ, b = Y^2+2XZ+WZ, c = X^2-Z^2+2XW, d = 3X^2+Z^2; */ \
    /* X' = 2XY a - 2YZ c, Y' = ab + dc, Z' = 2 (2YZ)(2Y^2), W' = 2 (2YW)(2Y^2) */ \
    {{P(6, 0, 1, 0, 1), P(7, 1, 1, 1, 1), P(8, 2, 1, 2, 1), P(9, 0, 1, 1, 1), P(10, 0, 2, 2, 1), P(11, 1, 1, 2, 1), P(12, SW, 1, 2, 1), \
      P(13, 0, 2, SW, 1), P(14, 1, 1, SW, 1), NOP}, \
     {L3(19, 7, 1, 10, -1, 12, -1), L3(20, 7, 1, 10, 1, 12, 1), L3(21, 6, 1, 8, -1, 13, 1), L4(22, 6, 1, 6, 1, 6, 1, 8, 1), NOP, NOP, NOP, NOP, NOP, NOP}, \
     {P(15, 19, 1, 20, 1), P(16, 9, 2, 19, 1), P(17, 22, 1, 21, 1), P(18, 11, 2, 21, 1), P(23, 11, 2, 7, 2), P(24, 14, 2, 7, 2), NOP, NOP, NOP, NOP}, \
     {L2(0, 16, 1, 18, -1), L2(1, 15, 1, 17, 1), L2(2, 23, 1, 23, 1), L2(SW, 24, 1, 24, 1), NOP, NOP, NOP, NOP, NOP, NOP}}, \
    /* OP_ADD_MIXED with the affine point (qx, qy) in slots 4, 5 (complete mixed addition, ecc.rs:330-404): */ \
    /* 6..15 = t0 = X qx, t1 = Y qy, (qx+qy)(X+Y), qx Z, qy Z, K Z, b3 X, K2 Z, b3 Y, K X; */ \
    /* 19 x3 = t1-W-qxZ-X, 20 z3 = t1+W+qxZ+X, 21 t1' = 3t0+Z, 22 t4' = KZ+b3X+t0-Z, 23 t5 = qyZ+Y, 24 t3, 16 u = b3 t5, 17 v = b3 t1'; */ \
    /* X' = t3 x3 - t5 t4', Y' = x3 z3 + t1' t4', Z' = t5 z3 + t3 t1', W' = u z3 + t3 v */ \
    {{P(6, 0, 1, 4, 1), P(7, 1, 1, 5, 1), P(8, 26, 1, 25, 1), P(9, 4, 1, 2, 1), P(10, 5, 1, 2, 1), P(11, SK, 1, 2, 1), P(12, 3, 1, 0, 1), \
      P(13, SK2, 1, 2, 1), P(14, 3, 1, 1, 1), P(15, SK, 1, 0, 1)}, \
     {L4(19, 7, 1, SW, -1, 9, -1, 0, -1), L4(20, 7, 1, SW, 1, 9, 1, 0, 1), L4(21, 6, 1, 6, 1, 6, 1, 2, 1), L4(22, 11, 1, 12, 1, 6, 1, 2, -1), \
      L2(23, 10, 1, 1, 1), L3(24, 8, 1, 6, -1, 7, -1), L2(16, 13, 1, 14, 1), L4(17, 15, 1, 15, 1, 15, 1, SW, 1), NOP, NOP}, \
     {P(6, 19, 1, 20, 1), P(7, 21, 1, 22, 1), P(8, 23, 1, 22, 1), P(9, 24, 1, 19, 1), P(10, 24, 1, 21, 1), P(11, 23, 1, 20, 1), P(12, 16, 1, 20, 1), \
      P(13, 24, 1, 17, 1), NOP, NOP}, \
     {L2(0, 9, 1, 8, -1), L2(1, 6, 1, 7, 1), L2(2, 11, 1, 10, 1), L2(SW, 12, 1, 13, 1), NOP, NOP, NOP, NOP, NOP, NOP}}, \
}
// operand sum that feeds the first product phase of the mixed addition (a "phase -1" run before the program): 25 = X + Y
// (26 = qx + qy is constant per ladder and set once)
#define CS_LADDER_PRE {L2(25, 0, 1, 1, 1)}
// The complete addition with the projective point in slots 27..29 (ecc.rs:244-328), one per transaction in k_trace_schnorr_final:
// X3 = ..., with the two products by b3 in a phase of their own.  "Phase -1": 20..25 = X1+Y1, X2+Y2, X1+Z1, X2+Z2, Y1+Z1, Y2+Z2
#define CS_FULL_PROG { \
    {P(6, 0, 1, 27, 1), P(7, 1, 1, 28, 1), P(8, 2, 1, 29, 1), P(9, 20, 1, 21, 1), P(10, 22, 1, 23, 1), P(11, 24, 1, 25, 1)}, \
    {L3(19, 10, 1, 6, -1, 8, -1), NOP, NOP, NOP, NOP, NOP}, \
    {P(12, 3, 1, 8, 1), P(13, 3, 1, 19, 1), NOP, NOP, NOP, NOP}, \
    {L3(20, 7, 1, 12, -1, 19, -1), L3(21, 7, 1, 12, 1, 19, 1), L2(22, 6, 3, 8, 1), L3(23, 13, 1, 6, 1, 8, -1), L3(24, 9, 1, 6, -1, 7, -1), \
     L3(25, 11, 1, 7, -1, 8, -1)}, \
    {P(14, 20, 1, 21, 1), P(15, 22, 1, 23, 1), P(16, 25, 1, 23, 1), P(17, 24, 1, 20, 1), P(18, 24, 1, 22, 1), P(26, 25, 1, 21, 1)}, \
    {L2(0, 17, 1, 16, -1), L2(1, 14, 1, 15, 1), L2(2, 26, 1, 18, 1), NOP, NOP, NOP}, \
}
#define CS_FULL_PRE {L2(20, 0, 1, 1, 1), L2(21, 27, 1, 28, 1), L2(22, 0, 1, 2, 1), L2(23, 27, 1, 29, 1), L2(24, 1, 1, 2, 1), L2(25, 28, 1, 29, 1)}
__constant__ Instr c_lprog[2][LPHASE][LROLE] = CS_LADDER_PROG;
__constant__ Instr c_lpre[1] = CS_LADDER_PRE;
__constant__ Instr c_fprog[FPHASE][FROLE] = CS_FULL_PROG;
__constant__ Instr c_fpre[FROLE] = CS_FULL_PRE;
constexpr Instr k_lprog[2][LPHASE][LROLE] = CS_LADDER_PROG;
constexpr Instr k_lpre[1] = CS_LADDER_PRE;
constexpr Instr k_fprog[FPHASE][FROLE] = CS_FULL_PROG;
constexpr Instr k_fpre[FROLE] = CS_FULL_PRE;
#undef CS_LADDER_PROG
#undef CS_LADDER_PRE
#undef CS_FULL_PROG
#undef CS_FULL_PRE
#undef NOP
#undef P
#undef L2
#undef L3
#undef L4
// shape of a linear phase: (number of leading terms any instruction uses) | (bit 4 + k set: term k only has coefficients 0, 1, -1)
template <int NR>
constexpr int lin_shape(const Instr (&ph)[NR]) {
    int nt = 0, unit = 15;
    for (int m = 0; m < NR; m++) {
        if (ph[m].out < 0) continue;
        for (int k = 0; k < 4; k++) {
            const int c = ph[m].a[k].coef;
            if (c != 0 && k + 1 > nt) nt = k + 1;
            if (c < -1 || c > 1) unit &= ~(1 << k);
        }
    }
    return nt | (unit << 4);
}
constexpr bool lin_shape_unit(int shape) { return (shape >> 4) == 15; }

// The programs live in LDS while a kernel runs: every lane fetches its own instruction each phase, and a divergent read
// of __constant__ memory is a vector load with global-memory latency.  A ladder holds its two programs only (0.9 KB: eight
// ladders share a CU's LDS with the transform workgroups), the final row's kernel the complete addition.
// small[c + 4] = the field element c for |c| <= 4: integer coefficients other than 0, +1, -1 are applied as one multiplication,
// the same code for every lane (a switch over the coefficient would run all of its cases serially in a wave whose lanes hold
// different instructions).  Only the complete addition has such a coefficient.
struct LadderLds { Instr prog[2][LPHASE][LROLE]; Instr pre[1]; };
struct FullLds { Instr prog[FPHASE][FROLE]; Instr pre[FROLE]; fp small[9]; };
__device__ __forceinline__ void copy_program(Instr *dst, const Instr *src, int count, int tid, int nthreads) {
    for (int i = tid; i < count; i += nthreads) dst[i] = src[i];
}
__device__ __forceinline__ void load_programs(LadderLds &p, int tid, int nthreads) {
    copy_program(&p.prog[0][0][0], &c_lprog[0][0][0], 2 * LPHASE * LROLE, tid, nthreads);
    copy_program(p.pre, c_lpre, 1, tid, nthreads);
}
__device__ __forceinline__ void load_programs(FullLds &p, int tid, int nthreads) {
    copy_program(&p.prog[0][0], &c_fprog[0][0], FPHASE * FROLE, tid, nthreads);
    copy_program(p.pre, c_fpre, FROLE, tid, nthreads);
    if (tid < 9) {
        const int c = tid - 4;
        const fp m = fp_mul((uint64_t)(c < 0 ? -c : c), FP_R2); // |c| in Montgomery form
        p.small[tid] = c < 0 ? fp_neg(m) : m;
    }
}

// F_p2 component `comp` (0..2) of an integer combination of slots.  SHAPE (lin_shape): only the terms the phase uses are walked, and a
// term whose coefficients are all 0 / +1 / -1 is a conditional negation instead of a product (a product by a small constant costs 52
// issue cycles per component, the negation and selects about 20); other coefficients are applied as one multiplication, the same
// code for every lane (`small` is not read by a phase whose terms are all of the first kind).
template <int SHAPE>
__device__ __forceinline__ Fp2 lincomb2(const fp (*slot)[6], const Term (&t)[4], int comp, const fp *small) {
    Fp2 r = {0, 0};
#pragma unroll
    for (int k = 0; k < (SHAPE & 15); k++) { // unused terms have coefficient 0 (and slot 0): they add 0
        const fp *s = slot[t[k].slot];
        const int cf = t[k].coef;
        fp va, vb;
        if ((SHAPE >> (4 + k)) & 1) {
            va = s[2 * comp]; vb = s[2 * comp + 1];
            if (cf < 0) { va = fp_neg(va); vb = fp_neg(vb); }
            if (cf == 0) { va = 0; vb = 0; }
        } else {
            const fp c = small[cf + 4];
            va = fp_mul(s[2 * comp], c); vb = fp_mul(s[2 * comp + 1], c);
        }
        r = fp2_add(r, {va, vb});
    }
    return r;
}

// single-slot product operand: component `comp` (+ comp2) of slot t.slot scaled by t.coef (1 or 2)
__device__ __forceinline__ Fp2 operand2(const fp (*slot)[6], const Term t, int comp, int comp2) {
    const fp *s = slot[t.slot];
    Fp2 v = {s[2 * comp], s[2 * comp + 1]};
    if (comp2 >= 0) v = fp2_add(v, {s[2 * comp2], s[2 * comp2 + 1]});
    if (t.coef == 2) v = fp2_dbl(v);
    return v;
}

// One phase of a program of NR instructions on the slots of one point, with the 64 lanes of one wave:
//   product phase  lane (m, q), q < 6: the q-th Karatsuba F_p2 product of instruction m  (3 base products per lane)
//   recombination  lane (m, r), r < 3: F_p2 coefficient r of the F_p6 result of instruction m
//   linear phase   lane (m, r): coefficient r of an integer combination of slots
// Called by all lanes of the workgroup (barriers inside).  prod = this point's [NR][6] F_p2 scratch.
template <int NR, int SHAPE>
__device__ __forceinline__ void run_linear_phase(const Instr *prog, const fp *small, fp (*slot)[6], int lane) {
    static_assert(3 * NR <= 64, "one lane per F_p2 coefficient");
    const int m = lane / 3, r = lane % 3;
    Fp2 c = {0, 0};
    int out = -1;
    if (m < NR) {
        const Instr ins = prog[m];
        out = ins.out;
        if (out >= 0) c = lincomb2<SHAPE>(slot, ins.a, r, small);
    }
    __syncthreads();
    if (out >= 0) { slot[out][2 * r] = c.a; slot[out][2 * r + 1] = c.b; }
    __syncthreads();
}

template <int NR>
__device__ __forceinline__ void run_product_phase(const Instr *prog, fp (*slot)[6], Fp2 (*prod)[6], int lane) {
    static_assert(6 * NR <= 64, "one lane per F_p2 product");
    const int m = lane / 6, q = lane % 6;
    if (m < NR) {
        const Instr ins = prog[m];
        if (ins.out >= 0) {
            const int c1 = q < 3 ? q : (q == 5 ? 1 : 0), c2 = q < 3 ? -1 : (q == 3 ? 1 : 2);
            prod[m][q] = fp2_mul(operand2(slot, ins.a[0], c1, c2), operand2(slot, ins.b, c1, c2));
        }
    }
    __syncthreads();
    const int m2 = lane / 3, r = lane % 3;
    if (m2 < NR) {
        const int out = prog[m2].out;
        if (out >= 0) {
            // r = 0: d0 + d1 + d2 - e12;  r = 1: e01 - e12 - d0;  r = 2: e02 + d1 - d0 - 2 d2.  One five-term form
            // t1 + t2 + t3 - t4 - t5 with the operands selected per lane: the three cases as branches would run one after
            // the other in the wave (nine F_p2 additions instead of six).
            const Fp2 zero = {0, 0};
            const Fp2 d0 = prod[m2][0], d1 = prod[m2][1], d2 = prod[m2][2];
            const Fp2 t1 = r == 0 ? d0 : prod[m2][r + 2];        // d0 | e01 | e02
            const Fp2 t2 = r == 1 ? zero : d1;
            const Fp2 t3 = r == 0 ? d2 : zero;
            const Fp2 t4 = r == 2 ? d0 : prod[m2][5];            // e12 | e12 | d0
            const Fp2 t5 = r == 0 ? zero : (r == 1 ? d0 : fp2_dbl(d2));
            const Fp2 c = fp2_sub(fp2_sub(fp2_add(fp2_add(t1, t2), t3), t4), t5);
            slot[out][2 * r] = c.a;
            slot[out][2 * r + 1] = c.b;
        }
    }
    __syncthreads();
}

// even phases of a program are product phases, odd ones linear
template <int OP, int PH = 0>
__device__ __forceinline__ void run_ladder_phases(const LadderLds &pg, fp (*slot)[6], Fp2 (*prod)[6], int lane) {
    if constexpr (PH < LPHASE) {
        if constexpr ((PH & 1) == 0) {
            run_product_phase<LROLE>(pg.prog[OP][PH], slot, prod, lane);
        } else {
            constexpr int shape = lin_shape(k_lprog[OP][PH]);
            static_assert(lin_shape_unit(shape), "the ladder programs carry no table of small multiples");
            run_linear_phase<LROLE, shape>(pg.prog[OP][PH], nullptr, slot, lane);
        }
        run_ladder_phases<OP, PH + 1>(pg, slot, prod, lane);
    }
}
template <int OP>
__device__ __forceinline__ void run_ladder_op(const LadderLds &pg, fp (*slot)[6], Fp2 (*prod)[6], int lane) {
    if constexpr (OP == OP_ADD_MIXED) {
        static_assert(lin_shape_unit(lin_shape(k_lpre)), "the ladder programs carry no table of small multiples");
        run_linear_phase<1, lin_shape(k_lpre)>(pg.pre, nullptr, slot, lane);
    }
    run_ladder_phases<OP>(pg, slot, prod, lane);
}
template <int PH = 0>
__device__ __forceinline__ void run_full_phases(const FullLds &pg, fp (*slot)[6], Fp2 (*prod)[6], int lane) {
    if constexpr (PH < FPHASE) {
        if constexpr ((PH & 1) == 0) run_product_phase<FROLE>(pg.prog[PH], slot, prod, lane);
        else run_linear_phase<FROLE, lin_shape(k_fprog[PH])>(pg.prog[PH], pg.small, slot, lane);
        run_full_phases<PH + 1>(pg, slot, prod, lane);
    }
}
__device__ __forceinline__ void run_full_add(const FullLds &pg, fp (*slot)[6], Fp2 (*prod)[6], int lane) {
    run_linear_phase<FROLE, lin_shape(k_fpre)>(pg.pre, pg.small, slot, lane);
    run_full_phases(pg, slot, prod, lane);
}

__device__ __forceinline__ int bit_le(const uint8_t *bytes, int i) { return (bytes[i >> 3] >> (i & 7)) & 1; }

// grid = 2 * n_tx workgroups of ONE wave: workgroup 2t is the ladder s*G of transaction t (registers 0..17), 2t+1 the ladder
// h*P (registers 19..36).  With a single wave per workgroup the phase barriers of run_ladder_op cost nothing and the two
// ladders of a transaction never wait for each other; 2 * n_tx independent waves keep every SIMD busy with two of them.
// The last step (S += h*P, X <- X/Z) needs both ladders: k_trace_schnorr_final, below.
// TR = rows of the staging tile (rows per flush).  64 is the fastest alone (3.99 ms of trace generation against 5.77 ms with 16);
// 16 leaves room in LDS for a transform workgroup beside the eight resident ladders of a CU and is the fastest when the
// ladders run beside the interpolation / extension of the other registers (prove.hip commit_columns: 43.1 vs 43.8 ms per proof).
template <bool STANDALONE, int TR>
__global__ __launch_bounds__(64) void k_trace_schnorr_ec(TxWitnessDev w, fp *__restrict__ trace, size_t n) {
    __builtin_amdgcn_s_setprio(CS_RECUR_PRIO); // latency-bound recurrence: issue ahead of the chip-filling kernels it runs beside
    constexpr int TG = 64 / TR; // column groups of a flush
    __shared__ fp tile[TR][19];
    __shared__ fp slots[NSLOT][6];
    __shared__ Fp2 prods[LROLE][6];
    __shared__ uint8_t sbytes[32];
    __shared__ LadderLds pg;
    const int t = blockIdx.x >> 1, g = blockIdx.x & 1, lane = threadIdx.x;
    fp(*slot)[6] = slots;
    load_programs(pg, lane, 64);

    // scalars: s from the signature, h from the message hash (little-endian bytes, Lsb0 bit order)
    if (lane < 32) sbytes[lane] = g == 0 ? w.sig_s[32 * (size_t)t + lane] : (uint8_t)(w.h_limbs[4 * (size_t)t + (lane >> 3)] >> (8 * (lane & 7)));
    // constant slots and the initial point (0 : 1 : 0), src/schnorr/trace.rs:22-27
    if (lane < 6) {
        slot[SX][lane] = 0;
        slot[SY][lane] = lane == 0 ? FP_ONE : 0;
        slot[SZ][lane] = 0;
        slot[SB3][lane] = c_b3[lane];
        slot[SPX][lane] = g == 0 ? c_generator[lane] : w.s_old[14 * (size_t)t + lane];
        slot[SPY][lane] = g == 0 ? c_generator[6 + lane] : w.s_old[14 * (size_t)t + 6 + lane];
        slot[26][lane] = fp_add(slot[SPX][lane], slot[SPY][lane]); // x2 + y2, operand of the mixed addition
        slot[SW][lane] = 0;                                        // W = b3 * Z
    }
    __syncthreads();
    // K = b3 * qx, K2 = b3 * qy: once per ladder
    if (lane < 2) fp6_store(slot[SK + lane], fp6_mul(fp6_load(slot[SB3]), fp6_load(slot[SPX + lane])));
    __syncthreads();
    if (lane < 18) tile[0][lane] = slot[lane / 6][lane % 6];
    const size_t gbase = STANDALONE ? (size_t)t * MERKLE_LEN : (size_t)t * TXC + MERKLE_LEN;

    for (int step = 0; step < MERKLE_LEN - 1; step++) {
        if (step < SCALAR_MUL_LEN) {
            if ((step & 1) == 0) {
                run_ladder_op<OP_DOUBLE>(pg, slot, prods, lane);
            } else {
                const int bit = bit_le(sbytes, 254 - (step >> 1)); // MSB first, src/schnorr/trace.rs:79-82
                if (bit) run_ladder_op<OP_ADD_MIXED>(pg, slot, prods, lane); // uniform over the wave
            }
        } // step == SCALAR_MUL_LEN: the row is a copy here; k_trace_schnorr_final rewrites registers 0..17 of it
        const int r = (step + 1) & (TR - 1);
        if (lane < 18) tile[r][lane] = slot[lane / 6][lane % 6];
        if (r == TR - 1) {
            __syncthreads();
            for (int c = lane / TR; c < 18; c += TG) trace[(size_t)(g * 19 + c) * n + gbase + (step + 1 - (TR - 1)) + (lane & (TR - 1))] = tile[lane & (TR - 1)][c];
            __syncthreads();
        }
    }
}
// S += h*P, then X <- X / Z  (src/schnorr/trace.rs:105-119): last row of the Schnorr block, registers 0..17.
// One wave per transaction; reads both ladders' results from the row before.
template <bool STANDALONE>
__global__ __launch_bounds__(64) void k_trace_schnorr_final(fp *__restrict__ trace, size_t n) {
    __shared__ fp slots[QZ + 1][6];
    __shared__ Fp2 prods[FROLE][6];
    __shared__ FullLds pg;
    const int t = blockIdx.x, lane = threadIdx.x;
    load_programs(pg, lane, 64);
    const size_t last = (STANDALONE ? (size_t)t * MERKLE_LEN : (size_t)t * TXC + MERKLE_LEN) + MERKLE_LEN - 1;
    if (lane < 18) {
        slots[lane / 6][lane % 6] = trace[(size_t)lane * n + last - 1];
        slots[QX + lane / 6][lane % 6] = trace[(size_t)(19 + lane) * n + last - 1];
    }
    if (lane < 6) slots[SB3][lane] = c_b3[lane];
    __syncthreads();
    run_full_add(pg, slots, prods, lane);
    if (lane == 0) fp6_store(slots[SX], fp6_mul(fp6_load(slots[SX]), fp6_inv(fp6_load(slots[SZ]))));
    __syncthreads();
    if (lane < 18) trace[(size_t)lane * n + last] = slots[lane / 6][lane % 6];
}

// ---------------------------------------------------------------------------------------------------
// Closed-form registers.  grid = (n_tx, 4), block = 256: one lane per row.
__device__ __forceinline__ fp small_to_fp(uint64_t x) { return fp_mul(x, FP_R2); } // x < p

// WHICH: 0 = every closed-form register; 1 = those that need the witness only; 2 = those that need the message hash h
// (register 37 and the h-limb accumulators 38..41), which k_trace_schnorr_hash leaves in w.h_limbs.
template <int WHICH>
__global__ __launch_bounds__(256) void k_trace_aux(TxWitnessDev w, fp *__restrict__ trace, size_t n) {
    constexpr bool PLAIN = WHICH != 2, WITH_H = WHICH != 1;
    const int t = blockIdx.x;
    const int r = blockIdx.y * 256 + threadIdx.x; // row inside the transaction
    const size_t g = (size_t)t * TXC + r;
    const fp *sv = w.s_old + 14 * (size_t)t, *rv = w.r_old + 14 * (size_t)t;
    const fp delta = w.deltas[t];
    const fp sigma = fp_sub(sv[12], delta);
    // copies: src/trace.rs:43-53 (constant over the whole transaction)
    if (PLAIN) {
        for (int i = 0; i < 12; i++) {
            trace[(size_t)(65 + i) * n + g] = sv[i];
            trace[(size_t)(77 + i) * n + g] = rv[i];
        }
        trace[(size_t)89 * n + g] = delta;
        trace[(size_t)90 * n + g] = sigma;
        trace[(size_t)91 * n + g] = sv[13];
    }
    if (r < MERKLE_LEN) {
        if (PLAIN) {
            trace[(size_t)92 * n + g] = 0;
            trace[(size_t)93 * n + g] = 0;
        }
        return;
    }
    const int q = r - MERKLE_LEN; // q = 0 is the Schnorr init row; row q is produced by step q-1
    const uint64_t dv = fp_to_u64(delta), sg = fp_to_u64(sigma);
    // range accumulators, src/range/prover.rs:65-84: after k = min(q,64) steps acc = value >> (64-k)
    if (PLAIN) {
        const int k = q < 64 ? q : 64;
        uint64_t dacc = k == 0 ? 0 : dv >> (64 - k), sacc = k == 0 ? 0 : sg >> (64 - k);
        trace[(size_t)56 * n + g] = (dacc & 1) ? FP_ONE : 0;
        trace[(size_t)57 * n + g] = small_to_fp(dacc);
        trace[(size_t)92 * n + g] = (sacc & 1) ? FP_ONE : 0;
        trace[(size_t)93 * n + g] = small_to_fp(sacc);
    }
    // scalar bit registers 18 / 37, src/schnorr/trace.rs:79-82 and :110
    const uint8_t *sb = w.sig_s + 32 * (size_t)t;
    const uint64_t *h = w.h_limbs + 4 * (size_t)t;
    fp bs = 0, bh = 0;
    if (q >= 1) {
        const int step = q - 1 < SCALAR_MUL_LEN - 1 ? q - 1 : SCALAR_MUL_LEN - 1;
        const int bi = 254 - (step >> 1);
        bs = bit_le(sb, bi) ? FP_ONE : 0;
        bh = ((h[bi >> 6] >> (bi & 63)) & 1) ? FP_ONE : 0;
        if (q == SCALAR_MUL_LEN + 1) bs = FP_ONE;
    }
    if (PLAIN) trace[(size_t)18 * n + g] = bs;
    if (!WITH_H) return;
    trace[(size_t)37 * n + g] = bh;
    // h-limb accumulators 38..41: k bits consumed MSB-first; chunk 0 = 63 bits into reg 41, then 64-bit chunks
    const int k = (q + 1) / 2 < 255 ? (q + 1) / 2 : 255;
    for (int c = 0; c < 4; c++) {
        const int width = c == 0 ? 63 : 64;
        const int start = c == 0 ? 0 : 63 + 64 * (c - 1);
        int kc = k - start;
        kc = kc < 0 ? 0 : kc > width ? width : kc;
        const uint64_t limb = h[3 - c];
        const uint64_t acc = kc == 0 ? 0 : (c == 0 ? (limb >> (63 - kc)) : (kc == 64 ? limb : limb >> (64 - kc)));
        trace[(size_t)(41 - c) * n + g] = small_to_fp(acc);
    }
}

} // namespace

// Unused dynamic LDS added to every ladder workgroup of the overlapped path (tuning: CSTARK_EC_LDS_PAD); measured best at 0.
static unsigned ladder_lds_pad() {
    static const unsigned pad = [] { const char *e = getenv("CSTARK_EC_LDS_PAD"); return e ? (unsigned)atoi(e) : LADDER_LDS_PAD; }();
    return pad;
}
hipError_t launch_trace_gen(const TxWitnessDev &w, fp *d_trace, hipStream_t stream, hipStream_t side, hipEvent_t fork, hipEvent_t join) {
    const size_t n = (size_t)w.n_tx * TXC;
    // the Merkle-phase recurrence is independent of the Schnorr half: run it beside the curve ladders (both are
    // latency-bound, one wave per transaction) on a side stream forked from / joined back into `stream`
    hipError_t e;
    if ((e = hipEventRecord(fork, stream)) != hipSuccess) return e;
    if ((e = hipStreamWaitEvent(side, fork, 0)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_trace_merkle<false, 64>), dim3(w.n_tx), dim3(64), 0, side, w, d_trace, n);
    if ((e = hipEventRecord(join, side)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_trace_schnorr_hash<false, 64>), dim3(w.n_tx), dim3(64), 0, stream, w, d_trace, n);
    hipLaunchKernelGGL((k_trace_schnorr_ec<false, 64>), dim3(2 * w.n_tx), dim3(64), 0, stream, w, d_trace, n);
    hipLaunchKernelGGL(k_trace_schnorr_final<false>, dim3(w.n_tx), dim3(64), 0, stream, d_trace, n);
    hipLaunchKernelGGL(k_trace_aux<0>, dim3(w.n_tx, 4), dim3(256), 0, stream, w, d_trace, n);
    if ((e = hipStreamWaitEvent(stream, join, 0)) != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t launch_trace_gen_split(const TxWitnessDev &w, fp *d_trace, hipStream_t stream, hipStream_t side_a, hipStream_t side_b, hipEvent_t fork,
                                  hipEvent_t join_a, hipEvent_t mid_b, hipEvent_t join_b) {
    const size_t n = (size_t)w.n_tx * TXC;
    hipError_t e;
    if ((e = hipEventRecord(fork, stream)) != hipSuccess) return e;
    // the closed-form registers first: the caller's stream transforms them next, and that chain of transforms is what a proof waits for
    // (launched after the recurrences it started ~45 us later)
    hipLaunchKernelGGL(k_trace_aux<1>, dim3(w.n_tx, 4), dim3(256), 0, stream, w, d_trace, n);
    if ((e = hipStreamWaitEvent(side_a, fork, 0)) != hipSuccess) return e;
    if ((e = hipStreamWaitEvent(side_b, fork, 0)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_trace_merkle<false, CS_RECUR_TILE_ROWS>), dim3(w.n_tx), dim3(64), 0, side_a, w, d_trace, n);
    if ((e = hipEventRecord(join_a, side_a)) != hipSuccess) return e;
    // the message hash produces the scalar h of the second ladder (w.h_limbs): the ladders run behind it
    hipLaunchKernelGGL((k_trace_schnorr_hash<false, CS_RECUR_TILE_ROWS>), dim3(w.n_tx), dim3(64), 0, side_b, w, d_trace, n);
    hipLaunchKernelGGL(k_trace_aux<2>, dim3(w.n_tx, 4), dim3(256), 0, side_b, w, d_trace, n);
    if ((e = hipEventRecord(mid_b, side_b)) != hipSuccess) return e;
    static const int ec_rows = [] { const char *e = getenv("CSTARK_EC_TILE_ROWS"); return e ? atoi(e) : 16; }(); // tuning: rows per flush of the ladders
    if (ec_rows == 64) hipLaunchKernelGGL((k_trace_schnorr_ec<false, 64>), dim3(2 * w.n_tx), dim3(64), ladder_lds_pad(), side_b, w, d_trace, n);
    else if (ec_rows == 32) hipLaunchKernelGGL((k_trace_schnorr_ec<false, 32>), dim3(2 * w.n_tx), dim3(64), ladder_lds_pad(), side_b, w, d_trace, n);
    else hipLaunchKernelGGL((k_trace_schnorr_ec<false, 16>), dim3(2 * w.n_tx), dim3(64), ladder_lds_pad(), side_b, w, d_trace, n);
    hipLaunchKernelGGL(k_trace_schnorr_final<false>, dim3(w.n_tx), dim3(64), 0, side_b, d_trace, n);
    if ((e = hipEventRecord(join_b, side_b)) != hipSuccess) return e;
    return hipGetLastError();
}

// standalone SchnorrAir: bit registers 18 / 37 and h-limb accumulators 38..41 (closed forms, as in k_trace_aux); grid (n, 2) x 256
__global__ __launch_bounds__(256) void k_trace_schnorr_bits(TxWitnessDev w, fp *__restrict__ trace, size_t n) {
    const int t = blockIdx.x;
    const int q = blockIdx.y * 256 + threadIdx.x; // row inside the signature block; row q is produced by step q-1
    const size_t g = (size_t)t * MERKLE_LEN + q;
    const uint8_t *sb = w.sig_s + 32 * (size_t)t;
    const uint64_t *h = w.h_limbs + 4 * (size_t)t;
    fp bs = 0, bh = 0;
    if (q >= 1) {
        const int step = q - 1 < SCALAR_MUL_LEN - 1 ? q - 1 : SCALAR_MUL_LEN - 1;
        const int bi = 254 - (step >> 1);
        bs = bit_le(sb, bi) ? FP_ONE : 0;
        bh = ((h[bi >> 6] >> (bi & 63)) & 1) ? FP_ONE : 0;
        if (q == SCALAR_MUL_LEN + 1) bs = FP_ONE;
    }
    trace[(size_t)18 * n + g] = bs;
    trace[(size_t)37 * n + g] = bh;
    const int k = (q + 1) / 2 < 255 ? (q + 1) / 2 : 255;
    for (int c = 0; c < 4; c++) {
        const int width = c == 0 ? 63 : 64, start = c == 0 ? 0 : 63 + 64 * (c - 1);
        int kc = k - start;
        kc = kc < 0 ? 0 : kc > width ? width : kc;
        const uint64_t limb = h[3 - c];
        const uint64_t acc = kc == 0 ? 0 : (c == 0 ? (limb >> (63 - kc)) : (kc == 64 ? limb : limb >> (64 - kc)));
        trace[(size_t)(41 - c) * n + g] = small_to_fp(acc);
    }
}
// (the same row rule, from the statement's messages and for one row: schnorr_aux_value in trace_check.hip -- keep the two in step)
__global__ __launch_bounds__(256) void k_schnorr_aux_columns(TxWitnessDev w, fp *__restrict__ out, size_t n) {
    const int t = blockIdx.x;
    const int q = blockIdx.y * 256 + threadIdx.x;
    const size_t g = (size_t)t * MERKLE_LEN + q;
    const fp *sv = w.s_old + 14 * (size_t)t, *rv = w.r_old + 14 * (size_t)t;
    for (int j = 0; j < 12; j++) out[(size_t)j * n + g] = sv[j];
    const bool chunk_row = q < 32 && (q & 7) == 7;
    for (int j = 0; j < 7; j++) {
        fp v = 0;
        if (chunk_row) {
            const int m = j + 7 * (q >> 3);
            v = m < 12 ? sv[m] : m < 24 ? rv[m - 12] : m == 24 ? w.deltas[t] : m == 25 ? sv[13] : w.msg_tail[2 * (size_t)t + m - 26];
        }
        out[(size_t)(12 + j) * n + g] = v;
    }
}
hipError_t launch_schnorr_trace(const TxWitnessDev &w, fp *d_trace, hipStream_t stream) {
    const size_t n = (size_t)w.n_tx * MERKLE_LEN;
    hipLaunchKernelGGL((k_trace_schnorr_hash<true, 64>), dim3(w.n_tx), dim3(64), 0, stream, w, d_trace, n);
    hipLaunchKernelGGL((k_trace_schnorr_ec<true, 64>), dim3(2 * w.n_tx), dim3(64), 0, stream, w, d_trace, n);
    hipLaunchKernelGGL(k_trace_schnorr_final<true>, dim3(w.n_tx), dim3(64), 0, stream, d_trace, n);
    hipLaunchKernelGGL(k_trace_schnorr_bits, dim3(w.n_tx, 2), dim3(256), 0, stream, w, d_trace, n);
    return hipGetLastError();
}
// The same kernels on an internal stream, so that the caller's stream can do work that does not depend on the trace (the public-input
// columns of SchnorrAir, then the interpolation and extension of registers 37..55) beside the latency-bound ladders (one wave per SIMD
// at 512 signatures).  join_a: registers 37..55 are complete (message hash, bit registers, limb accumulators); join_b: all of them.
// The ladders' staging tile: 64 rows while four ladders per CU leave room in LDS for a transform workgroup (13.5 KB each), else 16.
hipError_t launch_schnorr_trace_split(const TxWitnessDev &w, fp *d_trace, hipStream_t stream, hipStream_t side, hipEvent_t fork, hipEvent_t join_a,
                                      hipEvent_t join_b) {
    const size_t n = (size_t)w.n_tx * MERKLE_LEN;
    hipError_t e;
    if ((e = hipEventRecord(fork, stream)) != hipSuccess) return e;
    if ((e = hipStreamWaitEvent(side, fork, 0)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_trace_schnorr_hash<true, 64>), dim3(w.n_tx), dim3(64), 0, side, w, d_trace, n);
    hipLaunchKernelGGL(k_trace_schnorr_bits, dim3(w.n_tx, 2), dim3(256), 0, side, w, d_trace, n);
    if ((e = hipEventRecord(join_a, side)) != hipSuccess) return e;
    if (w.n_tx <= 512) hipLaunchKernelGGL((k_trace_schnorr_ec<true, 64>), dim3(2 * w.n_tx), dim3(64), 0, side, w, d_trace, n);
    else hipLaunchKernelGGL((k_trace_schnorr_ec<true, 16>), dim3(2 * w.n_tx), dim3(64), 0, side, w, d_trace, n);
    hipLaunchKernelGGL(k_trace_schnorr_final<true>, dim3(w.n_tx), dim3(64), 0, side, d_trace, n);
    if ((e = hipEventRecord(join_b, side)) != hipSuccess) return e;
    return hipGetLastError();
}
hipError_t launch_schnorr_aux_columns(const TxWitnessDev &w, fp *d_out, hipStream_t stream) {
    const size_t n = (size_t)w.n_tx * MERKLE_LEN;
    hipLaunchKernelGGL(k_schnorr_aux_columns, dim3(w.n_tx, 2), dim3(256), 0, stream, w, d_out, n);
    return hipGetLastError();
}

// RescueProver::build_trace (benches/rescue.rs:277-322): ONE chain -- 8 rows per link: seven Rescue rounds, then the capacity half reset
// to zero -- is a single sequential recurrence: one wave, lane e < 14 = state element e, 64 rows staged in LDS per coalesced flush.
// n = 8 * iterations rows, a multiple of 64.
struct RescueSeed { fp s[7]; };
__global__ __launch_bounds__(64) void k_trace_rescue_chain(RescueSeed seed, fp *__restrict__ trace, size_t n) {
    __shared__ fp tile[64][15];
    __shared__ fp xch[14];
    const int lane = threadIdx.x, e = lane < 14 ? lane : 0;
    const bool active = lane < 14;
    fp mrow[14];
#pragma unroll
    for (int j = 0; j < 14; j++) mrow[j] = c_mds[e * 14 + j];
    fp v = (active && lane < 7) ? seed.s[lane] : 0;
    if (active) tile[0][e] = v;
    for (size_t step = 0; step + 1 < n; step++) {
        const int cyc = (int)(step & 7);
        if (cyc < 7) v = rescue_round_lane(v, xch, mrow, e, cyc, active); // rescue::apply_round(state, step)
        else if (lane >= 7) v = 0;
        const int r = (int)((step + 1) & 63);
        if (active) tile[r][e] = v;
        if (r == 63) {
            __syncthreads();
            for (int c = 0; c < 14; c++) trace[(size_t)c * n + (step + 1 - 63) + lane] = tile[lane][c];
            __syncthreads();
        }
    }
}
hipError_t launch_rescue_chain_trace(const uint64_t seed[7], unsigned iterations, fp *d_trace, hipStream_t stream) {
    RescueSeed s;
    for (int i = 0; i < 7; i++) s.s[i] = seed[i];
    hipLaunchKernelGGL(k_trace_rescue_chain, dim3(1), dim3(64), 0, stream, s, d_trace, (size_t)iterations * 8);
    return hipGetLastError();
}

hipError_t launch_merkle_trace(const TxWitnessDev &w, fp *d_trace, hipStream_t stream) {
    const size_t n = (size_t)w.n_tx * MERKLE_LEN;
    hipLaunchKernelGGL((k_trace_merkle<true, 64>), dim3(w.n_tx), dim3(64), 0, stream, w, d_trace, n);
    return hipGetLastError();
}

// RangeProver::build_trace (src/range/prover.rs:24-43): row q holds bit (62 - (q-1)) and the top q bits of the 63-bit value
__global__ void k_trace_range(uint64_t number, fp *trace) {
    const int q = threadIdx.x; // 64 rows
    const uint64_t v63 = number & 0x7FFFFFFFFFFFFFFFULL; // bits 62..0 are consumed, MSB first
    const uint64_t acc = q == 0 ? 0 : v63 >> (63 - q);
    trace[q] = (q >= 1 && (acc & 1)) ? FP_ONE : 0;
    trace[64 + q] = fp_from_u64(acc);
}
hipError_t launch_range_trace(uint64_t number_canonical, fp *d_trace, hipStream_t stream) {
    hipLaunchKernelGGL(k_trace_range, dim3(1), dim3(64), 0, stream, number_canonical, d_trace);
    return hipGetLastError();
}

// The same accumulator over n = 2^log_n rows (synthetic long form of BASELINE.json's "range, 2^16 steps"): V is an (n-1)-bit integer,
// words[] its n/64 little-endian words; row q >= 1 holds bit (n-1-q) of V and acc_q = (V >> (n-1-q)) mod p.  With the MSB-first
// 64-bit chunks U_c = words[n/64 - 1 - c] the accumulator at the end of chunk c is E_c = sum_{c' <= c} U_c' (2^64)^(c-c') and inside
// the chunk acc_(64c+r) = E_(c-1) 2^(r+1) + (U_c >> (63-r)).
// Pass 1 (one workgroup): E_c for every chunk -- per-thread Horner over a segment, a scan of the 256 segment values, a second
// Horner pass.  Pass 2: one thread per row, coalesced stores.
__global__ __launch_bounds__(256) void k_range_chunk_prefix(const uint64_t *__restrict__ words, fp *__restrict__ prefix, unsigned n_chunks) {
    __shared__ fp seg[256], lead[256];
    const unsigned t = threadIdx.x, per = (n_chunks + 255) / 256, c0 = t * per, c1 = min(c0 + per, n_chunks);
    const fp B = FP_R2; // 2^64 in memory form is 2^128 mod p
    fp v = 0;
    for (unsigned c = c0; c < c1; c++) v = fp_add(fp_mul(v, B), fp_from_u64(words[n_chunks - 1 - c]));
    seg[t] = v;
    __syncthreads();
    if (t == 0) { // value carried into every segment: 256 dependent products, negligible
        const fp Bper = fp_pow(B, per);
        fp carry = 0;
        for (unsigned i = 0; i < 256; i++) { lead[i] = carry; carry = fp_add(fp_mul(carry, Bper), seg[i]); }
    }
    __syncthreads();
    v = lead[t];
    for (unsigned c = c0; c < c1; c++) { v = fp_add(fp_mul(v, B), fp_from_u64(words[n_chunks - 1 - c])); prefix[c] = v; }
}
__global__ __launch_bounds__(256) void k_trace_range_bits(const uint64_t *__restrict__ words, const fp *__restrict__ prefix, fp *__restrict__ trace,
                                                          unsigned log_n) {
    const size_t n = (size_t)1 << log_n, q = blockIdx.x * (size_t)256 + threadIdx.x;
    if (q >= n) return;
    const unsigned c = (unsigned)(q >> 6), r = (unsigned)(q & 63), n_chunks = (unsigned)(n >> 6);
    const uint64_t u = words[n_chunks - 1 - c];
    const fp before = c ? prefix[c - 1] : 0;
    const fp two_r1 = fp_pow(fp_from_u64(2), r + 1);
    trace[q] = ((u >> (63 - r)) & 1) ? FP_ONE : 0;
    trace[n + q] = fp_add(fp_mul(before, two_r1), fp_from_u64(u >> (63 - r)));
}
hipError_t launch_range_trace_bits(const uint64_t *d_words, fp *d_prefix, fp *d_trace, unsigned log_n, hipStream_t stream) {
    const size_t n = (size_t)1 << log_n;
    hipLaunchKernelGGL(k_range_chunk_prefix, dim3(1), dim3(256), 0, stream, d_words, d_prefix, (unsigned)(n >> 6));
    hipLaunchKernelGGL(k_trace_range_bits, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_words, (const fp *)d_prefix, d_trace, log_n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Signature check (cstark_schnorr_check_signatures): verify_signature (src/schnorr/mod.rs:220-245) for `count` signatures.  The
// programs of the SchnorrAir trace run for their verdict: the same message hash, the same two ladders (run_ladder_op) and the same
// complete addition and affine x (run_full_add, fp6_inv) as k_trace_schnorr_hash / _ec / _final, without a staging tile and without a
// trace store.  The values are therefore the trace's: the x that k_sig_final compares is registers 0..5 of row 511.
namespace {

// h = hash_message(R.x, message) as four canonical limbs.  14 lanes carry a hash: FOUR hashes per wave, as in k_ledger_merge (lanes
// 0..55 = (hash s, state element e); lanes 56..63 and the hashes of a partial last group only take part in the barriers).
__global__ __launch_bounds__(64) void k_sig_hash(const fp *__restrict__ messages, const fp *__restrict__ sig_rx, uint64_t *__restrict__ h_limbs,
                                                 uint32_t count) {
    __shared__ fp st[4][14];
    const int lane = threadIdx.x;
    const bool is_state = lane < 56;
    const int s = is_state ? lane / 14 : 0, e = is_state ? lane % 14 : 0;
    const uint32_t t = 4 * blockIdx.x + s;
    const bool active = is_state && t < count;
    fp mrow[14];
#pragma unroll
    for (int j = 0; j < 14; j++) mrow[j] = c_mds[e * 14 + j];
    const fp *msg = messages + 28 * (size_t)(active ? t : 0);
    fp v = (active && e < 6) ? sig_rx[6 * (size_t)t + e] : 0; // init_sig_verification_state, src/schnorr/trace.rs:18-30
    for (int step = 0; step < 39; step++) {                   // the steps of k_trace_schnorr_hash up to the one that yields h
        const int cyc = step & 7;
        if (cyc < 7) v = rescue_round_lane(v, st[s], mrow, e, cyc, active);
        else if (active && e >= 7) v = msg[7 * (step >> 3) + e - 7]; // message chunk, src/lib.rs:467-481 layout
    }
    if (active && e < 4) h_limbs[4 * (size_t)t + e] = fp_to_u64(v);
}

// grid = 2 * count workgroups of ONE wave, as k_trace_schnorr_ec: workgroup 2t is the ladder s*G of signature t, 2t + 1 the ladder
// h*P with P = message[0..12].  Each leaves its final (X, Y, Z) in points[2t + g][18]: what the trace holds in row 510.
__global__ __launch_bounds__(64) void k_sig_ladder(const fp *__restrict__ messages, const uint8_t *__restrict__ sig_s, const uint64_t *__restrict__ h_limbs,
                                                   fp *__restrict__ points, uint32_t count) {
    if (blockIdx.x >= 2 * count) return; // uniform over the workgroup, ahead of every barrier
    __shared__ fp slots[NSLOT][6];
    __shared__ Fp2 prods[LROLE][6];
    __shared__ uint8_t sbytes[32];
    __shared__ LadderLds pg;
    const uint32_t t = blockIdx.x >> 1;
    const int g = blockIdx.x & 1, lane = threadIdx.x;
    fp(*slot)[6] = slots;
    load_programs(pg, lane, 64);
    const fp *key = messages + 28 * (size_t)t;
    if (lane < 32) sbytes[lane] = g == 0 ? sig_s[32 * (size_t)t + lane] : (uint8_t)(h_limbs[4 * (size_t)t + (lane >> 3)] >> (8 * (lane & 7)));
    if (lane < 6) {
        slot[SX][lane] = 0;
        slot[SY][lane] = lane == 0 ? FP_ONE : 0;
        slot[SZ][lane] = 0;
        slot[SB3][lane] = c_b3[lane];
        slot[SPX][lane] = g == 0 ? c_generator[lane] : key[lane];
        slot[SPY][lane] = g == 0 ? c_generator[6 + lane] : key[6 + lane];
        slot[26][lane] = fp_add(slot[SPX][lane], slot[SPY][lane]);
        slot[SW][lane] = 0;
    }
    __syncthreads();
    if (lane < 2) fp6_store(slot[SK + lane], fp6_mul(fp6_load(slot[SB3]), fp6_load(slot[SPX + lane])));
    __syncthreads();
    for (int i = 254; i >= 0; i--) { // bits 254..0, MSB first (src/schnorr/trace.rs:79-82): bit 255 is never read
        run_ladder_op<OP_DOUBLE>(pg, slot, prods, lane);
        if (bit_le(sbytes, i)) run_ladder_op<OP_ADD_MIXED>(pg, slot, prods, lane); // uniform over the wave
    }
    if (lane < 18) points[18 * (size_t)blockIdx.x + lane] = slot[lane / 6][lane % 6];
}

// One wave per signature: S = s*G + h*P by the complete addition, x = X / Z (what k_trace_schnorr_final writes to row 511), then the
// verdict (cstark_sig_verdict): bit 255 of s, the curve equation of the key as 3 (y^2 - x^3 - x) = 3B, x against R.x.  Z = 0 -- the
// point at infinity -- is a mismatch whatever fp6_inv makes of it.  rx_out (optional) gets x for every signature.
__global__ __launch_bounds__(64) void k_sig_final(const fp *__restrict__ messages, const fp *__restrict__ sig_rx, const uint8_t *__restrict__ sig_s,
                                                  const fp *__restrict__ points, uint8_t *__restrict__ verdicts, fp *__restrict__ rx_out, uint32_t count) {
    if (blockIdx.x >= count) return; // uniform over the workgroup, ahead of every barrier
    __shared__ fp slots[QZ + 1][6];
    __shared__ Fp2 prods[FROLE][6];
    __shared__ FullLds pg;
    const uint32_t t = blockIdx.x;
    const int lane = threadIdx.x;
    load_programs(pg, lane, 64);
    if (lane < 18) {
        slots[lane / 6][lane % 6] = points[36 * (size_t)t + lane];
        slots[QX + lane / 6][lane % 6] = points[36 * (size_t)t + 18 + lane];
    }
    if (lane < 6) slots[SB3][lane] = c_b3[lane];
    __syncthreads();
    run_full_add(pg, slots, prods, lane);
    if (lane != 0) return;
    const Fp6 z = fp6_load(slots[SZ]);
    bool match = false;
#pragma unroll
    for (int i = 0; i < 6; i++) match |= z.c[i] != 0; // infinity never matches
    const Fp6 x = fp6_mul(fp6_load(slots[SX]), fp6_inv(z));
#pragma unroll
    for (int i = 0; i < 6; i++) {
        match &= x.c[i] == sig_rx[6 * (size_t)t + i];
        if (rx_out) rx_out[6 * (size_t)t + i] = x.c[i];
    }
    const Fp6 kx = fp6_load(messages + 28 * (size_t)t), ky = fp6_load(messages + 28 * (size_t)t + 6);
    const Fp6 d = fp6_sub(fp6_sub(fp6_sqr(ky), fp6_mul(fp6_sqr(kx), kx)), kx);
    const Fp6 d3 = fp6_add(fp6_dbl(d), d);
    bool on_curve = true;
#pragma unroll
    for (int i = 0; i < 6; i++) on_curve &= d3.c[i] == c_b3[i];
    verdicts[t] = (sig_s[32 * (size_t)t + 31] >> 7) ? SIG_SCALAR_RANGE : !on_curve ? SIG_KEY_NOT_ON_CURVE : !match ? SIG_MISMATCH : SIG_VALID;
}

} // namespace

hipError_t launch_signature_check(const uint64_t *d_messages, const uint64_t *d_sig_rx, const uint8_t *d_sig_s, uint64_t *d_h_limbs, uint64_t *d_points,
                                  uint8_t *d_verdicts, uint64_t *d_rx_out, uint32_t count, hipStream_t stream) {
    hipLaunchKernelGGL(k_sig_hash, dim3((count + 3) / 4), dim3(64), 0, stream, d_messages, d_sig_rx, d_h_limbs, count);
    hipLaunchKernelGGL(k_sig_ladder, dim3(2 * count), dim3(64), 0, stream, d_messages, d_sig_s, (const uint64_t *)d_h_limbs, d_points, count);
    hipLaunchKernelGGL(k_sig_final, dim3(count), dim3(64), 0, stream, d_messages, d_sig_rx, d_sig_s, (const fp *)d_points, d_verdicts, d_rx_out, count);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Signing (cstark_schnorr_sign ...): schnorr::sign (src/schnorr/mod.rs:197-217) with the integer scalar step of csrc/witness_gen.hip,
// s = r - sk*h accepted when 0 <= s < 2^255.  The base point of R = r*G is fixed, so a table T[w][d] = d * 16^w * G (w = 0..65,
// d = 1..15) turns the 264-bit scalar multiplication into at most 66 mixed additions and no doubling: a sixth of the dependent point
// operations of a 255-bit ladder, in a kernel whose time is the latency of that chain.  An entry is 24 words in memory form,
// (x, y, K = b3*x, K2 = b3*y): the mixed addition's two per-point constants are stored with the point (190 KB for the 990 entries),
// so that no F_p6 product by one lane sits between two additions.
namespace {

constexpr int SIGN_DIGITS = 15, SIGN_ENTRY = 24;
static_assert(SIGN_TABLE_WORDS == (size_t)SIGN_WINDOWS * SIGN_DIGITS * SIGN_ENTRY, "the context allocates what the kernels index");
static_assert(SK2 == SK + 1 && SPY == SPX + 1, "an entry is copied into two slot pairs");

// One wave per entry, k_sig_ladder's shape with a variable bit length: the ladder programs over the 4 + 4w bits of d * 16^w, then one
// fp6_inv for the affine x and y.  d >= 1 and d * 16^w < 2^264 is no multiple of the group order: Z != 0.
__global__ __launch_bounds__(64) void k_sign_table(fp *__restrict__ table) {
    if (blockIdx.x >= SIGN_WINDOWS * SIGN_DIGITS) return; // uniform over the workgroup, ahead of every barrier
    __shared__ fp slots[NSLOT][6];
    __shared__ Fp2 prods[LROLE][6];
    __shared__ LadderLds pg;
    const int w = blockIdx.x / SIGN_DIGITS, d = blockIdx.x % SIGN_DIGITS + 1, lane = threadIdx.x;
    fp(*slot)[6] = slots;
    load_programs(pg, lane, 64);
    if (lane < 6) {
        slot[SX][lane] = 0;
        slot[SY][lane] = lane == 0 ? FP_ONE : 0;
        slot[SZ][lane] = 0;
        slot[SB3][lane] = c_b3[lane];
        slot[SPX][lane] = c_generator[lane];
        slot[SPY][lane] = c_generator[6 + lane];
        slot[26][lane] = fp_add(slot[SPX][lane], slot[SPY][lane]);
        slot[SW][lane] = 0;
    }
    __syncthreads();
    if (lane < 2) fp6_store(slot[SK + lane], fp6_mul(fp6_load(slot[SB3]), fp6_load(slot[SPX + lane])));
    __syncthreads();
    for (int i = 4 * w + 3; i >= 0; i--) { // MSB first, as the trace's ladders
        run_ladder_op<OP_DOUBLE>(pg, slot, prods, lane);
        if (i >= 4 * w && ((d >> (i - 4 * w)) & 1)) run_ladder_op<OP_ADD_MIXED>(pg, slot, prods, lane); // uniform over the wave
    }
    if (lane != 0) return;
    const Fp6 zi = fp6_inv(fp6_load(slots[SZ])), b3 = fp6_load(slots[SB3]);
    const Fp6 x = fp6_mul(fp6_load(slots[SX]), zi), y = fp6_mul(fp6_load(slots[SY]), zi);
    fp *e = table + (size_t)SIGN_ENTRY * blockIdx.x;
    fp6_store(e, x);
    fp6_store(e + 6, y);
    fp6_store(e + 12, fp6_mul(b3, x));
    fp6_store(e + 18, fp6_mul(b3, y));
}

// One wave per nonce: acc = (0 : 1 : 0), then acc += T[w][digit_w(r)] for every non-zero base-16 digit of r (uniform over the wave).
// The mixed addition is the reference's complete formula (compute_add_mixed, src/utils/ecc.rs:330-404), valid for every pair of
// points: the partial sum meeting an equal table point, its negative, or the identity the sum starts from needs no special case.
// The next entry is fetched into registers while the current addition runs.  nonces [n][5] little-endian limbs, r < 2^264.
// points (optional) [n][12] affine (x, y), rx (optional) [n][6] affine x, infinity [n]: 1 where r*G is the point at infinity, whose
// coordinates are written as zeros.
__global__ __launch_bounds__(64) void k_sign_comb(const fp *__restrict__ table, const uint64_t *__restrict__ nonces, fp *__restrict__ points,
                                                  fp *__restrict__ rx, uint8_t *__restrict__ infinity, uint32_t n) {
    if (blockIdx.x >= n) return; // uniform over the workgroup, ahead of every barrier
    __builtin_amdgcn_s_setprio(CS_RECUR_PRIO);
    __shared__ fp slots[NSLOT][6];
    __shared__ Fp2 prods[LROLE][6];
    __shared__ uint8_t dig[SIGN_WINDOWS + 1];
    __shared__ LadderLds pg;
    const uint32_t t = blockIdx.x;
    const int lane = threadIdx.x;
    fp(*slot)[6] = slots;
    load_programs(pg, lane, 64);
    if (lane < 6) {
        slot[SX][lane] = 0;
        slot[SY][lane] = lane == 0 ? FP_ONE : 0;
        slot[SZ][lane] = 0;
        slot[SB3][lane] = c_b3[lane];
        slot[SW][lane] = 0;
    }
    for (int w = lane; w <= SIGN_WINDOWS; w += 64) dig[w] = w < SIGN_WINDOWS ? (uint8_t)((nonces[5 * (size_t)t + w / 16] >> (4 * (w % 16))) & 15) : 0;
    __syncthreads();
    // lanes 0..23 carry the entry's words into slots SPX, SPY, SK, SK2; lanes 24..29 the operand qx + qy (slot 26)
    const int part = lane / 6, word = lane % 6;
    const int dst = part < 2 ? SPX + part : part < 4 ? SK + part - 2 : 26;
    auto fetch = [&](int w, int d) -> fp {
        const fp *e = table + (size_t)SIGN_ENTRY * (SIGN_DIGITS * w + d - 1);
        return lane < 24 ? e[lane] : lane < 30 ? fp_add(e[word], e[6 + word]) : 0;
    };
    fp next = dig[0] ? fetch(0, dig[0]) : 0;
    for (int w = 0; w < SIGN_WINDOWS; w++) {
        const int d = dig[w], dn = dig[w + 1];
        const fp cur = next;
        if (dn) next = fetch(w + 1, dn);
        if (d) {
            if (lane < 30) slot[dst][word] = cur;
            __syncthreads();
            run_ladder_op<OP_ADD_MIXED>(pg, slot, prods, lane);
        }
    }
    if (lane != 0) return;
    const Fp6 z = fp6_load(slots[SZ]);
    bool finite = false;
#pragma unroll
    for (int i = 0; i < 6; i++) finite |= z.c[i] != 0;
    Fp6 x = {}, y = {};
    if (finite) { // Z = 0 is tested before anything uses fp6_inv(0)
        const Fp6 zi = fp6_inv(z);
        x = fp6_mul(fp6_load(slots[SX]), zi);
        y = fp6_mul(fp6_load(slots[SY]), zi);
    }
    if (points) {
        fp6_store(points + 12 * (size_t)t, x);
        fp6_store(points + 12 * (size_t)t + 6, y);
    }
    if (rx) fp6_store(rx + 6 * (size_t)t, x);
    infinity[t] = finite ? 0 : 1;
}

// the message of attempt a is that of the signature it belongs to: [count][28] gathered through owner [count]
__global__ __launch_bounds__(256) void k_sign_gather(const fp *__restrict__ messages, const uint32_t *__restrict__ owner, fp *__restrict__ out, uint32_t count) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)28 * count) return;
    out[i] = messages[28 * (size_t)owner[i / 28] + i % 28];
}

// One thread per attempt: the 320-bit two's-complement d = r - sk*h in five limbs (64 x 64 -> 128 products), sig_s = bits 0..255 of d
// whatever the status (the values of cstark_sign_status).  h: four canonical limbs, each below p; sk <= 255; r < 2^264: no limb is lost.
// owner (optional): the signature an attempt belongs to, whose secret it uses; null: attempt a uses secrets[a].
__global__ __launch_bounds__(256) void k_sign_scalar(const uint64_t *__restrict__ nonces, const uint64_t *__restrict__ secrets, const uint32_t *__restrict__ owner,
                                                     const uint64_t *__restrict__ h_limbs, const uint8_t *__restrict__ infinity, uint64_t *__restrict__ sig_s,
                                                     uint8_t *__restrict__ status, uint32_t count) {
    typedef unsigned __int128 u128;
    const size_t a = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= count) return;
    const uint64_t sk = secrets[owner ? owner[a] : a];
    uint64_t skh[5], d[5];
    u128 c = 0;
    for (int i = 0; i < 4; i++) { c += (u128)h_limbs[4 * a + i] * sk; skh[i] = (uint64_t)c; c >>= 64; }
    skh[4] = (uint64_t)c;
    uint64_t borrow = 0;
    for (int i = 0; i < 5; i++) {
        const u128 x = (u128)nonces[5 * a + i] - skh[i] - borrow;
        d[i] = (uint64_t)x;
        borrow = (uint64_t)(x >> 64) & 1;
    }
    for (int i = 0; i < 4; i++) sig_s[4 * a + i] = d[i];
    status[a] = infinity[a] ? SIGN_INFINITY : borrow ? SIGN_NEGATIVE : (d[4] != 0 || (d[3] >> 63)) ? SIGN_RANGE : SIGN_OK;
}

} // namespace

hipError_t launch_sign_table(uint64_t *d_table, hipStream_t stream) {
    hipLaunchKernelGGL(k_sign_table, dim3(SIGN_WINDOWS * SIGN_DIGITS), dim3(64), 0, stream, d_table);
    return hipGetLastError();
}

hipError_t launch_sign_points(const uint64_t *d_table, const uint64_t *d_nonces, uint64_t *d_points, uint64_t *d_rx, uint8_t *d_infinity, uint32_t count,
                              hipStream_t stream) {
    hipLaunchKernelGGL(k_sign_comb, dim3(count), dim3(64), 0, stream, (const fp *)d_table, d_nonces, d_points, d_rx, d_infinity, count);
    return hipGetLastError();
}

hipError_t launch_sign_attempts(const uint64_t *d_table, const uint64_t *d_messages, const uint32_t *d_owner, uint64_t *d_gathered, const uint64_t *d_secrets,
                                const uint64_t *d_nonces, uint64_t *d_rx, uint8_t *d_infinity, uint64_t *d_h_limbs, uint8_t *d_sig_s, uint8_t *d_status,
                                uint32_t count, hipStream_t stream) {
    hipLaunchKernelGGL(k_sign_comb, dim3(count), dim3(64), 0, stream, (const fp *)d_table, d_nonces, (fp *)nullptr, d_rx, d_infinity, count);
    if (d_owner) {
        hipLaunchKernelGGL(k_sign_gather, dim3((unsigned)(((size_t)28 * count + 255) / 256)), dim3(256), 0, stream, d_messages, d_owner, d_gathered, count);
        d_messages = d_gathered;
    }
    hipLaunchKernelGGL(k_sig_hash, dim3((count + 3) / 4), dim3(64), 0, stream, d_messages, (const fp *)d_rx, d_h_limbs, count);
    hipLaunchKernelGGL(k_sign_scalar, dim3((count + 255) / 256), dim3(256), 0, stream, d_nonces, d_secrets, d_owner, (const uint64_t *)d_h_limbs,
                       (const uint8_t *)d_infinity, (uint64_t *)d_sig_s, d_status, count);
    return hipGetLastError();
}

} // namespace cs
