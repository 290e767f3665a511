// The constraint bodies of the five AIRs as templates over an accumulator with add(slot, flag, value), and what they are written
// against: the frame view, the register / result / periodic-column indices, the Rescue round and curve gadgets.  Included by
// constraints.hip (the evaluators of the proof and of the verifier's out-of-domain check) and by trace_check.hip (trace validation): one
// statement of each constraint for both.  Everything here has internal linkage or is a template.
#pragma once
#include "constraints.h"
#include "rescue.cuh"
#include "tower.cuh"

namespace cs {
namespace {

constexpr int NT = 128; // threads per workgroup

// register / result / periodic-column indices (src/merkle/constants.rs:33-63, src/constants.rs:35-116)
enum {
    S_INIT = 0, S_UPD = 15, R_INIT = 29, R_UPD = 44, PREV_ROOT = 58, S_KEY = 65, R_KEY = 77, DELTA_COPY = 89, SIGMA_COPY = 90,
    NONCE_COPY = 91, DELTA_BIT = 56, DELTA_ACC = 57, SIGMA_BIT = 92, SIGMA_ACC = 93,
    VALUE_RES = 65, BALANCE_RES = 90, NONCE_UPD_RES = 91, INT_ROOT_RES = 92, PREV_MATCH_RES = 99, S_KEY_RES = 101, R_KEY_RES = 103,
    DELTA_COPY_RES = 105, SIGMA_COPY_RES = 106, NONCE_COPY_RES = 107, DELTA_RANGE_RES = 108, SIGMA_RANGE_RES = 109,
    P_SETUP = 0, P_MERKLE = 1, P_HASH_INPUT = 2, P_FINISH = 3, P_HASH = 4, P_SCHNORR = 5, P_SCALAR_MULT = 6, P_DOUBLING = 7,
    P_DIGEST = 8, P_SCHNORR_HASH = 12, P_HASH_INTERNAL = 13, P_RANGE_STEP = 17, P_RANGE_FINISH = 18, P_VALUE_COPY = 19, P_ARK = 20
};

// one evaluation frame: strided views of the current / next LDE rows and of the periodic values
struct Frame {
    const fp *cur_p, *next_p, *per_p; // element c at cur_p[c * n], per_p[c * pcycle]
    size_t n;
    unsigned pcycle;                  // rows per periodic cycle (1024 for the composite AIR)
    __device__ __forceinline__ fp cur(int c) const { return cur_p[(size_t)c * n]; }
    __device__ __forceinline__ fp next(int c) const { return next_p[(size_t)c * n]; }
    __device__ __forceinline__ fp pv(int c) const { return per_p[(size_t)c * pcycle]; }
};

// ---- accumulators ---------------------------------------------------------------------------------
// Parity/debug: every result slot is kept, in global memory: out[i * n + j] += flag * value.
struct AccAll {
    fp *out; // points at element j of slot 0
    size_t n;
    __device__ __forceinline__ void add(int i, fp flag, fp val) { out[(size_t)i * n] = fp_add(out[(size_t)i * n], fp_mul(flag, val)); }
};
__device__ __forceinline__ fp c_not(fp a) { return fp_sub(FP_ONE, a); }
__device__ __forceinline__ fp c_is_binary(fp a) { return fp_sub(fp_sqr(a), a); }

// sum_j m[j] * x[j] for a row of 14 constants: seven products per fold of the 128-bit accumulator, one reduction
__device__ __forceinline__ fp dot14_rows(const fp *__restrict__ m, const fp (&x)[14]) {
    Acc128 a = acc_zero();
#pragma unroll
    for (int j = 0; j < 7; j++) acc_mad(a, m[j], x[j]);
    acc_fold(a);
#pragma unroll
    for (int j = 7; j < 14; j++) acc_mad(a, m[j], x[j]);
    acc_fold(a);
    return acc_reduce(a);
}

// ---- Rescue round gadget (rescue.rs:269-300) on the 14-register window starting at `reg`; the same 14
// differences feed up to two (result base, flag) pairs.
template <class Acc>
__device__ __forceinline__ void enforce_round(Acc &acc, const Frame &f, int reg, int res_a, fp flag_a, int res_b, fp flag_b, bool two) {
    fp cube[14], d[14];
#pragma unroll
    for (int j = 0; j < 14; j++) {
        cube[j] = fp_cube(f.cur(reg + j));
        d[j] = fp_sub(f.next(reg + j), f.pv(P_ARK + 14 + j));
    }
#pragma unroll 1
    for (int i = 0; i < 14; i++) {
        // rows of the two matrices against the 14 cubes / differences: 128-bit accumulation, one reduction per row (dot14 below)
        const fp s1 = fp_add(f.pv(P_ARK + i), dot14_rows(c_mds + i * 14, cube));
        const fp s2 = dot14_rows(c_inv_mds + i * 14, d);
        const fp diff = fp_sub(fp_cube(s2), s1);
        acc.add(res_a + i, flag_a, diff);
        if (two) acc.add(res_b + i, flag_b, diff);
    }
}

// ---- curve gadgets (ecc.rs:73-172).  F_p6 products are real calls to keep the kernel inside the
// instruction cache: the five gadgets contain 69 of them.
#ifdef CS_EC_NOINLINE
__device__ __noinline__ Fp6 mul6(const Fp6 a, const Fp6 b) { return fp6_mul(a, b); }
#else
__device__ __forceinline__ Fp6 mul6(const Fp6 &a, const Fp6 &b) { return fp6_mul(a, b); }
#endif
// the parity/debug kernel keeps everything in one launch and must stay compact: always a call there
__device__ __noinline__ Fp6 mul6_call(const Fp6 a, const Fp6 b) { return fp6_mul(a, b); }

template <bool CALL>
__device__ __forceinline__ Fp6 MUL6_SEL(const Fp6 &a, const Fp6 &b) {
    if constexpr (CALL) return mul6_call(a, b);
    else return mul6(a, b);
}

struct Point { Fp6 x, y, z; };

__device__ __forceinline__ Fp6 load6(const Frame &f, int reg, bool next) {
    Fp6 r;
#pragma unroll
    for (int i = 0; i < 6; i++) r.c[i] = next ? f.next(reg + i) : f.cur(reg + i);
    return r;
}
__device__ __forceinline__ Fp6 const6(const fp *p) { return fp6_load(p); }

template <bool CALL>
__device__ __forceinline__ Point ec_double(const Point &p) {
#define mul6 MUL6_SEL<CALL> // complete doubling, ecc.rs:177-242
    const Fp6 b3 = const6(c_b3);
#ifdef CS_EC_SQR
    Fp6 t0 = fp6_sqr(p.x), t1 = fp6_sqr(p.y), t2 = fp6_sqr(p.z);
#else
    Fp6 t0 = mul6(p.x, p.x), t1 = mul6(p.y, p.y), t2 = mul6(p.z, p.z);
#endif
    Fp6 t3 = fp6_dbl(mul6(p.x, p.y));
    Fp6 z3 = fp6_dbl(mul6(p.x, p.z));
    Fp6 y3 = fp6_add(z3, mul6(b3, t2));
    Fp6 x3 = fp6_sub(t1, y3);
    y3 = fp6_add(t1, y3);
    y3 = mul6(x3, y3);
    x3 = mul6(t3, x3);
    z3 = mul6(b3, z3);
    t3 = fp6_add(fp6_sub(t0, t2), z3);
    t0 = fp6_add(fp6_add(fp6_dbl(t0), t0), t2);
    y3 = fp6_add(y3, mul6(t0, t3));
    t2 = fp6_dbl(mul6(p.y, p.z));
    x3 = fp6_sub(x3, mul6(t2, t3));
    z3 = fp6_dbl(fp6_dbl(mul6(t2, t1)));
    return {x3, y3, z3};
#undef mul6
}
template <bool CALL>
__device__ __forceinline__ Point ec_add_mixed(const Point &p, const Fp6 &qx, const Fp6 &qy) {
#define mul6 MUL6_SEL<CALL> // ecc.rs:330-404
    const Fp6 b3 = const6(c_b3);
    Fp6 t0 = mul6(p.x, qx), t1 = mul6(p.y, qy);
    Fp6 t3 = fp6_sub(mul6(fp6_add(qx, qy), fp6_add(p.x, p.y)), fp6_add(t0, t1));
    Fp6 t4 = fp6_add(mul6(qx, p.z), p.x);
    Fp6 t5 = fp6_add(mul6(qy, p.z), p.y);
    Fp6 z3 = fp6_add(mul6(p.z, b3), t4);
    Fp6 x3 = fp6_sub(t1, z3);
    z3 = fp6_add(t1, z3);
    Fp6 y3 = mul6(x3, z3);
    t1 = fp6_add(fp6_add(fp6_dbl(t0), t0), p.z);
    t4 = fp6_add(mul6(t4, b3), fp6_sub(t0, p.z));
    y3 = fp6_add(y3, mul6(t1, t4));
    x3 = fp6_sub(mul6(t3, x3), mul6(t5, t4));
    z3 = fp6_add(mul6(t5, z3), mul6(t3, t1));
    return {x3, y3, z3};
#undef mul6
}
template <bool CALL>
__device__ __forceinline__ Point ec_add(const Point &p, const Point &q) {
#define mul6 MUL6_SEL<CALL> // ecc.rs:244-328
    const Fp6 b3 = const6(c_b3);
    Fp6 t0 = mul6(p.x, q.x), t1 = mul6(p.y, q.y), t2 = mul6(p.z, q.z);
    Fp6 t3 = fp6_sub(mul6(fp6_add(p.x, p.y), fp6_add(q.x, q.y)), fp6_add(t0, t1));
    Fp6 t4 = fp6_sub(mul6(fp6_add(p.x, p.z), fp6_add(q.x, q.z)), fp6_add(t0, t2));
    Fp6 t5 = fp6_sub(mul6(fp6_add(p.y, p.z), fp6_add(q.y, q.z)), fp6_add(t1, t2));
    Fp6 z3 = fp6_add(mul6(b3, t2), t4);
    Fp6 x3 = fp6_sub(t1, z3);
    z3 = fp6_add(t1, z3);
    Fp6 y3 = mul6(x3, z3);
    t1 = fp6_add(fp6_add(fp6_dbl(t0), t0), t2);
    t4 = fp6_add(mul6(b3, t4), fp6_sub(t0, t2));
    y3 = fp6_add(y3, mul6(t1, t4));
    x3 = fp6_sub(mul6(t3, x3), mul6(t5, t4));
    z3 = fp6_add(mul6(t5, z3), mul6(t3, t1));
    return {x3, y3, z3};
#undef mul6
}

// doubling + conditional mixed addition constraints for the point at registers [reg, reg+19)
template <class Acc>
__device__ __forceinline__ void enforce_scalar_mult_step(Acc &acc, const Frame &f, int reg, const Fp6 &qx, const Fp6 &qy, fp doubling, fp addition) {
    const Point p = {load6(f, reg, false), load6(f, reg + 6, false), load6(f, reg + 12, false)};
    const fp bit = f.cur(reg + 18);
    {   // enforce_point_doubling ecc.rs:73-98
        const Point d = ec_double<true>(p);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            acc.add(reg + i, doubling, fp_sub(f.next(reg + i), d.x.c[i]));
            acc.add(reg + 6 + i, doubling, fp_sub(f.next(reg + 6 + i), d.y.c[i]));
            acc.add(reg + 12 + i, doubling, fp_sub(f.next(reg + 12 + i), d.z.c[i]));
        }
        acc.add(reg + 18, doubling, c_is_binary(bit));
    }
    {   // enforce_point_addition_mixed ecc.rs:102-138: next = bit * (p + q) + (1 - bit) * p
        const Point a = ec_add_mixed<true>(p, qx, qy);
        const fp nb = c_not(bit);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            acc.add(reg + i, addition, fp_sub(f.next(reg + i), fp_add(fp_mul(bit, a.x.c[i]), fp_mul(nb, p.x.c[i]))));
            acc.add(reg + 6 + i, addition, fp_sub(f.next(reg + 6 + i), fp_add(fp_mul(bit, a.y.c[i]), fp_mul(nb, p.y.c[i]))));
            acc.add(reg + 12 + i, addition, fp_sub(f.next(reg + 12 + i), fp_add(fp_mul(bit, a.z.c[i]), fp_mul(nb, p.z.c[i]))));
        }
        acc.add(reg + 18, addition, fp_sub(bit, f.next(reg + 18)));
    }
}

// src/merkle/update/air.rs:291-369 without its two enforce_round calls (done by the caller per window)
template <class Acc>
__device__ __forceinline__ void merkle_auth_rest(Acc &acc, const Frame &f, int base, fp tx_hash, fp hash_input, fp hash_flag) {
    const fp hash_copy = fp_mul(tx_hash, c_not(fp_add(hash_flag, hash_input)));
    const fp hash_init = fp_mul(tx_hash, hash_input);
    const fp bit = f.next(base + 14), not_bit = c_not(bit);
    acc.add(base + 14, tx_hash, c_is_binary(bit));
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
        const int b = base + 15 * k;
#pragma unroll 1
        for (int i = 0; i < 7; i++) {
            const fp ci = f.cur(b + i), d = fp_sub(ci, f.next(b + i));
            acc.add(b + i, hash_copy, d);
            acc.add(b + i, hash_init, fp_mul(not_bit, d));
            acc.add(b + 7 + i, hash_init, fp_mul(bit, fp_sub(ci, f.next(b + 7 + i))));
        }
    }
#pragma unroll 1
    for (int i = 0; i < 7; i++) acc.add(base + i, hash_init, fp_mul(bit, fp_sub(f.next(base + 15 + i), f.next(base + i))));
#pragma unroll 1
    for (int i = 7; i < 14; i++) acc.add(base + i, hash_init, fp_mul(not_bit, fp_sub(f.next(base + 15 + i), f.next(base + i))));
}

// All 115 transition constraints at one point (src/air.rs:114-173, :383-610).
template <class Acc>
__device__ __forceinline__ void evaluate_transition(Acc &acc, const Frame &f) {
    const fp setup = f.pv(P_SETUP), tx_hash = f.pv(P_MERKLE), hash_input = f.pv(P_HASH_INPUT), finish = f.pv(P_FINISH), hash_flag = f.pv(P_HASH);
    const fp schnorr_mask = f.pv(P_SCHNORR), scalar_mult = f.pv(P_SCALAR_MULT), doubling = f.pv(P_DOUBLING), schnorr_hash = f.pv(P_SCHNORR_HASH);
    const fp range_flag = f.pv(P_RANGE_STEP), range_finish = f.pv(P_RANGE_FINISH), copy_values = f.pv(P_VALUE_COPY);
    const fp copy_hash = fp_mul(c_not(schnorr_hash), schnorr_mask);
    const fp final_add = fp_mul(c_not(scalar_mult), schnorr_mask);
    const fp addition = fp_mul(c_not(doubling), scalar_mult);

    // Rescue windows: merkle::init (setup flag, shifted result bases, src/merkle/init/air.rs:166-201) and
    // merkle::update (hash flag, src/merkle/update/air.rs:316-322) share their register windows.
    enforce_round(acc, f, S_INIT, S_INIT, setup, S_INIT, hash_flag, true);
    enforce_round(acc, f, S_UPD, S_UPD - 1, setup, S_UPD, hash_flag, true);
    enforce_round(acc, f, R_INIT, R_INIT - 1, setup, R_INIT, hash_flag, true);
    enforce_round(acc, f, R_UPD, R_UPD - 2, setup, R_UPD, hash_flag, true);
    enforce_round(acc, f, 42, 42, schnorr_hash, 0, 0, false); // src/schnorr/air.rs:488-494

    // transaction setup (src/air.rs:406-453)
#pragma unroll 1
    for (int i = 0; i < 12; i++) {
        acc.add(VALUE_RES + i, setup, fp_sub(f.cur(S_INIT + i), f.cur(S_UPD + i)));
        acc.add(VALUE_RES + 12 + i, setup, fp_sub(f.cur(R_INIT + i), f.cur(R_UPD + i)));
    }
    acc.add(VALUE_RES + 24, setup, fp_sub(f.cur(R_INIT + 13), f.cur(R_UPD + 13)));
    const fp s_spent = fp_sub(f.cur(S_INIT + 12), f.cur(S_UPD + 12));
    acc.add(BALANCE_RES, setup, fp_sub(s_spent, fp_sub(f.cur(R_UPD + 12), f.cur(R_INIT + 12))));
    acc.add(NONCE_UPD_RES, setup, fp_sub(f.cur(S_UPD + 13), fp_add(f.cur(S_INIT + 13), FP_ONE)));
    // key / delta / sigma / nonce copies (src/air.rs:456-529; result indices alias as in the reference)
#pragma unroll 1
    for (int o = 0; o < 12; o++) {
        const fp sk = f.next(S_KEY + o), rk = f.next(R_KEY + o);
        acc.add(S_KEY_RES + o, setup, fp_sub(sk, f.cur(S_INIT + o)));
        acc.add(R_KEY_RES + o, setup, fp_sub(rk, f.cur(R_INIT + o)));
        acc.add(S_KEY_RES + o, copy_values, fp_sub(sk, f.cur(S_KEY + o)));
        acc.add(R_KEY_RES + o, copy_values, fp_sub(rk, f.cur(R_KEY + o)));
    }
    acc.add(DELTA_COPY_RES, setup, fp_sub(f.next(DELTA_COPY), s_spent));
    acc.add(SIGMA_COPY_RES, setup, fp_sub(f.next(SIGMA_COPY), f.cur(S_UPD + 12)));
    acc.add(NONCE_COPY_RES, setup, fp_sub(f.next(NONCE_COPY), f.cur(S_INIT + 13)));
    acc.add(DELTA_COPY_RES, copy_values, fp_sub(f.next(DELTA_COPY), f.cur(DELTA_COPY)));
    acc.add(SIGMA_COPY_RES, copy_values, fp_sub(f.next(SIGMA_COPY), f.cur(SIGMA_COPY)));
    acc.add(NONCE_COPY_RES, copy_values, fp_sub(f.next(NONCE_COPY), f.cur(NONCE_COPY)));

    // merkle::update (src/merkle/update/air.rs:215-289)
    merkle_auth_rest(acc, f, S_INIT, tx_hash, hash_input, hash_flag);
    merkle_auth_rest(acc, f, R_INIT, tx_hash, hash_input, hash_flag);
    const fp not_finish = c_not(finish);
#pragma unroll 1
    for (int i = 0; i < 7; i++) {
        const fp nr = f.next(PREV_ROOT + i), cr = f.cur(PREV_ROOT + i);
        acc.add(PREV_ROOT + i, not_finish, fp_sub(nr, cr));
        acc.add(PREV_ROOT + i, finish, fp_sub(nr, f.next(R_UPD + i)));
        acc.add(INT_ROOT_RES + i, finish, fp_sub(f.cur(S_UPD + i), f.cur(R_INIT + i)));
        acc.add(PREV_MATCH_RES + i, finish, fp_sub(f.next(S_INIT + i), cr));
    }

    // schnorr (src/schnorr/air.rs:394-531) on registers / results [0, 56)
    {
        const Fp6 gx = const6(c_generator), gy = const6(c_generator + 6);
        enforce_scalar_mult_step(acc, f, 0, gx, gy, doubling, addition);
        const Fp6 px = load6(f, S_KEY, true), py = load6(f, S_KEY + 6, true); // pkey = next[S_KEY..], src/air.rs:575
        enforce_scalar_mult_step(acc, f, 19, px, py, doubling, addition);
    }
#pragma unroll 1
    for (int i = 0; i < 4; i++) { // h-limb double-and-add, accumulator copies (:451-484)
        const fp dflag = f.pv(P_DIGEST + i);
        const fp c = f.cur(41 - i), nx = f.next(41 - i);
        acc.add(41 - i, fp_mul(dflag, doubling), fp_sub(nx, fp_add(fp_dbl(c), f.next(37))));
        acc.add(41 - i, fp_mul(c_not(dflag), doubling), fp_sub(c, nx));
        acc.add(38 + i, addition, fp_sub(f.cur(38 + i), f.next(38 + i)));
        acc.add(38 + i, final_add, fp_sub(f.cur(38 + i), f.cur(42 + i))); // h == hash output (:521-530)
    }
    // enforce_hash_copy (:309-330) with the internal inputs of src/air.rs:543-565
#pragma unroll 1
    for (int i = 0; i < 7; i++) {
        acc.add(42 + i, copy_hash, fp_sub(f.cur(42 + i), f.next(42 + i)));
        fp inp = 0;
#pragma unroll 1
        for (int k = 0; k < 4; k++) {
            const int m = k * 7 + i;
            const fp cell = m < 12 ? f.next(S_KEY + m) : m < 24 ? f.next(R_KEY + m - 12) : m == 24 ? f.next(DELTA_COPY) : m == 25 ? f.next(NONCE_COPY) : 0;
            inp = fp_add(inp, fp_mul(f.pv(P_HASH_INTERNAL + k), cell));
        }
        acc.add(49 + i, copy_hash, fp_sub(f.next(49 + i), inp));
    }
    {   // final addition S + h*P with X reduced to affine (ecc.rs:146-172)
        const Point s = {load6(f, 0, false), load6(f, 6, false), load6(f, 12, false)};
        const Point hp = {load6(f, 19, false), load6(f, 25, false), load6(f, 31, false)};
        const Point r = ec_add<true>(s, hp);
        const Fp6 xz = mul6_call(load6(f, 0, true), r.z);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            acc.add(i, final_add, fp_sub(xz.c[i], r.x.c[i]));
            acc.add(6 + i, final_add, fp_sub(f.next(6 + i), r.y.c[i]));
            acc.add(12 + i, final_add, fp_sub(f.next(12 + i), r.z.c[i]));
        }
    }
    // range proofs (src/air.rs:583-609); SIGMA_RANGE_RES re-checks the delta registers, as in the reference
    {
        const fp db = f.next(DELTA_BIT), sb = f.next(SIGMA_BIT);
        acc.add(DELTA_ACC, range_flag, fp_sub(f.next(DELTA_ACC), fp_add(fp_dbl(f.cur(DELTA_ACC)), db)));
        acc.add(DELTA_BIT, range_flag, c_is_binary(db));
        acc.add(SIGMA_ACC, range_flag, fp_sub(f.next(SIGMA_ACC), fp_add(fp_dbl(f.cur(SIGMA_ACC)), sb)));
        acc.add(SIGMA_BIT, range_flag, c_is_binary(sb));
        const fp dr = fp_sub(f.next(DELTA_ACC), f.next(DELTA_COPY));
        acc.add(DELTA_RANGE_RES, range_finish, dr);
        acc.add(SIGMA_RANGE_RES, range_finish, dr);
    }
}

// the transition constraints of MerkleAir at one point, through any accumulator with add(slot, flag, value)
// ROUNDS = false: without the four Rescue round gadgets (k_merkle_rounds evaluates them in their folded form)
template <bool ROUNDS = true, class Acc>
__device__ __forceinline__ void merkle_transitions(Acc &acc, const Frame &f) {
    // periodic layout: setup, hash(tx), hash_input, finish, hash_mask, ark[28]; the gadget templates read the round
    // constants at P_ARK + i relative to per_p, so give them a view shifted by (5 - P_ARK) columns
    Frame fr = f;
    fr.per_p = f.per_p - (size_t)(P_ARK - 5) * f.pcycle;
    const fp setup = f.pv(0), tx_hash = f.pv(1), hash_input = f.pv(2), finish = f.pv(3), hash_flag = f.pv(4);
#pragma unroll 1
    for (int i = 0; i < 12; i++) {
        acc.add(VALUE_RES + i, setup, fp_sub(f.cur(S_INIT + i), f.cur(S_UPD + i)));
        acc.add(VALUE_RES + 12 + i, setup, fp_sub(f.cur(R_INIT + i), f.cur(R_UPD + i)));
    }
    acc.add(VALUE_RES + 24, setup, fp_sub(f.cur(R_INIT + 13), f.cur(R_UPD + 13)));
    acc.add(BALANCE_RES, setup, fp_sub(fp_sub(f.cur(S_INIT + 12), f.cur(S_UPD + 12)), fp_sub(f.cur(R_UPD + 12), f.cur(R_INIT + 12))));
    acc.add(NONCE_UPD_RES, setup, fp_sub(f.cur(S_UPD + 13), fp_add(f.cur(S_INIT + 13), FP_ONE)));
    if (ROUNDS) {
        enforce_round(acc, fr, S_INIT, S_INIT, hash_flag, 0, 0, false);
        enforce_round(acc, fr, S_UPD, S_UPD, hash_flag, 0, 0, false);
        enforce_round(acc, fr, R_INIT, R_INIT, hash_flag, 0, 0, false);
        enforce_round(acc, fr, R_UPD, R_UPD, hash_flag, 0, 0, false);
    }
    merkle_auth_rest(acc, f, S_INIT, tx_hash, hash_input, hash_flag);
    merkle_auth_rest(acc, f, R_INIT, tx_hash, hash_input, hash_flag);
    const fp not_finish = c_not(finish);
#pragma unroll 1
    for (int i = 0; i < 7; i++) {
        const fp nr = f.next(PREV_ROOT + i), cr = f.cur(PREV_ROOT + i);
        acc.add(PREV_ROOT + i, not_finish, fp_sub(nr, cr));
        acc.add(PREV_ROOT + i, finish, fp_sub(nr, f.next(R_UPD + i)));
        acc.add(INT_ROOT_RES + i, finish, fp_sub(f.cur(S_UPD + i), f.cur(R_INIT + i)));
        acc.add(PREV_MATCH_RES + i, finish, fp_sub(f.next(S_INIT + i), cr));
    }
}

// The body, shared by the table kernel and the free-standing-frame kernel: ax = element 0 of the 19 public-input values of the point,
// value c at ax[c * astride]; fr = f with column P_ARK at the first round-constant column (index 8 here).
template <int PART, class Acc>
__device__ __forceinline__ void schnorr_transitions(Acc &acc, const Frame &f, const Frame &fr, const fp *ax, size_t astride) {
    const fp global_mask = f.pv(0), scalar_mult = f.pv(1), doubling = f.pv(2), hash_flag = f.pv(7);
    const fp copy_hash = fp_mul(c_not(hash_flag), global_mask);
    const fp final_add = fp_mul(c_not(scalar_mult), global_mask);
    const fp addition = fp_mul(c_not(doubling), scalar_mult);
    if constexpr (PART == 0) {
        const Fp6 gx = const6(c_generator), gy = const6(c_generator + 6);
        enforce_scalar_mult_step(acc, f, 0, gx, gy, doubling, addition);
    }
    if constexpr (PART == 1) {
        const Fp6 px = fp6_load_strided(ax, astride), py = fp6_load_strided(ax + 6 * astride, astride); // periodic pkey columns
        enforce_scalar_mult_step(acc, f, 19, px, py, doubling, addition);
    }
    if constexpr (PART == 2) {
#pragma unroll 1
        for (int i = 0; i < 4; i++) {
            const fp dflag = f.pv(3 + i);
            const fp c = f.cur(41 - i), nx = f.next(41 - i);
            acc.add(41 - i, fp_mul(dflag, doubling), fp_sub(nx, fp_add(fp_dbl(c), f.next(37))));
            acc.add(41 - i, fp_mul(c_not(dflag), doubling), fp_sub(c, nx));
            acc.add(38 + i, addition, fp_sub(f.cur(38 + i), f.next(38 + i)));
            acc.add(38 + i, final_add, fp_sub(f.cur(38 + i), f.cur(42 + i)));
        }
        enforce_round(acc, fr, 42, 42, hash_flag, 0, 0, false);
#pragma unroll 1
        for (int i = 0; i < 7; i++) {
            acc.add(42 + i, copy_hash, fp_sub(f.cur(42 + i), f.next(42 + i)));
            acc.add(49 + i, copy_hash, fp_sub(f.next(49 + i), ax[(size_t)(12 + i) * astride]));
        }
    }
    if constexpr (PART == 3) {
        const Point s = {load6(f, 0, false), load6(f, 6, false), load6(f, 12, false)};
        const Point hp = {load6(f, 19, false), load6(f, 25, false), load6(f, 31, false)};
        const Point r = ec_add<true>(s, hp);
        const Fp6 xz = mul6_call(load6(f, 0, true), r.z);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            acc.add(i, final_add, fp_sub(xz.c[i], r.x.c[i]));
            acc.add(6 + i, final_add, fp_sub(f.next(6 + i), r.y.c[i]));
            acc.add(12 + i, final_add, fp_sub(f.next(12 + i), r.z.c[i]));
        }
    }
}

// RangeProofAir::evaluate_transition  src/range/air.rs:60-98 (enforce_double_and_add_step with flag ONE)
template <class Acc>
__device__ __forceinline__ void range_transitions(Acc &acc, const Frame &f) {
    const fp nb = f.next(0);
    acc.add(1, FP_ONE, fp_sub(f.next(1), fp_add(fp_dbl(f.cur(1)), nb))); // result[1]: accumulator
    acc.add(0, FP_ONE, c_is_binary(nb));                                 // result[0]: bit
}

} // namespace

// RescueAir::evaluate_transition, benches/rescue.rs:200-222 (+ enforce_hash_copy :254-264): the round gadget under the cycle mask, the
// copy of the rate half / reset of the capacity half under its complement.  ptab: [b][29][8] (mask, 28 round constants)
template <class Acc>
__device__ __forceinline__ void rescue_transitions(Acc &acc, const Frame &f) {
    const fp hash_flag = f.pv(0), copy_flag = c_not(hash_flag);
    Frame fr = f; // the gadget reads the round constants at P_ARK + i relative to per_p: a view shifted by (1 - P_ARK) columns
    fr.per_p = f.per_p - (size_t)(P_ARK - 1) * f.pcycle;
    enforce_round(acc, fr, 0, 0, hash_flag, 0, 0, false);
    for (int i = 0; i < 7; i++) {
        acc.add(i, copy_flag, fp_sub(f.cur(i), f.next(i)));
        acc.add(7 + i, copy_flag, f.next(7 + i));
    }
}

} // namespace cs
