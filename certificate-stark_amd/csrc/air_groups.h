// Host-only description of the standalone sub-AIRs (MerkleAir, SchnorrAir, RangeProofAir, RescueAir) and the grouping that the
// generic merge k_air_combine works from: which constraints share a degree adjustment, which assertions share a divisor, and the
// powers of every coset offset that complete x^e without a square-and-multiply per point.  Pure arithmetic over hostfield.h: no
// HIP header, compiles under plain g++ (tests/cpp/air_groups_check.cpp).
#pragma once
#include <stdint.h>
#include <vector>
#include "../../include/cstark_conventions.h"
#include "hostfield.h"

namespace cs {
namespace host {

// Static description of an AIR as the engine sees it: width, constraint degrees (base; cycles of length cycle_len),
// single-step assertions.  air ids as in cstark_air_id.
struct AirShape {
    uint32_t width = 0, n_constraints = 0, cycle_len = 0, n_periodic = 0;
    std::vector<uint32_t> base, cycles;
    std::vector<uint32_t> a_reg, a_last; // assertion register, 0 = first step / 1 = last step (single assertions)
    // generalisation (Assertion::periodic / ::sequence): when a_stride is non-empty assertion a holds at steps
    // a_first[a] + k * a_stride[a]; its value is the caller's assertion_values[a] or, if a_seq[a] >= 0, column a_seq[a] of
    // the extended sequence-value polynomials
    std::vector<uint32_t> a_first, a_stride;
    std::vector<int32_t> a_seq;
    std::vector<uint64_t> a_const; // built-in constant values (SchnorrAir), empty when the caller supplies them
    uint32_t log_ce_blowup() const {     // next power of two >= max(base + cycles), at least 2 [UPSTREAM-RECALL]
        uint32_t m = 2;
        for (size_t i = 0; i < base.size(); i++) m = base[i] + (cycle_len ? cycles[i] : 0) > m ? base[i] + (cycle_len ? cycles[i] : 0) : m;
        uint32_t l = 0;
        while ((1u << l) < m) l++;
        return l;
    }
    uint64_t eval_degree(size_t i, uint64_t n) const { return base[i] * (n - 1) + (cycle_len ? cycles[i] * (n / cycle_len) * (cycle_len - 1) : 0); }
    // assertion a holds on the n / stride steps first + k stride: its divisor is x^m - w_n^(first m), m = n / stride (single
    // assertions: m = 1, first = 0 or n - 1)
    uint64_t assertion_first(size_t a, uint64_t n) const { return a_stride.empty() ? (a_last[a] ? n - 1 : 0) : a_first[a]; }
    uint64_t assertion_steps(size_t a, uint64_t n) const { return (!a_stride.empty() && a_stride[a]) ? n / a_stride[a] : 1; }
};
inline bool air_shape(int air, AirShape &s, uint32_t n_items = 2) {
    s = AirShape{};
    if (air == 1) { // MerkleAir: transition_constraint_degrees(512), src/merkle/update/air.rs:371-401; 14 root assertions :142-170
        s.width = 65; s.n_constraints = 106; s.cycle_len = 512; s.n_periodic = 33;
        s.base.assign(106, 1); s.cycles.assign(106, 1);
        for (int b = 0; b < 58; b += 29) { for (int i = 0; i < 29; i++) s.base[b + i] = 3; s.base[b + 14] = 2; }
        for (int a = 0; a < 14; a++) { s.a_reg.push_back(58 + a % 7); s.a_last.push_back(a / 7); }
        return true;
    }
    if (air == 2) { // SchnorrAir: degrees src/schnorr/air.rs:533-585 (bit degree depends on the number of signatures),
                    // the 61 periodic / sequence assertions of get_assertions (:111-226) in order
        s.width = 56; s.n_constraints = 56; s.cycle_len = 512; s.n_periodic = 36;
        s.base.assign(56, 0); s.cycles.assign(56, 0);
        const uint32_t bit_degree = n_items == 1 ? 3 : 5;
        for (int i = 0; i < 6; i++) { s.base[i] = 5; s.cycles[i] = 2; }
        for (int i = 6; i < 18; i++) { s.base[i] = 4; s.cycles[i] = 2; }
        s.base[18] = 2; s.cycles[18] = 1;
        for (int i = 19; i < 37; i++) { s.base[i] = bit_degree; s.cycles[i] = 2; }
        s.base[37] = 2; s.cycles[37] = 1;
        for (int i = 38; i < 42; i++) { s.base[i] = 1; s.cycles[i] = 2; }
        for (int i = 42; i < 56; i++) { s.base[i] = 3; s.cycles[i] = 1; }
        auto add = [&](uint32_t r, uint32_t first, uint64_t v, int32_t q) {
            s.a_reg.push_back(r); s.a_last.push_back(0); s.a_first.push_back(first); s.a_stride.push_back(512); s.a_const.push_back(v); s.a_seq.push_back(q);
        };
        for (int i = 0; i < 18; i++) add(i, 0, i == 6 ? ONE : 0, -1);
        add(18, 0, 0, -1);
        for (int i = 0; i < 18; i++) add(19 + i, 0, i == 6 ? ONE : 0, -1);
        for (int i = 0; i < 5; i++) add(37 + i, 0, 0, -1);
        for (int k = 0; k < 6; k++) add(42 + k, 0, 0, k);
        for (int i = 0; i < 7; i++) add(48 + i, 0, 0, -1);
        for (int k = 0; k < 6; k++) add(k, 511, 0, 6 + k);
        return true;
    }
    if (air == 4) { // RescueAir of benches/rescue.rs: 14 x (3; one cycle of 8) :169-191, seed / result assertions :224-243
        s.width = 14; s.n_constraints = 14; s.cycle_len = 8; s.n_periodic = 29;
        s.base.assign(14, 3); s.cycles.assign(14, 1);
        for (int a = 0; a < 14; a++) { s.a_reg.push_back(a % 7); s.a_last.push_back(a / 7); }
        return true;
    }
    if (air == 3) { // RangeProofAir: degrees (2), (1), src/range/air.rs:100-105; assertions :79-86
        s.width = 2; s.n_constraints = 2; s.cycle_len = 0; s.n_periodic = 0;
        s.base = {2, 1}; s.cycles = {0, 0};
        s.a_reg = {1, 1}; s.a_last = {0, 1};
        return true;
    }
    return false;
}

// ---- grouping for the generic merge --------------------------------------------------------------------------------------------
// Constraint i contributes (alpha_i + beta_i x^tgrp_adj[t_grp[i]]) C_i(x); assertion a is divided by x^m - zc and lifted by x^badj of
// its group a_grp[a].  The kernel keeps one power per group, not per constraint, so the distinct values are collected here; it holds
// at most AIR_MAX_GROUPS of each (constraints.h states the same number for its parameter block, capi.hip asserts that they agree).
constexpr int AIR_MAX_GROUPS = 8, AIR_MAX_COSETS = 8;
struct AirGroups {
    uint32_t n_tgrp = 0, n_agrp = 0;
    uint64_t tgrp_adj[AIR_MAX_GROUPS] = {}, agrp_m[AIR_MAX_GROUPS] = {}, agrp_zc[AIR_MAX_GROUPS] = {}, agrp_badj[AIR_MAX_GROUPS] = {};
    std::vector<uint32_t> t_grp, a_grp; // group of every constraint / assertion
    // per LDE coset k < 2^log_b, shift_k = g w_{bn}^k: shift_k, shift_k^adj of every transition group, shift_k^badj and shift_k^m of
    // every assertion group, 1 / (shift_k^n - 1)
    uint64_t shifts[AIR_MAX_COSETS] = {};
    uint64_t tgrp_shift[AIR_MAX_COSETS][AIR_MAX_GROUPS] = {}, agrp_bshift[AIR_MAX_COSETS][AIR_MAX_GROUPS] = {}, agrp_mshift[AIR_MAX_COSETS][AIR_MAX_GROUPS] = {};
    uint64_t zinv_coset[AIR_MAX_COSETS] = {};
};
enum AirGroupsResult { AIR_GROUPS_OK = 0, AIR_GROUPS_TOO_MANY_DEGREES, AIR_GROUPS_TOO_MANY_DIVISORS };

// log_b <= 3 (the caller's check); the adjustments are those of the AIR's own constraint-evaluation domain n 2^log_ce_blowup()
inline AirGroupsResult air_groups(const AirShape &s, unsigned log_n, unsigned log_b, AirGroups &q) {
    q = AirGroups{};
    const uint64_t n = 1ull << log_n, ce = n << s.log_ce_blowup(), b = 1ull << log_b;
    const size_t nc = s.n_constraints, na = s.a_reg.size();
    const uint64_t wn = root_of_unity(log_n);
    q.t_grp.resize(nc);
    q.a_grp.resize(na);
    for (size_t i = 0; i < nc; i++) { // distinct degree adjustments
        const uint64_t adj = CSTARK_CONV_TRANSITION_ADJUSTMENT(ce, n, s.eval_degree(i, n));
        uint32_t g = 0;
        while (g < q.n_tgrp && q.tgrp_adj[g] != adj) g++;
        if (g == q.n_tgrp) {
            if (g == (uint32_t)AIR_MAX_GROUPS) return AIR_GROUPS_TOO_MANY_DEGREES;
            q.tgrp_adj[q.n_tgrp++] = adj;
        }
        q.t_grp[i] = g;
    }
    for (size_t a = 0; a < na; a++) { // distinct assertion divisors x^m - w^(first m)
        const uint64_t m = s.assertion_steps(a, n);
        const uint64_t zc = pow(wn, (s.assertion_first(a, n) * m) % n);
        uint32_t g = 0;
        while (g < q.n_agrp && !(q.agrp_m[g] == m && q.agrp_zc[g] == zc)) g++;
        if (g == q.n_agrp) {
            if (g == (uint32_t)AIR_MAX_GROUPS) return AIR_GROUPS_TOO_MANY_DIVISORS;
            q.agrp_m[g] = m; q.agrp_zc[g] = zc; q.agrp_badj[g] = CSTARK_CONV_BOUNDARY_ADJUSTMENT(ce, n, m);
            q.n_agrp++;
        }
        q.a_grp[a] = g;
    }
    const uint64_t wbn = root_of_unity(log_n + log_b);
    uint64_t sh = lde_offset();
    for (uint64_t k = 0; k < b; k++) { // (the kernel completes each power with a twiddle-table product per point)
        q.shifts[k] = sh;
        for (uint32_t g = 0; g < q.n_tgrp; g++) q.tgrp_shift[k][g] = pow(sh, q.tgrp_adj[g]);
        for (uint32_t g = 0; g < q.n_agrp; g++) {
            q.agrp_bshift[k][g] = pow(sh, q.agrp_badj[g]);
            q.agrp_mshift[k][g] = pow(sh, q.agrp_m[g]);
        }
        q.zinv_coset[k] = inv(sub(pow(sh, n), ONE));
        sh = mul(sh, wbn);
    }
    return AIR_GROUPS_OK;
}

} // namespace host
} // namespace cs
