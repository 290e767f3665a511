// csrc/air_groups.h on its own: the grouping that the generic merge of the sub-AIRs works from, against what the shape of each AIR says
// directly.  For MerkleAir, SchnorrAir (1 and 2 signatures), RangeProofAir and RescueAir, at two trace lengths and every blowup from the
// AIR's own up to 8: every constraint's group carries its degree adjustment, every assertion's group its divisor and boundary
// adjustment, every per-coset power is the power of that coset's offset, and no AIR needs more than AIR_MAX_GROUPS groups; a shape with
// too many distinct degrees or divisors is refused, the degrees first.  Built and run by tests/test_verify_cpu.py (host code only, no GPU).
#include <cstdio>
#include <set>
#include <utility>
#include "../../certificate-stark_amd/csrc/air_groups.h"

using namespace cs::host;

#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { std::printf("line %d: %s (%s)\n", __LINE__, #cond, what); return false; } \
    } while (0)

static bool check_case(int air, uint32_t n_items, unsigned log_n, unsigned log_b) {
    char what[96];
    std::snprintf(what, sizeof what, "air %d items %u log_n %u log_b %u", air, n_items, log_n, log_b);
    AirShape s;
    CHECK(air_shape(air, s, n_items));
    AirGroups q;
    CHECK(air_groups(s, log_n, log_b, q) == AIR_GROUPS_OK);
    const uint64_t n = 1ull << log_n, ce = n << s.log_ce_blowup(), b = 1ull << log_b;
    const uint64_t wn = root_of_unity(log_n);
    CHECK(q.n_tgrp >= 1 && q.n_tgrp <= (uint32_t)AIR_MAX_GROUPS && q.n_agrp >= 1 && q.n_agrp <= (uint32_t)AIR_MAX_GROUPS);
    CHECK(q.t_grp.size() == s.n_constraints && q.a_grp.size() == s.a_reg.size());

    // constraints: degree = base (n - 1) + cycles x (the degree of a periodic column: n / cycle_len copies of a polynomial of degree cycle_len - 1)
    std::set<uint64_t> adjs;
    for (size_t i = 0; i < s.n_constraints; i++) {
        const uint64_t periodic = s.cycle_len ? (uint64_t)s.cycles[i] * (n / s.cycle_len) * (s.cycle_len - 1) : 0;
        const uint64_t degree = (uint64_t)s.base[i] * (n - 1) + periodic;
        CHECK(degree < ce); // the constraint-evaluation domain holds every constraint
        CHECK(q.t_grp[i] < q.n_tgrp);
        CHECK(q.tgrp_adj[q.t_grp[i]] == CSTARK_CONV_TRANSITION_ADJUSTMENT(ce, n, degree));
        adjs.insert(q.tgrp_adj[q.t_grp[i]]);
    }
    CHECK(adjs.size() == q.n_tgrp); // no group twice, none unused

    // assertions: the divisor x^m - zc vanishes on exactly the m steps the assertion holds at
    std::set<std::pair<uint64_t, uint64_t>> divisors;
    for (size_t a = 0; a < s.a_reg.size(); a++) {
        const bool periodic = !s.a_stride.empty() && s.a_stride[a];
        const uint64_t stride = periodic ? s.a_stride[a] : n, m = n / stride;
        const uint64_t first = s.a_stride.empty() ? (s.a_last[a] ? n - 1 : 0) : s.a_first[a];
        const uint32_t g = q.a_grp[a];
        CHECK(g < q.n_agrp);
        CHECK(q.agrp_m[g] == m);
        for (uint64_t k = 0; k < m; k++) CHECK(pow(pow(wn, first + k * stride), m) == q.agrp_zc[g]);
        CHECK(q.agrp_badj[g] == CSTARK_CONV_BOUNDARY_ADJUSTMENT(ce, n, m));
        divisors.insert({q.agrp_m[g], q.agrp_zc[g]});
    }
    CHECK(divisors.size() == q.n_agrp);

    // per-coset powers of shift_k = g w_{bn}^k
    const uint64_t wbn = root_of_unity(log_n + log_b);
    for (uint64_t k = 0; k < b; k++) {
        const uint64_t shift = mul(lde_offset(), pow(wbn, k));
        CHECK(q.shifts[k] == shift);
        for (uint32_t g = 0; g < q.n_tgrp; g++) CHECK(q.tgrp_shift[k][g] == pow(shift, q.tgrp_adj[g]));
        for (uint32_t g = 0; g < q.n_agrp; g++) {
            CHECK(q.agrp_bshift[k][g] == pow(shift, q.agrp_badj[g]));
            CHECK(q.agrp_mshift[k][g] == pow(shift, q.agrp_m[g]));
        }
        CHECK(mul(q.zinv_coset[k], sub(pow(shift, n), ONE)) == ONE);
    }
    return true;
}

// nine distinct constraint degrees and / or nine distinct assertion divisors: one more than the kernel's parameter block holds
static AirShape crowded(bool degrees, bool divisors) {
    AirShape s;
    s.width = 9; s.n_constraints = 9;
    for (uint32_t i = 0; i < 9; i++) { s.base.push_back(degrees ? 1 + i : 2); s.cycles.push_back(0); }
    for (uint32_t a = 0; a < 9; a++) { s.a_reg.push_back(a); s.a_last.push_back(0); s.a_first.push_back(divisors ? a : 0); s.a_stride.push_back(512); }
    return s;
}
static bool check_refusals() {
    const char *what = "crowded shapes";
    AirGroups q;
    CHECK(air_groups(crowded(false, false), 10, 3, q) == AIR_GROUPS_OK && q.n_tgrp == 1 && q.n_agrp == 1);
    CHECK(air_groups(crowded(true, false), 10, 3, q) == AIR_GROUPS_TOO_MANY_DEGREES);
    CHECK(air_groups(crowded(false, true), 10, 3, q) == AIR_GROUPS_TOO_MANY_DIVISORS);
    CHECK(air_groups(crowded(true, true), 10, 3, q) == AIR_GROUPS_TOO_MANY_DEGREES); // the degrees are grouped first
    AirShape eight = crowded(true, true); // exactly AIR_MAX_GROUPS of each is fine
    eight.n_constraints = 8; eight.base.pop_back(); eight.cycles.pop_back();
    eight.a_reg.pop_back(); eight.a_last.pop_back(); eight.a_first.pop_back(); eight.a_stride.pop_back();
    CHECK(air_groups(eight, 10, 3, q) == AIR_GROUPS_OK && q.n_tgrp == 8 && q.n_agrp == 8);
    return true;
}

int main() {
    struct Case { int air; uint32_t n_items; unsigned log_n[2]; };
    const Case cases[] = {
        {1, 0, {9, 11}},  // MerkleAir: 1 and 4 transfers
        {2, 1, {9, 10}},  // SchnorrAir, bit degree of one signature (the second length: the degrees of 1, the rows of 2)
        {2, 2, {10, 12}}, // SchnorrAir, 2 and 8 signatures
        {3, 0, {6, 16}},  // RangeProofAir: the reference's 64 rows and the long form
        {4, 0, {6, 12}},  // RescueAir: chains of 8 and 512
    };
    unsigned runs = 0;
    for (const Case &c : cases) {
        AirShape s;
        if (!air_shape(c.air, s, c.n_items)) { std::printf("no shape for air %d\n", c.air); return 1; }
        for (unsigned log_n : c.log_n)
            for (unsigned log_b = s.log_ce_blowup(); log_b <= 3; log_b++, runs++)
                if (!check_case(c.air, c.n_items, log_n, log_b)) return 1;
    }
    AirShape none;
    if (air_shape(0, none, 1) || air_shape(5, none, 1)) { std::printf("air ids 0 and 5 have no generic shape\n"); return 1; }
    if (!check_refusals()) return 1;
    std::printf("ok: %u groupings checked\n", runs);
    return 0;
}
