// Host-only: the mixed addition of the CONSTANT generator G as a quadratic map of the first point, and the tables that let the
// doubling kernel (constraints.hip: k_ec_split<PART_DBL0>, k_schnorr_ec_split<PART_DBL0>) produce the generator addition's sums from
// the six products it forms anyway.  Pure arithmetic over hostgadgets.h: no HIP header, compiles under plain g++
// (tests/cpp/generator_fold_check.cpp).
//
// With the second point fixed, the steps t0, t1, t3, t4, t5, z3, x3 of the complete mixed addition (ecc.rs:330-404) are LINEAR in
// (X, Y, Z) and every output coordinate is a sum of products of two such forms, hence
//     a_coord = sum_m K[coord][m] * mono_m,   mono = (X^2, Y^2, Z^2, XY, XZ, YZ),   K[coord][m] in F_p6 fixed by G and b3.
// K is derived by replaying the formula on linear forms.  Multiplication by a constant of F_p6 is F_p-linear on the six components,
// so component i of the 18 outputs is sum_{m, c} J[i][6 m + c] * mono_m.c[c] with J[6 coord + r][6 m + c] = component r of
// K[coord][m] * e_c.  A sum over the outputs with per-proof coefficients is then ONE functional on the 36 monomial components:
//     sum_i coef_i a_i = sum_e Lambda[e] * mono[e],   Lambda[e] = sum_i coef_i J[i][e].
#pragma once
#include "hostgadgets.h"

namespace cs { namespace hostg {

constexpr int GF_OUTPUTS = 18, GF_MONOS = 6, GF_COMPONENTS = 36; // 18 output components; 6 monomials of 6 components each
constexpr int GF_FUNCTIONALS = 3;                                // alpha over all outputs | beta of x (group 0) | beta of y, z (group 1)
constexpr int GF_LAMBDA_WORDS = GF_FUNCTIONALS * GF_COMPONENTS;  // per coefficient set

struct LinForm { F6 c[3]; };          // c[0] X + c[1] Y + c[2] Z
struct QuadForm { F6 m[GF_MONOS]; };  // coefficients of X^2, Y^2, Z^2, XY, XZ, YZ

inline F6 zero6() { return F6{}; }
inline F6 one6() { F6 r{}; r.c[0].a = ONE; return r; }
inline LinForm lin_add(const LinForm &x, const LinForm &y) { return {{add6(x.c[0], y.c[0]), add6(x.c[1], y.c[1]), add6(x.c[2], y.c[2])}}; }
inline LinForm lin_sub(const LinForm &x, const LinForm &y) { return {{sub6(x.c[0], y.c[0]), sub6(x.c[1], y.c[1]), sub6(x.c[2], y.c[2])}}; }
inline LinForm lin_scale(const LinForm &x, const F6 &k) { return {{mul6(x.c[0], k), mul6(x.c[1], k), mul6(x.c[2], k)}}; }
inline QuadForm lin_mul(const LinForm &x, const LinForm &y) {
    QuadForm q;
    for (int v = 0; v < 3; v++) q.m[v] = mul6(x.c[v], y.c[v]);
    q.m[3] = add6(mul6(x.c[0], y.c[1]), mul6(x.c[1], y.c[0]));
    q.m[4] = add6(mul6(x.c[0], y.c[2]), mul6(x.c[2], y.c[0]));
    q.m[5] = add6(mul6(x.c[1], y.c[2]), mul6(x.c[2], y.c[1]));
    return q;
}
inline QuadForm quad_add(const QuadForm &x, const QuadForm &y) { QuadForm q; for (int m = 0; m < GF_MONOS; m++) q.m[m] = add6(x.m[m], y.m[m]); return q; }
inline QuadForm quad_sub(const QuadForm &x, const QuadForm &y) { QuadForm q; for (int m = 0; m < GF_MONOS; m++) q.m[m] = sub6(x.m[m], y.m[m]); return q; }

// pt_add_mixed (hostgadgets.h) step by step on the forms X, Y, Z: out[coord] = the quadratic form of x3, y3, z3
inline void generator_addition_forms(const F6 &qx, const F6 &qy, QuadForm out[3]) {
    const F6 b3 = load6(CS_B3_MONT);
    const LinForm X = {{one6(), zero6(), zero6()}}, Y = {{zero6(), one6(), zero6()}}, Z = {{zero6(), zero6(), one6()}};
    LinForm t0 = lin_scale(X, qx), t1 = lin_scale(Y, qy);
    LinForm t3 = lin_sub(lin_scale(lin_add(X, Y), add6(qx, qy)), lin_add(t0, t1));
    LinForm t4 = lin_add(lin_scale(Z, qx), X), t5 = lin_add(lin_scale(Z, qy), Y);
    LinForm z3 = lin_add(lin_scale(Z, b3), t4), x3 = lin_sub(t1, z3);
    z3 = lin_add(t1, z3);
    QuadForm y3 = lin_mul(x3, z3);
    t1 = lin_add(lin_add(lin_add(t0, t0), t0), Z);
    t4 = lin_add(lin_scale(t4, b3), lin_sub(t0, Z));
    out[1] = quad_add(y3, lin_mul(t1, t4));
    out[0] = quad_sub(lin_mul(t3, x3), lin_mul(t5, t4));
    out[2] = quad_add(lin_mul(t5, z3), lin_mul(t3, t1));
}

// The monomials of a point in the order of QuadForm, components as store6 lays them out: mono[6 m + c]
inline void generator_fold_monomials(const Pt &p, fp mono[GF_COMPONENTS]) {
    store6(mono, mul6(p.x, p.x));
    store6(mono + 6, mul6(p.y, p.y));
    store6(mono + 12, mul6(p.z, p.z));
    store6(mono + 18, mul6(p.x, p.y));
    store6(mono + 24, mul6(p.x, p.z));
    store6(mono + 30, mul6(p.y, p.z));
}

// J[i][e], i = 6 coord + r < 18, e = 6 m + c < 36 (Montgomery form, row-major): what the context uploads once
inline void generator_fold_matrix(fp J[GF_OUTPUTS * GF_COMPONENTS]) {
    QuadForm k[3];
    generator_addition_forms(load6(CS_GENERATOR_MONT), load6(CS_GENERATOR_MONT + 6), k);
    for (int coord = 0; coord < 3; coord++)
        for (int m = 0; m < GF_MONOS; m++)
            for (int c = 0; c < 6; c++) {
                fp e[6] = {0, 0, 0, 0, 0, 0}, col[6];
                e[c] = ONE;
                store6(col, mul6(k[coord].m[m], load6(e)));
                for (int r = 0; r < 6; r++) J[(6 * coord + r) * GF_COMPONENTS + 6 * m + c] = col[r];
            }
}

// The three functionals of one coefficient set (what the device folds per proof): alpha[18], beta[18] = the coefficients of the
// 18 coordinate slots; outputs 0..5 (x) are in the first degree group, 6..17 (y, z) in the second (tx_degree_group, constraints.h)
constexpr int gf_first(int f) { return f == 2 ? 6 : 0; }
constexpr int gf_last(int f) { return f == 1 ? 6 : GF_OUTPUTS; }
inline void generator_fold_lambda(const fp *J, const fp *alpha, const fp *beta, fp lambda[GF_LAMBDA_WORDS]) {
    for (int f = 0; f < GF_FUNCTIONALS; f++)
        for (int e = 0; e < GF_COMPONENTS; e++) {
            fp s = 0;
            for (int i = gf_first(f); i < gf_last(f); i++) s = add(s, mul(f == 0 ? alpha[i] : beta[i], J[i * GF_COMPONENTS + e]));
            lambda[f * GF_COMPONENTS + e] = s;
        }
}

}} // namespace cs::hostg
