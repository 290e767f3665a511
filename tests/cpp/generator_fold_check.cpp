// csrc/generator_fold.h on its own: the mixed addition of the constant generator as a quadratic map of the first point.
//   1. sum_m K[coord][m] mono_m (through the matrix J, component by component) equals hostgadgets.h's pt_add_mixed with G;
//   2. for random alpha and beta, the three folded functionals applied to the 36 monomial components equal the sums over the 18
//      output components (alpha over all, beta over x, beta over y and z).
// On 1200 random triples (X, Y, Z) of F_p6 -- NOT on the curve: the identity is polynomial -- and on every pattern of triples whose
// components are all 0, 1 or p - 1, plus triples that mix these values.  Built and run by tests/test_generator_fold_cpu.py (host code
// only, no GPU).
#include <cstdio>
#include <cstdint>
#include "../../certificate-stark_amd/csrc/generator_fold.h"

using namespace cs::hostg;

static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint64_t rnd() { // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
static fp rnd_fp() { return from_u64(rnd()); }

static fp J[GF_OUTPUTS * GF_COMPONENTS];

// the 18 components of (X, Y, Z) + G by the reference formula, and through J; then the functionals
static bool check_point(const fp xyz[18], const char *what, long idx) {
    const Pt p = {load6(xyz), load6(xyz + 6), load6(xyz + 12)};
    const Pt a = pt_add_mixed(p, load6(CS_GENERATOR_MONT), load6(CS_GENERATOR_MONT + 6));
    fp want[18], mono[GF_COMPONENTS];
    store6(want, a.x); store6(want + 6, a.y); store6(want + 12, a.z);
    generator_fold_monomials(p, mono);
    for (int i = 0; i < GF_OUTPUTS; i++) {
        fp s = 0;
        for (int e = 0; e < GF_COMPONENTS; e++) s = add(s, mul(J[i * GF_COMPONENTS + e], mono[e]));
        if (s != want[i]) { std::printf("%s %ld: output component %d differs\n", what, idx, i); return false; }
    }
    fp alpha[18], beta[18], lambda[GF_LAMBDA_WORDS];
    for (int i = 0; i < 18; i++) { alpha[i] = rnd_fp(); beta[i] = rnd_fp(); }
    generator_fold_lambda(J, alpha, beta, lambda);
    for (int f = 0; f < GF_FUNCTIONALS; f++) {
        fp direct = 0, folded = 0;
        for (int i = gf_first(f); i < gf_last(f); i++) direct = add(direct, mul(f == 0 ? alpha[i] : beta[i], want[i]));
        for (int e = 0; e < GF_COMPONENTS; e++) folded = add(folded, mul(lambda[f * GF_COMPONENTS + e], mono[e]));
        if (direct != folded) { std::printf("%s %ld: functional %d differs\n", what, idx, f); return false; }
    }
    return true;
}

int main() {
    generator_fold_matrix(J);
    long checked = 0;
    fp xyz[18];
    for (long t = 0; t < 1200; t++, checked++) {
        for (int i = 0; i < 18; i++) xyz[i] = rnd_fp();
        if (!check_point(xyz, "random triple", t)) return 1;
    }
    const fp edge[3] = {0, ONE, neg(ONE)}; // 0, 1, p - 1
    // every assignment of one edge value per coordinate (all six components alike): 27 triples
    for (int t = 0; t < 27; t++, checked++) {
        const int pick[3] = {t % 3, (t / 3) % 3, t / 9};
        for (int i = 0; i < 18; i++) xyz[i] = edge[pick[i / 6]];
        if (!check_point(xyz, "uniform edge triple", t)) return 1;
    }
    // every component its own edge value, chosen at random; and random triples with a few components forced to an edge
    for (long t = 0; t < 600; t++, checked++) {
        for (int i = 0; i < 18; i++) xyz[i] = (t & 1) && rnd() % 4 ? rnd_fp() : edge[rnd() % 3];
        if (!check_point(xyz, "mixed edge triple", t)) return 1;
    }
    // the neutral element (0 : 1 : 0) and G itself (the complete formula covers both)
    for (int i = 0; i < 18; i++) xyz[i] = 0;
    xyz[6] = ONE;
    if (!check_point(xyz, "neutral element", 0)) return 1;
    for (int i = 0; i < 12; i++) xyz[i] = CS_GENERATOR_MONT[i];
    for (int i = 12; i < 18; i++) xyz[i] = i == 12 ? ONE : 0;
    if (!check_point(xyz, "generator", 0)) return 1;
    checked += 2;
    std::printf("ok: %ld triples checked\n", checked);
    return 0;
}
