// csrc/transcript.h on its own: the host transcript replayed from a proof's own bytes -- roots, frame, layer roots, remainder and nonce, found
// with parse_layout -- printing every value the coin draws on the way, in canonical form.  tests/test_verify_cpu.py builds this with g++
// (host code only, no GPU) and compares the values with the restated verifier's replay of the same proof (oracle/verifier.py).
// usage: transcript_check <proof file> <transition constraints> <assertions> <public-input word (memory form)>...
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../certificate-stark_amd/csrc/transcript.h"

using namespace cs;

static void line(const char *name, const uint64_t *v, size_t n) { // field elements
    std::printf("%s", name);
    for (size_t i = 0; i < n; i++) std::printf(" %llu", (unsigned long long)host::to_u64(v[i]));
    std::printf("\n");
}
static void line(const char *name, const uint32_t *v, size_t n) {
    std::printf("%s", name);
    for (size_t i = 0; i < n; i++) std::printf(" %u", v[i]);
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> g;
    uint8_t buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) g.insert(g.end(), buf, buf + n);
    std::fclose(f);
    const size_t nc = std::strtoull(argv[2], nullptr, 10), na = std::strtoull(argv[3], nullptr, 10);
    std::vector<uint64_t> pub;
    for (int i = 4; i < argc; i++) pub.push_back(std::strtoull(argv[i], nullptr, 10));

    Layout L;
    if (parse_layout(g.data(), g.size(), L) != CSTARK_PROOF_OK) { std::printf("malformed proof\n"); return 1; }
    const uint8_t *b = g.data();
    const size_t m = L.m, W = L.width, ce = L.ce;
    cstark_options opt;
    memcpy(&opt, L.opt, sizeof opt);

    Coin coin;
    const std::vector<uint8_t> seed = transcript::channel_seed(L.width, L.log_n, opt, L.log_b, ilog2(opt.fri_max_remainder), pub.data(), pub.size());
    transcript::open(coin, opt.hash_fn, seed.data(), seed.size(), b + OFF_ROOTS);

    std::vector<uint64_t> dr(m * transcript::coefficient_draws(nc, na)), sets(dr.size()), flat(dr.size());
    transcript::CoefficientSets cs{};
    uint64_t *at = sets.data();
    for (size_t q = 0; q < m; q++) { cs.ta[q] = at; at += nc; cs.tb[q] = at; at += nc; cs.ba[q] = at; at += na; cs.bb[q] = at; at += na; }
    transcript::draw_coefficients(coin, m, nc, na, dr.data(), cs);
    auto tuples = [&](uint64_t *const set[3], size_t count) { // element-major: the m components of element i side by side
        for (size_t i = 0; i < count; i++)
            for (size_t q = 0; q < m; q++) flat[m * i + q] = set[q][i];
        return flat.data();
    };
    line("t_alpha", tuples(cs.ta, nc), m * nc);
    line("t_beta", tuples(cs.tb, nc), m * nc);
    line("b_alpha", tuples(cs.ba, na), m * na);
    line("b_beta", tuples(cs.bb, na), m * na);

    uint64_t z[3];
    transcript::draw_ood_point(coin, b + OFF_ROOTS + 32, m, z);
    line("z", z, m);

    std::vector<uint64_t> frame((ood_trace_bytes(L) + ood_comp_bytes(L)) / 8); // (a proof's sections are only 4-byte aligned)
    memcpy(frame.data(), b + L.ood, 8 * frame.size());
    transcript::absorb_frame(coin, m, W, ce, frame.data(), frame.data() + 2 * m * W);

    std::vector<uint64_t> ddr(m * transcript::deep_draws(W, ce)), alpha(m * W), beta(m * W), delta(m * ce);
    uint64_t deg_a[3], deg_b[3];
    transcript::draw_deep(coin, m, W, ce, ddr.data(), alpha.data(), beta.data(), delta.data(), deg_a, deg_b);
    line("deep_alpha", alpha.data(), alpha.size());
    line("deep_beta", beta.data(), beta.size());
    line("deep_delta", delta.data(), delta.size());
    line("deg_a", deg_a, m);
    line("deg_b", deg_b, m);

    std::vector<uint64_t> points(m * L.n_layers);
    for (unsigned l = 0; l < L.n_layers; l++) transcript::fri_layer(coin, b + OFF_N_LAYERS + 4 + 32 * l, m, points.data() + m * l);
    line("layer_points", points.data(), points.size());

    std::vector<uint64_t> rem(remainder_bytes(L) / 8);
    memcpy(rem.data(), b + L.rem, 8 * rem.size());
    uint8_t commit[32];
    transcript::commit_remainder(coin, rem.data(), rem.size(), commit);
    if (memcmp(commit, b + off_rem_commit(L), 32) != 0) { std::printf("remainder commitment differs from the proof's\n"); return 1; }

    const uint64_t nonce = rd64(b + L.nonce);
    if (transcript::host_nonce(coin, opt.grinding_factor) != nonce) { std::printf("nonce differs from the sequential search's\n"); return 1; }
    std::vector<uint32_t> pos(L.nq), folded((size_t)L.nq * (L.n_layers + 1));
    uint32_t counts[VMAX_LAYERS] = {};
    transcript::draw_queries(coin, L, nonce, pos.data(), folded.data(), L.nq, counts);
    line("positions", pos.data(), pos.size());
    line("folded_counts", counts, L.n_layers);
    for (unsigned l = 0; l < L.n_layers; l++) {
        if (counts[l] != L.npos[l]) { std::printf("layer %u: %u folded positions, the proof opens %u\n", l, counts[l], L.npos[l]); return 1; }
        char name[32];
        std::snprintf(name, sizeof name, "folded_%u", l);
        line(name, folded.data() + (size_t)L.nq * l, counts[l]);
    }
    return 0;
}
