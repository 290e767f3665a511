// csrc/proof_layout.h on its own: write_proof and parse_layout must agree on every section of every shape, and a proof the library
// wrote (argv[1]: the bytes of tests/golden/proof_2tx_d3.npz) must come back byte for byte when its parsed sections are written again.
// Built and run by tests/test_verify_cpu.py (host code only, no GPU).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../certificate-stark_amd/csrc/proof_layout.h"

using namespace cs;

#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { std::printf("line %d: %s (%s)\n", __LINE__, #cond, what); return false; } \
    } while (0)

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static std::vector<uint8_t> pattern(size_t n) { // fresh bytes for every part: no two parts of a proof look alike
    std::vector<uint8_t> v(n);
    for (uint8_t &x : v) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; x = (uint8_t)(rng >> 24); }
    return v;
}
static bool same(const std::vector<uint8_t> &proof, size_t off, const std::vector<uint8_t> &part) {
    return off + part.size() <= proof.size() && memcmp(proof.data() + off, part.data(), part.size()) == 0;
}

static bool round_trip(uint32_t air, uint32_t log_n, uint32_t ext, uint32_t fold, uint32_t blowup, uint32_t rem, uint32_t nq, bool expect_layers) {
    char what[128];
    std::snprintf(what, sizeof what, "air %u log_n %u ext %u fold %u blowup %u rem %u nq %u", air, log_n, ext, fold, blowup, rem, nq);
    const cstark_options opt{nq, blowup, 5, 1, ext, fold, rem};
    const ProofShape S = proof_shape(air, AIR_WIDTH[air], log_n, air == CSTARK_AIR_STATE_TRANSITION ? 7 : 0, opt);
    CHECK(S.m == ext + 1 && S.ce == AIR_CE[air] && S.f == fold && S.nq == nq && (1u << S.log_N) == (blowup << log_n));
    CHECK((S.n_layers > 1) == expect_layers && (expect_layers || S.n_layers == 0) && S.n_layers <= VMAX_LAYERS);
    CHECK(S.R << (S.n_layers * S.log_f) == 1u << S.log_N && S.R <= rem && (S.n_layers == 0 || S.R * fold > rem));
    uint32_t counts[VMAX_LAYERS];
    for (unsigned l = 0; l < S.n_layers; l++) counts[l] = l % 3 == 2 ? nq : 1 + (nq * (l + 2)) / (2 * l + 5); // below nq, and not all alike
    std::vector<uint8_t> troot = pattern(32), croot = pattern(32), lroots = pattern(32 * S.n_layers), remc = pattern(32);
    std::vector<uint8_t> ood_t = pattern(ood_trace_bytes(S)), ood_c = pattern(ood_comp_bytes(S)), trows = pattern(trace_row_bytes(S));
    std::vector<uint8_t> tpaths = pattern(path_bytes(S)), crows = pattern(comp_row_bytes(S)), cpaths = pattern(path_bytes(S)), remainder = pattern(remainder_bytes(S));
    std::vector<uint8_t> lrows[VMAX_LAYERS], lpaths[VMAX_LAYERS];
    ProofParts p{};
    p.trace_root = troot.data(); p.cons_root = croot.data(); p.layer_roots = lroots.data(); p.rem_commit = remc.data();
    p.ood_trace = ood_t.data(); p.ood_comp = ood_c.data(); p.nonce = 0x0123456789ABCDEFull;
    p.trows = trows.data(); p.tpaths = tpaths.data(); p.crows = crows.data(); p.cpaths = cpaths.data();
    p.counts = counts; p.remainder = remainder.data();
    size_t parts = 52 + 64 + 4 + lroots.size() + 32 + ood_t.size() + ood_c.size() + 8 + trows.size() + 2 * tpaths.size() + crows.size() + 4 + remainder.size();
    for (unsigned l = 0; l < S.n_layers; l++) {
        lrows[l] = pattern(layer_row_bytes(S, counts[l])); lpaths[l] = pattern(layer_path_bytes(S, l, counts[l]));
        p.lrows[l] = lrows[l].data(); p.lpaths[l] = lpaths[l].data();
        parts += 4 + lrows[l].size() + lpaths[l].size();
    }
    const size_t need = proof_size(S, counts);
    CHECK(need == parts); // the sections tile the proof: nothing overlaps, nothing is left out
    std::vector<uint8_t> proof(need + 16, 0xEE);
    size_t len = 0;
    CHECK(write_proof(S, p, proof.data(), proof.size(), &len) == CSTARK_OK && len == need);
    for (size_t i = need; i < proof.size(); i++) CHECK(proof[i] == 0xEE);
    proof.resize(need);

    Layout L;
    CHECK(parse_layout(proof.data(), proof.size(), L) == CSTARK_PROOF_OK);
    CHECK(memcmp(static_cast<const ProofShape *>(&L), &S, sizeof S) == 0);
    CHECK(same(proof, 52, troot) && same(proof, 84, croot) && same(proof, 120, lroots) && same(proof, 120 + lroots.size(), remc));
    CHECK(rd32(proof.data() + 116) == S.n_layers && L.ood == 120 + lroots.size() + 32);
    CHECK(same(proof, L.ood, ood_t) && same(proof, L.ood + ood_t.size(), ood_c) && rd64(proof.data() + L.nonce) == p.nonce);
    CHECK(same(proof, L.trows, trows) && same(proof, L.tpaths, tpaths) && same(proof, L.crows, crows) && same(proof, L.cpaths, cpaths));
    for (unsigned l = 0; l < S.n_layers; l++)
        CHECK(L.npos[l] == counts[l] && rd32(proof.data() + L.lrows[l] - 4) == counts[l] && same(proof, L.lrows[l], lrows[l]) && same(proof, L.lpaths[l], lpaths[l]));
    CHECK(rd32(proof.data() + L.rem - 4) == S.R && same(proof, L.rem, remainder) && L.rem + remainder.size() == need);
    CHECK(parse_layout(proof.data(), need - 1, L) == CSTARK_PROOF_MALFORMED);

    // one byte short, or no buffer at all: nothing is written, the needed length is reported
    std::vector<uint8_t> small(need - 1, 0xAB);
    len = 0;
    CHECK(write_proof(S, p, small.data(), small.size(), &len) == CSTARK_ERR_INVALID_ARG && len == need);
    for (uint8_t x : small) CHECK(x == 0xAB);
    len = 0;
    CHECK(write_proof(S, p, nullptr, need, &len) == CSTARK_ERR_INVALID_ARG && len == need);
    return true;
}

static bool golden_round_trip(const char *path) {
    const char *what = path;
    FILE *f = std::fopen(path, "rb");
    CHECK(f != nullptr);
    std::vector<uint8_t> g;
    uint8_t buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) g.insert(g.end(), buf, buf + n);
    std::fclose(f);
    Layout L;
    CHECK(parse_layout(g.data(), g.size(), L) == CSTARK_PROOF_OK);
    const uint8_t *b = g.data();
    ProofParts p{};
    p.trace_root = b + 52; p.cons_root = b + 84; p.layer_roots = b + 120; p.rem_commit = b + 120 + 32 * L.n_layers;
    p.ood_trace = b + L.ood; p.ood_comp = b + L.ood + ood_trace_bytes(L); p.nonce = rd64(b + L.nonce);
    p.trows = b + L.trows; p.tpaths = b + L.tpaths; p.crows = b + L.crows; p.cpaths = b + L.cpaths;
    p.counts = L.npos; p.remainder = b + L.rem;
    for (unsigned l = 0; l < L.n_layers; l++) { p.lrows[l] = b + L.lrows[l]; p.lpaths[l] = b + L.lpaths[l]; }
    cstark_options opt;
    memcpy(&opt, L.opt, sizeof opt);
    const ProofShape S = proof_shape(L.air, L.width, L.log_n, L.word, opt); // from the header alone, as a prover makes it
    std::vector<uint8_t> again(g.size(), 0);
    size_t len = 0;
    CHECK(write_proof(S, p, again.data(), again.size(), &len) == CSTARK_OK && len == g.size());
    CHECK(again == g);
    return true;
}

int main(int argc, char **argv) {
    int shapes = 0;
    for (uint32_t air = 0; air < 5; air++)
        for (uint32_t ext = 0; ext < 3; ext++)
            for (uint32_t fold : {4u, 8u, 16u}) {
                const uint32_t ce = AIR_CE[air];
                // several layers: a 2^12 trace at blowup 16 down to a remainder of at most 128
                if (!round_trip(air, 12, ext, fold, 16, 128, 27 + air, true)) return 1;
                shapes++;
                // no layer: the LDE domain is the remainder (TransactionAir has at least 2^10 rows at blowup 8: always layers)
                if (air != CSTARK_AIR_STATE_TRANSITION) {
                    if (!round_trip(air, 6, ext, fold, ce < 2 ? 2 : ce, 1024, 5, false)) return 1;
                    shapes++;
                }
            }
    if (argc > 1 && !golden_round_trip(argv[1])) return 1;
    std::printf("ok %d shapes%s\n", shapes, argc > 1 ? ", golden proof rewritten byte for byte" : "");
    return 0;
}
