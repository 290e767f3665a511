// convert_proof and convert_bound of csrc/proof_layout.h on their own (g++, host code only): the plain and the compact proof of the same
// synthetic parts are written by write_proof and parsed; each is then converted with the path sections taken from the OTHER one's parsed
// layout and must come out as the other's bytes -- so the two writers agree on everything outside the path sections, on the count words
// and on the magic.  A proof already in the target form is copied through, the bound is the plain length (plus one count word per tree
// for the compact form), and a buffer one byte short is left untouched.  Built and run by tests/test_convert_bound_cpu.py.
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
static uint64_t next() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }
static std::vector<uint8_t> pattern(size_t n) {
    std::vector<uint8_t> v(n);
    for (uint8_t &x : v) x = (uint8_t)(next() >> 24);
    return v;
}
// the "digest" of node (level, index) of tree t: every query below a node states the same sibling
static void node_bytes(unsigned t, unsigned level, uint64_t index, uint8_t *out) {
    uint64_t s = 0xD1B54A32D192ED03ull * (t + 1) ^ ((uint64_t)level << 56) ^ index;
    for (int i = 0; i < 32; i++) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; out[i] = (uint8_t)(s >> 32); }
}
static std::vector<uint8_t> paths_of(unsigned t, unsigned depth, const std::vector<uint32_t> &pos) {
    std::vector<uint8_t> p(32 * pos.size() * depth);
    for (size_t q = 0; q < pos.size(); q++)
        for (unsigned j = 0; j < depth; j++) node_bytes(t, depth - j, (pos[q] >> j) ^ 1, &p[32 * (q * depth + j)]);
    return p;
}
// np positions below 2^depth: distinct or, with `repeat`, every third one equal to an earlier one
static std::vector<uint32_t> positions(unsigned depth, uint32_t np, bool repeat) {
    std::vector<uint32_t> pos;
    while (pos.size() < np) {
        if (repeat && pos.size() % 3 == 2) { pos.push_back(pos[pos.size() / 2]); continue; }
        const uint32_t v = (uint32_t)(next() >> 20) & ((1u << depth) - 1);
        bool fresh = true;
        for (uint32_t u : pos) fresh = fresh && u != v;
        if (fresh) pos.push_back(v);
    }
    return pos;
}
// the path sections of a parsed proof, as convert_proof takes them
static PathSections sections_of(const std::vector<uint8_t> &proof, const Layout &L) {
    PathSections ps{};
    for (unsigned t = 0; t < 2 + L.n_layers; t++) {
        const TreeSection s = tree_section(L, t);
        ps.data[t] = proof.data() + (L.form == CSTARK_FORM_COMPACT ? s.at + 4 : s.at);
        ps.nodes[t] = L.form == CSTARK_FORM_COMPACT ? L.nodes[t] : 0xDEADBEEFu; // to the plain form the counts are not read
    }
    return ps;
}

static bool round_trip(uint32_t air, uint32_t log_n, uint32_t ext, uint32_t fold, uint32_t blowup, uint32_t rem, uint32_t nq, bool repeat) {
    char what[160];
    std::snprintf(what, sizeof what, "air %u log_n %u ext %u fold %u blowup %u rem %u nq %u repeat %d", air, log_n, ext, fold, blowup, rem, nq, (int)repeat);
    const cstark_options opt{nq, blowup, 0, 0, ext, fold, rem};
    const ProofShape S = proof_shape(air, AIR_WIDTH[air], log_n, air == CSTARK_AIR_STATE_TRANSITION ? 7 : 0, opt);
    CHECK(S.n_layers <= VMAX_LAYERS);
    const unsigned trees = 2 + S.n_layers;
    const std::vector<uint32_t> pos = positions(S.log_N, nq, repeat);
    std::vector<uint32_t> lpos[VMAX_LAYERS];
    uint32_t counts[VMAX_LAYERS] = {};
    const std::vector<uint32_t> *prev = &pos;
    for (unsigned l = 0; l < S.n_layers; l++) { // the distinct residues, in order of first appearance
        const uint32_t mask = (1u << layer_log_rows(S, l)) - 1;
        for (uint32_t p : *prev) {
            bool fresh = true;
            for (uint32_t u : lpos[l]) fresh = fresh && u != (p & mask);
            if (fresh) lpos[l].push_back(p & mask);
        }
        counts[l] = (uint32_t)lpos[l].size();
        prev = &lpos[l];
    }
    std::vector<uint8_t> troot = pattern(32), croot = pattern(32), lroots = pattern(32 * S.n_layers), remc = pattern(32);
    std::vector<uint8_t> ood_t = pattern(ood_trace_bytes(S)), ood_c = pattern(ood_comp_bytes(S)), trows = pattern(trace_row_bytes(S));
    std::vector<uint8_t> crows = pattern(comp_row_bytes(S)), remainder = pattern(remainder_bytes(S));
    std::vector<uint8_t> tpaths = paths_of(0, S.log_N, pos), cpaths = paths_of(1, S.log_N, pos);
    std::vector<uint8_t> lrows[VMAX_LAYERS], lpaths[VMAX_LAYERS];
    ProofParts p{};
    p.trace_root = troot.data(); p.cons_root = croot.data(); p.layer_roots = lroots.data(); p.rem_commit = remc.data();
    p.ood_trace = ood_t.data(); p.ood_comp = ood_c.data(); p.nonce = 0x0123456789ABCDEFull;
    p.trows = trows.data(); p.tpaths = tpaths.data(); p.crows = crows.data(); p.cpaths = cpaths.data();
    p.counts = counts; p.remainder = remainder.data(); p.pos = pos.data();
    for (unsigned l = 0; l < S.n_layers; l++) {
        lrows[l] = pattern(layer_row_bytes(S, counts[l])); lpaths[l] = paths_of(2 + l, layer_log_rows(S, l), lpos[l]);
        p.lrows[l] = lrows[l].data(); p.lpaths[l] = lpaths[l].data(); p.lpos[l] = lpos[l].data();
    }
    size_t len = 0;
    std::vector<uint8_t> plain(proof_size(S, counts)), compact(proof_size_bound(S, CSTARK_FORM_COMPACT));
    p.form = CSTARK_FORM_PLAIN;
    CHECK(write_proof(S, p, plain.data(), plain.size(), &len) == CSTARK_OK && len == plain.size());
    p.form = CSTARK_FORM_COMPACT;
    CHECK(write_proof(S, p, compact.data(), compact.size(), &len) == CSTARK_OK && len <= compact.size());
    compact.resize(len);
    Layout LP, LC;
    CHECK(parse_layout(plain.data(), plain.size(), LP) == CSTARK_PROOF_OK && LP.form == CSTARK_FORM_PLAIN);
    CHECK(parse_layout(compact.data(), compact.size(), LC) == CSTARK_PROOF_OK && LC.form == CSTARK_FORM_COMPACT);

    // ---- the bound: from either form, the plain length (+ a count word per tree)
    for (const Layout *L : {&LP, &LC}) {
        CHECK(convert_bound(*L, CSTARK_FORM_PLAIN) == plain.size());
        CHECK(convert_bound(*L, CSTARK_FORM_COMPACT) == plain.size() + 4 * trees);
    }
    CHECK(compact.size() <= convert_bound(LP, CSTARK_FORM_COMPACT));

    // ---- plain -> compact with the compact proof's nodes, compact -> plain with the plain proof's paths
    const PathSections nodes = sections_of(compact, LC), paths = sections_of(plain, LP);
    std::vector<uint8_t> out(convert_bound(LP, CSTARK_FORM_COMPACT) + 16, 0xEE);
    CHECK(convert_proof(plain.data(), LP, CSTARK_FORM_COMPACT, nodes, out.data(), convert_bound(LP, CSTARK_FORM_COMPACT), &len) == CSTARK_OK);
    CHECK(len == compact.size() && memcmp(out.data(), compact.data(), len) == 0);
    for (size_t i = len; i < out.size(); i++) CHECK(out[i] == 0xEE);
    out.assign(plain.size() + 16, 0xEE);
    CHECK(convert_proof(compact.data(), LC, CSTARK_FORM_PLAIN, paths, out.data(), plain.size(), &len) == CSTARK_OK);
    CHECK(len == plain.size() && memcmp(out.data(), plain.data(), len) == 0);
    for (size_t i = len; i < out.size(); i++) CHECK(out[i] == 0xEE);

    // ---- already in the target form: copied through, the sections are not read
    const PathSections none{};
    out.assign(plain.size(), 0xEE);
    CHECK(convert_proof(plain.data(), LP, CSTARK_FORM_PLAIN, none, out.data(), out.size(), &len) == CSTARK_OK && len == plain.size() && out == plain);
    out.assign(compact.size(), 0xEE);
    CHECK(convert_proof(compact.data(), LC, CSTARK_FORM_COMPACT, none, out.data(), out.size(), &len) == CSTARK_OK && len == compact.size() && out == compact);

    // ---- one byte short, or no buffer: nothing is written, the needed length is reported
    std::vector<uint8_t> small(compact.size() - 1, 0xAB);
    len = 0;
    CHECK(convert_proof(plain.data(), LP, CSTARK_FORM_COMPACT, nodes, small.data(), small.size(), &len) == CSTARK_ERR_INVALID_ARG && len == compact.size());
    for (uint8_t x : small) CHECK(x == 0xAB);
    small.assign(plain.size() - 1, 0xAB);
    CHECK(convert_proof(compact.data(), LC, CSTARK_FORM_PLAIN, paths, small.data(), small.size(), &len) == CSTARK_ERR_INVALID_ARG && len == plain.size());
    for (uint8_t x : small) CHECK(x == 0xAB);
    CHECK(convert_proof(plain.data(), LP, CSTARK_FORM_PLAIN, none, small.data(), small.size(), &len) == CSTARK_ERR_INVALID_ARG && len == plain.size());
    for (uint8_t x : small) CHECK(x == 0xAB);
    CHECK(convert_proof(compact.data(), LC, CSTARK_FORM_PLAIN, paths, nullptr, plain.size(), &len) == CSTARK_ERR_INVALID_ARG && len == plain.size());
    return true;
}

int main() {
    int shapes = 0;
    for (uint32_t air = 0; air < 5; air++)
        for (uint32_t ext = 0; ext < 3; ext++)
            for (uint32_t fold : {4u, 8u, 16u}) {
                const uint32_t ce = AIR_CE[air];
                if (!round_trip(air, 12, ext, fold, 16, 128, 27 + air, false)) return 1;             // several layers
                if (!round_trip(air, 10, ext, fold, 8, 128, 128, (air + ext) % 2 == 1)) return 1;      // 128 queries; repeats
                shapes += 2;
                if (air != CSTARK_AIR_STATE_TRANSITION) {                                              // no layer: two trees only
                    if (!round_trip(air, 6, ext, fold, ce < 2 ? 2 : ce, 1024, 5, false)) return 1;
                    if (!round_trip(air, 6, ext, fold, ce < 2 ? 2 : ce, 1024, 1, false)) return 1;     // one query: the multiproof is its path
                    shapes += 2;
                }
            }
    std::printf("ok %d shapes\n", shapes);
    return 0;
}
