// The compact form of csrc/proof_layout.h on its own (g++, host code only): write_proof's selection of each tree's multiproof from
// synthetic per-query paths must equal an independent walk over sets, parse_layout must return the offsets the writer used, the plain
// and the compact proof of the same parts must agree outside the path sections, and the parser must refuse what it has to.
// Built and run by tests/test_compact_reference_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>
#include "../../certificate-stark_amd/csrc/proof_layout.h"

using namespace cs;

#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { std::printf("line %d: %s (%s)\n", __LINE__, #cond, what); return false; } \
    } while (0)

static uint64_t rng = 0x2545F4914F6CDD1Dull;
static uint64_t next() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }
static std::vector<uint8_t> pattern(size_t n) {
    std::vector<uint8_t> v(n);
    for (uint8_t &x : v) x = (uint8_t)(next() >> 24);
    return v;
}
// the "digest" of node (level, index) of tree t: a function of the three alone, so every query below a node states the same sibling
static void node_bytes(unsigned t, unsigned level, uint64_t index, uint8_t *out) {
    uint64_t s = 0x9E3779B97F4A7C15ull * (t + 1) ^ ((uint64_t)level << 56) ^ index;
    for (int i = 0; i < 32; i++) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; out[i] = (uint8_t)(s >> 32); }
}
// paths [np][depth][32] of the positions, siblings leaf-upwards
static std::vector<uint8_t> paths_of(unsigned t, unsigned depth, const std::vector<uint32_t> &pos) {
    std::vector<uint8_t> p(32 * pos.size() * depth);
    for (size_t q = 0; q < pos.size(); q++)
        for (unsigned j = 0; j < depth; j++) node_bytes(t, depth - j, (pos[q] >> j) ^ 1, &p[32 * (q * depth + j)]);
    return p;
}
// the multiproof by the definition, over sets (no code shared with multiproof_plan.h)
static std::vector<uint8_t> multiproof_of(unsigned t, unsigned depth, const std::vector<uint32_t> &pos) {
    std::set<uint64_t> k(pos.begin(), pos.end());
    std::vector<uint8_t> out;
    for (unsigned l = depth; l >= 1; l--) {
        std::set<uint64_t> up;
        for (uint64_t x : k) {
            if (!k.count(x ^ 1)) { out.resize(out.size() + 32); node_bytes(t, l, x ^ 1, &out[out.size() - 32]); }
            up.insert(x >> 1);
        }
        k.swap(up);
    }
    return out;
}
static bool same(const std::vector<uint8_t> &proof, size_t off, const std::vector<uint8_t> &part) {
    return off + part.size() <= proof.size() && (part.empty() || memcmp(proof.data() + off, part.data(), part.size()) == 0);
}
// np positions below 2^depth: distinct or, with `repeat`, every third one equal to an earlier one (CSTARK_CONV_QUERY_DEDUP off)
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

static bool round_trip(uint32_t air, uint32_t log_n, uint32_t ext, uint32_t fold, uint32_t blowup, uint32_t rem, uint32_t nq, bool repeat, bool every_cut) {
    char what[160];
    std::snprintf(what, sizeof what, "air %u log_n %u ext %u fold %u blowup %u rem %u nq %u repeat %d", air, log_n, ext, fold, blowup, rem, nq, (int)repeat);
    const cstark_options opt{nq, blowup, 0, 0, ext, fold, rem};
    const ProofShape S = proof_shape(air, AIR_WIDTH[air], log_n, air == CSTARK_AIR_STATE_TRANSITION ? 7 : 0, opt);
    CHECK(S.n_layers <= VMAX_LAYERS);
    const std::vector<uint32_t> pos = positions(S.log_N, nq, repeat);
    std::vector<uint32_t> lpos[VMAX_LAYERS];
    uint32_t counts[VMAX_LAYERS] = {};
    {   // the folded positions of every layer: the distinct residues, in order of first appearance (transcript.h: draw_queries)
        const std::vector<uint32_t> *prev = &pos;
        for (unsigned l = 0; l < S.n_layers; l++) {
            const uint32_t mask = (1u << layer_log_rows(S, l)) - 1;
            for (uint32_t p : *prev) {
                bool fresh = true;
                for (uint32_t u : lpos[l]) fresh = fresh && u != (p & mask);
                if (fresh) lpos[l].push_back(p & mask);
            }
            counts[l] = (uint32_t)lpos[l].size();
            prev = &lpos[l];
        }
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
    // the plain proof of these parts, then the compact one
    std::vector<uint8_t> plain(proof_size(S, counts));
    size_t len = 0;
    p.form = CSTARK_FORM_PLAIN;
    CHECK(write_proof(S, p, plain.data(), plain.size(), &len) == CSTARK_OK && len == plain.size());
    Layout LP;
    CHECK(parse_layout(plain.data(), plain.size(), LP) == CSTARK_PROOF_OK && LP.form == CSTARK_FORM_PLAIN);

    std::vector<uint8_t> want[MAX_TREES];
    want[0] = multiproof_of(0, S.log_N, pos); want[1] = multiproof_of(1, S.log_N, pos);
    for (unsigned l = 0; l < S.n_layers; l++) want[2 + l] = multiproof_of(2 + l, layer_log_rows(S, l), lpos[l]);
    size_t need = plain.size() + 4 * (2 + S.n_layers);
    for (unsigned t = 0; t < 2 + S.n_layers; t++) need += want[t].size();
    need -= 2 * path_bytes(S);
    for (unsigned l = 0; l < S.n_layers; l++) need -= layer_path_bytes(S, l, counts[l]);

    p.form = CSTARK_FORM_COMPACT;
    std::vector<uint8_t> proof(need + 16, 0xEE);
    CHECK(write_proof(S, p, proof.data(), proof.size(), &len) == CSTARK_OK);
    CHECK(len == need && len <= proof_size_bound(S, CSTARK_FORM_COMPACT));
    for (size_t i = need; i < proof.size(); i++) CHECK(proof[i] == 0xEE);
    proof.resize(need);
    CHECK(proof_form_of(proof.data(), proof.size()) == CSTARK_FORM_COMPACT && proof_form_of(plain.data(), plain.size()) == CSTARK_FORM_PLAIN);

    Layout L;
    CHECK(parse_layout(proof.data(), proof.size(), L) == CSTARK_PROOF_OK && L.form == CSTARK_FORM_COMPACT);
    CHECK(memcmp(static_cast<const ProofShape *>(&L), &S, sizeof S) == 0);
    // everything up to the end of the trace rows is the plain proof's but for the magic; the rows and the remainder are where the parser says
    CHECK(memcmp(proof.data(), "CSTC", 4) == 0 && memcmp(proof.data() + 4, plain.data() + 4, LP.tpaths - 4) == 0 && L.trows == LP.trows);
    CHECK(same(proof, L.trows, trows) && same(proof, L.crows, crows) && same(proof, L.rem, remainder) && L.rem + remainder.size() == need);
    CHECK(rd32(proof.data() + L.tpaths - 4) == want[0].size() / 32 && L.nodes[0] == want[0].size() / 32 && same(proof, L.tpaths, want[0]));
    CHECK(rd32(proof.data() + L.cpaths - 4) == want[1].size() / 32 && L.nodes[1] == want[1].size() / 32 && same(proof, L.cpaths, want[1]));
    CHECK(L.crows == L.tpaths + want[0].size());
    for (unsigned l = 0; l < S.n_layers; l++) {
        CHECK(L.npos[l] == counts[l] && rd32(proof.data() + L.lrows[l] - 4) == counts[l] && same(proof, L.lrows[l], lrows[l]));
        CHECK(L.nodes[2 + l] == want[2 + l].size() / 32 && rd32(proof.data() + L.lpaths[l] - 4) == L.nodes[2 + l] && same(proof, L.lpaths[l], want[2 + l]));
    }
    CHECK(rd32(proof.data() + L.rem - 4) == S.R);
    // a multiproof never holds more nodes than the paths it was selected from, and fewer once two positions share an ancestor below the root
    CHECK(want[0].size() <= tpaths.size() && (nq < 2 || want[0].size() < tpaths.size()));

    // ---- what the parser refuses
    Layout X;
    std::vector<uint8_t> t = proof;
    t.push_back(0);
    CHECK(parse_layout(t.data(), t.size(), X) == CSTARK_PROOF_MALFORMED); // one trailing byte
    if (every_cut)
        for (size_t cut = 0; cut < need; cut++) CHECK(parse_layout(proof.data(), cut, X) == CSTARK_PROOF_MALFORMED);
    else
        for (size_t cut : {(size_t)0, (size_t)3, (size_t)51, L.tpaths - 4, L.tpaths - 1, L.tpaths, L.crows, L.cpaths + 31, L.rem - 4, need - 1})
            CHECK(parse_layout(proof.data(), cut, X) == CSTARK_PROOF_MALFORMED);
    t = proof;
    const uint32_t over = nq * S.log_N + 1; // above n_positions * depth: refused before it sizes anything
    memcpy(t.data() + L.tpaths - 4, &over, 4);
    CHECK(parse_layout(t.data(), t.size(), X) == CSTARK_PROOF_MALFORMED);
    t = proof;
    const uint32_t huge = 0xffffffffu;
    memcpy(t.data() + L.cpaths - 4, &huge, 4);
    CHECK(parse_layout(t.data(), t.size(), X) == CSTARK_PROOF_MALFORMED);
    // a node count that stays within its bound but is not the section's: the total length no longer matches
    t = proof;
    const uint32_t off_by_one = L.nodes[0] + 1;
    if (off_by_one <= nq * S.log_N) {
        memcpy(t.data() + L.tpaths - 4, &off_by_one, 4);
        CHECK(parse_layout(t.data(), t.size(), X) == CSTARK_PROOF_MALFORMED);
    }
    // each body under the other magic (these shapes: the lengths differ, so neither parses)
    if (need != plain.size()) {
        t = proof; memcpy(t.data(), "CSTK", 4);
        CHECK(parse_layout(t.data(), t.size(), X) == CSTARK_PROOF_MALFORMED);
        t = plain; memcpy(t.data(), "CSTC", 4);
        CHECK(parse_layout(t.data(), t.size(), X) == CSTARK_PROOF_MALFORMED);
    }
    t = proof; memcpy(t.data(), "CSTX", 4);
    CHECK(parse_layout(t.data(), t.size(), X) == CSTARK_PROOF_MALFORMED && proof_form_of(t.data(), t.size()) == -1);

    // one byte short, or no buffer at all: nothing is written, the needed length is reported
    std::vector<uint8_t> small(need - 1, 0xAB);
    len = 0;
    CHECK(write_proof(S, p, small.data(), small.size(), &len) == CSTARK_ERR_INVALID_ARG && len == need);
    for (uint8_t x : small) CHECK(x == 0xAB);
    return true;
}

int main() {
    int shapes = 0;
    for (uint32_t air = 0; air < 5; air++)
        for (uint32_t ext = 0; ext < 3; ext++)
            for (uint32_t fold : {4u, 8u, 16u}) {
                const uint32_t ce = AIR_CE[air];
                if (!round_trip(air, 12, ext, fold, 16, 128, 27 + air, false, false)) return 1; // several layers
                if (!round_trip(air, 10, ext, fold, 8, 128, 128, (air + ext) % 2 == 1, false)) return 1; // 128 queries: dense upper layers; repeats
                shapes += 2;
                if (air != CSTARK_AIR_STATE_TRANSITION) { // no layer: two trees only; every truncation length
                    if (!round_trip(air, 6, ext, fold, ce < 2 ? 2 : ce, 1024, 5, false, true)) return 1;
                    if (!round_trip(air, 6, ext, fold, ce < 2 ? 2 : ce, 1024, 1, false, false)) return 1; // one query: the multiproof is its path
                    shapes += 2;
                }
            }
    std::printf("ok %d shapes\n", shapes);
    return 0;
}
