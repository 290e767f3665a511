// The byte layout of a proof, once: the shape that fixes it, the walk over its sections, the writer the provers use (prove.hip) and
// the parser the verifier and cstark_proof_inspect use (verify.hip).  The format itself is stated in include/cstark.h ("Proof
// layout"); nothing else under csrc/ knows it.  Host code only (no HIP): tests/cpp/proof_layout_check.cpp builds it with g++.
// Two forms share everything but the path sections: the plain form ("CSTK") holds one authentication path per opened row, the compact
// form ("CSTC") one Merkle multiproof per tree (multiproof_plan.h states the definition; tests/cpp/proof_compact_check.cpp checks it).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/cstark.h"
#include "hostfield.h"
#include "multiproof_plan.h"

namespace cs {

constexpr uint32_t VMAX_LAYERS = 16;
// per AIR (CSTARK_AIR_*): trace width, composition columns (= the constraint-evaluation blowup)
constexpr uint32_t AIR_WIDTH[5] = {94, 65, 56, 2, 14}, AIR_CE[5] = {8, 4, 8, 2, 4};

inline uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline uint64_t rd64(const uint8_t *p) { uint64_t v; memcpy(&v, p, 8); return v; }
inline unsigned ilog2(uint32_t v) { unsigned l = 0; while ((1u << (l + 1)) <= v) l++; return l; }

// What fixes the size of every section but the FRI layers' (those also depend on the number of distinct folded positions).
struct ProofShape {
    uint32_t air, width, log_n, word, opt[7];                // the header: word = Merkle depth / signature count / 0; opt = cstark_options
    uint32_t nq, log_b, log_f, f, m, ce, log_N, n_layers, R; // derived: m words per drawn-field element, ce composition columns, R remainder length
};
// the derived half from a header whose options are valid (check_options in prove.hip, parse_layout below)
inline void shape_derive(ProofShape &S) {
    S.ce = AIR_CE[S.air];
    S.nq = S.opt[0]; S.log_b = ilog2(S.opt[1]); S.log_f = ilog2(S.opt[5]); S.f = S.opt[5]; S.m = S.opt[4] + 1; S.log_N = S.log_n + S.log_b;
    unsigned lg = S.log_N, nl = 0;
    const unsigned log_rem = ilog2(S.opt[6]);
    while (lg > log_rem) { lg -= S.log_f; nl++; }
    S.n_layers = nl; S.R = 1u << lg;
}
inline ProofShape proof_shape(uint32_t air, uint32_t width, uint32_t log_n, uint32_t word, const cstark_options &o) {
    ProofShape S{air, width, log_n, word, {o.num_queries, o.blowup_factor, o.grinding_factor, o.hash_fn, o.field_extension, o.fri_folding_factor, o.fri_max_remainder}};
    shape_derive(S);
    return S;
}

// ---- sections: sizes in bytes --------------------------------------------------------------------------------------------------
// header (52 bytes: magic, version, air, width, log_n, word, 7 options) | trace root | constraint root | n_layers | layer roots |
// remainder commitment | everything below
constexpr size_t OFF_ROOTS = 52, OFF_N_LAYERS = 116;
inline size_t off_rem_commit(const ProofShape &S) { return OFF_N_LAYERS + 4 + 32 * (size_t)S.n_layers; }
inline size_t ood_trace_bytes(const ProofShape &S) { return 8 * 2 * (size_t)S.width * S.m; }
inline size_t ood_comp_bytes(const ProofShape &S) { return 8 * (size_t)S.ce * S.m; }
inline size_t trace_row_bytes(const ProofShape &S) { return 8 * (size_t)S.nq * S.width; }
inline size_t comp_row_bytes(const ProofShape &S) { return 8 * (size_t)S.nq * S.ce * S.m; }
inline size_t path_bytes(const ProofShape &S) { return 32 * (size_t)S.nq * S.log_N; } // trace and composition trees alike
inline unsigned layer_log_rows(const ProofShape &S, unsigned l) { return S.log_N - (l + 1) * S.log_f; }
inline size_t layer_row_bytes(const ProofShape &S, uint32_t np) { return 8 * (size_t)np * S.f * S.m; }
inline size_t layer_path_bytes(const ProofShape &S, unsigned l, uint32_t np) { return 32 * (size_t)np * layer_log_rows(S, l); }
inline size_t remainder_bytes(const ProofShape &S) { return 8 * (size_t)S.R * S.m; }

constexpr uint32_t MAX_TREES = 2 + VMAX_LAYERS; // tree 0: the trace, 1: the composition, 2 + l: FRI layer l
struct Layout : ProofShape {
    size_t ood, nonce, trows, tpaths, crows, cpaths, lrows[VMAX_LAYERS], lpaths[VMAX_LAYERS], rem; // offsets of the sections
    uint32_t npos[VMAX_LAYERS];                                                                    // opened positions per layer
    // compact form: tpaths, cpaths and lpaths[l] are the offsets of the first node (behind the section's count word)
    uint32_t form, nodes[MAX_TREES];
};
// The walk, in three steps so that the parser can check each count word before it sizes anything: every step takes the offset where
// its part begins and returns where the next begins (layers and tail: at their u32 count word).
inline size_t walk_fixed(Layout &L) {
    size_t o = off_rem_commit(L) + 32;
    L.ood = o; o += ood_trace_bytes(L) + ood_comp_bytes(L);
    L.nonce = o; o += 8;
    L.trows = o; o += trace_row_bytes(L);
    L.tpaths = o; o += path_bytes(L);
    L.crows = o; o += comp_row_bytes(L);
    L.cpaths = o; o += path_bytes(L);
    return o;
}
inline size_t walk_layer(Layout &L, unsigned l, uint32_t np, size_t o) {
    L.npos[l] = np;
    o += 4;
    L.lrows[l] = o; o += layer_row_bytes(L, np);
    L.lpaths[l] = o; o += layer_path_bytes(L, l, np);
    return o;
}
inline size_t walk_tail(Layout &L, size_t o) {
    o += 4;
    L.rem = o;
    return o + remainder_bytes(L);
}
// all of it for known counts (counts[l] opened positions in layer l); returns the proof's length
inline size_t walk(const ProofShape &S, const uint32_t *counts, Layout &L) {
    static_cast<ProofShape &>(L) = S;
    size_t o = walk_fixed(L);
    for (unsigned l = 0; l < S.n_layers; l++) o = walk_layer(L, l, counts[l], o);
    return walk_tail(L, o);
}

// ---- the compact form ------------------------------------------------------------------------------------------------------------
// The same walk with every path section replaced by u32 n_nodes | nodes[n_nodes][32].  The counts come from `src`, which answers at the
// offset of each count word: the parser reads and bounds them there, the writer states the ones it selected.
//     bool positions(size_t o, unsigned l, uint32_t &np)                          layer l's u32 n_positions
//     bool nodes(size_t o, uint32_t np, unsigned depth, uint32_t &n)              a tree's u32 n_nodes (np rows opened, depth levels)
//     bool tail(size_t o)                                                         u32 remainder_len
// false: src refused a count.  *end: the proof's length.
template <class Src> inline bool walk_compact(Layout &L, Src &&src, size_t *end) {
    L.form = CSTARK_FORM_COMPACT;
    size_t o = off_rem_commit(L) + 32;
    L.ood = o; o += ood_trace_bytes(L) + ood_comp_bytes(L);
    L.nonce = o; o += 8;
    L.trows = o; o += trace_row_bytes(L);
    if (!src.nodes(o, L.nq, L.log_N, L.nodes[0])) return false;
    L.tpaths = o + 4; o = L.tpaths + 32 * (size_t)L.nodes[0];
    L.crows = o; o += comp_row_bytes(L);
    if (!src.nodes(o, L.nq, L.log_N, L.nodes[1])) return false;
    L.cpaths = o + 4; o = L.cpaths + 32 * (size_t)L.nodes[1];
    for (unsigned l = 0; l < L.n_layers; l++) {
        if (!src.positions(o, l, L.npos[l])) return false;
        o += 4;
        L.lrows[l] = o; o += layer_row_bytes(L, L.npos[l]);
        if (!src.nodes(o, L.npos[l], layer_log_rows(L, l), L.nodes[2 + l])) return false;
        L.lpaths[l] = o + 4; o = L.lpaths[l] + 32 * (size_t)L.nodes[2 + l];
    }
    if (!src.tail(o)) return false;
    o += 4;
    L.rem = o;
    *end = o + remainder_bytes(L);
    return true;
}

// The multiproof of one tree by selection from the gathered paths: paths [np][depth][32] in proof order, path q the siblings of
// pos[q] leaf-upwards, so node (l, x ^ 1) is entry depth - l of the path of any query below x.  Positions may repeat (the multiproof is
// over the distinct ones).  The nodes go to `out` in the canonical order (room for np * depth of them: a multiproof never holds more
// nodes than the paths it is selected from); returns their number.
inline uint32_t select_multiproof(unsigned depth, uint32_t np, const uint32_t *pos, const uint8_t *paths, uint8_t *out) {
    std::vector<std::pair<uint32_t, uint32_t>> order(np); // (position, query)
    for (uint32_t q = 0; q < np; q++) order[q] = {pos[q], q};
    std::sort(order.begin(), order.end());
    std::vector<uint64_t> k;      // K_l, ascending
    std::vector<uint32_t> below;  // a query below each entry of K_l
    for (uint32_t i = 0; i < np; i++)
        if (i == 0 || order[i].first != order[i - 1].first) { k.push_back(order[i].first); below.push_back(order[i].second); }
    uint32_t n = 0;
    for (unsigned l = depth; l >= 1; l--)
        multi::detail::walk_level(
            k, [&](size_t i, size_t, size_t m) { below[m] = below[i]; }, // m <= i: the entries still to be read are untouched
            [&](size_t i, size_t m) {
                memcpy(out + 32 * (size_t)n++, paths + 32 * ((size_t)below[i] * depth + (depth - l)), 32);
                below[m] = below[i];
            });
    return n;
}

// ---- writer ----------------------------------------------------------------------------------------------------------------------
// The pieces a prover has in hand.  Rows and paths are the gathered openings in proof order; counts[l] of them in layer l.
struct ProofParts {
    const uint8_t *trace_root, *cons_root, *layer_roots, *rem_commit;
    const void *ood_trace, *ood_comp; // T(z) | T(z w), then H_i(z^ce)
    uint64_t nonce;
    const uint8_t *trows, *tpaths, *crows, *cpaths;
    const uint32_t *counts;
    const uint8_t *lrows[VMAX_LAYERS], *lpaths[VMAX_LAYERS];
    const void *remainder;
    // CSTARK_FORM_COMPACT also needs the opened positions, in proof order: pos [nq] of the trace and composition trees, lpos[l] [counts[l]]
    uint32_t form;
    const uint32_t *pos, *lpos[VMAX_LAYERS];
};
inline size_t proof_size(const ProofShape &S, const uint32_t *counts) {
    Layout L;
    return walk(S, counts, L);
}
// a capacity that holds the proof of this shape in either form whatever the positions: nq distinct positions in every layer, and a
// multiproof never holds more nodes than the paths it was selected from
inline size_t proof_size_bound(const ProofShape &S, uint32_t form) {
    uint32_t all_nq[VMAX_LAYERS];
    for (unsigned l = 0; l < VMAX_LAYERS; l++) all_nq[l] = S.nq;
    return proof_size(S, all_nq) + (form == CSTARK_FORM_COMPACT ? 4 * (size_t)(2 + S.n_layers) : 0);
}
// The proof bytes go straight into the caller's buffer (a 0.6 MB temporary per proof would be fresh pages from the allocator every
// time).  *len is always set; a buffer that is null or too small is left untouched and the call returns CSTARK_ERR_INVALID_ARG.
// p.form == CSTARK_FORM_COMPACT: the path sections are selected from the same gathered paths (select_multiproof), nothing else differs.
inline int write_proof(const ProofShape &S, const ProofParts &p, uint8_t *dst, size_t capacity, size_t *len) {
    Layout L;
    const bool compact = p.form == CSTARK_FORM_COMPACT;
    // the selected nodes of every tree, one after the other, in a block as large as the paths they are selected from; kept per thread
    // and only ever grown: a fresh vector of a few hundred KB per proof would be new pages from the allocator every time, like the
    // temporary the plain form avoids
    static thread_local std::vector<uint8_t> sel;
    size_t sel_at[MAX_TREES + 1] = {};
    if (compact) {
        size_t room = 2 * path_bytes(S);
        for (unsigned l = 0; l < S.n_layers; l++) room += layer_path_bytes(S, l, p.counts[l]);
        if (sel.size() < room) sel.resize(room);
        uint32_t count[MAX_TREES];
        auto select = [&](unsigned t, unsigned depth, uint32_t np, const uint32_t *pos, const uint8_t *paths) {
            count[t] = select_multiproof(depth, np, pos, paths, sel.data() + sel_at[t]);
            sel_at[t + 1] = sel_at[t] + 32 * (size_t)count[t];
        };
        select(0, S.log_N, S.nq, p.pos, p.tpaths);
        select(1, S.log_N, S.nq, p.pos, p.cpaths);
        for (unsigned l = 0; l < S.n_layers; l++) select(2 + l, layer_log_rows(S, l), p.counts[l], p.lpos[l], p.lpaths[l]);
        struct Known {
            const uint32_t *counts, *count; unsigned tree;
            bool positions(size_t, unsigned l, uint32_t &np) { np = counts[l]; return true; }
            bool nodes(size_t, uint32_t, unsigned, uint32_t &n) { n = count[tree++]; return true; }
            bool tail(size_t) { return true; }
        } known{p.counts, count, 0};
        static_cast<ProofShape &>(L) = S;
        walk_compact(L, known, len);
    } else *len = walk(S, p.counts, L);
    if (!dst || capacity < *len) return CSTARK_ERR_INVALID_ARG;
    auto u32 = [dst](size_t o, uint32_t v) { memcpy(dst + o, &v, 4); };
    // a path section: the gathered paths as they are, or the count word and the selected nodes of tree t
    auto paths = [&](size_t o, const uint8_t *plain, size_t plain_bytes, unsigned t) {
        if (!compact) { memcpy(dst + o, plain, plain_bytes); return; }
        u32(o - 4, L.nodes[t]);
        if (L.nodes[t]) memcpy(dst + o, sel.data() + sel_at[t], 32 * (size_t)L.nodes[t]);
    };
    memcpy(dst, compact ? "CSTC" : "CSTK", 4); u32(4, CSTARK_PROOF_VERSION);
    u32(8, S.air); u32(12, S.width); u32(16, S.log_n); u32(20, S.word);
    memcpy(dst + 24, S.opt, sizeof S.opt);
    memcpy(dst + OFF_ROOTS, p.trace_root, 32); memcpy(dst + OFF_ROOTS + 32, p.cons_root, 32);
    u32(OFF_N_LAYERS, S.n_layers);
    if (S.n_layers) memcpy(dst + OFF_N_LAYERS + 4, p.layer_roots, 32 * (size_t)S.n_layers);
    memcpy(dst + off_rem_commit(S), p.rem_commit, 32);
    memcpy(dst + L.ood, p.ood_trace, ood_trace_bytes(S)); memcpy(dst + L.ood + ood_trace_bytes(S), p.ood_comp, ood_comp_bytes(S));
    memcpy(dst + L.nonce, &p.nonce, 8);
    memcpy(dst + L.trows, p.trows, trace_row_bytes(S)); paths(L.tpaths, p.tpaths, path_bytes(S), 0);
    memcpy(dst + L.crows, p.crows, comp_row_bytes(S)); paths(L.cpaths, p.cpaths, path_bytes(S), 1);
    for (unsigned l = 0; l < S.n_layers; l++) {
        u32(L.lrows[l] - 4, L.npos[l]);
        memcpy(dst + L.lrows[l], p.lrows[l], layer_row_bytes(S, L.npos[l]));
        paths(L.lpaths[l], p.lpaths[l], layer_path_bytes(S, l, L.npos[l]), 2 + l);
    }
    u32(L.rem - 4, S.R);
    memcpy(dst + L.rem, p.remainder, remainder_bytes(S));
    return CSTARK_OK;
}

// ---- parser ----------------------------------------------------------------------------------------------------------------------
// the header bounds the prover enforces for TransactionAir's Merkle depth (cstark_tx_witness_upload)
inline bool tx_depth_ok(uint32_t d) { return d != 0 && ((d + 1) & d) == 0 && 8ull * d + 7 <= 511; }

// the form the magic states: CSTARK_FORM_PLAIN, CSTARK_FORM_COMPACT, or -1 for neither (or fewer than four bytes)
inline int proof_form_of(const uint8_t *b, size_t len) {
    if (!b || len < 4) return -1;
    return memcmp(b, "CSTK", 4) == 0 ? CSTARK_FORM_PLAIN : memcmp(b, "CSTC", 4) == 0 ? CSTARK_FORM_COMPACT : -1;
}

// Structure only, O(number of sections): returns CSTARK_PROOF_OK or CSTARK_PROOF_MALFORMED.  Every count is checked against the stated
// options before it sizes anything; the offsets never overflow (every factor is bounded first).  Compact form: a tree's n_nodes is
// bounded by n_positions * depth here; whether it is the count the positions ask for is known only after the transcript replay, so
// that is the tree's opening verdict (verify.hip), not MALFORMED.
inline int parse_layout(const uint8_t *b, size_t len, Layout &L) {
    memset(&L, 0, sizeof L);
    const int form = proof_form_of(b, len);
    if (len < OFF_ROOTS || form < 0) return CSTARK_PROOF_MALFORMED;
    const uint32_t version = rd32(b + 4);
    L.air = rd32(b + 8); L.width = rd32(b + 12); L.log_n = rd32(b + 16); L.word = rd32(b + 20);
    for (int i = 0; i < 7; i++) L.opt[i] = rd32(b + 24 + 4 * i);
    if (version != CSTARK_PROOF_VERSION || L.air > 4 || L.width != AIR_WIDTH[L.air]) return CSTARK_PROOF_MALFORMED;
    const uint32_t nq = L.opt[0], blowup = L.opt[1], grinding = L.opt[2], hash = L.opt[3], ext = L.opt[4], fold = L.opt[5], rem = L.opt[6];
    auto pow2 = [](uint32_t v) { return v != 0 && (v & (v - 1)) == 0; };
    if (nq < 1 || nq > 128 || !pow2(blowup) || blowup < 2 || blowup > 16 || blowup < AIR_CE[L.air] || grinding > 32 || hash > 1 || ext > 2 ||
        (fold != 4 && fold != 8 && fold != 16) || !pow2(rem) || rem < 128 || rem > 1024 || L.log_n < 6 || L.log_n > 21)
        return CSTARK_PROOF_MALFORMED;
    if (L.air == CSTARK_AIR_STATE_TRANSITION && (L.log_n < 10 || !tx_depth_ok(L.word))) return CSTARK_PROOF_MALFORMED;
    shape_derive(L);
    if (len < OFF_N_LAYERS + 4) return CSTARK_PROOF_MALFORMED;
    if (rd32(b + OFF_N_LAYERS) != L.n_layers || L.n_layers > VMAX_LAYERS) return CSTARK_PROOF_MALFORMED;
    if (form == CSTARK_FORM_COMPACT) {
        struct Stated { // every count word lies inside the proof and within its bound
            const uint8_t *b; size_t len; uint32_t nq, R;
            bool word(size_t o, uint32_t &v) { if (o > len || len - o < 4) return false; v = rd32(b + o); return true; }
            bool positions(size_t o, unsigned, uint32_t &np) { return word(o, np) && np <= nq; }
            bool nodes(size_t o, uint32_t np, unsigned depth, uint32_t &n) { return word(o, n) && n <= np * depth; }
            bool tail(size_t o) { uint32_t r; return word(o, r) && r == R; }
        } stated{b, len, nq, L.R};
        size_t end = 0;
        if (!walk_compact(L, stated, &end) || end != len) return CSTARK_PROOF_MALFORMED; // truncated or trailing bytes
        return CSTARK_PROOF_OK;
    }
    size_t o = walk_fixed(L);
    for (unsigned l = 0; l < L.n_layers; l++) {
        if (len < o + 4) return CSTARK_PROOF_MALFORMED;
        const uint32_t np = rd32(b + o);
        if (np > nq || L.log_N < (l + 1) * L.log_f) return CSTARK_PROOF_MALFORMED;
        o = walk_layer(L, l, np, o);
        if (o > len) return CSTARK_PROOF_MALFORMED;
    }
    if (len < o + 4) return CSTARK_PROOF_MALFORMED;
    if (rd32(b + o) != L.R) return CSTARK_PROOF_MALFORMED;
    if (walk_tail(L, o) != len) return CSTARK_PROOF_MALFORMED; // truncated or trailing bytes
    return CSTARK_PROOF_OK;
}

// ---- conversion between the forms ------------------------------------------------------------------------------------------------
// Tree t of a parsed proof (0: trace, 1: composition, 2 + l: layer l): the rows opened in it, its depth, where its path section begins
// in the proof (compact: at the count word) and how long it is.
struct TreeSection { uint32_t count; unsigned depth; size_t at, bytes; };
inline TreeSection tree_section(const Layout &L, unsigned t) {
    const uint32_t count = t < 2 ? L.nq : L.npos[t - 2];
    const unsigned depth = t < 2 ? L.log_N : layer_log_rows(L, t - 2);
    const size_t paths = t == 0 ? L.tpaths : t == 1 ? L.cpaths : L.lpaths[t - 2];
    if (L.form == CSTARK_FORM_COMPACT) return {count, depth, paths - 4, 4 + 32 * (size_t)L.nodes[t]};
    return {count, depth, paths, 32 * (size_t)count * depth};
}
// a capacity that holds the parsed proof in `form` whatever its positions: the exact plain length (it follows from the header and every
// layer's n_positions), plus one count word per tree for the compact form (a multiproof never holds more nodes than the paths it is
// selected from)
inline size_t convert_bound(const Layout &L, uint32_t form) {
    return proof_size(L, L.npos) + (form == CSTARK_FORM_COMPACT ? 4 * (size_t)(2 + L.n_layers) : 0);
}
// The new path sections of a proof that changes its form, tree by tree.  To the plain form: data[t] = paths [count][depth][32] in proof
// order (nodes[t] is not read).  To the compact form: data[t] = nodes[t] multiproof nodes in the canonical order.
struct PathSections { const uint8_t *data[MAX_TREES]; uint32_t nodes[MAX_TREES]; };
// `src` (parsed into L) in `form`: everything outside the path sections is copied, the magic states the form, every path section is
// replaced by ps's.  A proof already in `form` is copied as it is (ps is not read).  *len is always set; a buffer that is null or too
// small is left untouched and the call returns CSTARK_ERR_INVALID_ARG, as write_proof does.
inline int convert_proof(const uint8_t *src, const Layout &L, uint32_t form, const PathSections &ps, uint8_t *dst, size_t capacity, size_t *len) {
    const size_t src_len = L.rem + remainder_bytes(L);
    const unsigned trees = 2 + L.n_layers;
    const bool same = L.form == form, compact = form == CSTARK_FORM_COMPACT;
    size_t n = src_len;
    for (unsigned t = 0; !same && t < trees; t++) {
        const TreeSection s = tree_section(L, t);
        n = n - s.bytes + (compact ? 4 + 32 * (size_t)ps.nodes[t] : 32 * (size_t)s.count * s.depth);
    }
    *len = n;
    if (!dst || capacity < n) return CSTARK_ERR_INVALID_ARG;
    if (same) { memcpy(dst, src, src_len); return CSTARK_OK; }
    size_t from = 0, to = 0;
    for (unsigned t = 0; t < trees; t++) {
        const TreeSection s = tree_section(L, t);
        memcpy(dst + to, src + from, s.at - from);
        to += s.at - from; from = s.at + s.bytes;
        if (compact) { memcpy(dst + to, &ps.nodes[t], 4); to += 4; }
        const size_t bytes = compact ? 32 * (size_t)ps.nodes[t] : 32 * (size_t)s.count * s.depth;
        if (bytes) memcpy(dst + to, ps.data[t], bytes);
        to += bytes;
    }
    memcpy(dst + to, src + from, src_len - from);
    memcpy(dst, compact ? "CSTC" : "CSTK", 4);
    return CSTARK_OK;
}

// every field element section below p (the kernels check the same on the device; this host scan runs only where no kernel reads the
// proof: a proof whose options differ from the expected ones)
inline bool elements_canonical(const uint8_t *b, const Layout &L) {
    auto sec = [&](size_t off, size_t bytes) { for (size_t i = 0; i < bytes; i += 8) if (rd64(b + off + i) >= host::P) return false; return true; };
    bool ok = sec(L.ood, ood_trace_bytes(L) + ood_comp_bytes(L)) && sec(L.trows, trace_row_bytes(L)) && sec(L.crows, comp_row_bytes(L)) &&
              sec(L.rem, remainder_bytes(L));
    for (unsigned l = 0; ok && l < L.n_layers; l++) ok = sec(L.lrows[l], layer_row_bytes(L, L.npos[l]));
    return ok;
}

} // namespace cs
