// The byte layout of a proof, once: the shape that fixes it, the walk over its sections, the writer the provers use (prove.hip) and
// the parser the verifier and cstark_proof_inspect use (verify.hip).  The format itself is stated in include/cstark.h ("Proof
// layout"); nothing else under csrc/ knows it.  Host code only (no HIP): tests/cpp/proof_layout_check.cpp builds it with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/cstark.h"
#include "hostfield.h"

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

struct Layout : ProofShape {
    size_t ood, nonce, trows, tpaths, crows, cpaths, lrows[VMAX_LAYERS], lpaths[VMAX_LAYERS], rem; // offsets of the sections
    uint32_t npos[VMAX_LAYERS];                                                                    // opened positions per layer
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
};
inline size_t proof_size(const ProofShape &S, const uint32_t *counts) {
    Layout L;
    return walk(S, counts, L);
}
// The proof bytes go straight into the caller's buffer (a 0.6 MB temporary per proof would be fresh pages from the allocator every
// time).  *len is always set; a buffer that is null or too small is left untouched and the call returns CSTARK_ERR_INVALID_ARG.
inline int write_proof(const ProofShape &S, const ProofParts &p, uint8_t *dst, size_t capacity, size_t *len) {
    Layout L;
    *len = walk(S, p.counts, L);
    if (!dst || capacity < *len) return CSTARK_ERR_INVALID_ARG;
    auto u32 = [dst](size_t o, uint32_t v) { memcpy(dst + o, &v, 4); };
    memcpy(dst, "CSTK", 4); u32(4, CSTARK_PROOF_VERSION);
    u32(8, S.air); u32(12, S.width); u32(16, S.log_n); u32(20, S.word);
    memcpy(dst + 24, S.opt, sizeof S.opt);
    memcpy(dst + OFF_ROOTS, p.trace_root, 32); memcpy(dst + OFF_ROOTS + 32, p.cons_root, 32);
    u32(OFF_N_LAYERS, S.n_layers);
    if (S.n_layers) memcpy(dst + OFF_N_LAYERS + 4, p.layer_roots, 32 * (size_t)S.n_layers);
    memcpy(dst + off_rem_commit(S), p.rem_commit, 32);
    memcpy(dst + L.ood, p.ood_trace, ood_trace_bytes(S)); memcpy(dst + L.ood + ood_trace_bytes(S), p.ood_comp, ood_comp_bytes(S));
    memcpy(dst + L.nonce, &p.nonce, 8);
    memcpy(dst + L.trows, p.trows, trace_row_bytes(S)); memcpy(dst + L.tpaths, p.tpaths, path_bytes(S));
    memcpy(dst + L.crows, p.crows, comp_row_bytes(S)); memcpy(dst + L.cpaths, p.cpaths, path_bytes(S));
    for (unsigned l = 0; l < S.n_layers; l++) {
        u32(L.lrows[l] - 4, L.npos[l]);
        memcpy(dst + L.lrows[l], p.lrows[l], layer_row_bytes(S, L.npos[l]));
        memcpy(dst + L.lpaths[l], p.lpaths[l], layer_path_bytes(S, l, L.npos[l]));
    }
    u32(L.rem - 4, S.R);
    memcpy(dst + L.rem, p.remainder, remainder_bytes(S));
    return CSTARK_OK;
}

// ---- parser ----------------------------------------------------------------------------------------------------------------------
// the header bounds the prover enforces for TransactionAir's Merkle depth (cstark_tx_witness_upload)
inline bool tx_depth_ok(uint32_t d) { return d != 0 && ((d + 1) & d) == 0 && 8ull * d + 7 <= 511; }

// Structure only, O(number of sections): returns CSTARK_PROOF_OK or CSTARK_PROOF_MALFORMED.  Every count is checked against the stated
// options before it sizes anything; the offsets never overflow (every factor is bounded first).
inline int parse_layout(const uint8_t *b, size_t len, Layout &L) {
    memset(&L, 0, sizeof L);
    if (len < OFF_ROOTS || memcmp(b, "CSTK", 4) != 0) return CSTARK_PROOF_MALFORMED;
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
