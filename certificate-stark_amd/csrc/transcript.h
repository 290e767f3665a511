// The Fiat-Shamir transcript on the host, once: the order in which a proof's commitments enter the coin (coin.h) and what is drawn after
// each, as steps that every host-channel prover calls (prove.hip: the generic phases and the batched range prover) and that
// tests/cpp/transcript_check.cpp replays from a proof's own bytes.  Host code only (no HIP); builds with g++.
//
// Protocol order [UPSTREAM-RECALL winterfell v0.3, parity unpinned -- the engine is absent from the reference tree]:
//   open               seed = H(context || public inputs) (channel_seed), reseed(trace root)
//   draw_coefficients  (alpha, beta) per transition constraint, then per assertion
//   draw_ood_point     reseed(constraint root), z
//   absorb_frame       reseed(H(T(z) || T(z w))), reseed(H(H_i(z^ce)))
//   draw_deep          per register alpha, beta and the convention's unused draws; delta per composition column; the two degree-
//                      adjustment elements
//   fri_layer          per FRI layer: reseed(layer root), the folding point
//   commit_remainder   reseed(H(remainder))
//   host_nonce         proof of work on the seed (or the device-side searches of prove.hip: same nonce)
//   draw_queries       reseed_int(nonce), the distinct query positions, every layer's folded positions
// Every drawn element is m consecutive draws (m = 1 + field_extension words).  A reseed resets the draw counter, so a step with one draw
// too many or too few leaves no trace in the later steps: the counts below are part of the protocol.
// Each step takes the coin and storage of the caller's; none allocates beyond Coin::draw_integers' and fold_positions' vectors (the
// batched prover runs them per proof on several threads).  The device-side channel (channel.hip) and the GPU verifier's transcript
// kernel (verify.hip) state the same order for the device.
#pragma once
#include <vector>
#include "coin.h"
#include "proof_layout.h"

namespace cs {
namespace transcript {

// The channel seed (the verifier replays it): trace width, log2 n, p, the seven option bytes -- these 17 bytes are also the prefix the
// device-side channel starts from (SEED_PREFIX) -- then the public inputs in canonical form (PublicInputs::write_into, src/air.rs:57-62
// and the sub-AIRs' equivalents) and further public material verbatim (Schnorr: the s halves of the signatures).
constexpr size_t SEED_PREFIX = 17;
inline std::vector<uint8_t> channel_seed(uint32_t width, unsigned log_n, const cstark_options &opt, unsigned log_b, unsigned log_rem, const uint64_t *pub = nullptr,
                                         size_t n_pub = 0, const uint8_t *pub_bytes = nullptr, size_t n_bytes = 0) {
    std::vector<uint8_t> s(SEED_PREFIX + 8 * n_pub + n_bytes);
    const uint8_t head[2] = {(uint8_t)width, (uint8_t)log_n};
    const uint8_t options[7] = {(uint8_t)opt.num_queries, (uint8_t)log_b, (uint8_t)opt.grinding_factor, (uint8_t)opt.hash_fn,
                                (uint8_t)opt.field_extension, (uint8_t)opt.fri_folding_factor, (uint8_t)log_rem};
    memcpy(&s[0], head, 2); memcpy(&s[2], &host::P, 8); memcpy(&s[10], options, 7);
    for (size_t i = 0; i < n_pub; i++) { const uint64_t v = host::to_u64(pub[i]); memcpy(&s[SEED_PREFIX + 8 * i], &v, 8); }
    if (n_bytes) memcpy(&s[SEED_PREFIX + 8 * n_pub], pub_bytes, n_bytes);
    return s;
}

// elements drawn by draw_coefficients and by draw_deep (m words each)
constexpr size_t coefficient_draws(size_t nc, size_t na) { return 2 * (nc + na); }
constexpr size_t deep_draws(size_t W, size_t ce) { return CSTARK_CONV_DEEP_DRAWS_PER_REGISTER * W + ce + 2; }

inline void open(Coin &coin, uint32_t hash_fn, const uint8_t *seed, size_t seed_len, const uint8_t trace_root[32]) {
    coin.hash_fn = hash_fn;
    coin.init(seed, seed_len);
    coin.reseed(trace_root);
}

// Component q of every element goes to coefficient set q: ta[q][nc], tb[q][nc], ba[q][na], bb[q][na].  dr: m coefficient_draws(nc, na) words.
struct CoefficientSets { uint64_t *ta[3], *tb[3], *ba[3], *bb[3]; };
inline void draw_coefficients(Coin &coin, size_t m, size_t nc, size_t na, uint64_t *dr, const CoefficientSets &s) {
    coin.draw_many(m * coefficient_draws(nc, na), dr);
    const uint64_t *t = dr, *b = dr + 2 * m * nc;
    for (size_t q = 0; q < m; q++) {
        for (size_t i = 0; i < nc; i++) { s.ta[q][i] = t[m * 2 * i + q]; s.tb[q][i] = t[m * (2 * i + 1) + q]; }
        for (size_t i = 0; i < na; i++) { s.ba[q][i] = b[m * 2 * i + q]; s.bb[q][i] = b[m * (2 * i + 1) + q]; }
    }
}

inline void draw_ood_point(Coin &coin, const uint8_t cons_root[32], size_t m, uint64_t *z) {
    coin.reseed(cons_root);
    for (size_t q = 0; q < m; q++) z[q] = coin.draw();
}

// ood_trace: T(z) | T(z w), 2 m W words; ood_comp: H_i(z^ce), m ce words
inline void absorb_frame(Coin &coin, size_t m, size_t W, size_t ce, const uint64_t *ood_trace, const uint64_t *ood_comp) {
    uint8_t dg[32];
    hash_elements(coin.hash_fn, ood_trace, 2 * m * W, dg); coin.reseed(dg);
    hash_elements(coin.hash_fn, ood_comp, m * ce, dg); coin.reseed(dg);
}

// alpha (point z) and beta (point z w) [W] m-tuples, delta [ce] m-tuples, deg_a and deg_b one m-tuple each.  dr: m deep_draws(W, ce) words.
inline void draw_deep(Coin &coin, size_t m, size_t W, size_t ce, uint64_t *dr, uint64_t *alpha, uint64_t *beta, uint64_t *delta, uint64_t *deg_a, uint64_t *deg_b) {
    constexpr size_t PER = CSTARK_CONV_DEEP_DRAWS_PER_REGISTER; // beyond alpha and beta: what only the engine's conjugate term uses
    coin.draw_many(m * deep_draws(W, ce), dr);
    for (size_t i = 0; i < W; i++)
        for (size_t q = 0; q < m; q++) { alpha[m * i + q] = dr[m * PER * i + q]; beta[m * i + q] = dr[m * (PER * i + 1) + q]; }
    const uint64_t *rest = dr + m * PER * W;
    for (size_t i = 0; i < m * ce; i++) delta[i] = rest[i];
    for (size_t q = 0; q < m; q++) { deg_a[q] = rest[m * ce + q]; deg_b[q] = rest[m * (ce + 1) + q]; }
}

// alpha = null: the reseed alone (a prover whose layers' points were drawn on the device replays the roots on its own coin)
inline void fri_layer(Coin &coin, const uint8_t root[32], size_t m, uint64_t *alpha) {
    coin.reseed(root);
    for (size_t q = 0; alpha && q < m; q++) alpha[q] = coin.draw();
}

inline void commit_remainder(Coin &coin, const uint64_t *remainder, size_t words, uint8_t commit[32]) {
    hash_elements(coin.hash_fn, remainder, words, commit);
    coin.reseed(commit);
}

// Proof of work, the sequential search: the smallest nonce >= 1 whose digest with the seed has `bits` low zero bits (0 bits: nonce 1).
// `coin`: after commit_remainder.
inline uint64_t host_nonce(const Coin &coin, unsigned bits) {
    for (uint64_t nonce = 1;; nonce++) {
        uint8_t out[32];
        coin.with_int(coin.seed, nonce, out);
        if (bits == 0 || (rd64(out) & ((1ull << bits) - 1)) == 0) return nonce;
    }
}

// pos[S.nq]: the drawn positions; layer l's folded positions: counts[l] of them at folded + l * layer_stride, zeros up to S.nq
inline void draw_queries(Coin &coin, const ProofShape &S, uint64_t nonce, uint32_t *pos, uint32_t *folded, size_t layer_stride, uint32_t *counts) {
    coin.reseed_int(nonce);
    std::vector<uint32_t> cur;
    coin.draw_integers(S.nq, (uint64_t)1 << S.log_N, cur);
    memcpy(pos, cur.data(), 4 * (size_t)S.nq);
    for (unsigned l = 0; l < S.n_layers; l++) {
        cur = fold_positions(cur, 1u << layer_log_rows(S, l));
        counts[l] = (uint32_t)cur.size();
        uint32_t *out = folded + l * layer_stride;
        memcpy(out, cur.data(), 4 * cur.size());
        memset(out + cur.size(), 0, 4 * (S.nq - cur.size()));
    }
}

} // namespace transcript
} // namespace cs
