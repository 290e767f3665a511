// The Fiat-Shamir coin on the host, shared by the prover (prove.hip) and the verifier (verify.hip) so that both replay the same
// transcript from the same code.  The coin's rules: the header of prove.hip; the order of the transcript, as steps over this coin:
// transcript.h.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/cstark_conventions.h"
#include "hostblake3.h"
#include "hostfield.h"
#include "keccak.cuh"

namespace cs {

// the proof's hash function on the host (channel, small commitments): 0 = Blake3_256, 1 = Sha3_256
inline void digest(uint32_t hash_fn, const uint8_t *p, size_t n, uint8_t out[32]) {
    if (hash_fn == 1) keccak::sha3_256(p, n, out);
    else hostb3::hash(p, n, out);
}

struct Coin {
    uint8_t seed[32];
    uint64_t counter = CSTARK_CONV_COIN_FIRST_COUNTER - 1; // pre-incremented by every draw
    uint32_t hash_fn = 0;
    void init(const uint8_t *p, size_t n) { digest(hash_fn, p, n, seed); counter = CSTARK_CONV_COIN_FIRST_COUNTER - 1; }
    void reseed(const uint8_t d[32]) {
        uint8_t buf[64];
        memcpy(buf, seed, 32); memcpy(buf + 32, d, 32);
        digest(hash_fn, buf, 64, seed);
        counter = CSTARK_CONV_COIN_FIRST_COUNTER - 1;
    }
    void with_int(const uint8_t s[32], uint64_t v, uint8_t out[32]) const {
        uint8_t buf[40];
        memcpy(buf, s, 32);
        for (int i = 0; i < 8; i++) buf[32 + i] = (uint8_t)(v >> (8 * i));
        digest(hash_fn, buf, 40, out);
    }
    void reseed_int(uint64_t v) { with_int(seed, v, seed); counter = CSTARK_CONV_COIN_FIRST_COUNTER - 1; }
    uint64_t next_u64() {
        uint8_t out[32];
        with_int(seed, ++counter, out);
        uint64_t v = 0;
        for (int i = 0; i < 8; i++) v |= (uint64_t)out[i] << (8 * i);
        return v;
    }
    uint64_t draw() { // a field element, memory form
        for (;;) {
            const uint64_t v = next_u64();
            if (!CSTARK_CONV_COIN_REJECT_ABOVE_P || v < host::P) return host::from_u64(v); // from_u64 reduces
        }
    }
    // the next `count` draws, in order -- the same values and the same final counter as `count` calls of draw().  Blake3 coin: the
    // candidates of eight consecutive counters per pass of the vectorised compression (hostblake3.h); candidates computed beyond the
    // last accepted one are simply not consumed.
    void draw_many(size_t count, uint64_t *out) {
        static const bool scalar = [] { const char *e = getenv("CSTARK_COIN_SCALAR"); return e && atoi(e) != 0; }(); // tuning / debugging
        if (hash_fn != 0 || scalar) { for (size_t i = 0; i < count; i++) out[i] = draw(); return; }
        size_t got = 0;
        while (got < count) {
            uint64_t cand[8];
            hostb3::coin_candidates_x8(seed, counter + 1, cand);
            for (int l = 0; l < 8 && got < count; l++) {
                counter++;
                if (!CSTARK_CONV_COIN_REJECT_ABOVE_P || cand[l] < host::P) out[got++] = host::from_u64(cand[l]);
            }
        }
    }
    void draw_integers(size_t count, uint64_t domain, std::vector<uint32_t> &out) {
        out.clear();
        while (out.size() < count) {
            const uint32_t v = (uint32_t)(next_u64() & (domain - 1));
            if (!CSTARK_CONV_QUERY_DEDUP || std::find(out.begin(), out.end(), v) == out.end()) out.push_back(v);
        }
    }
};

// digest of field elements: their little-endian bytes in memory form, or canonical (CSTARK_CONV_HASHED_ELEMENT_BYTES_MONTGOMERY)
inline void hash_elements(uint32_t hash_fn, const uint64_t *e, size_t n, uint8_t out[32]) {
#if CSTARK_CONV_HASHED_ELEMENT_BYTES_MONTGOMERY
    digest(hash_fn, (const uint8_t *)e, 8 * n, out); // little-endian host
#else
    std::vector<uint64_t> can(n);
    for (size_t i = 0; i < n; i++) can[i] = host::to_u64(e[i]);
    digest(hash_fn, (const uint8_t *)can.data(), 8 * n, out);
#endif
}

// positions folded into the next layer's row indices, first occurrence order
inline std::vector<uint32_t> fold_positions(const std::vector<uint32_t> &pos, uint32_t rows) {
    std::vector<uint32_t> out;
    for (uint32_t p : pos) {
        const uint32_t r = p & (rows - 1);
        if (std::find(out.begin(), out.end(), r) == out.end()) out.push_back(r);
    }
    return out;
}

} // namespace cs
