// Host-side plan of the seeded signer (cstark_schnorr_sign): pure integer work, no HIP, no hashing.
//
// A signature is found by rejection sampling: attempt a of signature t draws a nonce r from the signature's own SplitMix64 stream and
// is accepted when 0 <= r - sk*h < 2^255, with probability about 2 / (sk + 2).  The result of signature t is that of its FIRST accepted
// attempt a = 0, 1, 2, ...; which attempts the device runs together is a matter of schedule only.  This header holds the three things
// that make it so:
//   the stream      the nonces of the host sign() of csrc/witness_gen.hip, attempt by attempt;
//   the schedule    rounds of speculative attempts, (sk + 2) / 2 per pending signature unless the caller fixes another size, the
//                   attempts of one signature consecutive in its stream and consecutive in the round;
//   the selection   from the statuses of a round, the first accepted attempt of every signature in it; a signature without one stays
//                   pending until max_attempts of its attempts have run, then it is exhausted.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <utility>
#include <vector>

namespace cs {
namespace sign {

constexpr uint64_t MAX_SECRET = 255;          // CSTARK_SIG_MAX_SECRET
constexpr uint32_t MAX_ATTEMPTS = 4096;       // the largest max_attempts
constexpr uint32_t MAX_COUNT = 1u << 20;
constexpr uint32_t ROUND_ATTEMPTS = 1u << 18; // attempts of one round at the most: 10 MB of nonces, 100 MB of device scratch
enum Status : uint8_t { OK = 0, NEGATIVE = 1, RANGE = 2, INFINITY_POINT = 3, EXHAUSTED = 4, PENDING = 255 }; // cstark_sign_status

inline uint64_t splitmix64(uint64_t *s) {
    uint64_t z = (*s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// the stream of signature t under `seed`
inline uint64_t stream_state(uint64_t seed, uint32_t t) { return seed ^ (0xD1B54A32D192ED03ULL * ((uint64_t)t + 1)); }

// one attempt's nonce: five outputs of the stream, r uniform in [0, (sk + 2) * 2^254), below 2^263 for sk <= 255
inline void next_nonce(uint64_t *state, uint64_t sk, uint64_t r[5]) {
    for (int i = 0; i < 4; i++) r[i] = splitmix64(state);
    const uint64_t hi = splitmix64(state) % (sk + 2);
    r[3] &= 0x3FFFFFFFFFFFFFFFULL;
    const unsigned __int128 top = (unsigned __int128)r[3] + ((unsigned __int128)hi << 62);
    r[3] = (uint64_t)top;
    r[4] = (uint64_t)(top >> 64);
}

struct Signature {
    uint64_t sk = 0, state = 0; // state: the stream behind the attempts drawn so far
    uint32_t drawn = 0;         // attempts drawn so far
    uint8_t status = PENDING;   // OK, EXHAUSTED or PENDING
    uint32_t attempts = 0;      // OK: index of the accepted attempt + 1; EXHAUSTED: max_attempts
};

// the attempts of one round, in the order the device gets them: attempt row k belongs to signature owner[k] and carries nonces[5 k ..]
struct Round {
    std::vector<uint32_t> owner;
    std::vector<uint64_t> nonces;
    std::vector<uint32_t> first; // per signature of the round, in order: its first row; one more entry = the number of rows
    std::vector<uint32_t> sigs;  // the signatures of the round
    size_t rows() const { return owner.size(); }
};

struct Plan {
    uint32_t max_attempts = 0;
    uint32_t round_size = 0; // attempts per pending signature and round; 0: (sk + 2) / 2, the expected number an acceptance takes
    std::vector<Signature> sigs;
    std::vector<uint32_t> pending; // in ascending order
    size_t rounds = 0, total_attempts = 0;

    Plan(uint32_t count, const uint64_t *secrets, uint64_t seed, uint32_t max_attempts_, uint32_t round_size_ = 0)
        : max_attempts(max_attempts_), round_size(round_size_), sigs(count), pending(count) {
        for (uint32_t t = 0; t < count; t++) {
            sigs[t].sk = secrets[t];
            sigs[t].state = stream_state(seed, t);
            pending[t] = t;
        }
    }

    // the next round: false when no signature is pending.  Pending signatures are served in order until the round is full; the rest wait.
    bool next_round(Round &r) {
        r.owner.clear(); r.nonces.clear(); r.first.clear(); r.sigs.clear();
        if (pending.empty()) return false;
        for (const uint32_t t : pending) {
            Signature &s = sigs[t];
            uint32_t k = round_size ? round_size : (uint32_t)((s.sk + 2) / 2);
            if (k > max_attempts - s.drawn) k = max_attempts - s.drawn;
            if (!r.sigs.empty() && r.rows() + k > ROUND_ATTEMPTS) break;
            r.sigs.push_back(t);
            r.first.push_back((uint32_t)r.rows());
            for (uint32_t a = 0; a < k; a++) {
                uint64_t nonce[5];
                next_nonce(&s.state, s.sk, nonce);
                r.owner.push_back(t);
                r.nonces.insert(r.nonces.end(), nonce, nonce + 5);
            }
            s.drawn += k;
        }
        r.first.push_back((uint32_t)r.rows());
        rounds++;
        total_attempts += r.rows();
        return true;
    }

    // the statuses of the round's rows are in: every signature of the round takes its first accepted row, or stays pending, or is
    // exhausted.  accepted gets (signature, row) for the former.  The attempts a signature drew behind its accepted one are discarded:
    // the signature is done and its stream is never read again.
    void select(const Round &r, const uint8_t *status, std::vector<std::pair<uint32_t, uint32_t>> &accepted) {
        std::vector<uint32_t> still;
        size_t next_pending = 0;
        for (size_t i = 0; i < r.sigs.size(); i++) {
            const uint32_t t = r.sigs[i], lo = r.first[i], hi = r.first[i + 1];
            Signature &s = sigs[t];
            uint32_t row = lo;
            while (row < hi && status[row] != OK) row++;
            if (row < hi) {
                s.status = OK;
                s.attempts = s.drawn - (hi - lo) + (row - lo) + 1;
                accepted.emplace_back(t, row);
            } else if (s.drawn >= max_attempts) {
                s.status = EXHAUSTED;
                s.attempts = max_attempts;
            } else {
                still.push_back(t);
            }
            next_pending++;
        }
        // the round took a prefix of `pending`: its leftovers, then those it had no room for, are in ascending order again
        still.insert(still.end(), pending.begin() + next_pending, pending.end());
        pending.swap(still);
    }
};

} // namespace sign
} // namespace cs
