// csrc/sign_plan.h on the CPU, stand-alone (tests/test_sign_reference_cpu.py builds it with AddressSanitizer and UBSan and runs it).
// A few thousand synthetic status tables status(t, a): for each, the rounds and the selection of the plan, with round sizes
// 0 (the default, (sk + 2) / 2 per pending signature), 1, 3 and 64, must give what a plain scan of the attempts a = 0, 1, 2 ... gives --
// the same accepted attempt, attempts count and exhaustion -- and every row of every round must carry the nonce that an independent walk
// of the signature's stream gives for that attempt.  One batch large enough to overflow a round is included.
// With the argument "nonces" the program prints the first nonces of a few streams for the Python restatement to compare.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <utility>
#include <vector>
#include "../../certificate-stark_amd/csrc/sign_plan.h"

using namespace cs::sign;

static uint64_t mix(uint64_t x) {
    uint64_t s = x;
    return splitmix64(&s);
}

// the status of attempt a of signature t in table `table`: accepted with a probability that depends on the signature (never, always,
// and everything between), one of the three rejections otherwise
static uint8_t status_of(uint64_t table, uint32_t t, uint32_t a) {
    const uint64_t kind = mix(table * 1315423911u + t) % 8; // 0: never accepted, 7: always
    const uint64_t draw = mix(mix(table ^ ((uint64_t)t << 32)) + a);
    if (draw % 7 < kind) return OK;
    return (uint8_t)(1 + draw % 3);
}

static int fail(const char *what, uint64_t table, uint32_t t) {
    printf("FAILED: %s (table %llu, signature %u)\n", what, (unsigned long long)table, t);
    return 1;
}

static int run_table(uint64_t table, uint32_t count, const std::vector<uint64_t> &secrets, uint64_t seed, uint32_t max_attempts, uint32_t round_size,
                     size_t *rounds_out) {
    // the plain scan
    std::vector<uint32_t> want_attempts(count);
    std::vector<uint8_t> want_status(count);
    for (uint32_t t = 0; t < count; t++) {
        uint32_t a = 0;
        while (a < max_attempts && status_of(table, t, a) != OK) a++;
        want_status[t] = a < max_attempts ? OK : EXHAUSTED;
        want_attempts[t] = a < max_attempts ? a + 1 : max_attempts;
    }
    // the plan
    Plan plan(count, secrets.data(), seed, max_attempts, round_size);
    std::vector<uint64_t> walk(count); // an independent walk of every stream
    std::vector<uint32_t> walked(count, 0);
    for (uint32_t t = 0; t < count; t++) walk[t] = stream_state(seed, t);
    std::vector<std::pair<uint32_t, uint32_t>> accepted;
    std::vector<uint32_t> got_row_attempt(count, 0);
    std::vector<uint8_t> hit(count, 0);
    Round round;
    std::vector<uint8_t> status;
    std::vector<uint32_t> attempt_of_row;
    while (plan.next_round(round)) {
        const size_t rows = round.rows();
        if (rows == 0 || rows > ROUND_ATTEMPTS || round.nonces.size() != 5 * rows || round.first.size() != round.sigs.size() + 1) return fail("round shape", table, 0);
        status.assign(rows, 0);
        attempt_of_row.assign(rows, 0);
        for (size_t i = 0; i < round.sigs.size(); i++) {
            const uint32_t t = round.sigs[i];
            if (hit[t]) return fail("a finished signature is in a round", table, t);
            for (uint32_t row = round.first[i]; row < round.first[i + 1]; row++) {
                if (round.owner[row] != t) return fail("owner", table, t);
                uint64_t r[5];
                next_nonce(&walk[t], secrets[t], r);
                if (memcmp(r, &round.nonces[5 * (size_t)row], 40) != 0) return fail("a row's nonce is not its attempt's", table, t);
                if ((r[4] >> 8) != 0) return fail("nonce >= 2^264", table, t);
                attempt_of_row[row] = walked[t]++;
                if (attempt_of_row[row] >= max_attempts) return fail("an attempt beyond max_attempts", table, t);
                status[row] = status_of(table, t, attempt_of_row[row]);
            }
        }
        accepted.clear();
        plan.select(round, status.data(), accepted);
        for (const auto &h : accepted) {
            if (hit[h.first]) return fail("accepted twice", table, h.first);
            hit[h.first] = 1;
            if (round.owner[h.second] != h.first || status[h.second] != OK) return fail("accepted row", table, h.first);
            got_row_attempt[h.first] = attempt_of_row[h.second];
        }
        for (size_t i = 1; i < plan.pending.size(); i++)
            if (plan.pending[i - 1] >= plan.pending[i]) return fail("pending order", table, plan.pending[i]);
    }
    for (uint32_t t = 0; t < count; t++) {
        const Signature &s = plan.sigs[t];
        if (s.status != want_status[t] || s.attempts != want_attempts[t]) return fail("status / attempts differ from the scan", table, t);
        if (s.status == OK && (!hit[t] || got_row_attempt[t] + 1 != want_attempts[t])) return fail("the accepted row is not the first accepted attempt", table, t);
        if (s.status == EXHAUSTED && hit[t]) return fail("an exhausted signature was accepted", table, t);
    }
    if (rounds_out) *rounds_out = plan.rounds;
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && strcmp(argv[1], "nonces") == 0) {
        const uint64_t seeds[] = {0, 0x51C4A7, 0xFFFFFFFFFFFFFFFFull};
        const uint32_t ts[] = {0, 5}, sks[] = {1, 255};
        for (uint64_t seed : seeds)
            for (uint32_t t : ts)
                for (uint32_t sk : sks) {
                    uint64_t state = stream_state(seed, t);
                    for (uint32_t a = 0; a < 3; a++) {
                        uint64_t r[5];
                        next_nonce(&state, sk, r);
                        printf("nonce %llx %u %u %u %02llx%016llx%016llx%016llx%016llx\n", (unsigned long long)seed, t, sk, a, (unsigned long long)r[4],
                               (unsigned long long)r[3], (unsigned long long)r[2], (unsigned long long)r[1], (unsigned long long)r[0]);
                    }
                }
        return 0;
    }
    const uint32_t sizes[] = {0, 1, 3, 64};
    size_t tables = 0;
    for (uint64_t table = 1; table <= 1000; table++) {
        const uint32_t count = 1 + (uint32_t)(mix(table) % 40);
        const uint32_t max_attempts = table % 5 == 0 ? 1 + (uint32_t)(mix(table + 77) % 4096) : 1 + (uint32_t)(mix(table + 77) % 70);
        std::vector<uint64_t> secrets(count);
        for (uint32_t t = 0; t < count; t++) secrets[t] = 1 + mix(table * 977 + t) % (table % 3 ? 8 : 255);
        for (uint32_t size : sizes) {
            if (run_table(table, count, secrets, mix(table + 5), max_attempts, size, nullptr)) return 1;
            tables++;
        }
    }
    // more attempts than one round holds: 3000 signatures of the largest key draw 128 attempts each per round
    {
        std::vector<uint64_t> secrets(3000, MAX_SECRET);
        size_t rounds = 0;
        if (run_table(4242, 3000, secrets, 99, 200, 0, &rounds)) return 1;
        if (rounds < 3) return fail("the large batch fitted one round", 4242, 0);
        tables++;
    }
    printf("ok: round sizes 0 1 3 64, %zu status tables\n", tables);
    return 0;
}
