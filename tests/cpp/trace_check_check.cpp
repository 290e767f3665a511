// csrc/trace_check.h alone under g++ (host code only): the shapes, the boundary lists and the decoding of a per-cycle code that
// cstark_air_validate_trace works from, at the extremes -- one signature and 4096 of them, the shortest and the longest trace of every
// AIR, the first and the last code of the first and the last cycle.  Built with AddressSanitizer and UBSan and run directly.
//   trace_check_check        all checks; prints one "ok" line per AIR
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../certificate-stark_amd/csrc/trace_check.h"

using namespace cs;
using namespace cs::host;

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            failures++;                                    \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);    \
            printf(__VA_ARGS__);                           \
            printf("\n");                                  \
        }                                                  \
    } while (0)

static const char *NAMES[5] = {"TransactionAir", "MerkleAir", "SchnorrAir", "RangeProofAir", "RescueAir"};
static const uint32_t WIDTH[5] = {94, 65, 56, 2, 14}, NC[5] = {115, 106, 56, 2, 14}, MIN_LOG[5] = {10, 9, 9, 1, 3};

// every occurrence of every entry stays inside the trace and inside the sequence table
static void check_entries(int air, uint32_t log_n, const std::vector<ValidateEntry> &e, const std::vector<uint64_t> &seq) {
    const uint64_t n = 1ull << log_n;
    for (size_t a = 0; a < e.size(); a++) {
        CHECK(e[a].reg < WIDTH[air], "%s entry %zu: register %u", NAMES[air], a, e[a].reg);
        CHECK(e[a].first < n, "%s entry %zu: first step %u of %llu", NAMES[air], a, e[a].first, (unsigned long long)n);
        CHECK(e[a].value < P, "%s entry %zu: value is no field element", NAMES[air], a);
        const uint64_t n_occ = e[a].stride ? n / e[a].stride : 1;
        if (e[a].stride) CHECK(e[a].first < e[a].stride && e[a].first + (n_occ - 1) * e[a].stride < n, "%s entry %zu: last occurrence outside the trace", NAMES[air], a);
        if (e[a].seq >= 0) CHECK(((uint64_t)e[a].seq + 1) * n_occ <= seq.size(), "%s entry %zu: sequence %d outside the table", NAMES[air], a, e[a].seq);
        CHECK((uint64_t)a << 24 >> 24 == a && e[a].first + (n_occ - 1) * (uint64_t)e[a].stride < (1u << 24), "%s entry %zu: verdict word overflows", NAMES[air], a);
    }
}

int main() {
    uint64_t pub[14];
    for (int i = 0; i < 14; i++) pub[i] = from_u64(1000 + i);
    for (int air = 0; air < 5; air++) {
        TraceCheckShape s;
        CHECK(!trace_check_shape(air, MIN_LOG[air] - 1, s), "%s: a trace shorter than one cycle is accepted", NAMES[air]);
        CHECK(!trace_check_shape(air, VALIDATE_MAX_LOG_N + 1, s), "%s: 2^25 rows are accepted", NAMES[air]);
        for (uint32_t log_n : {MIN_LOG[air], VALIDATE_MAX_LOG_N}) {
            CHECK(trace_check_shape(air, log_n, s), "%s: 2^%u rows refused", NAMES[air], log_n);
            CHECK(s.width == WIDTH[air] && s.nc == NC[air], "%s: shape", NAMES[air]);
            const uint64_t n = 1ull << log_n, cyc = 1ull << s.log_cycle, n_cycles = n >> s.log_cycle;
            // the largest code of the last cycle: it must fit 32 bits below CLEAN and decode to the frame before the last row
            const uint64_t top = (cyc - 1) * s.nc + (s.nc - 1);
            CHECK(top < VALIDATE_CLEAN, "%s: the largest code collides with CLEAN", NAMES[air]);
            TraceViolation v = trace_check_decode(s, n_cycles - 1, (uint32_t)top);
            CHECK(v.step == n - 1 && v.row_in_cycle == cyc - 1 && v.constraint == s.nc - 1 && v.cycle == n_cycles - 1, "%s: decode of the last code", NAMES[air]);
            v = trace_check_decode(s, 0, 0);
            CHECK(v.step == 0 && v.row_in_cycle == 0 && v.constraint == 0 && v.cycle == 0, "%s: decode of code 0", NAMES[air]);
            v = trace_check_decode(s, n_cycles - 1, s.nc);
            CHECK(v.step == (n_cycles - 1) * cyc + 1 && v.constraint == 0, "%s: decode of the second row", NAMES[air]);
            if (air == 2) continue; // below, by signatures
            std::vector<ValidateEntry> e;
            std::vector<uint64_t> seq;
            CHECK(trace_check_entries(air, log_n, pub, nullptr, e, seq), "%s: no list", NAMES[air]);
            CHECK(e.size() == (air == 3 ? 2u : 14u) && seq.empty(), "%s: %zu entries", NAMES[air], e.size());
            check_entries(air, log_n, e, seq);
            if (air == 3) CHECK(e[0].value == 0 && e[0].first == 0 && e[1].value == pub[0] && e[1].first == n - 1 && e[0].reg == 1 && e[1].reg == 1, "RangeProofAir: list");
            else
                for (uint32_t a = 0; a < 14; a++)
                    CHECK(e[a].reg == (air == 4 ? 0u : 58u) + a % 7 && e[a].first == (a < 7 ? 0 : n - 1) && e[a].stride == 0 && e[a].seq < 0 && e[a].value == pub[a],
                          "%s: entry %u", NAMES[air], a);
        }
        printf("ok: %s\n", NAMES[air]);
    }
    // SchnorrAir: 61 assertions every 512 rows; sequences k and 6 + k hold R.x word k of every signature
    for (uint32_t log_sig : {0u, 12u}) {
        const uint64_t n_sig = 1ull << log_sig;
        std::vector<uint64_t> rx(6 * n_sig);
        for (size_t i = 0; i < rx.size(); i++) rx[i] = from_u64(7 * i + 3);
        std::vector<ValidateEntry> e;
        std::vector<uint64_t> seq;
        CHECK(trace_check_entries(2, 9 + log_sig, nullptr, rx.data(), e, seq), "SchnorrAir: no list for %llu signatures", (unsigned long long)n_sig);
        CHECK(e.size() == 61 && seq.size() == 12 * n_sig, "SchnorrAir: %zu entries, %zu sequence words", e.size(), seq.size());
        check_entries(2, 9 + log_sig, e, seq);
        int n_seq = 0;
        for (size_t a = 0; a < e.size(); a++) {
            CHECK(e[a].stride == 512 && (e[a].first == 0 || e[a].first == 511), "SchnorrAir: entry %zu is not periodic over the blocks", a);
            if (e[a].seq < 0) continue;
            n_seq++;
            CHECK(e[a].reg == (e[a].first == 0 ? 42u : 0u) + e[a].seq % 6 && (e[a].seq < 6) == (e[a].first == 0), "SchnorrAir: sequence entry %zu", a);
            for (uint64_t t : {(uint64_t)0, n_sig - 1}) CHECK(seq[e[a].seq * n_sig + t] == rx[6 * t + e[a].seq % 6], "SchnorrAir: sequence %d at signature %llu", e[a].seq, (unsigned long long)t);
        }
        CHECK(n_seq == 12, "SchnorrAir: %d sequence entries", n_seq);
        CHECK(e[6].value == ONE && e[25].value == ONE && e[0].value == 0, "SchnorrAir: the points at infinity");
        printf("ok: SchnorrAir, %llu signatures\n", (unsigned long long)n_sig);
    }
    CHECK(trace_check_depth(1) && trace_check_depth(3) && trace_check_depth(7) && trace_check_depth(15) && trace_check_depth(31), "depths");
    CHECK(!trace_check_depth(0) && !trace_check_depth(2) && !trace_check_depth(32) && !trace_check_depth(63), "depths refused");
    return failures ? 1 : 0;
}
