// The host-only message builder of csrc/ledger_plan.h (plan_apply's optional `messages`) alone under g++: the messages the transfers of
// a batch sign (build_tx_message, src/lib.rs:467-481) are compared with a case written by tests/sig_cases.py (write_messages_case), and every
// message is then verified against its signature with the host arithmetic of hostgadgets.h (verify_signature, src/schnorr/mod.rs:220-245)
// -- the CPU baseline of the device check.
//   ledger_messages_check CASE          all checks
//   ledger_messages_check CASE --time   additionally: seconds the host verification of the signatures takes on this CPU
// CASE: little-endian 64-bit words -- depth, n_acc, n_tx, n_msg, refused_at (2^64 - 1: none), reason | acc_idx [n_acc] | acc_val [n_acc][14] |
// s_idx, r_idx, deltas [n_tx] | messages [n_msg][28] | sig_rx [n_msg][6] | sig_s [n_msg][32 bytes]
#include <stdio.h>
#include <stdlib.h>
#include <chrono>
#include <string>
#include <vector>
#include "../../certificate-stark_amd/csrc/hostgadgets.h"
#include "../../certificate-stark_amd/csrc/ledger_plan.h"

using namespace cs::ledger;
using namespace cs::hostg;
typedef std::vector<uint64_t> Words;

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

static bool read_words(FILE *f, Words &w, size_t n) {
    w.resize(n);
    return n == 0 || fread(w.data(), 8, n, f) == n;
}

// k * (bx, by) in projective coordinates, bits 254..0 of the little-endian scalar, MSB first (the ladders of the SchnorrAir trace)
static Pt ladder(const uint8_t *k, const F6 &bx, const F6 &by) {
    Pt acc{};
    acc.y.c[0].a = cs::host::ONE;
    for (int i = 254; i >= 0; i--) {
        acc = pt_double(acc);
        if ((k[i >> 3] >> (i & 7)) & 1) acc = pt_add_mixed(acc, bx, by);
    }
    return acc;
}
static bool is_zero(const F6 &x) {
    uint64_t w[6];
    store6(w, x);
    return !(w[0] | w[1] | w[2] | w[3] | w[4] | w[5]);
}

// x(s*G + h*P) == R.x, with h*P brought to affine form for the complete mixed addition (h*P at infinity never happens for a valid
// signature: reported as invalid)
static bool verify_signature(const uint64_t *msg, const uint64_t *rx, const uint8_t *s) {
    uint64_t h[7];
    hash_message(rx, msg, h);
    uint8_t hb[32];
    for (int i = 0; i < 4; i++) {
        const uint64_t limb = cs::host::to_u64(h[i]);
        for (int b = 0; b < 8; b++) hb[8 * i + b] = (uint8_t)(limb >> (8 * b));
    }
    const Pt sg = ladder(s, load6(CS_GENERATOR_MONT), load6(CS_GENERATOR_MONT + 6));
    const Pt hp = ladder(hb, load6(msg), load6(msg + 6));
    if (is_zero(hp.z)) return false;
    const F6 zi = inv6(hp.z);
    const Pt sum = pt_add_mixed(sg, mul6(hp.x, zi), mul6(hp.y, zi));
    if (is_zero(sum.z)) return false;
    uint64_t x[6];
    store6(x, mul6(sum.x, inv6(sum.z)));
    return memcmp(x, rx, sizeof x) == 0;
}

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: ledger_messages_check CASE [--time]\n"); return 2; }
    const bool timing = argc > 2 && std::string(argv[2]) == "--time";
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot read %s\n", argv[1]); return 2; }
    uint64_t head[6];
    if (fread(head, 8, 6, f) != 6) { fclose(f); printf("short case\n"); return 2; }
    const uint32_t depth = (uint32_t)head[0], n_acc = (uint32_t)head[1], n_tx = (uint32_t)head[2], n_msg = (uint32_t)head[3];
    const int32_t refused_at = head[4] == ~(uint64_t)0 ? -1 : (int32_t)head[4], reason = (int32_t)head[5];
    Words acc_idx, acc_val, s_idx, r_idx, deltas, expect, sig_rx, sig_s;
    const bool ok = read_words(f, acc_idx, n_acc) && read_words(f, acc_val, (size_t)14 * n_acc) && read_words(f, s_idx, n_tx) && read_words(f, r_idx, n_tx) &&
                    read_words(f, deltas, n_tx) && read_words(f, expect, (size_t)28 * n_msg) && read_words(f, sig_rx, (size_t)6 * n_msg) &&
                    read_words(f, sig_s, (size_t)4 * n_msg);
    fclose(f);
    if (!ok) { printf("short case\n"); return 2; }

    // the plan reads the index only: accounts go in directly
    Index ix(depth);
    for (uint32_t i = 0; i < n_acc; i++) {
        Value v;
        memcpy(v.data(), &acc_val[(size_t)14 * i], sizeof v);
        ix.accounts[acc_idx[i]] = v;
    }
    const uint32_t scratch_base = EMPTY_SLOTS + (n_acc + 4 * n_tx) * (depth + 1) + 16;
    Plan with, without;
    Words messages;
    CHECK(plan_apply(ix, scratch_base, n_tx, s_idx.data(), r_idx.data(), deltas.data(), with, &messages), "the batch could not be planned");
    CHECK(plan_apply(ix, scratch_base, n_tx, s_idx.data(), r_idx.data(), deltas.data(), without), "the batch could not be planned");
    CHECK(with.refused_at == refused_at && with.reason == reason, "refused_at %d reason %d, expected %d / %d", with.refused_at, with.reason, refused_at, reason);
    CHECK(with.refused_at == without.refused_at && with.reason == without.reason && with.upload == without.upload && with.launch == without.launch,
          "asking for the messages changed the plan");
    CHECK(messages.size() == (size_t)28 * n_msg, "%zu message words, expected %zu", messages.size(), (size_t)28 * n_msg);
    if (messages.size() == expect.size())
        for (size_t i = 0; i < expect.size(); i++)
            if (messages[i] != expect[i]) { CHECK(false, "messages[%zu][%zu] differs", i / 28, i % 28); break; }

    // verify_signature on the host for every message the plan built
    uint32_t valid = 0;
    const auto t0 = std::chrono::steady_clock::now();
    if (messages.size() == (size_t)28 * n_msg)
        for (uint32_t t = 0; t < n_msg; t++) valid += verify_signature(&messages[(size_t)28 * t], &sig_rx[(size_t)6 * t], (const uint8_t *)&sig_s[(size_t)4 * t]);
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("ok: depth %u, %u transfers, refused_at %d, %u messages, %u signatures valid on the host", depth, n_tx, refused_at, n_msg, valid);
    if (timing) printf(" seconds=%.6f", seconds);
    printf("\n");
    return 0;
}
