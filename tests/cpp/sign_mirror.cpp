// Exercises the signing calls of include/cstark.hpp the way an operator would.  cstark::schnorr_public_keys gives the keys of the secrets
// 1..8; matching them against the accounts of TransactionMetadata::build_random(16, depth 3, seed 3) recovers every sender's secret.  A
// ledger holding those accounts then signs the batch's own transfers (Ledger::sign), is refused a wrong secret with CSTARK_LEDGER_KEY,
// and applies the signed batch with Ledger::apply_checked.  cstark::schnorr_sign and cstark::schnorr_sign_nonces sign the ledger's
// messages (Ledger::messages) once more on their own.
// usage: sign_mirror <out_prefix>      writes <prefix>.keys (8 x 12 u64), .secrets (16 u64), .msg (16 x 28 u64), .rx (16 x 6 u64), .s (16 x 32
// bytes), .attempts (16 u32), .nonce_rx (3 x 6 u64), .nonce_s (3 x 32 bytes), .nonce_status (3 bytes), .root (7 u64); prints a summary
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include "cstark.hpp"

static void dump(const std::string &path, const void *p, size_t n) {
    std::ofstream f(path, std::ios::binary);
    f.write((const char *)p, (std::streamsize)n);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string prefix = argv[1];
    try {
        cstark::Context ctx;
        const std::vector<uint64_t> all_secrets{1, 2, 3, 4, 5, 6, 7, 8};
        const auto keys = cstark::schnorr_public_keys(ctx, all_secrets);
        dump(prefix + ".keys", keys[0].data(), keys.size() * sizeof keys[0]);

        const cstark::TransactionMetadata ref = cstark::TransactionMetadata::build_random(16, 3, 3);
        std::map<uint64_t, std::array<cstark::BaseElement, 14>> first;
        for (size_t t = 0; t < ref.len(); t++) {
            first.emplace(ref.s_indices[t], ref.s_old_values[t]);
            first.emplace(ref.r_indices[t], ref.r_old_values[t]);
        }
        std::vector<uint64_t> indices;
        std::vector<std::array<cstark::BaseElement, 14>> values;
        for (const auto &kv : first) { indices.push_back(kv.first); values.push_back(kv.second); }
        std::vector<uint64_t> secrets(ref.len(), 0);
        for (size_t t = 0; t < ref.len(); t++)
            for (size_t k = 0; k < keys.size(); k++)
                if (std::memcmp(keys[k].data(), ref.s_old_values[t].data(), sizeof keys[k]) == 0) secrets[t] = all_secrets[k];
        bool recovered = true;
        for (const uint64_t sk : secrets) recovered = recovered && sk != 0;
        dump(prefix + ".secrets", secrets.data(), secrets.size() * 8);

        cstark::Ledger ledger(ctx, 3);
        ledger.set_accounts(indices, values);
        const cstark::Transfers unsigned_batch{ref.s_indices, ref.r_indices, ref.deltas, {}, {}};
        const auto messages = ledger.messages(unsigned_batch);
        dump(prefix + ".msg", messages[0].data(), messages.size() * sizeof messages[0]);
        const cstark::Transfers signed_batch = ledger.sign(unsigned_batch, secrets, 11, 256);
        dump(prefix + ".rx", signed_batch.sig_rx[0].data(), signed_batch.sig_rx.size() * 48);
        dump(prefix + ".s", signed_batch.sig_s[0].data(), signed_batch.sig_s.size() * 32);

        bool key_refused = false;
        try {
            std::vector<uint64_t> wrong = secrets;
            wrong[6] = wrong[6] % 8 + 1;
            ledger.sign(unsigned_batch, wrong, 11);
        } catch (const cstark::TransferRefused &r) {
            key_refused = r.index == 6 && r.reason == CSTARK_LEDGER_KEY && ledger.root() == ref.initial_roots[0] && ledger.accounts(indices) == values;
        }

        // the stand-alone signer on the same messages and seed gives the same signatures
        std::vector<cstark::BaseElement> flat(28 * messages.size());
        std::memcpy(flat.data(), messages[0].data(), flat.size() * 8);
        const cstark::Signatures again = cstark::schnorr_sign(ctx, flat, secrets, 11, 256);
        bool same_signer = std::memcmp(again.sig_rx.data(), signed_batch.sig_rx[0].data(), again.sig_rx.size() * 8) == 0 &&
                           std::memcmp(again.sig_s.data(), signed_batch.sig_s[0].data(), again.sig_s.size()) == 0;
        for (const uint8_t st : again.status) same_signer = same_signer && st == CSTARK_SIGN_OK;
        dump(prefix + ".attempts", again.attempts.data(), again.attempts.size() * 4);
        const bool valid = cstark::schnorr_check(ctx, flat, again.sig_rx, again.sig_s) == std::vector<uint8_t>(messages.size(), CSTARK_SIG_VALID);

        // chosen nonces: 0, 1 and 2^255 on the first three messages
        const std::vector<uint64_t> nonces{0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1ull << 63, 0};
        const cstark::Signatures tries = cstark::schnorr_sign_nonces(ctx, std::vector<cstark::BaseElement>(flat.begin(), flat.begin() + 84),
                                                                     std::vector<uint64_t>(secrets.begin(), secrets.begin() + 3), nonces);
        dump(prefix + ".nonce_rx", tries.sig_rx.data(), tries.sig_rx.size() * 8);
        dump(prefix + ".nonce_s", tries.sig_s.data(), tries.sig_s.size());
        dump(prefix + ".nonce_status", tries.status.data(), tries.status.size());

        const cstark::TransactionMetadata m = ledger.apply_checked(signed_batch);
        const bool applied = m.initial_roots == ref.initial_roots && m.final_root == ref.final_root && m.s_old_values == ref.s_old_values &&
                             m.r_old_values == ref.r_old_values && m.s_paths == ref.s_paths && m.r_paths == ref.r_paths && m.sig_rx == signed_batch.sig_rx &&
                             m.sig_s == signed_batch.sig_s;
        const cstark::Hash root = ledger.root();
        dump(prefix + ".root", root.data(), sizeof root);
        std::printf("recovered=%d key_refused=%d same_signer=%d valid=%d applied=%d\n", (int)recovered, (int)key_refused, (int)same_signer, (int)valid, (int)applied);
        return recovered && key_refused && same_signer && valid && applied ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
