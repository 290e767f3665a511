// Exercises the signature check of include/cstark.hpp the way an operator would: cstark::schnorr_check on generated signatures and on a
// tampered one, then a ledger that applies a batch with Ledger::apply_checked -- once with a forged signature (refused, nothing changed),
// once as signed.  The transfers are those of TransactionMetadata::build_random(16, depth 3, seed 3): its repeated senders sign nonces
// that earlier transfers of the same batch moved.
// usage: sig_check_mirror <out_prefix>      writes <prefix>.root (7 u64), <prefix>.rx (6 u64: x of the tampered signature), prints a summary
#include <cstdio>
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
        const cstark::ProofOptions options(42, 8, 0, cstark::HashFunction::Blake3_256, cstark::FieldExtension::None, 4, 256);

        // the stand-alone check: five generated signatures are valid; one flipped scalar bit is a mismatch of that signature alone
        cstark::SchnorrExample example(options, 5, ctx);
        bool check_ok = example.check_signatures() == std::vector<uint8_t>(5, CSTARK_SIG_VALID);
        std::vector<uint8_t> bent = example.sig_s;
        bent[32 * 3] ^= 1;
        std::vector<cstark::BaseElement> x;
        const std::vector<uint8_t> verdicts = cstark::schnorr_check(ctx, example.messages, example.sig_rx, bent, &x);
        check_ok = check_ok && verdicts == std::vector<uint8_t>{0, 0, 0, CSTARK_SIG_MISMATCH, 0} && x.size() == 30;
        for (size_t i = 0; check_ok && i < 30; i++) check_ok = (x[i] == example.sig_rx[i]) == (i / 6 != 3);
        dump(prefix + ".rx", x.data() + 18, 48);

        const cstark::TransactionMetadata ref = cstark::TransactionMetadata::build_random(16, 3, 3);
        std::map<uint64_t, std::array<cstark::BaseElement, 14>> first;
        for (size_t t = 0; t < ref.len(); t++) {
            first.emplace(ref.s_indices[t], ref.s_old_values[t]);
            first.emplace(ref.r_indices[t], ref.r_old_values[t]);
        }
        std::vector<uint64_t> indices;
        std::vector<std::array<cstark::BaseElement, 14>> values;
        for (const auto &kv : first) { indices.push_back(kv.first); values.push_back(kv.second); }
        cstark::Ledger ledger(ctx, 3);
        ledger.set_accounts(indices, values);
        const cstark::Transfers transfers{ref.s_indices, ref.r_indices, ref.deltas, ref.sig_rx, ref.sig_s};

        bool refused = false;
        try {
            cstark::Transfers forged = transfers;
            forged.sig_s[11][0] ^= 1;
            ledger.apply_checked(forged);
        } catch (const cstark::TransferRefused &r) {
            refused = r.index == 11 && r.reason == CSTARK_LEDGER_SIGNATURE && ledger.root() == ref.initial_roots[0] && ledger.accounts(indices) == values;
        }
        const cstark::TransactionMetadata m = ledger.apply_checked(transfers);
        const bool same = m.initial_roots == ref.initial_roots && m.final_root == ref.final_root && m.s_old_values == ref.s_old_values &&
                          m.r_old_values == ref.r_old_values && m.s_paths == ref.s_paths && m.r_paths == ref.r_paths && m.s_indices == ref.s_indices &&
                          m.r_indices == ref.r_indices && m.deltas == ref.deltas && m.sig_rx == ref.sig_rx && m.sig_s == ref.sig_s;
        const cstark::Hash root = ledger.root();
        dump(prefix + ".root", root.data(), sizeof root);
        std::printf("check=%d refused=%d witness_same=%d\n", (int)check_ok, (int)refused, (int)same);
        return check_ok && refused && same ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
