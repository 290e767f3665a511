// Exercises cstark::Ledger (include/cstark.hpp) the way an operator would: accounts into the ledger, a batch of signed transfers applied,
// the resident batch proved without an upload.  The transfers are those of TransactionMetadata::build_random(2, depth 3, seed 2); an
// account's value at its first appearance in the generated old values is its initial value.
// usage: ledger_mirror <out_prefix>      writes <prefix>.root (7 u64), <prefix>.proof, prints a summary
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
        const cstark::TransactionMetadata ref = cstark::TransactionMetadata::build_random(2, 3, 2);
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
        const bool root_before = ledger.root() == ref.initial_roots[0];
        cstark::Transfers transfers{ref.s_indices, ref.r_indices, ref.deltas, ref.sig_rx, ref.sig_s};
        // a transfer of an account to itself is refused and changes nothing
        bool refused = false;
        try {
            cstark::Transfers bad = transfers;
            bad.r_indices[1] = bad.s_indices[1];
            ledger.apply(bad);
        } catch (const cstark::TransferRefused &r) { refused = r.index == 1 && r.reason == CSTARK_LEDGER_SELF_TRANSFER && ledger.root() == ref.initial_roots[0]; }
        const cstark::TransactionMetadata m = ledger.apply(transfers);
        const bool same = m.initial_roots == ref.initial_roots && m.final_root == ref.final_root && m.s_old_values == ref.s_old_values &&
                          m.r_old_values == ref.r_old_values && m.s_paths == ref.s_paths && m.r_paths == ref.r_paths && m.s_indices == ref.s_indices &&
                          m.r_indices == ref.r_indices && m.deltas == ref.deltas && m.sig_rx == ref.sig_rx && m.sig_s == ref.sig_s;
        const cstark::Hash root = ledger.root();
        dump(prefix + ".root", root.data(), sizeof root);
        const std::vector<uint8_t> proof = cstark::TransactionProver(options, ctx).prove_resident(m.len());
        dump(prefix + ".proof", proof.data(), proof.size());
        std::printf("root_before=%d refused=%d witness_same=%d proof_bytes=%zu\n", (int)root_before, (int)refused, (int)same, proof.size());
        return root_before && refused && same ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
