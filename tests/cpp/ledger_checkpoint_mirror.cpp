// Exercises the checkpoints and the audit of cstark::Ledger (include/cstark.hpp) the way an operator would: the accounts of
// TransactionMetadata::build_random(2, depth 3, seed 2) go into a ledger, a checkpoint is taken, the batch is applied, the accounts are
// opened under the checkpoint's root and under the new one, both states are audited, the batch is taken back and applied again.
// usage: ledger_checkpoint_mirror <out_prefix>   writes <prefix>.old_paths and <prefix>.new_paths ([n][4][7] u64: all accounts opened at
//        the checkpoint and at the head), <prefix>.roots ([4][7] u64: at the checkpoint, after the batch, after the revert, after the
//        second apply) and prints a summary
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
        const uint64_t cp = ledger.checkpoint();
        const cstark::Transfers transfers{ref.s_indices, ref.r_indices, ref.deltas, ref.sig_rx, ref.sig_s};
        const cstark::TransactionMetadata m = ledger.apply(transfers);
        const bool applied = m.initial_roots == ref.initial_roots && m.final_root == ref.final_root && m.s_paths == ref.s_paths && m.r_paths == ref.r_paths;

        std::vector<cstark::Hash> roots = {ledger.root(cp), ledger.root()};
        const cstark::AccountOpening past = ledger.open(indices, cp), now = ledger.open(indices), head = ledger.open(indices, 0);
        const bool opened = past.root == ref.initial_roots[0] && past.values == values && now.root == ref.final_root && head.paths == now.paths &&
                            head.root == now.root && head.values == now.values && ledger.root(0) == now.root;
        const std::vector<uint8_t> old_verdicts = cstark::check_account_paths(ctx, past.depth, past.indices, past.paths, {past.root}, &past.values, &past.present);
        bool valid = true;
        for (const uint8_t v : old_verdicts) valid = valid && v == CSTARK_PATH_VALID;
        const cstark_ledger_audit_report a_now = ledger.audit(), a_past = ledger.audit(cp);
        const bool audited = a_now.consistent && a_past.consistent && a_now.n_bad == 0 && a_past.n_bad == 0 && a_now.slots_held > 0 &&
                             a_now.slots_live == a_now.n_nodes && a_past.n_nodes == a_now.n_nodes;

        ledger.revert(cp);
        roots.push_back(ledger.root());
        const cstark_ledger_audit_report a_back = ledger.audit();
        const bool reverted = ledger.root() == ref.initial_roots[0] && ledger.accounts(indices) == values && a_back.consistent && a_back.slots_held == 0 &&
                              a_back.slots_free == a_now.slots_held;
        const cstark::TransactionMetadata again = ledger.apply(transfers); // the same batch on the restored state: the same witness
        roots.push_back(ledger.root());
        const bool reapplied = again.initial_roots == m.initial_roots && again.final_root == m.final_root && again.s_old_values == m.s_old_values &&
                               again.r_old_values == m.r_old_values && again.s_paths == m.s_paths && again.r_paths == m.r_paths;
        ledger.release(cp);
        bool gone = false;
        try {
            ledger.root(cp);
        } catch (const cstark::Error &) { gone = true; }
        const cstark_ledger_audit_report a_end = ledger.audit();

        dump(prefix + ".old_paths", past.paths.data(), 8 * past.paths.size());
        dump(prefix + ".new_paths", now.paths.data(), 8 * now.paths.size());
        dump(prefix + ".roots", roots.data(), sizeof(cstark::Hash) * roots.size());
        std::printf("accounts=%zu checkpoint=%llu applied=%d opened=%d valid=%d audited=%d reverted=%d reapplied=%d gone=%d nodes=%llu held=%llu free=%llu\n",
                    indices.size(), (unsigned long long)cp, (int)applied, (int)opened, (int)valid, (int)audited, (int)reverted, (int)reapplied, (int)gone,
                    (unsigned long long)a_end.n_nodes, (unsigned long long)a_end.slots_held, (unsigned long long)a_end.slots_free);
        return applied && opened && valid && audited && reverted && reapplied && gone && a_end.consistent ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
