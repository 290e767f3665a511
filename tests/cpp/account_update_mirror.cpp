// Exercises cstark::check_account_update (include/cstark.hpp) the way a holder of roots would: the accounts of
// TransactionMetadata::build_random(2, depth 3, seed 2) go into a ledger, all of them and one absent index are opened with ONE
// multiproof, then the ledger moves on (one account gets the balance word of another, the absent index gets an account) and the opening,
// the accounts' new values and the two roots are checked without the ledger: the stated transition, compute-only, a stale new root, and
// an opening with its last node dropped.
// usage: account_update_mirror <out_prefix>      writes <prefix>.indices (u64), <prefix>.new_values ([count][14] u64), <prefix>.new_root and
//        <prefix>.computed (7 u64 each) and prints the four results
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
        uint64_t absent = 0;
        while (first.count(absent)) absent++;

        cstark::Ledger ledger(ctx, 3);
        ledger.set_accounts(indices, values);
        std::vector<uint64_t> asked = indices;
        asked.push_back(absent);
        const cstark::AccountMultiOpening o = ledger.open_multi(asked);
        const cstark::Hash old_root = ledger.root();

        // the ledger moves on: account 0 takes account 1's balance word, the absent index gets account 0's old value
        auto changed = values[0];
        changed[12] = values[1][12];
        ledger.set_accounts({indices[0], absent}, {changed, values[0]});
        const cstark::Hash new_root = ledger.root();
        std::vector<uint8_t> new_present;
        const std::vector<std::array<cstark::BaseElement, 14>> new_values = ledger.accounts(o.indices, &new_present);

        const cstark::UpdateCheck stated = cstark::check_account_update(ctx, o, new_values, &new_present, &new_root);
        const cstark::UpdateCheck computed = cstark::check_account_update(ctx, o, new_values, &new_present);
        const cstark::UpdateCheck stale = cstark::check_account_update(ctx, o, new_values, &new_present, &old_root);
        cstark::AccountMultiOpening shorter = o;
        shorter.nodes.resize(shorter.nodes.size() - 7);
        const cstark::UpdateCheck dropped = cstark::check_account_update(ctx, shorter, new_values, &new_present, &new_root);
        dump(prefix + ".indices", o.indices.data(), 8 * o.indices.size());
        dump(prefix + ".new_values", new_values[0].data(), 112 * new_values.size());
        dump(prefix + ".new_root", new_root.data(), sizeof new_root);
        dump(prefix + ".computed", computed.new_root.data(), sizeof computed.new_root);
        std::printf("opened=%d n_nodes=%zu stated=%u,%u,%u,%d computed=%u,%u,%d stale=%u,%u,%d dropped=%u,%u\n", (int)(o.root == old_root), o.nodes.size() / 7,
                    stated.verdict, stated.at, stated.n_changed, (int)(stated.new_root == new_root), computed.verdict, computed.n_changed,
                    (int)(computed.new_root == new_root), stale.verdict, stale.n_changed, (int)(stale.new_root == new_root), dropped.verdict, dropped.at);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
