// Exercises cstark::Ledger::open_multi and cstark::check_account_multiproof (include/cstark.hpp) the way a client of a verified root
// would: the accounts of TransactionMetadata::build_random(2, depth 3, seed 2) go into a ledger, two of them and one absent index are
// opened with ONE multiproof (asked for out of order), the opening is checked, then one word of its last node is changed and it is
// checked again, then its last node is dropped and it is checked a third time.
// usage: ledger_multi_mirror <out_prefix>      writes <prefix>.nodes ([n_nodes][7] u64), <prefix>.root (7 u64), <prefix>.folded (7 u64, of
//        the changed opening) and prints the opened indices and the three results
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
        const cstark::AccountMultiOpening o = ledger.open_multi({indices[1], absent, indices[0], indices[1]});
        bool as_stored = o.indices.size() == 3 && o.depth == 3 && o.root == ref.initial_roots[0] && o.root == ledger.root() && !o.nodes.empty();
        for (size_t k = 0; as_stored && k < 3; k++) {
            const auto it = first.find(o.indices[k]);
            as_stored = (k == 0 || o.indices[k] > o.indices[k - 1]) && o.present[k] == (it != first.end()) && (it == first.end() || o.values[k] == it->second);
        }
        if (!as_stored) { std::printf("as_stored=0\n"); return 1; }
        const cstark::MultiproofCheck honest = cstark::check_account_multiproof(ctx, o.depth, o.indices, o.nodes, o.root, &o.values, &o.present);
        std::vector<cstark::BaseElement> nodes = o.nodes;
        nodes[nodes.size() - 3] ^= 1;
        const cstark::MultiproofCheck changed = cstark::check_account_multiproof(ctx, o.depth, o.indices, nodes, o.root, &o.values, &o.present);
        nodes.resize(nodes.size() - 7);
        const cstark::MultiproofCheck dropped = cstark::check_account_multiproof(ctx, o.depth, o.indices, nodes, o.root, &o.values, &o.present);
        dump(prefix + ".nodes", o.nodes.data(), 8 * o.nodes.size());
        dump(prefix + ".root", o.root.data(), sizeof o.root);
        dump(prefix + ".folded", changed.root.data(), sizeof changed.root);
        std::printf("as_stored=1 indices=%llu,%llu,%llu n_nodes=%zu honest=%u,%u,%u,%d changed=%u,%u,%u dropped=%u,%u\n", (unsigned long long)o.indices[0],
                    (unsigned long long)o.indices[1], (unsigned long long)o.indices[2], o.nodes.size() / 7, honest.verdict, honest.at, honest.n_merges,
                    (int)(honest.root == o.root), changed.verdict, changed.at, changed.n_merges, dropped.verdict, dropped.at);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
