// Exercises cstark::Ledger::open and cstark::check_account_paths (include/cstark.hpp) the way a client of a verified root would: the
// accounts of TransactionMetadata::build_random(2, depth 3, seed 2) go into a ledger, two of them and one absent index are opened, the
// opening is checked, then one word of it is changed and it is checked again.
// usage: ledger_paths_mirror <out_prefix>      writes <prefix>.paths ([3][4][7] u64), <prefix>.root (7 u64), <prefix>.folded ([3][7]
//        u64, of the changed opening) and prints the opened indices and both verdict vectors
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
        const cstark::AccountOpening o = ledger.open({indices[0], absent, indices[1]});
        const bool as_stored = o.root == ref.initial_roots[0] && o.root == ledger.root() && o.values[0] == values[0] && o.values[2] == values[1] &&
                               o.present == std::vector<uint8_t>{1, 0, 1};
        const std::vector<uint8_t> honest = cstark::check_account_paths(ctx, o.depth, o.indices, o.paths, {o.root}, &o.values, &o.present);
        // one word of the absent index's sibling at level 2 is changed
        std::vector<cstark::BaseElement> paths = o.paths;
        paths[(1 * 4 + 2) * 7 + 5] ^= 1;
        std::vector<cstark::BaseElement> folded;
        const std::vector<uint8_t> changed = cstark::check_account_paths(ctx, o.depth, o.indices, paths, {o.root}, &o.values, &o.present, &folded);
        dump(prefix + ".paths", o.paths.data(), 8 * o.paths.size());
        dump(prefix + ".root", o.root.data(), sizeof o.root);
        dump(prefix + ".folded", folded.data(), 8 * folded.size());
        std::printf("as_stored=%d indices=%llu,%llu,%llu honest=%d,%d,%d changed=%d,%d,%d\n", (int)as_stored, (unsigned long long)o.indices[0],
                    (unsigned long long)o.indices[1], (unsigned long long)o.indices[2], honest[0], honest[1], honest[2], changed[0], changed[1], changed[2]);
        return as_stored ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
