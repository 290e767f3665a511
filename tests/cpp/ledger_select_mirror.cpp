// cstark::Ledger::select (include/cstark.hpp) the way an operator would use it.  The accounts and transfers of
// TransactionMetadata::build_random(16, depth 3, seed 3) are signed with Ledger::sign (the senders' secrets recovered from
// cstark::schnorr_public_keys, as sign_mirror.cpp does); the pool is that batch with one scalar bit flipped in candidate 5 and a
// self transfer spliced in at position 9.  The program selects read-only (the library's chunk and chunk 3), then selects with the cut to
// a power of two and applies on one ledger, and applies that selection's transfers with Ledger::apply_checked on a twin.
// usage: ledger_select_mirror <out_prefix>   writes <prefix>.idx (accounts, u64), .val ([..][14] u64), .s .r .d ([17] u64), .rx ([17][6] u64),
// .ss ([17][32] bytes), .status ([17] bytes), .selected (u32), .msg ([17][28] u64), .applied (u32: the applied selection), .root (7 u64: the root
// it leaves); prints a summary
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

        cstark::Ledger ledger(ctx, 3), twin(ctx, 3);
        ledger.set_accounts(indices, values);
        twin.set_accounts(indices, values);
        cstark::Transfers pool = ledger.sign(cstark::Transfers{ref.s_indices, ref.r_indices, ref.deltas, {}, {}}, secrets, 11, 256);
        pool.sig_s[5][3] ^= 0x04;
        pool.s_indices.insert(pool.s_indices.begin() + 9, ref.s_indices[12]);
        pool.r_indices.insert(pool.r_indices.begin() + 9, ref.s_indices[12]);
        pool.deltas.insert(pool.deltas.begin() + 9, ref.deltas[12]);
        pool.sig_rx.insert(pool.sig_rx.begin() + 9, pool.sig_rx[12]);
        pool.sig_s.insert(pool.sig_s.begin() + 9, pool.sig_s[12]);
        const size_t n = pool.s_indices.size();
        dump(prefix + ".idx", indices.data(), indices.size() * 8);
        dump(prefix + ".val", values[0].data(), values.size() * sizeof values[0]);
        dump(prefix + ".s", pool.s_indices.data(), n * 8);
        dump(prefix + ".r", pool.r_indices.data(), n * 8);
        dump(prefix + ".d", pool.deltas.data(), n * 8);
        dump(prefix + ".rx", pool.sig_rx[0].data(), n * 48);
        dump(prefix + ".ss", pool.sig_s[0].data(), n * 32);

        // read-only, with the library's chunk and with passes of three
        const cstark::Hash root_before = ledger.root();
        const uint32_t flags = CSTARK_SELECT_CHECK_SIGNATURES;
        const cstark::Ledger::Selection whole = ledger.select(pool, 16, flags, 0, true);
        const cstark::Ledger::Selection passes = ledger.select(pool, 16, flags, 3, true);
        const bool read_only = ledger.root() == root_before && ledger.accounts(indices) == values;
        bool chunk_free = whole.status == passes.status && whole.selected == passes.selected && whole.report.n_chunks == 1 && passes.report.n_chunks > 1;
        for (const uint32_t t : whole.selected) chunk_free = chunk_free && whole.messages[t] == passes.messages[t];
        dump(prefix + ".status", whole.status.data(), n);
        dump(prefix + ".selected", whole.selected.data(), whole.selected.size() * 4);
        dump(prefix + ".msg", whole.messages[0].data(), n * 224);

        // selected and applied in one call, against apply_checked of the selection's transfers on the twin
        // (cut to a power of two: a prefix of the selection above)
        const cstark::Ledger::Selection applied = ledger.select(pool, 16, flags | CSTARK_SELECT_POW2 | CSTARK_SELECT_APPLY);
        const cstark::TransactionMetadata m = twin.apply_checked(applied.transfers);
        const cstark::TransactionMetadata &w = applied.witness;
        const size_t k = applied.selected.size();
        dump(prefix + ".applied", applied.selected.data(), k * 4);
        const bool same = k && !(k & (k - 1)) && 2 * k > whole.selected.size() && k <= whole.selected.size() &&
                          std::equal(applied.selected.begin(), applied.selected.end(), whole.selected.begin()) && w.len() == m.len() && w.initial_roots == m.initial_roots &&
                          w.final_root == m.final_root && w.s_old_values == m.s_old_values && w.r_old_values == m.r_old_values && w.s_indices == m.s_indices &&
                          w.r_indices == m.r_indices && w.s_paths == m.s_paths && w.r_paths == m.r_paths && w.deltas == m.deltas && w.sig_rx == m.sig_rx &&
                          w.sig_s == m.sig_s && ledger.root() == twin.root() && std::memcmp(applied.report.root_after, m.final_root.data(), 56) == 0;
        const cstark::Hash root = ledger.root();
        dump(prefix + ".root", root.data(), sizeof root);
        std::printf("n=%zu selected=%zu read_only=%d chunk_free=%d same=%d\n", n, whole.selected.size(), (int)read_only, (int)chunk_free, (int)same);
        return read_only && chunk_free && same ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
