// Exercises cstark::Ledger::from_multiproof, known and partial_info (include/cstark.hpp) the way a prover that does not hold the state
// would: the accounts of TransactionMetadata::build_random(2, depth 3, seed 2) go into a full ledger, the batch's accounts and one absent
// index are opened with ONE multiproof, a partial ledger is built from it, and the batch is applied to both: the witnesses and roots must
// be equal field for field and the reference's.  Then a transfer that names an unopened account is refused as CSTARK_LEDGER_UNKNOWN, an
// unopened index throws, and an opening with one word changed gives no ledger (verdict ROOT).
// usage: ledger_partial_check      prints one line of results
#include <cstdio>
#include <map>
#include "cstark.hpp"

int main() {
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
        uint64_t absent = 0, unopened = 7;
        while (first.count(absent)) absent++;
        while (first.count(unopened) || unopened == absent) unopened--;

        cstark::Ledger full(ctx, 3);
        full.set_accounts(indices, values);
        std::vector<uint64_t> asked = indices;
        asked.push_back(absent);
        const cstark::AccountMultiOpening o = full.open_multi(asked);
        uint32_t verdict = 99;
        cstark::Ledger part = cstark::Ledger::from_multiproof(ctx, o, &verdict);
        const auto info = part.partial_info(), full_info = full.partial_info();
        const std::vector<uint8_t> known = part.known({indices[0], absent, unopened, 8}), full_known = full.known({indices[0], absent, unopened, 8});
        const bool built = verdict == CSTARK_MULTI_VALID && part.root() == o.root && info.is_partial && info.n_known == o.indices.size() &&
                           info.n_opaque == o.nodes.size() / 7 && !full_info.is_partial && full_info.n_known == indices.size() && full_info.n_opaque == 0 &&
                           known == std::vector<uint8_t>{1, 1, 0, 0} && full_known == std::vector<uint8_t>{1, 1, 1, 0};

        cstark::Transfers t;
        t.s_indices = ref.s_indices; t.r_indices = ref.r_indices; t.deltas = ref.deltas; t.sig_rx = ref.sig_rx; t.sig_s = ref.sig_s;
        // an unknown receiver in the second transfer: refused, nothing changed
        cstark::Transfers bad = t;
        bad.r_indices[1] = unopened;
        int refused_at = -1, reason = -1;
        try { part.apply(bad); } catch (const cstark::TransferRefused &e) { refused_at = e.index; reason = e.reason; }
        const bool unchanged = part.root() == o.root;
        int threw = 0;
        try { part.open({unopened}); } catch (const cstark::Error &) { threw++; }
        try { part.open_multi({indices[0], unopened}); } catch (const cstark::Error &) { threw++; }
        try { part.accounts({unopened}); } catch (const cstark::Error &) { threw++; }
        try { part.set_accounts({unopened}, {values[0]}); } catch (const cstark::Error &) { threw++; }

        const cstark::TransactionMetadata wf = full.apply(t), wp = part.apply(t);
        const bool same = wf.initial_roots == wp.initial_roots && wf.final_root == wp.final_root && wf.s_old_values == wp.s_old_values &&
                          wf.r_old_values == wp.r_old_values && wf.s_paths == wp.s_paths && wf.r_paths == wp.r_paths && wf.s_indices == wp.s_indices &&
                          wf.r_indices == wp.r_indices && wf.deltas == wp.deltas && wf.sig_rx == wp.sig_rx && wf.sig_s == wp.sig_s;
        const bool as_reference = wp.final_root == ref.final_root && wp.s_paths == ref.s_paths && wp.r_paths == ref.r_paths && part.root() == full.root();
        const bool audit_ok = part.audit().consistent == 1;

        cstark::AccountMultiOpening changed = o;
        changed.nodes[3] ^= 1;
        uint32_t bad_verdict = 99;
        int no_ledger = 0;
        try { cstark::Ledger p = cstark::Ledger::from_multiproof(ctx, changed, &bad_verdict); } catch (const cstark::Error &) { no_ledger = 1; }
        std::printf("built=%d refused=%d,%d unchanged=%d threw=%d same=%d as_reference=%d audit=%d tampered=%d,%u\n", (int)built, refused_at, reason, (int)unchanged,
                    threw, (int)same, (int)as_reference, (int)audit_ok, no_ledger, bad_verdict);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
