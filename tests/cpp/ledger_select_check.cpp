// The host half of cstark_ledger_select (csrc/ledger_plan.h: select_prepare, select_walk, select_chunk, select_finish, select_batch)
// alone under g++: the preparation runs once, the resumable walk is fed steered signature verdicts pass by pass at chunk sizes 1, 3
// and n, and the selection is handed to plan_apply, whose plan is executed with the host `merge` (hostgadgets.h) over a host pool as
// ledger_plan_check.cpp executes it.  The program checks that nothing but the number of checked signatures depends on the chunk size
// and prints statuses, selection, messages and the root the applied selection leaves; tests/test_ledger_select_cpu.py compares them
// with tests/select_model.py.
//   ledger_select_check CASE
// CASE: little-endian 64-bit words -- depth, n_acc, n, want, flags (1: signatures are checked, 2: pow2), n_known (0: a full ledger) |
// acc_idx [n_acc] | acc_val [n_acc][14] | known [n_known] ascending | s_idx, r_idx, deltas [n] | sig_rx [n][6] | then n bytes: the
// verdict (cstark_sig_verdict) the device would give candidate t
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../certificate-stark_amd/csrc/hostgadgets.h"
#include "../../certificate-stark_amd/csrc/ledger_plan.h"

using namespace cs::ledger;
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

// the device's work on the host: the upload block, the launches in order, the commit list (the witness is not looked at here)
static void execute(const Plan &p, Words &pool, size_t stored_words) {
    if (pool.size() < 7 * p.pool_slots) pool.resize(7 * p.pool_slots);
    uint64_t *block = &pool[(size_t)7 * p.upload_slot];
    if (!p.upload.empty()) memcpy(block, p.upload.data(), 8 * p.upload.size());
    std::vector<Job> jobs(p.jobs.size());
    if (!jobs.empty()) memcpy(jobs.data(), block + p.jobs_word, 16 * jobs.size());
    for (const Job &q : jobs) { // the lists are in launch order
        if (q.left >= p.pool_slots || q.right >= p.pool_slots || q.out >= p.pool_slots) { CHECK(false, "a job names a slot outside the pool"); continue; }
        uint64_t out[7];
        cs::hostg::merge(&pool[(size_t)7 * q.left], &pool[(size_t)7 * q.right], out);
        memcpy(&pool[(size_t)7 * q.out], out, 56);
    }
    std::vector<Emit> ce(p.commit.size());
    if (!ce.empty()) memcpy(ce.data(), block + p.commit_word, 8 * ce.size());
    for (const Emit &e : ce) {
        if ((size_t)e.word + 7 > stored_words || e.slot >= p.pool_slots) { CHECK(false, "a commit emit is out of range"); continue; }
        uint64_t digest[7];
        memcpy(digest, &pool[(size_t)7 * e.slot], 56);
        memcpy(&pool[e.word], digest, 56);
    }
}

struct Run {
    Selection s;
    uint32_t n_checked = 0, n_chunks = 0;
    std::vector<uint8_t> sent; // [n] the candidate went up in a pass
};

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: ledger_select_check CASE\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot read %s\n", argv[1]); return 2; }
    uint64_t head[6];
    if (fread(head, 8, 6, f) != 6) { fclose(f); printf("short case\n"); return 2; }
    const uint32_t depth = (uint32_t)head[0], n_acc = (uint32_t)head[1], n = (uint32_t)head[2], want = (uint32_t)head[3], flags = (uint32_t)head[4],
                   n_known = (uint32_t)head[5];
    Words acc_idx, acc_val, known, s_idx, r_idx, deltas, sig_rx;
    std::vector<uint8_t> verdicts(n);
    const bool ok = read_words(f, acc_idx, n_acc) && read_words(f, acc_val, (size_t)14 * n_acc) && read_words(f, known, n_known) && read_words(f, s_idx, n) &&
                    read_words(f, r_idx, n) && read_words(f, deltas, n) && read_words(f, sig_rx, (size_t)6 * n) && fread(verdicts.data(), 1, n, f) == n;
    fclose(f);
    if (!ok || n == 0 || depth == 0 || depth > MAX_DEPTH) { printf("short case\n"); return 2; }
    const bool check = flags & 1, pow2 = flags & 2;

    // the ledger: an empty tree, then the accounts
    Index ix(depth);
    const uint32_t scratch_base = EMPTY_SLOTS + (n_acc + 4 * n) * (depth + 1) + 16;
    const size_t stored_words = (size_t)7 * scratch_base;
    Words pool(stored_words, 0);
    {
        Plan e, a;
        plan_empty_digests(depth, scratch_base, e);
        execute(e, pool, stored_words);
        CHECK(plan_set_accounts(ix, scratch_base, n_acc, acc_idx.data(), acc_val.data(), a), "set_accounts");
        execute(a, pool, stored_words);
        commit(ix, a);
    }
    if (n_known) { // what the walk reads of a partial ledger: the leaves it knows
        ix.partial = true;
        ix.known = known;
        ix.opaque.resize(depth + 1);
    }

    const uint32_t chunks[3] = {1, 3, n};
    Run runs[3];
    for (int v = 0; v < 3; v++) {
        Run &run = runs[v];
        run.sent.assign(n, 0);
        select_prepare(ix, n, s_idx.data(), r_idx.data(), deltas.data(), check ? sig_rx.data() : nullptr, want, check, run.s);
        std::vector<uint32_t> list;
        while (!select_walk(run.s)) {
            CHECK(check, "the walk asks for a verdict though signatures are not checked");
            select_chunk(run.s, chunks[v], list);
            CHECK(!list.empty() && list[0] == run.s.at && list.size() <= chunks[v], "chunk %u: a pass of %zu entries that starts at %u, the walk stands at %u", chunks[v],
                  list.size(), list.empty() ? 0 : list[0], run.s.at);
            if (list.empty() || list[0] != run.s.at) { printf("%d checks failed\n", failures); return 1; }
            for (size_t j = 0; j < list.size(); j++) {
                const uint32_t t = list[j];
                CHECK(t < n && (j == 0 || list[j - 1] < t) && !run.sent[t], "chunk %u: candidate %u goes up twice or out of order", chunks[v], t);
                CHECK(run.s.fixed[t] == REASON_NONE && run.s.rx_ok[t], "chunk %u: candidate %u is not checkable and goes up", chunks[v], t);
                run.sent[t] = 1;
                run.s.verdict[t] = verdicts[t];
            }
            run.n_checked += (uint32_t)list.size();
            run.n_chunks++;
        }
        select_finish(run.s, pow2);
    }
    for (int v = 0; v < 2; v++) {
        CHECK(runs[v].s.status == runs[2].s.status, "the statuses at chunk %u differ from those at chunk n", chunks[v]);
        CHECK(runs[v].s.selected == runs[2].s.selected, "the selection at chunk %u differs from that at chunk n", chunks[v]);
    }
    CHECK(runs[0].n_checked <= runs[2].n_checked, "one candidate per pass checked more signatures than one pass for all");
    const Selection &s = runs[2].s;
    CHECK(s.n_selected == s.selected.size() && s.n_selected <= want, "%u selected, want %u", s.n_selected, want);

    printf("status");
    for (uint32_t t = 0; t < n; t++) printf(" %u", s.status[t]);
    printf("\nselected");
    for (const uint32_t t : s.selected) printf(" %u", t);
    printf("\n");
    if (check)
        for (uint32_t t = 0; t < n; t++) {
            if (!(s.status[t] == REASON_NONE || (s.status[t] == REASON_SIGNATURE && s.rx_ok[t]))) continue;
            for (int v = 0; v < 3; v++) CHECK(runs[v].sent[t], "candidate %u got its status from a verdict and never went up at chunk %u", t, chunks[v]);
            uint64_t m[28];
            select_message(s, t, m);
            printf("message %u", t);
            for (int k = 0; k < 28; k++) printf(" %016llx", (unsigned long long)m[k]);
            printf("\n");
        }

    // the selection goes to plan_apply unchanged
    if (s.n_selected) {
        Words bs, br, bd;
        select_batch(s, s_idx.data(), r_idx.data(), deltas.data(), bs, br, bd);
        Plan p;
        const bool planned = plan_apply(ix, scratch_base, s.n_selected, bs.data(), br.data(), bd.data(), p);
        CHECK(planned && p.refused_at == -1, "the plan refuses selected candidate %d (reason %d)", p.refused_at, p.reason);
        if (planned && p.refused_at == -1) {
            execute(p, pool, stored_words);
            commit(ix, p);
        }
    }
    printf("root");
    for (int k = 0; k < 7; k++) printf(" %016llx", (unsigned long long)pool[(size_t)7 * ix.root_slot() + k]);
    printf("\nchecked %u %u %u passes %u %u %u\n", runs[0].n_checked, runs[1].n_checked, runs[2].n_checked, runs[0].n_chunks, runs[1].n_chunks, runs[2].n_chunks);
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
