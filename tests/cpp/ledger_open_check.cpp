// csrc/ledger_plan.h alone under g++ (host code only): plan_open, the read side of the account ledger.  An index is built by running
// plan_set_accounts and plan_apply with the host executor (the host `merge` of hostgadgets.h over a host pool, as
// tests/cpp/ledger_plan_check.cpp does), then plan_open's emit list is run on that pool and every opened path is folded to the root
// with the host `merge`.  Every emit must stay inside the pool and inside the staging area.  Covers accounts, absent indices, the
// same index twice, an empty ledger, an index out of range, and depths 1 .. 31.
//   ledger_open_check                all checks; prints one "ok" line per depth
//   ledger_open_check --time FILE    instead: seconds the folds of the paths in FILE take on this CPU (tools/bench_ledger_paths.py)
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <string>
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

// upload block, launches in order, commit emits: the writing plans on the host pool
static void execute(const Plan &p, Words &pool, size_t stored_words) {
    if (pool.size() < 7 * p.pool_slots) pool.resize(7 * p.pool_slots);
    uint64_t *block = &pool[(size_t)7 * p.upload_slot];
    if (!p.upload.empty()) memcpy(block, p.upload.data(), 8 * p.upload.size());
    std::vector<Job> jobs(p.jobs.size());
    if (!jobs.empty()) memcpy(jobs.data(), block + p.jobs_word, 16 * jobs.size());
    for (const Job &q : jobs) {
        if (q.left >= p.pool_slots || q.right >= p.pool_slots || q.out >= p.pool_slots) { CHECK(false, "a job names a slot outside the pool"); continue; }
        uint64_t out[7];
        cs::hostg::merge(&pool[(size_t)7 * q.left], &pool[(size_t)7 * q.right], out);
        memcpy(&pool[(size_t)7 * q.out], out, 56);
    }
    std::vector<Emit> ce(p.commit.size());
    if (!ce.empty()) memcpy(ce.data(), block + p.commit_word, 8 * ce.size());
    for (const Emit &m : ce) {
        if ((size_t)m.word + 7 > stored_words || m.slot >= p.pool_slots) { CHECK(false, "a commit emit is out of range"); continue; }
        memcpy(&pool[m.word], &pool[(size_t)7 * m.slot], 56);
    }
}

struct Ledger {
    Index ix;
    Words pool;
    uint32_t scratch_base;
    Ledger(uint32_t depth, uint32_t reserve_nodes) : ix(depth), scratch_base(EMPTY_SLOTS + reserve_nodes) {
        pool.assign((size_t)7 * scratch_base, 0);
        Plan p;
        plan_empty_digests(depth, scratch_base, p);
        execute(p, pool, (size_t)7 * scratch_base);
    }
    const uint64_t *root() const { return &pool[(size_t)7 * ix.root_slot()]; }
};

static bool same(const uint64_t *a, const uint64_t *b) { return memcmp(a, b, 56) == 0; }

// plan_open on `indices`, its emit list run on the pool as the device runs it; every path folded to the root
static void open_and_fold(Ledger &L, const Words &indices, const char *what) {
    const uint32_t d = L.ix.depth, count = (uint32_t)indices.size();
    const Index before = L.ix;
    const Words stored(L.pool.begin(), L.pool.begin() + (size_t)7 * L.scratch_base);
    Plan p;
    CHECK(plan_open(L.ix, L.scratch_base, count, indices.data(), p), "%s: plan_open refused", what);
    const size_t n = (size_t)count * (d + 1);
    CHECK(p.witness.size() == n && p.jobs.empty() && p.commit.empty() && p.new_nodes.empty() && p.new_values.empty() && p.launch.empty(),
          "%s: an opening is one emit list of count (depth + 1) entries and nothing else", what);
    CHECK(p.upload_slot == L.scratch_base && p.stage_slot >= p.upload_slot + (n + 6) / 7 && p.stage_slot + n <= p.pool_slots &&
              p.pool_slots - L.scratch_base == open_scratch_slots(d, count),
          "%s: list and staging area do not fit the scratch the caller reserves", what);
    if (L.pool.size() < 7 * p.pool_slots) L.pool.resize(7 * p.pool_slots, 0xDEADBEEFDEADBEEFull);
    uint64_t *block = &L.pool[(size_t)7 * p.upload_slot];
    memcpy(block, p.upload.data(), 8 * p.upload.size());
    std::vector<Emit> list(n);
    memcpy(list.data(), block + p.witness_word, 8 * n);
    uint64_t *stage = &L.pool[(size_t)7 * p.stage_slot];
    std::vector<bool> written(n, false);
    for (size_t m = 0; m < n; m++) {
        const Emit &em = list[m];
        if (em.slot >= L.scratch_base || (size_t)em.word + 7 > 7 * n || em.word % 7) { CHECK(false, "%s: emit %zu leaves the stored nodes or the staging area", what, m); continue; }
        CHECK(!written[em.word / 7], "%s: emit %zu writes a staging slot twice", what, m);
        written[em.word / 7] = true;
        memcpy(stage + em.word, &L.pool[(size_t)7 * em.slot], 56);
    }
    CHECK(same(&L.pool[(size_t)7 * p.final_root_slot], L.root()), "%s: the plan names another root slot", what);
    for (uint32_t i = 0; i < count; i++) {
        const uint64_t *path = stage + (size_t)7 * (d + 1) * i;
        uint64_t leaf[7] = {0}, cur[7], t[7];
        const auto it = L.ix.accounts.find(indices[i]);
        if (it != L.ix.accounts.end()) cs::hostg::merge(it->second.data(), it->second.data() + 7, leaf);
        CHECK(same(path, leaf), "%s: path %u: the leaf is not the account's (all-zero for an absent one)", what, i);
        memcpy(cur, path, 56);
        for (uint32_t k = 0; k < d; k++) {
            const uint64_t *sib = path + 7 * (k + 1);
            if ((indices[i] >> k) & 1) cs::hostg::merge(sib, cur, t);
            else cs::hostg::merge(cur, sib, t);
            memcpy(cur, t, 56);
        }
        CHECK(same(cur, L.root()), "%s: path %u (index %llu) does not fold to the root", what, i, (unsigned long long)indices[i]);
    }
    CHECK(L.ix.n_stored == before.n_stored && L.ix.node == before.node && L.ix.accounts == before.accounts, "%s: an opening changed the index", what);
    CHECK(memcmp(stored.data(), L.pool.data(), 8 * stored.size()) == 0, "%s: an opening changed the stored nodes", what);
}

static void one_depth(uint32_t d) {
    using cs::host::from_u64;
    const uint64_t size = (uint64_t)1 << d, top = size - 1;
    // accounts at both ends of the tree, a pair of siblings in the middle and one leaf on its own, as far as the depth has room
    Words acc = {0, top};
    for (uint64_t x : {size / 2, size / 2 + 1, size / 3})
        if (x < size && std::find(acc.begin(), acc.end(), x) == acc.end()) acc.push_back(x);
    const uint32_t na = (uint32_t)acc.size();
    Words val((size_t)14 * na);
    for (size_t i = 0; i < val.size(); i++) val[i] = from_u64(1000 + 17 * i);
    Ledger L(d, (na + 8) * (d + 1) + 16);

    // an empty ledger opens to empty-subtree digests
    open_and_fold(L, {0, top, 0}, "empty ledger");
    {
        Plan p;
        CHECK(plan_set_accounts(L.ix, L.scratch_base, na, acc.data(), val.data(), p), "set_accounts");
        execute(p, L.pool, (size_t)7 * L.scratch_base);
        commit(L.ix, p);
    }
    Words ask = acc;
    for (uint64_t x : acc)
        for (uint64_t y : {x ^ 1, x + 2, x - 2})
            if (y < size && !L.ix.accounts.count(y)) ask.push_back(y); // absent neighbours
    ask.push_back(acc[0]);
    ask.push_back(top); // duplicates
    open_and_fold(L, ask, "after set_accounts");
    {
        // two transfers between the ends: stored nodes are overwritten and new ones appear
        const Words s = {0, top}, r = {top, 0}, dl = {from_u64(5), from_u64(3)};
        Plan p;
        CHECK(plan_apply(L.ix, L.scratch_base, 2, s.data(), r.data(), dl.data(), p) && p.refused_at == -1, "apply");
        execute(p, L.pool, (size_t)7 * L.scratch_base);
        commit(L.ix, p);
    }
    open_and_fold(L, ask, "after apply");
    open_and_fold(L, {top}, "one path");
    {
        Plan p, q, r;
        const uint64_t big = size, huge = ~(uint64_t)0;
        const Words mixed = {0, big};
        CHECK(!plan_open(L.ix, L.scratch_base, 1, &big, p), "index 2^depth was accepted");
        CHECK(!plan_open(L.ix, L.scratch_base, 1, &huge, q), "index 2^64 - 1 was accepted");
        CHECK(!plan_open(L.ix, L.scratch_base, 2, mixed.data(), r), "index 2^depth behind a good one was accepted");
        CHECK(!plan_open(L.ix, L.scratch_base, 0, mixed.data(), r), "count 0 was accepted");
    }
    printf("ok: depth %u, %u accounts, %zu paths opened and folded\n", d, na, ask.size());
}

// tools/bench_ledger_paths.py: FILE holds count, depth, indices [count], paths [count][depth + 1][7] as little-endian 64-bit words; every
// path is folded with the host `merge`, one after the other, and the roots go to FILE.roots
static int time_folds(const char *file) {
    FILE *f = fopen(file, "rb");
    uint64_t h[2];
    if (!f || fread(h, 8, 2, f) != 2 || h[0] == 0 || h[0] > MAX_TRANSFERS || h[1] == 0 || h[1] > MAX_DEPTH) { printf("cannot read %s\n", file); return 2; }
    const size_t count = h[0], d = h[1];
    Words idx(count), paths(count * (d + 1) * 7), roots(count * 7);
    const bool ok = fread(idx.data(), 8, idx.size(), f) == idx.size() && fread(paths.data(), 8, paths.size(), f) == paths.size();
    fclose(f);
    if (!ok) { printf("%s is too short\n", file); return 2; }
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t i = 0; i < count; i++) {
        const uint64_t *path = &paths[i * (d + 1) * 7];
        uint64_t cur[7], t[7];
        memcpy(cur, path, 56);
        for (size_t k = 0; k < d; k++) {
            if ((idx[i] >> k) & 1) cs::hostg::merge(path + 7 * (k + 1), cur, t);
            else cs::hostg::merge(cur, path + 7 * (k + 1), t);
            memcpy(cur, t, 56);
        }
        memcpy(&roots[7 * i], cur, 56);
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    FILE *g = fopen((std::string(file) + ".roots").c_str(), "wb");
    if (!g || fwrite(roots.data(), 8, roots.size(), g) != roots.size()) { printf("cannot write the roots\n"); return 2; }
    fclose(g);
    printf("ok: %zu paths of depth %zu, %zu merges seconds=%.6f\n", count, d, count * d, seconds);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && std::string(argv[1]) == "--time") return time_folds(argv[2]);
    for (uint32_t d : {1u, 2u, 3u, 7u, 15u, 31u}) one_depth(d);
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    return 0;
}
