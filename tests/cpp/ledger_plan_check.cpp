// csrc/ledger_plan.h alone under g++ (host code only): the plans of the account ledger are executed here with the host `merge`
// (hostgadgets.h) over a host pool, exactly as the device executes them -- upload block, one pass per launch, emit lists -- and every
// witness array is compared with a case written by tests/ledger_cases.py (flat little-endian 64-bit words, see read_case).
//   ledger_plan_check CASE          all checks; a case that ends in the pair (refused_at, reason) is a batch the plan must refuse there
//                                   (expect_refused_batch), any other case a batch it must apply
//   ledger_plan_check CASE --time   additionally: seconds the job lists of the whole batch take on this CPU (tools/bench_ledger.py)
#include <stdio.h>
#include <stdlib.h>
#include <chrono>
#include <string>
#include <unordered_set>
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

struct Case {
    uint32_t depth, n_acc, n_tx;
    uint64_t absent; // an index without an account, UINT64_MAX when every leaf has one
    Words acc_idx, acc_val, final_val, initial_roots, final_root, s_old, r_old, s_idx, r_idx, s_paths, r_paths, deltas;
    bool refusal = false; // the case ends in a pair of words: the plan must refuse the batch at transfer `refused_at` for `reason`
    uint32_t refused_at = 0;
    int32_t reason = REASON_NONE;
};

static bool read_case(const char *path, Case &c) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint64_t h[4];
    if (fread(h, 8, 4, f) != 4) { fclose(f); return false; }
    c.depth = (uint32_t)h[0]; c.n_acc = (uint32_t)h[1]; c.n_tx = (uint32_t)h[2]; c.absent = h[3];
    const size_t n = c.n_tx, a = c.n_acc, d = c.depth;
    struct { Words *w; size_t len; } parts[] = {{&c.acc_idx, a}, {&c.acc_val, 14 * a}, {&c.final_val, 14 * a}, {&c.initial_roots, 7 * n}, {&c.final_root, 7},
                                               {&c.s_old, 14 * n}, {&c.r_old, 14 * n}, {&c.s_idx, n}, {&c.r_idx, n}, {&c.s_paths, 7 * (d + 1) * n},
                                               {&c.r_paths, 7 * (d + 1) * n}, {&c.deltas, n}};
    bool ok = true;
    for (auto &p : parts) {
        p.w->resize(p.len);
        if (p.len && fread(p.w->data(), 8, p.len, f) != p.len) ok = false;
    }
    uint64_t extra[3];
    const size_t trailing = fread(extra, 8, 3, f); // none, or the expected refusal
    if (trailing == 2 && extra[0] < c.n_tx && extra[1] >= REASON_INDEX && extra[1] <= REASON_BALANCE) {
        c.refusal = true; c.refused_at = (uint32_t)extra[0]; c.reason = (int32_t)extra[1];
    } else if (trailing != 0) ok = false;
    fclose(f);
    return ok;
}

// the device's work on the host: copy the upload block into the pool, run the launches in order (reading the lists from the pool,
// where the device reads them), then the two emit lists.  Returns the number of merges.
static size_t execute(const Plan &p, Words &pool, Words *witness, size_t stored_words, bool check_launches = true) {
    if (pool.size() < 7 * p.pool_slots) pool.resize(7 * p.pool_slots);
    uint64_t *block = &pool[(size_t)7 * p.upload_slot];
    if (!p.upload.empty()) memcpy(block, p.upload.data(), 8 * p.upload.size());
    std::vector<Job> jobs(p.jobs.size());
    if (!jobs.empty()) memcpy(jobs.data(), block + p.jobs_word, 16 * jobs.size());
    for (size_t k = 0; k + 1 < p.launch.size(); k++) {
        if (check_launches) { // no job of a launch reads what a job of the same launch writes, and no slot is written twice
            std::unordered_set<uint32_t> outs;
            for (uint32_t j = p.launch[k]; j < p.launch[k + 1]; j++) CHECK(outs.insert(jobs[j].out).second, "launch %zu writes slot %u twice", k, jobs[j].out);
            for (uint32_t j = p.launch[k]; j < p.launch[k + 1]; j++)
                CHECK(!outs.count(jobs[j].left) && !outs.count(jobs[j].right), "launch %zu, job %u reads a slot the launch writes", k, j);
        }
        for (uint32_t j = p.launch[k]; j < p.launch[k + 1]; j++) {
            const Job &q = jobs[j];
            if (q.left >= p.pool_slots || q.right >= p.pool_slots || q.out >= p.pool_slots) { CHECK(false, "job %u names a slot outside the pool", j); continue; }
            uint64_t out[7];
            cs::hostg::merge(&pool[(size_t)7 * q.left], &pool[(size_t)7 * q.right], out);
            memcpy(&pool[(size_t)7 * q.out], out, 56);
        }
    }
    const Emit *we = (const Emit *)(block + p.witness_word), *ce = (const Emit *)(block + p.commit_word);
    for (size_t i = 0; i < p.witness.size(); i++) {
        if (!witness || (size_t)we[i].word + 7 > witness->size() || we[i].slot >= p.pool_slots) { CHECK(false, "witness emit %zu out of range", i); continue; }
        memcpy(&(*witness)[we[i].word], &pool[(size_t)7 * we[i].slot], 56);
    }
    for (size_t i = 0; i < p.commit.size(); i++) {
        if ((size_t)ce[i].word + 7 > stored_words || ce[i].slot >= p.pool_slots) { CHECK(false, "commit emit %zu out of range", i); continue; }
        memcpy(&pool[ce[i].word], &pool[(size_t)7 * ce[i].slot], 56);
    }
    return jobs.size();
}

static bool same(const uint64_t *a, const uint64_t *b, size_t n) { return n == 0 || memcmp(a, b, 8 * n) == 0; }

struct Ledger {
    Index ix;
    Words pool;
    uint32_t scratch_base;
    Ledger(uint32_t depth, uint32_t reserve_nodes) : ix(depth), scratch_base(EMPTY_SLOTS + reserve_nodes) {
        pool.assign((size_t)7 * scratch_base, 0);
        Plan p;
        plan_empty_digests(depth, scratch_base, p);
        execute(p, pool, nullptr, (size_t)7 * scratch_base);
    }
    const uint64_t *root() const { return &pool[(size_t)7 * ix.root_slot()]; }
    bool set_accounts(uint32_t count, const uint64_t *idx, const uint64_t *val) {
        Plan p;
        if (!plan_set_accounts(ix, scratch_base, count, idx, val, p)) return false;
        CHECK(EMPTY_SLOTS + ix.n_stored + p.new_nodes.size() <= scratch_base, "stored nodes run into the scratch");
        execute(p, pool, nullptr, (size_t)7 * scratch_base);
        commit(ix, p);
        return true;
    }
};

// the witness of transfers [t0, t0 + n) of the case applied to `L`, compared with the case's arrays
static size_t apply_and_compare(Ledger &L, const Case &c, uint32_t t0, uint32_t n, const char *what, double *seconds = nullptr) {
    const uint32_t d = c.depth;
    Plan p;
    const bool planned = plan_apply(L.ix, L.scratch_base, n, &c.s_idx[t0], &c.r_idx[t0], &c.deltas[t0], p);
    CHECK(planned && p.refused_at == -1 && p.reason == REASON_NONE, "%s: the batch was refused at %d (reason %d)", what, p.refused_at, p.reason);
    if (!planned || p.refused_at != -1) return 0;
    CHECK(p.launch.size() == d + 2, "%s: %zu launches, expected depth + 1", what, p.launch.size() - 1);
    CHECK(EMPTY_SLOTS + L.ix.n_stored + p.new_nodes.size() <= L.scratch_base, "stored nodes run into the scratch");
    size_t sz[cs::WIT_NUM_SEGMENTS], off[cs::WIT_NUM_SEGMENTS + 1];
    cs::witness_segments(n, d, sz, off);
    Words wit(off[cs::WIT_NUM_SEGMENTS] / 8, 0xDEADBEEFDEADBEEFull);
    const auto t_start = std::chrono::steady_clock::now();
    const size_t merges = execute(p, L.pool, &wit, (size_t)7 * L.scratch_base, seconds == nullptr);
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    uint64_t final_root[7];
    memcpy(final_root, &L.pool[(size_t)7 * p.final_root_slot], 56);
    commit(L.ix, p);
    const size_t path = (size_t)7 * (d + 1);
    CHECK(same(&wit[off[cs::WIT_INITIAL_ROOTS] / 8], &c.initial_roots[(size_t)7 * t0], (size_t)7 * n), "%s: initial_roots differ", what);
    CHECK(same(&wit[off[cs::WIT_S_OLD] / 8], &c.s_old[(size_t)14 * t0], (size_t)14 * n), "%s: s_old_values differ", what);
    CHECK(same(&wit[off[cs::WIT_R_OLD] / 8], &c.r_old[(size_t)14 * t0], (size_t)14 * n), "%s: r_old_values differ", what);
    CHECK(same(&wit[off[cs::WIT_S_PATHS] / 8], &c.s_paths[path * t0], path * n), "%s: s_paths differ", what);
    CHECK(same(&wit[off[cs::WIT_R_PATHS] / 8], &c.r_paths[path * t0], path * n), "%s: r_paths differ", what);
    const uint64_t *expect_root = t0 + n == c.n_tx ? c.final_root.data() : &c.initial_roots[(size_t)7 * (t0 + n)];
    CHECK(same(final_root, expect_root, 7), "%s: the root after the batch differs", what);
    CHECK(same(L.root(), expect_root, 7), "%s: the stored root after the batch differs", what);
    return merges;
}

static void expect_refusal(const Ledger &L, const Case &c, uint32_t at, Words s, Words r, Words dl, int32_t reason, const char *what) {
    Plan p;
    const bool planned = plan_apply(L.ix, L.scratch_base, c.n_tx, s.data(), r.data(), dl.data(), p);
    CHECK(planned && p.refused_at == (int32_t)at && p.reason == reason, "%s: refused_at %d reason %d, expected %u / %d", what, p.refused_at, p.reason, at, reason);
    CHECK(p.jobs.empty() && p.witness.empty() && p.commit.empty() && p.new_nodes.empty() && p.new_values.empty(), "%s: a refused plan carries work", what);
}

// A case with an expected refusal: the arrays describe transfers [0, refused_at) only (initial_roots[refused_at] is the root they
// leave, final_val the accounts they leave).  The whole batch must be refused at that transfer for that reason without a change to the
// index; the ledger then applies the valid prefix.
static int expect_refused_batch(const Case &c) {
    const uint32_t d = c.depth, n = c.n_tx, na = c.n_acc, at = c.refused_at;
    Ledger L(d, (na + 4 * n) * (d + 1) + 16);
    CHECK(L.set_accounts(na, c.acc_idx.data(), c.acc_val.data()), "set_accounts");
    CHECK(same(L.root(), c.initial_roots.data(), 7), "the root after set_accounts is not initial_roots[0]");
    const Index before = L.ix;
    const Words pool_before = L.pool;
    expect_refusal(L, c, at, c.s_idx, c.r_idx, c.deltas, c.reason, "the steered batch");
    CHECK(L.ix.depth == before.depth && L.ix.n_stored == before.n_stored && L.ix.node == before.node && L.ix.accounts == before.accounts,
          "a refused plan changed the index");
    CHECK(L.pool == pool_before, "a refused plan changed the pool");
    size_t merges = 0;
    if (at > 0) merges = apply_and_compare(L, c, 0, at, "the valid prefix");
    for (uint32_t i = 0; i < na; i++) {
        const auto it = L.ix.accounts.find(c.acc_idx[i]);
        CHECK(it != L.ix.accounts.end() && same(it->second.data(), &c.final_val[(size_t)14 * i], 14), "account %u: value after the valid prefix differs", i);
    }
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("ok: depth %u, %u accounts, refused at %u of %u (reason %d), %zu merges in the valid prefix\n", d, na, at, n, c.reason, merges);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: ledger_plan_check CASE [--time]\n"); return 2; }
    const bool timing = argc > 2 && std::string(argv[2]) == "--time";
    Case c;
    if (!read_case(argv[1], c)) { printf("cannot read %s\n", argv[1]); return 2; }
    if (c.refusal) return expect_refused_batch(c);
    const uint32_t d = c.depth, n = c.n_tx, na = c.n_acc;
    const uint32_t reserve = (na + 4 * n) * (d + 1) + 16;

    // an empty ledger: depth merges of the zero digest
    Ledger L(d, reserve);
    {
        uint64_t e[7] = {0}, t[7];
        for (uint32_t l = 0; l < d; l++) { cs::hostg::merge(e, e, t); memcpy(e, t, 56); }
        CHECK(same(L.root(), e, 7), "the empty ledger's root");
    }
    // set_accounts in two calls, in one call on a second ledger, and an overwrite
    const uint32_t h = na / 2;
    CHECK(h == 0 || L.set_accounts(h, c.acc_idx.data(), c.acc_val.data()), "set_accounts, first half");
    CHECK(L.set_accounts(na - h, &c.acc_idx[h], &c.acc_val[(size_t)14 * h]), "set_accounts, second half");
    CHECK(same(L.root(), c.initial_roots.data(), 7), "the root after set_accounts is not initial_roots[0]");
    Ledger one(d, reserve);
    CHECK(one.set_accounts(na, c.acc_idx.data(), c.acc_val.data()) && same(one.root(), L.root(), 7), "one call and two calls give different roots");
    CHECK(one.set_accounts(na, c.acc_idx.data(), c.final_val.data()), "overwrite with the final values");
    // misuse of set_accounts: an index twice, an index out of range
    {
        Plan p;
        Words twice = {c.acc_idx[0], c.acc_idx[0]}, vals(28, 1);
        CHECK(!plan_set_accounts(L.ix, L.scratch_base, 2, twice.data(), vals.data(), p), "an index given twice was accepted");
        Plan q;
        const uint64_t big = (uint64_t)1 << d;
        CHECK(!plan_set_accounts(L.ix, L.scratch_base, 1, &big, vals.data(), q), "an index out of range was accepted");
    }
    // refusals, each in the middle of the otherwise valid batch; the plan reads the index only
    const uint32_t mid = n / 2;
    {
        Words s = c.s_idx, r = c.r_idx, dl = c.deltas;
        r[mid] = (uint64_t)1 << d;
        expect_refusal(L, c, mid, s, r, dl, REASON_INDEX, "receiver index 2^depth");
        r = c.r_idx; s[mid] = ~(uint64_t)0;
        expect_refusal(L, c, mid, s, r, dl, REASON_INDEX, "sender index 2^64 - 1");
        s = c.s_idx; r[mid] = s[mid];
        expect_refusal(L, c, mid, s, r, dl, REASON_SELF, "sender equals receiver");
        r = c.r_idx;
        if (c.absent != ~(uint64_t)0) {
            r[mid] = c.absent;
            expect_refusal(L, c, mid, s, r, dl, REASON_ABSENT, "absent receiver");
            r = c.r_idx; s[mid] = c.absent;
            expect_refusal(L, c, mid, s, r, dl, REASON_ABSENT, "absent sender");
            s = c.s_idx;
        }
        dl[mid] = cs::host::from_u64(cs::host::P - 1); // canonical p - 1: above every balance the generator draws
        expect_refusal(L, c, mid, s, r, dl, REASON_BALANCE, "delta above the balance");
        CHECK(same(L.root(), c.initial_roots.data(), 7), "a refusal changed the root");
    }
    // batches compose: the two halves applied one after the other (on a copy), then the whole batch
    if (n >= 2) {
        Ledger two = L;
        apply_and_compare(two, c, 0, mid, "first half");
        apply_and_compare(two, c, mid, n - mid, "second half");
    }
    double seconds = 0;
    const size_t merges = apply_and_compare(L, c, 0, n, "whole batch", timing ? &seconds : nullptr);
    for (uint32_t i = 0; i < na; i++) {
        const auto it = L.ix.accounts.find(c.acc_idx[i]);
        CHECK(it != L.ix.accounts.end() && same(it->second.data(), &c.final_val[(size_t)14 * i], 14), "account %u: final value differs", i);
    }
    CHECK(same(one.root(), c.final_root.data(), 7), "a ledger overwritten with the final values has another root than the applied one");
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("ok: depth %u, %u accounts, %u transfers, %zu merges in %u launches", d, na, n, merges, d + 1);
    if (timing) printf(" seconds=%.6f", seconds);
    printf("\n");
    return 0;
}
