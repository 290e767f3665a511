// csrc/multiproof_plan.h alone under g++ (host code only): multiproof_shape, plan_open_multi and plan_check, the plans of the ledger's
// multi-openings.  An index is built by running plan_set_accounts and plan_apply with the host executor (the host `merge` of
// hostgadgets.h over a host pool, as tests/cpp/ledger_open_check.cpp does).  Then, for sparse and dense sets of leaves, plan_open_multi's
// emit list is run on that pool as the device runs it, and plan_check's job lists are run level by level on a host block of digest slots
// that remembers which slots are defined: every source of a job must be a leaf, a proof node or an output of a DEEPER level, every slot
// and every emit must be in bounds, every proof node must be read exactly once, and the fold must be the root the host tree has.
//   ledger_multi_check               all checks; prints one "ok" line per depth
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <set>
#include <string>
#include <vector>
#include "../../certificate-stark_amd/csrc/hostgadgets.h"
#include "../../certificate-stark_amd/csrc/multiproof_plan.h"

using namespace cs::ledger;
namespace M = cs::multi;
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

// n_nodes and n_merges by plain sets
static void brute_shape(uint32_t d, const Words &indices, uint32_t *n_nodes, uint32_t *n_merges) {
    std::set<uint64_t> k(indices.begin(), indices.end());
    *n_nodes = *n_merges = 0;
    for (uint32_t l = d; l >= 1; l--) {
        std::set<uint64_t> up;
        for (uint64_t x : k) {
            if (!k.count(x ^ 1)) ++*n_nodes;
            up.insert(x >> 1);
        }
        k.swap(up);
        *n_merges += (uint32_t)k.size();
    }
}

// the multi-opening of the ascending `indices`: opened with plan_open_multi on the pool, folded with plan_check on a block of its own
static void open_and_fold(Ledger &L, const Words &indices, const char *what) {
    const uint32_t d = L.ix.depth, count = (uint32_t)indices.size();
    const Index before = L.ix;
    const Words stored(L.pool.begin(), L.pool.begin() + (size_t)7 * L.scratch_base);
    const M::Shape s = M::multiproof_shape(d, count, indices.data());
    uint32_t want_nodes, want_merges;
    brute_shape(d, indices, &want_nodes, &want_merges);
    CHECK(s.ok && s.n_nodes == want_nodes && s.n_merges == want_merges, "%s: the shape is (%u, %u), plain sets give (%u, %u)", what, s.n_nodes, s.n_merges,
          want_nodes, want_merges);
    if (!s.ok) return;

    // ---- open: one emit list, the proof nodes in order and the root
    Plan p;
    CHECK(M::plan_open_multi(L.ix, HEAD, L.scratch_base, count, indices.data(), p), "%s: plan_open_multi refused", what);
    const size_t n = (size_t)s.n_nodes + 1;
    CHECK(p.witness.size() == n && p.jobs.empty() && p.commit.empty() && p.new_nodes.empty() && p.new_values.empty() && p.launch.empty(),
          "%s: a multi-opening is one emit list of n_nodes + 1 entries and nothing else", what);
    CHECK(p.upload_slot == L.scratch_base && p.stage_slot >= p.upload_slot + (n + 6) / 7 && p.stage_slot + n <= p.pool_slots &&
              p.pool_slots - L.scratch_base == M::open_multi_scratch_slots(s.n_nodes),
          "%s: list and staging area do not fit the scratch the caller reserves", what);
    if (p.witness.size() != n) return;
    if (L.pool.size() < 7 * p.pool_slots) L.pool.resize(7 * p.pool_slots, 0xDEADBEEFDEADBEEFull);
    uint64_t *block = &L.pool[(size_t)7 * p.upload_slot];
    memcpy(block, p.upload.data(), 8 * p.upload.size());
    std::vector<Emit> list(n);
    memcpy(list.data(), block + p.witness_word, 8 * n);
    Words stage(7 * n, 0xDEADBEEFDEADBEEFull);
    for (size_t m = 0; m < n; m++) {
        const Emit &em = list[m];
        if (em.slot >= L.scratch_base || em.word != 7 * m) { CHECK(false, "%s: emit %zu leaves the stored nodes or its place in the staging area", what, m); continue; }
        memcpy(&stage[em.word], &L.pool[(size_t)7 * em.slot], 56);
    }
    CHECK(same(&L.pool[(size_t)7 * p.final_root_slot], L.root()) && same(&stage[7 * (n - 1)], L.root()), "%s: the opening states another root", what);
    CHECK(L.ix.n_stored == before.n_stored && L.ix.node == before.node && L.ix.accounts == before.accounts, "%s: an opening changed the index", what);
    CHECK(memcmp(stored.data(), L.pool.data(), 8 * stored.size()) == 0, "%s: an opening changed the stored nodes", what);

    // ---- check: the job lists on a block whose slots know whether they are defined
    M::CheckPlan cp;
    CHECK(M::plan_check(d, count, indices.data(), cp), "%s: plan_check refused", what);
    CHECK(cp.shape.n_nodes == s.n_nodes && cp.shape.n_merges == s.n_merges && cp.jobs.size() == s.n_merges && cp.launch.size() == (size_t)d + 1 &&
              cp.slots == count + s.n_nodes + s.n_merges && (uint64_t)cp.slots < M::MAX_BLOCK_SLOTS,
          "%s: the check plan has another shape", what);
    if (cp.launch.size() != (size_t)d + 1 || cp.jobs.size() != s.n_merges) return;
    CHECK(cp.launch[0] == 0 && cp.launch[d] == cp.jobs.size() && cp.launch[d] - cp.launch[d - 1] == 1, "%s: the launch of level 0 has one job", what);
    Words slots((size_t)7 * cp.slots, 0xDEADBEEFDEADBEEFull);
    std::vector<uint8_t> defined(cp.slots, 0);
    std::vector<uint32_t> reads(cp.slots, 0);
    for (uint32_t i = 0; i < count; i++) {
        const auto it = L.ix.accounts.find(indices[i]);
        if (it != L.ix.accounts.end()) cs::hostg::merge(it->second.data(), it->second.data() + 7, &slots[(size_t)7 * i]);
        else memset(&slots[(size_t)7 * i], 0, 56);
        defined[i] = 1;
    }
    for (uint32_t k = 0; k < s.n_nodes; k++) {
        memcpy(&slots[(size_t)7 * (count + k)], &stage[(size_t)7 * k], 56);
        defined[count + k] = 1;
    }
    uint32_t next_out = count + s.n_nodes;
    for (uint32_t k = 0; k < d; k++) {
        CHECK(cp.launch[k] < cp.launch[k + 1], "%s: launch %u is empty", what, k);
        for (uint32_t j = cp.launch[k]; j < cp.launch[k + 1]; j++) {
            const Job &q = cp.jobs[j];
            if (q.left >= cp.slots || q.right >= cp.slots || q.out >= cp.slots) { CHECK(false, "%s: job %u names a slot outside the block", what, j); continue; }
            // the outputs of this launch are marked after it: a source defined now is a leaf, a proof node or an output of a deeper level
            CHECK(defined[q.left] && defined[q.right], "%s: job %u reads a slot no earlier launch has written", what, j);
            CHECK(q.out == next_out, "%s: job %u writes slot %u, the computed nodes are numbered in job order", what, j, q.out);
            next_out++;
            reads[q.left]++;
            reads[q.right]++;
            if (defined[q.left] && defined[q.right]) cs::hostg::merge(&slots[(size_t)7 * q.left], &slots[(size_t)7 * q.right], &slots[(size_t)7 * q.out]);
        }
        for (uint32_t j = cp.launch[k]; j < cp.launch[k + 1]; j++)
            if (cp.jobs[j].out < cp.slots) defined[cp.jobs[j].out] = 1;
    }
    bool once = true;
    for (uint32_t t = 0; t < cp.slots; t++) once = once && reads[t] == (t == cp.root_slot ? 0u : 1u);
    CHECK(once, "%s: every leaf, proof node and computed node but the root is read exactly once", what);
    CHECK(cp.root_slot == cp.slots - 1 && defined[cp.root_slot] && same(&slots[(size_t)7 * cp.root_slot], L.root()),
          "%s: the multiproof does not fold to the root of the tree", what);
}

static Words ascending(Words v) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
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
    for (size_t i = 0; i < val.size(); i++) val[i] = from_u64(2000 + 13 * i);
    Ledger L(d, (na + 8) * (d + 1) + 16);

    open_and_fold(L, ascending({0, top}), "empty ledger");
    {
        Plan p;
        CHECK(plan_set_accounts(L.ix, L.scratch_base, na, acc.data(), val.data(), p), "set_accounts");
        execute(p, L.pool, (size_t)7 * L.scratch_base);
        commit(L.ix, p);
    }
    // sparse: the accounts and their absent neighbours (at depth 31 the indices reach 2^31 - 1, far above 2^24)
    Words sparse = acc;
    for (uint64_t x : acc)
        for (uint64_t y : {x ^ 1, x + 2, x - 2})
            if (y < size) sparse.push_back(y);
    sparse = ascending(sparse);
    open_and_fold(L, sparse, "sparse, after set_accounts");
    {
        const Words s = {0, top}, r = {top, 0}, dl = {from_u64(5), from_u64(3)};
        Plan p;
        CHECK(plan_apply(L.ix, L.scratch_base, 2, s.data(), r.data(), dl.data(), p) && p.refused_at == -1, "apply");
        execute(p, L.pool, (size_t)7 * L.scratch_base);
        commit(L.ix, p);
    }
    open_and_fold(L, sparse, "sparse, after apply");
    open_and_fold(L, {top}, "one leaf");
    open_and_fold(L, {size / 2}, "one leaf in the middle");
    // dense: runs of consecutive leaves around the sibling pair in the middle (unaligned, so both kinds of single appear), at the upper end
    // of the tree, and the whole tree where it is small
    const uint64_t run = std::min<uint64_t>(size, 70);
    Words dense;
    for (uint64_t x = size / 2 > run / 2 ? size / 2 - run / 2 + (size > run ? 1 : 0) : 0; dense.size() < run && x < size; x++) dense.push_back(x);
    open_and_fold(L, dense, "dense, in the middle");
    Words upper;
    for (uint64_t x = size - std::min<uint64_t>(size, 64); x < size; x++) upper.push_back(x);
    open_and_fold(L, upper, "dense, the upper end");
    if (d <= 7) {
        Words all;
        for (uint64_t x = 0; x < size; x++) all.push_back(x);
        const M::Shape s = M::multiproof_shape(d, (uint32_t)size, all.data());
        CHECK(s.ok && s.n_nodes == 0 && s.n_merges == size - 1, "all leaves need no proof node");
        open_and_fold(L, all, "all leaves");
    }
    if (d == 31) {
        Words high = {((uint64_t)1 << 24) + 1, ((uint64_t)1 << 30), ((uint64_t)1 << 30) + 1, ((uint64_t)1 << 30) + (1 << 24), top - 1, top};
        open_and_fold(L, high, "above 2^24");
    }
    {
        // no shape: out of range, a repeat, a descent; the first offending position is named
        const Words big = {0, size}, twice = {0, top, top}, down = {top, 0};
        M::Shape s = M::multiproof_shape(d, 2, big.data());
        CHECK(!s.ok && s.bad_at == 1, "index 2^depth was accepted");
        s = M::multiproof_shape(d, 3, twice.data());
        CHECK(!s.ok && s.bad_at == 2, "a repeated index was accepted");
        s = M::multiproof_shape(d, 2, down.data());
        CHECK(!s.ok && s.bad_at == 1, "a descending index was accepted");
        Plan p, q;
        M::CheckPlan cp;
        CHECK(!M::plan_open_multi(L.ix, HEAD, L.scratch_base, 2, big.data(), p) && !M::plan_open_multi(L.ix, HEAD, L.scratch_base, 2, down.data(), q) &&
                  !M::plan_open_multi(L.ix, HEAD, L.scratch_base, 0, down.data(), q) && !M::plan_check(d, 3, twice.data(), cp) && cp.shape.bad_at == 2,
              "a plan was made for indices without a shape");
    }
    printf("ok: depth %u, %u accounts, sparse set of %zu, dense run of %zu\n", d, na, sparse.size(), dense.size());
}

int main() {
    for (uint32_t d : {1u, 2u, 3u, 7u, 15u, 31u}) one_depth(d);
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    return 0;
}
