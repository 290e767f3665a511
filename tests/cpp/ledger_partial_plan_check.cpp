// csrc/multiproof_plan.h and csrc/ledger_plan.h alone under g++ (host code only): plan_seed and commit_seed, the host side of
// cstark_ledger_create_partial, run with the host executor (the host `merge` of hostgadgets.h over a host pool, as
// tests/cpp/ledger_multi_check.cpp does).  For depths 1, 3 and 7 and index sets of one leaf, a sibling pair, all leaves (no proof node) and
// alternating leaves, a FULL index holds a tree and a PARTIAL index is seeded from its multi-opening.  Then:
//   - the seed plan stores exactly the present opened leaves, the proof nodes and the nodes of the fold, each in a slot of its own inside
//     the stored region, uploads the proof nodes into their final slots, and folds to the full tree's root;
//   - a leaf is known by the opaque-ancestor rule iff it is an opened index, for every leaf of the tree;
//   - every stored node of the partial index holds the digest the full index holds for it;
//   - plan_apply on the partial index emits the same launches, jobs and emits as on the full index, modulo slot numbers: run on its own
//     pool, every witness word and the final root are the same digests, and the index after commit agrees again;
//   - plan_open and plan_audit on the partial index: paths equal the full index's, no audit job expects an opaque slot, every job passes;
//   - a transfer with an unknown account is refused as UNKNOWN after SELF and before ABSENT, on the partial index only.
//   ledger_partial_plan_check        all checks; prints one "ok" line per depth
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <vector>
#include "../../certificate-stark_amd/csrc/hostgadgets.h"
#include "../../certificate-stark_amd/csrc/multiproof_plan.h"

using namespace cs::ledger;
namespace M = cs::multi;
typedef std::vector<uint64_t> Words;
typedef std::set<std::pair<uint32_t, uint64_t>> NodeSet; // (level, x)

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

static const uint64_t POISON = 0xDEADBEEFDEADBEEFull;
static bool same(const uint64_t *a, const uint64_t *b) { return memcmp(a, b, 56) == 0; }

// upload block, launches in order, witness emits into `witness`, commit emits into the stored nodes
static void execute(const Plan &p, Words &pool, size_t stored_words, Words *witness = nullptr) {
    if (pool.size() < 7 * p.pool_slots) pool.resize(7 * p.pool_slots, POISON);
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
    if (witness)
        for (const Emit &m : p.witness) {
            if (m.slot >= p.pool_slots) { CHECK(false, "a witness emit is out of range"); continue; }
            if (witness->size() < (size_t)m.word + 7) witness->resize((size_t)m.word + 7, POISON);
            memcpy(&(*witness)[m.word], &pool[(size_t)7 * m.slot], 56);
        }
    for (const Emit &m : p.commit) {
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
    const uint64_t *digest(uint32_t l, uint64_t x) const { return &pool[(size_t)7 * ix.slot(l, x)]; }
    const uint64_t *root() const { return digest(0, 0); }
    // the stored region grows: the scratch moves up (the host pool only; the device's reserve_pool copies likewise)
    void reserve(uint32_t more) {
        const uint32_t need = EMPTY_SLOTS + ix.n_stored + more;
        if (need > scratch_base) scratch_base = need;
        if (pool.size() < (size_t)7 * scratch_base) pool.resize((size_t)7 * scratch_base, POISON);
    }
};

static void one_set(uint32_t d, const Words &accounts, const Words &values, const Words &indices, const std::string &what_s) {
    const char *what = what_s.c_str();
    const uint64_t size = (uint64_t)1 << d;
    const uint32_t count = (uint32_t)indices.size(), na = (uint32_t)accounts.size();
    Ledger F(d, (na + 8) * (d + 1) + 16);
    {
        Plan p;
        CHECK(plan_set_accounts(F.ix, F.scratch_base, na, accounts.data(), values.data(), p), "%s: set_accounts", what);
        execute(p, F.pool, (size_t)7 * F.scratch_base);
        commit(F.ix, p);
    }
    // ---- the opening out of the full index
    Words ovalues((size_t)14 * count, 0), onodes;
    std::vector<uint8_t> present(count);
    uint32_t n_present = 0;
    for (uint32_t i = 0; i < count; i++) {
        const auto it = F.ix.accounts.find(indices[i]);
        present[i] = it != F.ix.accounts.end();
        n_present += present[i];
        if (present[i]) memcpy(&ovalues[14 * i], it->second.data(), 112);
    }
    NodeSet proof, fold, leaves;
    {
        std::set<uint64_t> k(indices.begin(), indices.end());
        for (uint32_t l = d; l >= 1; l--) {
            std::set<uint64_t> up;
            for (uint64_t x : k) {
                if (!k.count(x ^ 1)) { proof.insert({l, x ^ 1}); onodes.insert(onodes.end(), F.digest(l, x ^ 1), F.digest(l, x ^ 1) + 7); }
                up.insert(x >> 1);
            }
            k.swap(up);
            for (uint64_t x : k) fold.insert({l - 1, x});
        }
        for (uint32_t i = 0; i < count; i++)
            if (present[i]) leaves.insert({d, indices[i]});
    }
    const M::Shape s = M::multiproof_shape(d, count, indices.data());
    CHECK(s.ok && s.n_nodes == proof.size() && s.n_merges == fold.size(), "%s: the shape differs from plain sets", what);

    // ---- the seed plan
    M::SeedPlan sp;
    CHECK(M::plan_seed(d, count, indices.data(), ovalues.data(), present.data(), onodes.empty() ? nullptr : onodes.data(), sp), "%s: plan_seed refused", what);
    const Plan &p = sp.plan;
    const uint32_t stored = (uint32_t)M::seed_stored_slots(n_present, s.n_nodes, s.n_merges);
    CHECK(sp.n_leaves == n_present && p.extended == stored && p.from_free == 0 && p.launch.size() == (size_t)d + 2 && p.jobs.size() == n_present + s.n_merges,
          "%s: the seed plan has another shape", what);
    CHECK(p.upload_slot == EMPTY_SLOTS + stored - s.n_nodes, "%s: the upload block does not start at the first proof slot", what);
    NodeSet got, want = leaves;
    want.insert(proof.begin(), proof.end());
    want.insert(fold.begin(), fold.end());
    std::set<uint32_t> slots;
    for (const NewNode &nn : p.new_nodes) {
        got.insert({nn.level, nn.x});
        slots.insert(nn.slot);
        CHECK(nn.slot >= EMPTY_SLOTS && nn.slot < EMPTY_SLOTS + stored, "%s: node (%u, %llu) is stored outside the stored region", what, nn.level,
              (unsigned long long)nn.x);
        if (proof.count({nn.level, nn.x})) CHECK(nn.slot >= p.upload_slot, "%s: a proof node is not in the upload block", what);
        else CHECK(nn.slot < p.upload_slot, "%s: a computed node lies in the upload block", what);
    }
    CHECK(got == want && p.new_nodes.size() == want.size() && slots.size() == want.size(), "%s: the seed plan does not store exactly leaves, proof and fold nodes", what);
    CHECK(NodeSet(sp.opaque.begin(), sp.opaque.end()) == proof && sp.opaque.size() == proof.size(), "%s: opaque is not the proof", what);
    for (const Job &q : p.jobs) CHECK(!(q.out >= p.upload_slot), "%s: a job writes a proof slot or the scratch", what);

    Ledger P(d, stored);
    CHECK(P.scratch_base == EMPTY_SLOTS + stored, "%s: the scratch does not follow the stored nodes", what);
    execute(p, P.pool, (size_t)7 * P.scratch_base);
    CHECK(same(&P.pool[(size_t)7 * p.final_root_slot], F.root()), "%s: the seed does not fold to the root of the tree", what);
    M::commit_seed(P.ix, sp, count, indices.data());
    CHECK(P.ix.partial && P.ix.n_stored == stored && P.ix.n_opaque == proof.size() && P.ix.live_nodes() == want.size() && same(P.root(), F.root()),
          "%s: the committed index has another shape", what);
    for (const auto &lx : want) CHECK(same(P.digest(lx.first, lx.second), F.digest(lx.first, lx.second)), "%s: node (%u, %llu) differs", what, lx.first, (unsigned long long)lx.second);

    // ---- known = opened, for every leaf of the tree
    for (uint64_t x = 0; x < size; x++) {
        bool under_opaque = false;
        for (uint32_t k = 0; k <= d; k++) under_opaque = under_opaque || P.ix.is_opaque(d - k, x >> k);
        const bool is_opened = std::binary_search(indices.begin(), indices.end(), x);
        CHECK(!under_opaque == is_opened && P.ix.is_known(x) == is_opened && F.ix.is_known(x), "%s: leaf %llu: known by ancestors %d, opened %d", what,
              (unsigned long long)x, !under_opaque, is_opened);
    }
    CHECK(!P.ix.is_known(size) && !F.ix.is_known(size), "%s: index 2^depth is known", what);

    // ---- open and audit
    auto open_both = [&]() {
        Plan a, b;
        CHECK(plan_open(F.ix, F.scratch_base, count, indices.data(), a) && plan_open(P.ix, P.scratch_base, count, indices.data(), b), "%s: plan_open", what);
        CHECK(a.witness.size() == b.witness.size(), "%s: openings of different size", what);
        for (size_t m = 0; m < a.witness.size() && m < b.witness.size(); m++)
            CHECK(a.witness[m].word == b.witness[m].word && same(&F.pool[(size_t)7 * a.witness[m].slot], &P.pool[(size_t)7 * b.witness[m].slot]),
                  "%s: path entry %zu differs", what, m);
    };
    auto audit = [&]() {
        const NodeMap nodes = nodes_at(P.ix, HEAD);
        Plan a;
        CHECK(plan_audit(P.ix, HEAD, nodes, P.scratch_base, a), "%s: plan_audit", what);
        CHECK(a.jobs.size() == d + P.ix.live_nodes() - P.ix.n_opaque && a.audited.size() == a.jobs.size(), "%s: the audit has %zu jobs", what, a.jobs.size());
        Words pool = P.pool;
        if (pool.size() < 7 * a.pool_slots) pool.resize(7 * a.pool_slots, POISON);
        memcpy(&pool[(size_t)7 * a.upload_slot], a.upload.data(), 8 * a.upload.size());
        for (size_t j = 0; j < a.jobs.size(); j++) {
            const Job &q = a.jobs[j];
            const NewNode &node = a.audited[j];
            CHECK(j < d || !P.ix.is_opaque(node.level, node.x), "%s: audit job %zu expects an opaque node", what, j);
            uint64_t out[7];
            cs::hostg::merge(&pool[(size_t)7 * q.left], &pool[(size_t)7 * q.right], out);
            CHECK(same(out, &pool[(size_t)7 * q.out]), "%s: audit job %zu fails", what, j);
        }
    };
    open_both();
    audit();

    // ---- plan_apply: two transfers among the opened present accounts, on both indices
    Words inside;
    for (uint32_t i = 0; i < count; i++)
        if (present[i]) inside.push_back(indices[i]);
    if (inside.size() >= 2) {
        const Words sv = {inside.front(), inside.back()}, rv = {inside.back(), inside.front()}, dl = {cs::host::from_u64(3), cs::host::from_u64(1)};
        F.reserve((uint32_t)max_new_nodes(d, 4));
        P.reserve((uint32_t)max_new_nodes(d, 4));
        Plan a, b;
        CHECK(plan_apply(F.ix, F.scratch_base, 2, sv.data(), rv.data(), dl.data(), a) && a.refused_at == -1, "%s: apply on the full index", what);
        CHECK(plan_apply(P.ix, P.scratch_base, 2, sv.data(), rv.data(), dl.data(), b) && b.refused_at == -1, "%s: apply on the partial index", what);
        CHECK(a.launch == b.launch && a.jobs.size() == b.jobs.size() && a.witness.size() == b.witness.size() && a.commit.size() == b.commit.size() &&
                  a.new_values.size() == b.new_values.size(),
              "%s: the two apply plans have different shapes", what);
        Words wa, wb;
        execute(a, F.pool, (size_t)7 * F.scratch_base, &wa);
        execute(b, P.pool, (size_t)7 * P.scratch_base, &wb);
        for (size_t m = 0; m < a.witness.size() && m < b.witness.size(); m++) CHECK(a.witness[m].word == b.witness[m].word, "%s: witness emit %zu goes elsewhere", what, m);
        CHECK(wa == wb && !wa.empty(), "%s: the witnesses differ", what);
        CHECK(same(&F.pool[(size_t)7 * a.final_root_slot], &P.pool[(size_t)7 * b.final_root_slot]), "%s: the final roots differ", what);
        commit(F.ix, a);
        commit(P.ix, b);
        CHECK(same(P.root(), F.root()) && P.ix.n_opaque == proof.size(), "%s: the roots differ after commit", what);
        for (const auto &lx : proof) CHECK(same(P.digest(lx.first, lx.second), F.digest(lx.first, lx.second)), "%s: a write reached an opaque node", what);
        open_both();
        audit();
    }

    // ---- refusals: unknown after self, before absent; a full index never says unknown
    Words unknown_leaf;
    for (uint64_t x = 0; x < size && unknown_leaf.empty(); x++)
        if (!P.ix.is_known(x)) unknown_leaf.push_back(x);
    if (!unknown_leaf.empty() && !inside.empty()) {
        const uint64_t u = unknown_leaf[0], k = inside[0], zero = cs::host::from_u64(0);
        auto reason = [&](const Index &ix, uint64_t sidx, uint64_t ridx) {
            Plan q;
            plan_apply(ix, EMPTY_SLOTS + ix.n_stored + (uint32_t)max_new_nodes(d, 2), 1, &sidx, &ridx, &zero, q);
            return q.refused_at == 0 ? q.reason : -1;
        };
        CHECK(reason(P.ix, u, k) == REASON_UNKNOWN && reason(P.ix, k, u) == REASON_UNKNOWN, "%s: an unknown account is not refused as UNKNOWN", what);
        CHECK(reason(P.ix, u, u) == REASON_SELF && reason(P.ix, u, size) == REASON_INDEX, "%s: UNKNOWN comes before SELF or INDEX", what);
        CHECK(reason(F.ix, u, k) != REASON_UNKNOWN && reason(F.ix, k, u) != REASON_UNKNOWN, "%s: a full index says UNKNOWN", what);
        for (uint32_t i = 0; i < count; i++)
            if (!present[i]) CHECK(reason(P.ix, indices[i], u) == REASON_UNKNOWN && reason(P.ix, indices[i], k) == REASON_ABSENT, "%s: a known absent account", what);
    }
}

static void one_depth(uint32_t d) {
    const uint64_t size = (uint64_t)1 << d;
    Words accounts;
    for (uint64_t x = 0; x < size; x++)
        if (x % 3 != 1 || x == size - 1) accounts.push_back(x); // absent accounts everywhere, both ends present
    Words values((size_t)14 * accounts.size());
    for (size_t i = 0; i < values.size(); i++) values[i] = cs::host::from_u64(3000 + 17 * i);
    for (size_t a = 0; a < accounts.size(); a++) values[14 * a + 12] = cs::host::from_u64(1000 + a); // balances the transfers can draw on
    std::vector<std::pair<std::string, Words>> sets;
    sets.push_back({"one leaf", {size / 3}});
    sets.push_back({"a sibling pair", {size - 2, size - 1}});
    Words all, alternating;
    for (uint64_t x = 0; x < size; x++) all.push_back(x);
    for (uint64_t x = 0; x < size; x += 2) alternating.push_back(x);
    sets.push_back({"all leaves", all});
    sets.push_back({"alternating leaves", alternating});
    for (const auto &set : sets) one_set(d, accounts, values, set.second, "depth " + std::to_string(d) + ", " + set.first);
    printf("ok: depth %u, %zu accounts, %zu index sets\n", d, accounts.size(), sets.size());
}

int main() {
    for (uint32_t d : {1u, 3u, 7u}) one_depth(d);
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    return 0;
}
