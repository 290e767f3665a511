// csrc/multiproof_plan.h alone under g++ (host code only): update_states, plan_update and update_new_slot, the host side of
// cstark_account_check_update.  For depths 1, 3 and 7, for index sets of one leaf, a sibling pair, all leaves (no proof node), alternating
// leaves and a sparse set, and for the changes none / one / all / absent -> present / present -> absent, the WHOLE tree of both states is
// built with the host `merge` of hostgadgets.h, and then:
//   - the changed flag of every job equals "some changed leaf lies below the job's output", by the leaves' index ranges;
//   - the plan is run as k_multi_update runs it, on a block whose slots know whether they are defined: the old side over plan_check's
//     slots, the new side through update_new_slot, hashing only where the flag is set and copying the old digest elsewhere; every slot is
//     in bounds, no two nodes share a new slot, a proof node keeps its slot, and both folds are the roots of the two whole trees;
//   - the new side hashes exactly the nodes on the changed leaves' paths (one changed leaf: depth of them).
//   account_update_plan_check        all checks; prints one "ok" line per depth
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <set>
#include <string>
#include <vector>
#include "../../certificate-stark_amd/csrc/hostgadgets.h"
#include "../../certificate-stark_amd/csrc/multiproof_plan.h"

using cs::ledger::Job;
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

static const uint64_t POISON = 0xDEADBEEFDEADBEEFull;
static bool same(const uint64_t *a, const uint64_t *b) { return memcmp(a, b, 56) == 0; }

// every node of a tree of depth d over the given leaf digests: level l holds 2^l digests, tree[l][7 x ..]
static std::vector<Words> whole_tree(uint32_t d, const Words &leaves) {
    std::vector<Words> t(d + 1);
    t[d] = leaves;
    for (uint32_t l = d; l >= 1; l--) {
        t[l - 1].resize((size_t)7 << (l - 1));
        for (uint64_t x = 0; x < ((uint64_t)1 << (l - 1)); x++) cs::hostg::merge(&t[l][14 * x], &t[l][14 * x + 7], &t[l - 1][7 * x]);
    }
    return t;
}

struct State {
    Words values;                 // [2^d][14]
    std::vector<uint8_t> present; // [2^d]
};

static Words leaf_digests(uint32_t d, const State &s) {
    Words leaves((size_t)7 << d, 0);
    for (uint64_t x = 0; x < ((uint64_t)1 << d); x++)
        if (s.present[x]) cs::hostg::merge(&s.values[14 * x], &s.values[14 * x + 7], &leaves[7 * x]);
    return leaves;
}

// old and new state of the whole tree differ at most at the opened indices
static void one_case(uint32_t d, const Words &indices, const State &before, const State &after, bool null_present, const std::string &what_s) {
    const char *what = what_s.c_str();
    const uint32_t count = (uint32_t)indices.size();
    const std::vector<Words> old_tree = whole_tree(d, leaf_digests(d, before)), new_tree = whole_tree(d, leaf_digests(d, after));
    Words old_values((size_t)14 * count), new_values((size_t)14 * count);
    std::vector<uint8_t> old_present(count), new_present(count);
    uint32_t want_changed = 0;
    std::set<uint64_t> changed_leaves;
    for (uint32_t i = 0; i < count; i++) {
        const uint64_t x = indices[i];
        memcpy(&old_values[14 * i], &before.values[14 * x], 112);
        memcpy(&new_values[14 * i], &after.values[14 * x], 112);
        old_present[i] = before.present[x];
        new_present[i] = after.present[x];
        const bool differ = old_present[i] != new_present[i] || (old_present[i] && memcmp(&old_values[14 * i], &new_values[14 * i], 112) != 0);
        if (differ) changed_leaves.insert(x);
        want_changed += differ;
    }
    std::vector<uint8_t> state;
    const uint32_t n_changed = M::update_states(count, old_values.data(), null_present ? nullptr : old_present.data(), new_values.data(),
                                                null_present ? nullptr : new_present.data(), state);
    CHECK(n_changed == want_changed && state.size() == count, "%s: update_states counts %u changed positions, there are %u", what, n_changed, want_changed);
    for (uint32_t i = 0; i < count && i < state.size(); i++)
        CHECK(state[i] == ((old_present[i] ? M::STATE_OLD_PRESENT : 0) | (new_present[i] ? M::STATE_NEW_PRESENT : 0) |
                           (changed_leaves.count(indices[i]) ? M::STATE_CHANGED : 0)),
              "%s: state[%u] is %u", what, i, state[i]);

    M::CheckPlan p, plain;
    CHECK(M::plan_update(d, count, indices.data(), state.data(), p) && M::plan_check(d, count, indices.data(), plain), "%s: a plan was refused", what);
    CHECK(p.jobs.size() == plain.jobs.size() && p.launch == plain.launch && p.slots == plain.slots && p.root_slot == plain.root_slot,
          "%s: the update plan is not plan_check's", what);
    if (p.jobs.size() != plain.jobs.size() || p.launch.size() != (size_t)d + 1) return;
    const uint32_t n_nodes = p.shape.n_nodes, n_merges = p.shape.n_merges;
    const uint32_t block_slots = (uint32_t)M::update_block_slots(count, n_nodes, n_merges);
    CHECK(block_slots == p.slots + count + n_merges && (uint64_t)block_slots < 2 * M::MAX_BLOCK_SLOTS, "%s: the block has %u slots", what, block_slots);

    // ---- the flags: job j of launch k writes node (d - 1 - k, the j-th parent in ascending order)
    std::set<uint64_t> level(indices.begin(), indices.end());
    uint32_t want_hashes = 0;
    for (uint32_t k = 0; k < d; k++) {
        std::set<uint64_t> up;
        for (uint64_t x : level) up.insert(x >> 1);
        level.swap(up);
        CHECK(p.launch[k + 1] - p.launch[k] == level.size(), "%s: launch %u has another size than its level", what, k);
        uint32_t j = p.launch[k];
        for (uint64_t x : level) {
            if (j >= p.jobs.size()) break;
            const uint32_t shift = k + 1; // leaves [x << shift, (x + 1) << shift) lie below
            const auto it = changed_leaves.lower_bound(x << shift);
            const bool below = it != changed_leaves.end() && *it < ((x + 1) << shift);
            CHECK(p.jobs[j].reserved == (below ? 1u : 0u), "%s: job %u (level %u, node %llu) is flagged %u", what, j, d - 1 - k, (unsigned long long)x,
                  p.jobs[j].reserved);
            CHECK(p.jobs[j].left == plain.jobs[j].left && p.jobs[j].right == plain.jobs[j].right && p.jobs[j].out == plain.jobs[j].out,
                  "%s: job %u names other slots than plan_check's", what, j);
            want_hashes += below;
            j++;
        }
    }

    // ---- the slot map: proof nodes stay, everything else lands in [slots, block_slots), one to one
    std::set<uint32_t> images;
    for (uint32_t s = 0; s < p.slots; s++) {
        const uint32_t t = M::update_new_slot(s, count, n_nodes, p.slots);
        const bool proof = s >= count && s < count + n_nodes;
        CHECK(proof ? t == s : (t >= p.slots && t < block_slots), "%s: slot %u maps to %u", what, s, t);
        images.insert(t);
    }
    CHECK(images.size() == p.slots, "%s: two slots share an image", what);

    // ---- the run, as k_multi_update does it
    Words block((size_t)7 * block_slots, POISON);
    std::vector<uint8_t> defined(block_slots, 0);
    auto new_slot = [&](uint32_t s) { return M::update_new_slot(s, count, n_nodes, p.slots); };
    for (uint32_t i = 0; i < count; i++) {
        if (state[i] & M::STATE_OLD_PRESENT) cs::hostg::merge(&old_values[14 * i], &old_values[14 * i + 7], &block[(size_t)7 * i]);
        else memset(&block[(size_t)7 * i], 0, 56);
        uint64_t *fresh = &block[(size_t)7 * new_slot(i)];
        if (!(state[i] & M::STATE_CHANGED)) memcpy(fresh, &block[(size_t)7 * i], 56);
        else if (state[i] & M::STATE_NEW_PRESENT) cs::hostg::merge(&new_values[14 * i], &new_values[14 * i + 7], fresh);
        else memset(fresh, 0, 56);
        defined[i] = defined[new_slot(i)] = 1;
    }
    // the proof nodes in canonical order out of the old tree
    {
        std::set<uint64_t> k(indices.begin(), indices.end());
        uint32_t next = count;
        for (uint32_t l = d; l >= 1; l--) {
            std::set<uint64_t> up;
            for (uint64_t x : k) {
                if (!k.count(x ^ 1)) {
                    CHECK(same(&old_tree[l][7 * (x ^ 1)], &new_tree[l][7 * (x ^ 1)]), "%s: a proof node differs between the states", what);
                    if (next < count + n_nodes) memcpy(&block[(size_t)7 * next], &old_tree[l][7 * (x ^ 1)], 56);
                    if (next < block_slots) defined[next] = 1;
                    next++;
                }
                up.insert(x >> 1);
            }
            k.swap(up);
        }
        CHECK(next == count + n_nodes, "%s: the walk gives %u proof nodes, the shape %u", what, next - count, n_nodes);
    }
    uint32_t hashes = 0;
    for (uint32_t k = 0; k < d; k++) {
        std::vector<uint32_t> written;
        for (uint32_t j = p.launch[k]; j < p.launch[k + 1]; j++) {
            const Job &q = p.jobs[j];
            if (q.left >= p.slots || q.right >= p.slots || q.out >= p.slots) { CHECK(false, "%s: job %u names a slot outside the old side", what, j); continue; }
            CHECK(defined[q.left] && defined[q.right], "%s: job %u reads an old slot no earlier launch has written", what, j);
            cs::hostg::merge(&block[(size_t)7 * q.left], &block[(size_t)7 * q.right], &block[(size_t)7 * q.out]);
            const uint32_t out = new_slot(q.out);
            if (out >= block_slots) { CHECK(false, "%s: job %u writes outside the block", what, j); continue; }
            if (q.reserved) {
                const uint32_t left = new_slot(q.left), right = new_slot(q.right);
                if (left >= block_slots || right >= block_slots) { CHECK(false, "%s: job %u reads outside the block", what, j); continue; }
                CHECK(defined[left] && defined[right], "%s: job %u reads a new slot no earlier launch has written", what, j);
                cs::hostg::merge(&block[(size_t)7 * left], &block[(size_t)7 * right], &block[(size_t)7 * out]);
                hashes++;
            } else {
                memcpy(&block[(size_t)7 * out], &block[(size_t)7 * q.out], 56);
            }
            written.push_back(q.out);
            written.push_back(out);
        }
        for (uint32_t s : written) defined[s] = 1; // after the launch: a source defined now is an output of a DEEPER level
    }
    bool all_defined = true;
    for (uint32_t s = 0; s < block_slots; s++) all_defined = all_defined && defined[s];
    CHECK(all_defined, "%s: a slot of the block is never written", what);
    CHECK(same(&block[(size_t)7 * p.root_slot], &old_tree[0][0]), "%s: the old side does not fold to the old root", what);
    CHECK(same(&block[(size_t)7 * new_slot(p.root_slot)], &new_tree[0][0]), "%s: the new side does not fold to the new root", what);
    CHECK(hashes == want_hashes, "%s: the new side hashed %u nodes, %u lie above a changed leaf", what, hashes, want_hashes);
    if (changed_leaves.size() == 1) CHECK(hashes == d, "%s: one changed leaf costs %u hashes on the new side, not depth", what, hashes);
    if (changed_leaves.empty()) CHECK(hashes == 0 && same(&old_tree[0][0], &new_tree[0][0]), "%s: no change, and yet the new side works", what);
}

static State accounts(uint32_t d, uint64_t seed) {
    const uint64_t size = (uint64_t)1 << d;
    State s;
    s.values.resize((size_t)14 * size);
    s.present.resize(size);
    for (size_t i = 0; i < s.values.size(); i++) s.values[i] = cs::host::from_u64(seed + 13 * i);
    for (uint64_t x = 0; x < size; x++) s.present[x] = x % 5 != 3; // some absent accounts everywhere
    return s;
}

static void one_depth(uint32_t d) {
    const uint64_t size = (uint64_t)1 << d;
    std::vector<std::pair<std::string, Words>> sets;
    sets.push_back({"one leaf", {size / 3}});
    sets.push_back({"a sibling pair", {size - 2, size - 1}});
    Words all, alternating, sparse;
    for (uint64_t x = 0; x < size; x++) all.push_back(x);
    for (uint64_t x = 0; x < size; x += 2) alternating.push_back(x);
    for (uint64_t x : {(uint64_t)0, size / 4 + 1, size / 2, size / 2 + 1, size - 1})
        if (std::find(sparse.begin(), sparse.end(), x) == sparse.end() && x < size) sparse.push_back(x);
    std::sort(sparse.begin(), sparse.end());
    sets.push_back({"all leaves", all});
    sets.push_back({"alternating leaves", alternating});
    sets.push_back({"a sparse set", sparse});
    const State before = accounts(d, 1000);
    size_t cases = 0;
    for (const auto &set : sets) {
        const Words &idx = set.second;
        auto touch = [&](State &s, uint64_t x) { s.values[14 * x + 12] = cs::host::from_u64(77 + x); s.present[x] = 1; };
        // none
        one_case(d, idx, before, before, false, set.first + ", no change");
        // value words of an account absent on both sides differ: no change
        {
            State b = before, a = before;
            b.present[idx[0]] = a.present[idx[0]] = 0;
            a.values[14 * idx[0] + 3] = cs::host::from_u64(5);
            one_case(d, idx, b, a, false, set.first + ", absent on both sides");
        }
        // one changed leaf: the last opened one
        {
            State a = before;
            touch(a, idx.back());
            State b = before;
            b.present[idx.back()] = 1;
            one_case(d, idx, b, a, false, set.first + ", one change");
        }
        // all changed, every account present: the null present arrays
        {
            State b = before, a = before;
            for (uint64_t x : idx) { b.present[x] = 1; touch(a, x); }
            one_case(d, idx, b, a, true, set.first + ", all changed");
        }
        // absent -> present at the first, present -> absent at the last
        {
            State b = before, a = before;
            b.present[idx[0]] = 0;
            a.present[idx[0]] = 1;
            if (idx.size() > 1) { b.present[idx.back()] = 1; a.present[idx.back()] = 0; }
            one_case(d, idx, b, a, false, set.first + ", presence flips");
        }
        cases += 5;
    }
    {
        const Words down = {size - 1, 0};
        const uint8_t state[2] = {0, 0};
        M::CheckPlan p;
        CHECK(!M::plan_update(d, 2, down.data(), state, p) && p.shape.bad_at == 1, "a plan was made for descending indices");
    }
    printf("ok: depth %u, %zu index sets, %zu cases\n", d, sets.size(), cases);
}

int main() {
    for (uint32_t d : {1u, 3u, 7u}) one_depth(d);
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    return 0;
}
