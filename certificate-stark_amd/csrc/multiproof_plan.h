// Host-side plans of the ledger's multi-openings (ledger.hip: cstark_ledger_open_multi, cstark_account_check_multiproof): pure integer
// work, no HIP, no hashing.
//
// The multiproof of a tree of depth d and a strictly ascending list of leaf indices I (include/cstark.h):
//     K_d = I;  for l = d .. 1: every x of K_l, ascending, contributes the proof node (l, x ^ 1) iff x ^ 1 is not in K_l;
//     K_{l-1} = the parents {x >> 1} of K_l.
// nodes[n_nodes][7] holds those digests in that order (level d first, ascending x within a level); n_merges = sum over l < d of |K_l|,
// the merges that fold the opening to the root (the count leaf hashes are not among them).  Within a level the parents of an ascending
// K_l are ascending, and x ^ 1 ascends with x over the unpaired x, so one walk per level serves every function here.
//
// The check runs over ONE device block of 7-word digest slots:
//     [0, count)                           the leaves, in index order
//     [count, count + n_nodes)             the proof nodes, in canonical order
//     [count + n_nodes, ... + n_merges)    the computed nodes, level d - 1 first, ascending x within a level; the last one is the root
// Bound: count <= 2^20 and depth <= 31, so n_nodes <= 31 count and n_merges <= 31 count: the block stays below 2^20 * 63 slots, every
// slot number and every word offset 7 * slot + k (< 2^20 * 63 * 7 < 2^29) fits in 32 bits.
#pragma once
#include "ledger_plan.h"

namespace cs {
namespace multi {

using ledger::Emit;
using ledger::Job;

constexpr uint32_t MAX_DEPTH = ledger::MAX_DEPTH;
constexpr uint32_t MAX_COUNT = 1u << 20;
constexpr uint64_t MAX_BLOCK_SLOTS = (uint64_t)MAX_COUNT * 63;

// cstark_multi_verdict (include/cstark.h)
enum Verdict : uint32_t { VALID = 0, INDEX = 1, NODE_COUNT = 2, ROOT = 3 };

struct Shape {
    bool ok = false;       // false: indices[bad_at] is >= 2^depth or not above its predecessor
    uint32_t bad_at = 0;
    uint32_t n_nodes = 0, n_merges = 0;
};

namespace detail {
// one level of the walk: k holds K_l ascending and becomes K_{l-1}; paired(i, j) is called for siblings at positions i, i + 1 = j of K_l,
// single(i) for an x whose sibling comes from the proof; both in ascending x, with the position of the parent in K_{l-1} as last argument
template <class Paired, class Single>
inline void walk_level(std::vector<uint64_t> &k, Paired paired, Single single) {
    size_t m = 0;
    for (size_t i = 0; i < k.size();) {
        const uint64_t x = k[i];
        const bool pair = !(x & 1) && i + 1 < k.size() && k[i + 1] == x + 1;
        if (pair) paired(i, i + 1, m);
        else single(i, m);
        k[m++] = x >> 1; // m <= i: the entries still to be read are untouched
        i += pair ? 2 : 1;
    }
    k.resize(m);
}
} // namespace detail

// depth 1 .. 31 and count 1 .. 2^20 are the caller's to check
inline Shape multiproof_shape(uint32_t depth, uint32_t count, const uint64_t *indices) {
    Shape s;
    const uint64_t size = (uint64_t)1 << depth;
    for (uint32_t i = 0; i < count; i++)
        if (indices[i] >= size || (i && indices[i] <= indices[i - 1])) {
            s.bad_at = i;
            return s;
        }
    std::vector<uint64_t> k(indices, indices + count);
    for (uint32_t l = depth; l >= 1; l--) {
        detail::walk_level(k, [](size_t, size_t, size_t) {}, [&](size_t, size_t) { s.n_nodes++; });
        s.n_merges += (uint32_t)k.size();
    }
    s.ok = true;
    return s;
}

// slots of the check's device block
inline uint64_t check_block_slots(uint64_t count, uint64_t n_nodes, uint64_t n_merges) { return count + n_nodes + n_merges; }

// The check plan: one job list (left slot, right slot, out slot) per level d - 1 .. 0.  Every source slot of a level is a leaf, a proof
// node or an output of a deeper level, so the launches need the stream's order only.
struct CheckPlan {
    Shape shape;
    uint32_t slots = 0;            // check_block_slots: every slot a job names is below it
    std::vector<Job> jobs;         // level depth - 1 first; the last job writes the root
    std::vector<uint32_t> launch;  // launch k (level depth - 1 - k) runs jobs [launch[k], launch[k + 1]); depth launches, the last of one job
    uint32_t root_slot = 0;
};

// false: the indices have no shape (p.shape says where)
inline bool plan_check(uint32_t depth, uint32_t count, const uint64_t *indices, CheckPlan &p) {
    p.shape = multiproof_shape(depth, count, indices);
    if (!p.shape.ok) return false;
    p.slots = (uint32_t)check_block_slots(count, p.shape.n_nodes, p.shape.n_merges); // below 2^20 * 63
    p.jobs.reserve(p.shape.n_merges);
    std::vector<uint64_t> k(indices, indices + count);
    std::vector<uint32_t> slot(count), above;
    for (uint32_t i = 0; i < count; i++) slot[i] = i;
    uint32_t next_proof = count, next_out = count + p.shape.n_nodes;
    p.launch.push_back(0);
    for (uint32_t l = depth; l >= 1; l--) {
        above.clear();
        detail::walk_level(
            k,
            [&](size_t i, size_t j, size_t) {
                p.jobs.push_back({slot[i], slot[j], next_out, 0});
                above.push_back(next_out++);
            },
            [&](size_t i, size_t) {
                const uint32_t proof = next_proof++;
                const bool right = k[i] & 1; // k[i] is still x here: walk_level overwrites position m <= i after the call
                p.jobs.push_back({right ? proof : slot[i], right ? slot[i] : proof, next_out, 0});
                above.push_back(next_out++);
            });
        slot.swap(above);
        p.launch.push_back((uint32_t)p.jobs.size());
    }
    p.root_slot = slot[0];
    return true;
}

// cstark_account_check_update: the fold of the SAME multiproof over two states of the opened accounts, in one pass.  The
// plan is plan_check's job list; the fourth word of a job says whether a changed leaf lies below the job's output, and only such a job
// hashes on the new side -- everywhere else the new digest is the old one.  The old side runs over plan_check's block [0, slots); the new
// side has its own leaves and computed nodes behind it and reads the proof nodes where the old side reads them:
//     [slots, slots + count)                        the new leaves
//     [slots + count, slots + count + n_merges)     the new computed nodes, in the order of the old ones
// Bound: below 2^20 * 126 slots, so every word offset 7 * slot + k stays below 2^30.
enum UpdateVerdict : uint32_t { UPDATE_VALID = 0, UPDATE_INDEX = 1, UPDATE_NODE_COUNT = 2, UPDATE_OLD_ROOT = 3, UPDATE_NEW_ROOT = 4 };

// per opened position: what the leaf launch needs to know of it
enum : uint8_t { STATE_OLD_PRESENT = 1, STATE_NEW_PRESENT = 2, STATE_CHANGED = 4 };

// the new side's slot of an old-side slot s < slots: a proof node is shared.  constexpr: the kernel maps slots by the same function
constexpr uint32_t update_new_slot(uint32_t s, uint32_t count, uint32_t n_nodes, uint32_t slots) {
    return s < count ? slots + s : s < count + n_nodes ? s : slots + (s - n_nodes);
}
inline uint64_t update_block_slots(uint64_t count, uint64_t n_nodes, uint64_t n_merges) { return 2 * (count + n_merges) + n_nodes; }

// state[i] of every position (a null present: all present) -> the number of changed positions: presence differs, or both are present and
// a value word differs.  Two absent positions are equal whatever their value words.
inline uint32_t update_states(uint32_t count, const uint64_t *old_values, const uint8_t *old_present, const uint64_t *new_values, const uint8_t *new_present,
                              std::vector<uint8_t> &state) {
    state.resize(count);
    uint32_t n_changed = 0;
    for (uint32_t i = 0; i < count; i++) {
        const bool was = old_present ? old_present[i] != 0 : true, is = new_present ? new_present[i] != 0 : true;
        const bool changed = was != is || (was && memcmp(old_values + (size_t)14 * i, new_values + (size_t)14 * i, 112) != 0);
        state[i] = (uint8_t)((was ? STATE_OLD_PRESENT : 0) | (is ? STATE_NEW_PRESENT : 0) | (changed ? STATE_CHANGED : 0));
        n_changed += changed;
    }
    return n_changed;
}

// plan_check with the changed flags in Job::reserved.  The jobs of a level only read leaves, proof nodes and outputs of deeper levels, and
// the list holds the deeper levels first: one pass over it carries the flags upwards.  false: the indices have no shape
inline bool plan_update(uint32_t depth, uint32_t count, const uint64_t *indices, const uint8_t *state, CheckPlan &p) {
    if (!plan_check(depth, count, indices, p)) return false;
    std::vector<uint8_t> below(p.slots, 0); // per old-side slot: a changed leaf at or below it (a proof node: never)
    for (uint32_t i = 0; i < count; i++) below[i] = (state[i] & STATE_CHANGED) != 0;
    for (Job &job : p.jobs) {
        job.reserved = below[job.left] | below[job.right];
        below[job.out] = (uint8_t)job.reserved;
    }
    return true;
}

// cstark_ledger_create_partial: plan_check's walk with pool slots.  The new ledger stores, in this order of slots from
// ledger::EMPTY_SLOTS on: the leaf of every opened PRESENT account (an opened absent leaf is not stored and reads the all-zero slot
// `depth`, as in a full ledger), the computed nodes of the fold (level depth - 1 first, ascending x within a level), and last the proof
// nodes in canonical order.  The scratch follows the stored nodes at once (the caller reserves exactly n_stored slots), so ONE upload
// block that starts at the first proof slot puts the proof nodes straight into their final slots and the present accounts' values (two
// slots each) and the job list into the scratch behind them.  Launch 0 hashes the leaves from the value halves, launch k the level
// depth - k: k_ledger_merge's job lists, written straight into the stored nodes.  new_nodes / new_values / extended are what
// ledger::commit makes of it once the fold has met the stated root; `opaque` receives the proof nodes' (level, x).
struct SeedPlan {
    ledger::Plan plan;
    uint32_t n_leaves = 0;                             // present opened accounts
    std::vector<std::pair<uint32_t, uint64_t>> opaque; // (level, x) of the proof nodes, canonical order
};
inline uint64_t seed_stored_slots(uint64_t present, uint64_t n_nodes, uint64_t n_merges) { return present + n_merges + n_nodes; }
// values: [count][14]; present: [count] or null (all present); nodes: [n_nodes][7] (n_nodes is the shape's).  false: no shape, or too large
inline bool plan_seed(uint32_t depth, uint32_t count, const uint64_t *indices, const uint64_t *values, const uint8_t *present, const uint64_t *nodes,
                      SeedPlan &sp) {
    using ledger::EMPTY_SLOTS;
    const Shape s = multiproof_shape(depth, count, indices);
    if (!s.ok) return false;
    ledger::Plan &p = sp.plan;
    for (uint32_t i = 0; i < count; i++) sp.n_leaves += present ? present[i] != 0 : 1;
    const uint32_t stored = (uint32_t)seed_stored_slots(sp.n_leaves, s.n_nodes, s.n_merges);
    const uint32_t scratch_base = EMPTY_SLOTS + stored;
    uint32_t next_leaf = EMPTY_SLOTS, next_out = EMPTY_SLOTS + sp.n_leaves, next_proof = next_out + s.n_merges;
    p.upload_slot = next_proof;
    p.upload.reserve((size_t)7 * s.n_nodes + (size_t)14 * sp.n_leaves + 2 * (size_t)(s.n_merges + sp.n_leaves));
    if (s.n_nodes) p.upload.assign(nodes, nodes + (size_t)7 * s.n_nodes);
    p.jobs.reserve((size_t)sp.n_leaves + s.n_merges);
    p.new_nodes.reserve((size_t)stored);
    p.new_values.reserve(sp.n_leaves);
    sp.opaque.reserve(s.n_nodes);
    std::vector<uint32_t> slot(count), above;
    p.launch.push_back(0);
    for (uint32_t i = 0, k = 0; i < count; i++) {
        if (present && !present[i]) { slot[i] = depth; continue; } // the all-zero empty leaf
        slot[i] = next_leaf++;
        p.upload.insert(p.upload.end(), values + (size_t)14 * i, values + (size_t)14 * (i + 1));
        p.jobs.push_back({scratch_base + 2 * k, scratch_base + 2 * k + 1, slot[i], 0});
        p.new_nodes.push_back({depth, indices[i], slot[i]});
        ledger::Value v;
        memcpy(v.data(), values + (size_t)14 * i, sizeof v);
        p.new_values.emplace_back(indices[i], v);
        k++;
    }
    p.launch.push_back((uint32_t)p.jobs.size());
    std::vector<uint64_t> k(indices, indices + count);
    for (uint32_t l = depth; l >= 1; l--) {
        above.clear();
        detail::walk_level(
            k,
            [&](size_t i, size_t j, size_t) {
                p.jobs.push_back({slot[i], slot[j], next_out, 0});
                p.new_nodes.push_back({l - 1, k[i] >> 1, next_out});
                above.push_back(next_out++);
            },
            [&](size_t i, size_t) {
                const uint32_t proof = next_proof++;
                const uint64_t x = k[i]; // still x here: walk_level overwrites position m <= i after the call
                sp.opaque.emplace_back(l, x ^ 1);
                p.new_nodes.push_back({l, x ^ 1, proof});
                p.jobs.push_back({(x & 1) ? proof : slot[i], (x & 1) ? slot[i] : proof, next_out, 0});
                p.new_nodes.push_back({l - 1, x >> 1, next_out});
                above.push_back(next_out++);
            });
        slot.swap(above);
        p.launch.push_back((uint32_t)p.jobs.size());
    }
    p.final_root_slot = slot[0];
    p.extended = stored;
    ledger::detail::pack_lists(p);
    return p.pool_slots <= ledger::MAX_POOL_SLOTS;
}
// after the fold has met the stated root: the index of the new partial ledger
inline void commit_seed(ledger::Index &ix, const SeedPlan &sp, uint32_t count, const uint64_t *indices) {
    std::vector<size_t> per_level(ix.depth + 1, 0); // the maps are filled once: size them first
    for (const ledger::NewNode &nn : sp.plan.new_nodes) per_level[nn.level]++;
    for (uint32_t l = 0; l <= ix.depth; l++) ix.node[l].reserve(per_level[l]);
    ix.accounts.reserve(sp.plan.new_values.size());
    ledger::commit(ix, sp.plan);
    ix.partial = true;
    ix.known.assign(indices, indices + count);
    ix.opaque.assign(ix.depth + 1, {});
    for (const auto &lx : sp.opaque) ix.opaque[lx.first].insert(lx.second);
    ix.n_opaque = sp.opaque.size();
}

// cstark_ledger_open_multi: ONE emit list built from Index::slot_at -- the n_nodes proof nodes in canonical order, then the root -- whose
// word offsets count from the staging area [stage_slot, stage_slot + n_nodes + 1) that follows the list in the scratch, as plan_open
// places them: node k at word 7 k, the root at word 7 n_nodes.  No leaf entries: the values carry them.  An untouched sibling reads the
// level's empty-subtree slot.  `at`: the checkpoint position whose state is opened (ledger::HEAD: the current one).  Nothing of the
// index changes and nothing is hashed.  false: the indices have no shape, or the call is too large to plan.
inline uint64_t open_multi_scratch_slots(uint64_t n_nodes) { return (n_nodes + 1 + 6) / 7 + n_nodes + 1; }
inline bool plan_open_multi(const ledger::Index &ix, size_t at, uint32_t scratch_base, uint32_t count, const uint64_t *indices, ledger::Plan &p) {
    const uint32_t d = ix.depth;
    if (count == 0 || count > MAX_COUNT) return false;
    const Shape s = multiproof_shape(d, count, indices);
    if (!s.ok || (uint64_t)scratch_base + open_multi_scratch_slots(s.n_nodes) > ledger::MAX_POOL_SLOTS) return false;
    p.upload_slot = scratch_base;
    p.witness.reserve((size_t)s.n_nodes + 1);
    std::vector<uint64_t> k(indices, indices + count);
    for (uint32_t l = d; l >= 1; l--)
        detail::walk_level(k, [](size_t, size_t, size_t) {},
                           [&](size_t i, size_t) { p.witness.push_back({ix.slot_at(at, l, k[i] ^ 1), 7 * (uint32_t)p.witness.size()}); });
    p.final_root_slot = ix.slot_at(at, 0, 0);
    p.witness.push_back({p.final_root_slot, 7 * s.n_nodes}); // below 2^20 * 31 * 7
    ledger::detail::pack_lists(p);
    p.stage_slot = (uint32_t)p.pool_slots;
    p.pool_slots += p.witness.size();
    return p.pool_slots <= ledger::MAX_POOL_SLOTS;
}

} // namespace multi
} // namespace cs
