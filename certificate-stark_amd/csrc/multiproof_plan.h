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
