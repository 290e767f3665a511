// Host-side plan of the account ledger (ledger.hip): pure integer work, no HIP, no hashing.
//
// The reference applies a batch of transfers in a sequential loop (TransactionMetadata::build_random, /root/reference/src/lib.rs:341-422):
// record the root and the sender's path, apply the transfer, re-hash two leaf-to-root paths, record the receiver's path.  That loop is
// sequential by transfer order only, not by level.  Number the leaf updates e = 2t (sender) and e = 2t + 1 (receiver) and let D[l][e]
// be the digest of the level-l ancestor of the updated leaf right after event e (level 0 = root, level depth = leaves).  Then
//     D[l-1][e] = merge(D[l][e], S[l][e])          (left / right by the index bit)
// where S[l][e], the sibling's digest at that moment, is D[l][e'] of the latest earlier event e' under the sibling node, or the tree's
// stored node, or the empty-subtree digest of the level.  The map e -> e' is bookkeeping ("last event per node", one table per level),
// and every hash of a level depends on the level below only: a batch is depth + 1 dependent launches of 2 n_tx independent merges.
//
// All digests live in ONE device pool of 7-word slots:
//     [0, EMPTY_SLOTS)            slot l = digest of an empty subtree rooted at level l (empty leaves are the all-zero digest)
//     EMPTY_SLOTS + k             stored node k of the tree (only touched nodes are stored)
//     scratch_base ...            per call: event versions D[l][e], then the upload block (account values as slot pairs, then the lists)
// A plan is job lists (left slot, right slot, output slot), one per launch, and emit lists (pool slot -> 64-bit word offset): one into
// the resident witness (witness_layout.h), one back into the pool (the touched nodes' last versions become the stored nodes).
// Values, jobs and emit lists form one contiguous block: one host-to-device copy.
#pragma once
#include <stdint.h>
#include <string.h>
#include <array>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>
#include "hostfield.h"
#include "witness_layout.h"

namespace cs {
namespace ledger {

constexpr uint32_t EMPTY_SLOTS = 33;
constexpr uint32_t MAX_DEPTH = 31;
constexpr uint32_t MAX_TRANSFERS = 1u << 20;
constexpr uint64_t MAX_POOL_SLOTS = 1ull << 28; // 15 GB of digests: far beyond any batch, keeps every slot and word offset in 32 bits

struct Job { uint32_t left, right, out, reserved; };
struct Emit { uint32_t slot, word; };
static_assert(sizeof(Job) == 16 && sizeof(Emit) == 8, "lists are copied to the device as they are");

// cstark_ledger_reason (include/cstark.h)
enum Reason : int32_t { REASON_NONE = 0, REASON_INDEX = 1, REASON_SELF = 2, REASON_ABSENT = 3, REASON_BALANCE = 4, REASON_SIGNATURE = 5 };

typedef std::array<uint64_t, 14> Value; // pk.x(6) pk.y(6) balance nonce, memory form

// what the host keeps of a ledger: which nodes exist (and their pool slots) and the account values the balance walk needs
struct Index {
    uint32_t depth;
    uint32_t n_stored = 0;
    std::vector<std::unordered_map<uint64_t, uint32_t>> node; // [depth + 1]: index within the level -> pool slot
    std::unordered_map<uint64_t, Value> accounts;             // by leaf index
    explicit Index(uint32_t d) : depth(d), node(d + 1) {}
    uint32_t slot(uint32_t level, uint64_t x) const {
        const auto it = node[level].find(x);
        return it == node[level].end() ? level : it->second;
    }
    uint32_t root_slot() const { return slot(0, 0); }
};

struct NewNode { uint32_t level; uint64_t x; uint32_t slot; };

struct Plan {
    int32_t refused_at = -1, reason = REASON_NONE;
    uint32_t upload_slot = 0;        // pool slot the upload block starts at
    std::vector<uint64_t> upload;    // value slots, then jobs, witness emits, commit emits
    size_t jobs_word = 0, witness_word = 0, commit_word = 0; // 64-bit word offsets of the lists inside `upload`
    std::vector<Job> jobs;
    std::vector<uint32_t> launch;    // launch k runs jobs [launch[k], launch[k + 1])
    std::vector<Emit> witness, commit;
    uint32_t final_root_slot = 0;    // the root after the call (a scratch slot for plan_apply)
    uint64_t pool_slots = 0;         // slots the pool must hold for this call
    uint32_t stage_slot = 0;         // plan_open: the staging area its emit list fills
    // what commit() changes in the index
    std::vector<NewNode> new_nodes;
    std::vector<std::pair<uint64_t, Value>> new_values;
};

// slots a call may add to the stored nodes: the caller places scratch_base beyond EMPTY_SLOTS + n_stored + this bound
inline uint64_t max_new_nodes(uint32_t depth, uint64_t leaves) { return leaves * (depth + 1); }

namespace detail {
inline void pack_lists(Plan &p) {
    p.jobs_word = p.upload.size();
    p.witness_word = p.jobs_word + 2 * p.jobs.size();
    p.commit_word = p.witness_word + p.witness.size();
    p.upload.resize(p.commit_word + p.commit.size());
    if (!p.jobs.empty()) memcpy(&p.upload[p.jobs_word], p.jobs.data(), 16 * p.jobs.size());
    if (!p.witness.empty()) memcpy(&p.upload[p.witness_word], p.witness.data(), 8 * p.witness.size());
    if (!p.commit.empty()) memcpy(&p.upload[p.commit_word], p.commit.data(), 8 * p.commit.size());
    p.pool_slots = (uint64_t)p.upload_slot + (p.upload.size() + 6) / 7;
}
} // namespace detail

// cstark_ledger_set_accounts: leaf hashes of the given accounts, then the unique parents level by level, written straight into the
// stored nodes (every node is written once per call).  false: misuse (an index out of range or given twice, a value word >= p).
inline bool plan_set_accounts(const Index &ix, uint32_t scratch_base, uint32_t count, const uint64_t *indices, const uint64_t *values, Plan &p) {
    const uint32_t d = ix.depth;
    const uint64_t size = (uint64_t)1 << d;
    std::vector<std::unordered_map<uint64_t, uint32_t>> fresh(d + 1);
    uint32_t n_stored = ix.n_stored;
    auto lookup = [&](uint32_t l, uint64_t x) -> uint32_t {
        const auto it = fresh[l].find(x);
        return it != fresh[l].end() ? it->second : ix.slot(l, x);
    };
    auto stored = [&](uint32_t l, uint64_t x) -> uint32_t {
        const auto it = ix.node[l].find(x);
        if (it != ix.node[l].end()) return it->second;
        const uint32_t s = EMPTY_SLOTS + n_stored++;
        fresh[l][x] = s;
        p.new_nodes.push_back({l, x, s});
        return s;
    };
    p.upload_slot = scratch_base;
    p.upload.assign(values, values + (size_t)14 * count);
    for (size_t i = 0; i < (size_t)14 * count; i++)
        if (values[i] >= host::P) return false;
    std::vector<uint64_t> touched;
    std::unordered_set<uint64_t> seen;
    p.launch.push_back(0);
    for (uint32_t i = 0; i < count; i++) {
        const uint64_t x = indices[i];
        if (x >= size || !seen.insert(x).second) return false;
        p.jobs.push_back({scratch_base + 2 * i, scratch_base + 2 * i + 1, stored(d, x), 0});
        touched.push_back(x);
        Value v;
        memcpy(v.data(), values + (size_t)14 * i, sizeof v);
        p.new_values.emplace_back(x, v);
    }
    p.launch.push_back((uint32_t)p.jobs.size());
    for (uint32_t l = d; l >= 1; l--) {
        std::vector<uint64_t> parents;
        seen.clear();
        for (const uint64_t x : touched)
            if (seen.insert(x >> 1).second) parents.push_back(x >> 1);
        for (const uint64_t q : parents) p.jobs.push_back({lookup(l, 2 * q), lookup(l, 2 * q + 1), stored(l - 1, q), 0});
        p.launch.push_back((uint32_t)p.jobs.size());
        touched.swap(parents);
    }
    p.final_root_slot = lookup(0, 0);
    detail::pack_lists(p);
    return p.pool_slots <= MAX_POOL_SLOTS;
}

// cstark_ledger_apply: the balance walk with its refusals, the per-level predecessor map, the jobs of the depth + 1 launches and the
// two emit lists.  A refusal sets refused_at / reason and nothing else.  false: the batch is too large to plan.
// Deltas are reduced field elements (the caller checks).  Witness word offsets are those of witness_segments(n_tx, depth).
// messages (optional, cstark_ledger_apply_checked): the message every transfer signs, 28 words each (build_tx_message, src/lib.rs:467-481:
// sender's key, receiver's key, delta, sender's nonce, two zeros), keys and nonce as the walk holds them BEFORE the transfer, that is as
// the transfers before it in the same batch leave them.  One message per transfer that passed the four refusal tests: all n_tx of an
// applied batch, the transfers [0, refused_at) of a refused one.
inline bool plan_apply(const Index &ix, uint32_t scratch_base, uint32_t n_tx, const uint64_t *s_idx, const uint64_t *r_idx, const uint64_t *deltas, Plan &p,
                       std::vector<uint64_t> *messages = nullptr) {
    using namespace cs::host;
    const uint32_t d = ix.depth, ne = 2 * n_tx;
    const uint64_t size = (uint64_t)1 << d;
    if (n_tx == 0 || n_tx > MAX_TRANSFERS || (uint64_t)scratch_base + (uint64_t)(d + 1) * ne + 4ull * ne > MAX_POOL_SLOTS) return false;
    const uint32_t d_base = scratch_base;              // D[l][e] at d_base + l * ne + e
    const uint32_t v_base = d_base + (d + 1) * ne;     // the new value of event e at v_base + 2 e (two slots)
    const uint32_t f_base = v_base + 2 * ne;           // first-touch old values, two slots each
    auto D = [&](uint32_t l, uint32_t e) { return d_base + l * ne + e; };

    // the balance walk (src/lib.rs:373-375: field arithmetic), in transfer order
    std::unordered_map<uint64_t, Value> cur;
    std::unordered_map<uint64_t, uint32_t> last_on_account;
    std::vector<uint32_t> old_slot(ne);
    std::vector<uint64_t> first;
    p.upload_slot = v_base;
    p.upload.resize((size_t)14 * ne);
    auto value_of = [&](uint64_t a) -> Value * {
        const auto it = cur.find(a);
        if (it != cur.end()) return &it->second;
        const auto st = ix.accounts.find(a);
        if (st == ix.accounts.end()) return nullptr;
        return &cur.emplace(a, st->second).first->second;
    };
    auto refuse = [&](uint32_t t, Reason r) { p.refused_at = (int32_t)t; p.reason = r; return true; };
    for (uint32_t t = 0; t < n_tx; t++) {
        const uint64_t si = s_idx[t], ri = r_idx[t], delta = deltas[t];
        if (si >= size || ri >= size) return refuse(t, REASON_INDEX);
        if (si == ri) return refuse(t, REASON_SELF);
        Value *sv = value_of(si), *rv = value_of(ri);
        if (!sv || !rv) return refuse(t, REASON_ABSENT);
        if (to_u64(delta) > to_u64((*sv)[12])) return refuse(t, REASON_BALANCE);
        if (messages) {
            messages->insert(messages->end(), sv->begin(), sv->begin() + 12);
            messages->insert(messages->end(), rv->begin(), rv->begin() + 12);
            const uint64_t tail[4] = {delta, (*sv)[13], 0, 0};
            messages->insert(messages->end(), tail, tail + 4);
        }
        for (int k = 0; k < 2; k++) {
            const uint32_t e = 2 * t + k;
            const uint64_t a = k ? ri : si;
            const auto it = last_on_account.find(a);
            if (it != last_on_account.end()) old_slot[e] = v_base + 2 * it->second;
            else {
                old_slot[e] = f_base + (uint32_t)(first.size() / 7);
                first.insert(first.end(), (k ? rv : sv)->begin(), (k ? rv : sv)->end());
            }
            last_on_account[a] = e;
        }
        (*sv)[12] = sub((*sv)[12], delta);
        (*sv)[13] = add((*sv)[13], ONE);
        (*rv)[12] = add((*rv)[12], delta);
        memcpy(&p.upload[(size_t)14 * (2 * t)], sv->data(), 112);
        memcpy(&p.upload[(size_t)14 * (2 * t + 1)], rv->data(), 112);
    }
    p.upload.insert(p.upload.end(), first.begin(), first.end());

    // the predecessor map: S[l][e] for l = 1 .. depth, the leaf before the event, the root before the event
    std::vector<std::unordered_map<uint64_t, uint32_t>> last(d + 1); // per level: node -> its latest event so far
    std::vector<uint32_t> S((size_t)(d + 1) * ne), leaf_before(ne);
    for (uint32_t e = 0; e < ne; e++) {
        const uint64_t a = (e & 1) ? r_idx[e >> 1] : s_idx[e >> 1];
        for (uint32_t l = d; l >= 1; l--) {
            const uint64_t x = a >> (d - l);
            const auto it = last[l].find(x ^ 1);
            S[(size_t)l * ne + e] = it != last[l].end() ? D(l, it->second) : ix.slot(l, x ^ 1);
            if (l == d) {
                const auto me = last[l].find(x);
                leaf_before[e] = me != last[l].end() ? D(l, me->second) : ix.slot(l, x);
            }
            last[l][x] = e;
        }
    }
    last[0][0] = ne - 1;

    // launch 0: the leaves; launch j: level depth - j from level depth - j + 1
    p.launch.push_back(0);
    for (uint32_t e = 0; e < ne; e++) p.jobs.push_back({v_base + 2 * e, v_base + 2 * e + 1, D(d, e), 0});
    p.launch.push_back((uint32_t)p.jobs.size());
    for (uint32_t l = d; l >= 1; l--) {
        for (uint32_t e = 0; e < ne; e++) {
            const uint64_t a = (e & 1) ? r_idx[e >> 1] : s_idx[e >> 1];
            const uint32_t own = D(l, e), sib = S[(size_t)l * ne + e];
            const bool right = (a >> (d - l)) & 1; // the updated node is the right child
            p.jobs.push_back({right ? sib : own, right ? own : sib, D(l - 1, e), 0});
        }
        p.launch.push_back((uint32_t)p.jobs.size());
    }

    // the witness: roots, old values and paths (path[0] = the leaf, path[k + 1] = the sibling at level depth - k)
    size_t sz[WIT_NUM_SEGMENTS], off[WIT_NUM_SEGMENTS + 1];
    witness_segments(n_tx, d, sz, off);
    if (off[WIT_NUM_SEGMENTS] / 8 > 0xFFFFFFFFull) return false;
    auto W = [&](int seg, size_t word) { return (uint32_t)(off[seg] / 8 + word); };
    for (uint32_t t = 0; t < n_tx; t++) {
        p.witness.push_back({t == 0 ? ix.root_slot() : D(0, 2 * t - 1), W(WIT_INITIAL_ROOTS, (size_t)7 * t)});
        for (uint32_t h = 0; h < 2; h++) {
            p.witness.push_back({old_slot[2 * t] + h, W(WIT_S_OLD, (size_t)14 * t + 7 * h)});
            p.witness.push_back({old_slot[2 * t + 1] + h, W(WIT_R_OLD, (size_t)14 * t + 7 * h)});
        }
        const size_t path = (size_t)7 * (d + 1) * t;
        p.witness.push_back({leaf_before[2 * t], W(WIT_S_PATHS, path)});
        p.witness.push_back({D(d, 2 * t + 1), W(WIT_R_PATHS, path)}); // the receiver's NEW leaf: the reference proves it after both updates
        for (uint32_t k = 0; k < d; k++) {
            p.witness.push_back({S[(size_t)(d - k) * ne + 2 * t], W(WIT_S_PATHS, path + 7 * (k + 1))});
            p.witness.push_back({S[(size_t)(d - k) * ne + 2 * t + 1], W(WIT_R_PATHS, path + 7 * (k + 1))});
        }
    }

    // the ledger advances: every touched node's last version becomes the stored node
    uint32_t n_stored = ix.n_stored;
    for (uint32_t l = 0; l <= d; l++)
        for (const auto &kv : last[l]) {
            const auto it = ix.node[l].find(kv.first);
            uint32_t dst;
            if (it != ix.node[l].end()) dst = it->second;
            else {
                dst = EMPTY_SLOTS + n_stored++;
                p.new_nodes.push_back({l, kv.first, dst});
            }
            p.commit.push_back({D(l, kv.second), dst * 7});
        }
    p.final_root_slot = D(0, ne - 1);
    for (const auto &kv : cur) p.new_values.emplace_back(kv.first, kv.second);
    detail::pack_lists(p);
    return p.pool_slots <= MAX_POOL_SLOTS;
}

// cstark_ledger_open_accounts: the authentication paths of `count` leaves of the tree as it stands, in the witness's form (path[0] = the
// leaf, path[k + 1] = the sibling at level depth - k).  One emit list of count (depth + 1) entries, `witness`, whose word offsets count
// from the staging area [stage_slot, stage_slot + count (depth + 1)) that follows the list in the scratch: path i starts at word
// 7 (depth + 1) i.  An absent leaf and an untouched sibling read the level's empty-subtree slot (Index::slot).  Indices may repeat.
// Nothing of the index changes and nothing is hashed.  false: an index is out of range, or the call is too large to plan.
inline uint64_t open_scratch_slots(uint32_t depth, uint64_t count) { return (count * (depth + 1) + 6) / 7 + count * (depth + 1); }
inline bool plan_open(const Index &ix, uint32_t scratch_base, uint32_t count, const uint64_t *indices, Plan &p) {
    const uint32_t d = ix.depth;
    const uint64_t size = (uint64_t)1 << d;
    if (count == 0 || count > MAX_TRANSFERS || (uint64_t)scratch_base + open_scratch_slots(d, count) > MAX_POOL_SLOTS) return false;
    for (uint32_t i = 0; i < count; i++)
        if (indices[i] >= size) return false;
    p.upload_slot = scratch_base;
    p.witness.reserve((size_t)count * (d + 1));
    for (uint32_t i = 0; i < count; i++) {
        const uint64_t a = indices[i];
        const uint32_t word = 7 * (d + 1) * i; // below 2^20 * 32 * 7
        p.witness.push_back({ix.slot(d, a), word});
        for (uint32_t k = 0; k < d; k++) p.witness.push_back({ix.slot(d - k, (a >> k) ^ 1), word + 7 * (k + 1)});
    }
    p.final_root_slot = ix.root_slot();
    detail::pack_lists(p);
    p.stage_slot = (uint32_t)p.pool_slots;
    p.pool_slots += p.witness.size();
    return p.pool_slots <= MAX_POOL_SLOTS;
}

// after the device work of a plan has been enqueued: the index follows
inline void commit(Index &ix, const Plan &p) {
    for (const NewNode &nn : p.new_nodes) ix.node[nn.level][nn.x] = nn.slot;
    ix.n_stored += (uint32_t)p.new_nodes.size();
    for (const auto &kv : p.new_values) ix.accounts[kv.first] = kv.second;
}

// the depth launches that fill the empty-subtree digests of a new ledger (slot depth is the all-zero leaf): one job each
inline void plan_empty_digests(uint32_t depth, uint32_t scratch_base, Plan &p) {
    p.upload_slot = scratch_base;
    p.launch.push_back(0);
    for (uint32_t l = depth; l >= 1; l--) {
        p.jobs.push_back({l, l, l - 1, 0});
        p.launch.push_back((uint32_t)p.jobs.size());
    }
    detail::pack_lists(p);
}

} // namespace ledger
} // namespace cs
