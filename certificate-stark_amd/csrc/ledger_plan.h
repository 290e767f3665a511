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
//
// Checkpoints (cstark_ledger_checkpoint ...) keep old states by NOT overwriting them.  While a checkpoint is live, the first write of a
// node since the newest checkpoint goes to a fresh slot, Index::node is redirected to it, and the newest checkpoint's log records
// (level, x) -> the old slot, or ABSENT_SLOT for a node that did not exist (it reads as the level's empty-subtree slot).  Old account
// values are logged the same way.  The log of checkpoint c_i therefore holds the state at c_i of exactly the nodes first changed in
// [c_i, c_i+1): the state at c is found by searching the log of c, then the logs after it in order, then the index (Index::slot_at).
// The plans only name other slots: no launch and no copy is added.  Freed slots go on Index::free_slots and are taken before the pool
// is extended; Index::n_stored counts the slots ever allocated, the upper end of the stored nodes in the pool.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
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
constexpr uint32_t MAX_CHECKPOINTS = 16;        // live checkpoints of one ledger: a lookup walks at most this many logs
constexpr uint32_t ABSENT_SLOT = 0xFFFFFFFFu;   // in a checkpoint's log: the node did not exist at the checkpoint
constexpr size_t HEAD = ~(size_t)0;             // a checkpoint position that names the current state

struct Job { uint32_t left, right, out, reserved; };
struct Emit { uint32_t slot, word; };
static_assert(sizeof(Job) == 16 && sizeof(Emit) == 8, "lists are copied to the device as they are");

// cstark_ledger_reason (include/cstark.h)
enum Reason : int32_t { REASON_NONE = 0, REASON_INDEX = 1, REASON_SELF = 2, REASON_ABSENT = 3, REASON_BALANCE = 4, REASON_SIGNATURE = 5, REASON_UNKNOWN = 6, REASON_KEY = 7 };

typedef std::array<uint64_t, 14> Value; // pk.x(6) pk.y(6) balance nonce, memory form

typedef std::vector<std::unordered_map<uint64_t, uint32_t>> NodeMap; // [depth + 1]: index within the level -> pool slot

// the log of one checkpoint: what the nodes and accounts first changed since it (and before the next checkpoint) were at the checkpoint
struct Checkpoint {
    uint64_t id;
    NodeMap node;                                                   // -> the old slot, or ABSENT_SLOT
    std::unordered_map<uint64_t, std::pair<bool, Value>> accounts; // -> (present, the old value)
    Checkpoint(uint64_t i, uint32_t depth) : id(i), node(depth + 1) {}
};

// what the host keeps of a ledger: which nodes exist (and their pool slots) and the account values the balance walk needs
struct Index {
    uint32_t depth;
    uint32_t n_stored = 0;                        // slots allocated so far: stored nodes live in [EMPTY_SLOTS, EMPTY_SLOTS + n_stored)
    NodeMap node;
    std::unordered_map<uint64_t, Value> accounts; // by leaf index
    std::vector<uint32_t> free_slots;             // allocated slots nothing names any more; taken (from the back) before the pool is extended
    std::vector<Checkpoint> checkpoints;          // live ones, oldest first
    uint64_t next_id = 1;                         // ids count from 1 and are never reused
    // a partial ledger (cstark_ledger_create_partial): built from a multi-opening, it holds the opened leaves, the proof
    // nodes and the nodes of the fold.  `opaque` names the proof nodes: taken on trust under the root, nothing stored beneath them.  A leaf
    // is known iff it has no opaque ancestor-or-self, which is the sorted list `known` of the opened indices.  Both are fixed for the
    // ledger's life: no known leaf's path holds an opaque node, so no write ever reaches one.  A full ledger knows every leaf.
    bool partial = false;
    std::vector<uint64_t> known;
    std::vector<std::unordered_set<uint64_t>> opaque; // [depth + 1] when partial
    uint64_t n_opaque = 0;
    explicit Index(uint32_t d) : depth(d), node(d + 1) {}
    bool is_known(uint64_t a) const { return partial ? std::binary_search(known.begin(), known.end(), a) : !(a >> depth); }
    bool is_opaque(uint32_t level, uint64_t x) const { return partial && opaque[level].count(x) != 0; }
    uint32_t slot(uint32_t level, uint64_t x) const {
        const auto it = node[level].find(x);
        return it == node[level].end() ? level : it->second;
    }
    uint32_t root_slot() const { return slot(0, 0); }
    // the position of a live checkpoint in `checkpoints`; id 0 is the current state (HEAD); -1: no such live checkpoint
    ptrdiff_t position(uint64_t id) const {
        if (id == 0) return (ptrdiff_t)checkpoints.size();
        for (size_t k = 0; k < checkpoints.size(); k++)
            if (checkpoints[k].id == id) return (ptrdiff_t)k;
        return -1;
    }
    // Index::slot in the state at checkpoint position `at`: the first log from `at` on that holds the node answers, else the index
    uint32_t slot_at(size_t at, uint32_t level, uint64_t x) const {
        for (size_t k = at; k < checkpoints.size(); k++) {
            const auto it = checkpoints[k].node[level].find(x);
            if (it != checkpoints[k].node[level].end()) return it->second == ABSENT_SLOT ? level : it->second;
        }
        return slot(level, x);
    }
    // the account's value in that state, nullptr where it had none
    const Value *value_at(size_t at, uint64_t a) const {
        for (size_t k = at; k < checkpoints.size(); k++) {
            const auto it = checkpoints[k].accounts.find(a);
            if (it != checkpoints[k].accounts.end()) return it->second.first ? &it->second.second : nullptr;
        }
        const auto it = accounts.find(a);
        return it == accounts.end() ? nullptr : &it->second;
    }
    // the slot a write of this node goes to in place, or ABSENT_SLOT where it must take a fresh one: the node has none yet, or this is
    // its first write since the newest checkpoint.  Without a live checkpoint this is the one lookup the plans always did.
    uint32_t slot_in_place(uint32_t level, uint64_t x) const {
        const auto it = node[level].find(x);
        if (it == node[level].end()) return ABSENT_SLOT;
        if (!checkpoints.empty() && !checkpoints.back().node[level].count(x)) return ABSENT_SLOT;
        return it->second;
    }
    uint64_t live_nodes() const {
        uint64_t n = 0;
        for (const auto &level : node) n += level.size();
        return n;
    }
};

// the slots a plan takes: from the back of the free list first, then by extending the stored nodes; commit() makes it so
struct SlotTaker {
    const Index &ix;
    uint32_t from_free = 0, extended = 0;
    explicit SlotTaker(const Index &i) : ix(i) {}
    uint32_t take() {
        if (from_free < ix.free_slots.size()) return ix.free_slots[ix.free_slots.size() - 1 - from_free++];
        return EMPTY_SLOTS + ix.n_stored + extended++;
    }
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
    // what commit() changes in the index: nodes created or redirected to a fresh slot, the slots they took, the accounts' new values
    std::vector<NewNode> new_nodes;
    uint32_t from_free = 0, extended = 0;
    std::vector<std::pair<uint64_t, Value>> new_values;
    // plan_audit: the node every job tests, in job order (jobs [0, depth) test the empty-subtree slots, x = 0), and the leaf count
    std::vector<NewNode> audited;
    uint32_t audit_leaves = 0;
};

// slots a call may add to the stored nodes (the number of touched nodes: under a live checkpoint every one of them may take a fresh
// slot): the caller places scratch_base beyond EMPTY_SLOTS + n_stored + this bound
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
// stored nodes (every node is written once per call; under a live checkpoint the first write since it takes a fresh slot).
// false: misuse (an index out of range or given twice, a value word >= p).
inline bool plan_set_accounts(const Index &ix, uint32_t scratch_base, uint32_t count, const uint64_t *indices, const uint64_t *values, Plan &p) {
    const uint32_t d = ix.depth;
    const uint64_t size = (uint64_t)1 << d;
    std::vector<std::unordered_map<uint64_t, uint32_t>> fresh(d + 1);
    SlotTaker slots(ix);
    auto lookup = [&](uint32_t l, uint64_t x) -> uint32_t {
        const auto it = fresh[l].find(x);
        return it != fresh[l].end() ? it->second : ix.slot(l, x);
    };
    auto stored = [&](uint32_t l, uint64_t x) -> uint32_t {
        const uint32_t in_place = ix.slot_in_place(l, x);
        if (in_place != ABSENT_SLOT) return in_place;
        const uint32_t s = slots.take();
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
    p.from_free = slots.from_free;
    p.extended = slots.extended;
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
        if (!ix.is_known(si) || !ix.is_known(ri)) return refuse(t, REASON_UNKNOWN); // a partial ledger only; a full one knows every leaf
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

    // the ledger advances: every touched node's last version becomes the stored node (in a fresh slot where the node is new or a live
    // checkpoint still names the old one)
    SlotTaker slots(ix);
    for (uint32_t l = 0; l <= d; l++)
        for (const auto &kv : last[l]) {
            uint32_t dst = ix.slot_in_place(l, kv.first);
            if (dst == ABSENT_SLOT) {
                dst = slots.take();
                p.new_nodes.push_back({l, kv.first, dst});
            }
            p.commit.push_back({D(l, kv.second), dst * 7});
        }
    p.from_free = slots.from_free;
    p.extended = slots.extended;
    p.final_root_slot = D(0, ne - 1);
    for (const auto &kv : cur) p.new_values.emplace_back(kv.first, kv.second);
    detail::pack_lists(p);
    return p.pool_slots <= MAX_POOL_SLOTS;
}

// ---- cstark_ledger_select: a provable batch out of a pool of candidates ------------------------------------------------------------
// Candidates are examined in list order, each against the accounts as the candidates selected before it leave them, and get the first
// status that applies: NOT_REACHED (`want` are selected already), INDEX, SELF, UNKNOWN, ABSENT, HELD, BALANCE, SIGNATURE, else selected
// (REASON_NONE).  THE HOLD: a refused candidate whose sender index is in range holds that sender for the rest of the call -- its later
// candidates are HELD whatever they say; a held account still receives.  A wallet signs nonce n, n + 1, ... expecting all of them to
// be accepted, so after one refusal the sender's later candidates carry the wrong nonce anyway.  With the hold, every candidate that
// reaches the signature test has all earlier candidates of its sender selected, so its message is known before any verdict is:
// sender's key, receiver's key (keys never change in a transfer), delta, the STORED nonce + k_t (k_t = earlier candidates in the list
// with the same sender index), two zeros.  Signatures are therefore checked in passes over many candidates, not in rounds.
//   select_prepare   once per call: the static tests (INDEX, SELF, UNKNOWN, ABSENT: they read the index only), k_t, the table of the
//                    distinct accounts that checkable candidates name (a candidate is checkable when it passes the static tests), and
//                    per candidate {sender row, receiver row, delta, k_t in memory form}: what k_select_gather (ledger.hip) reads
//   select_walk      resumable: HELD, BALANCE (plan_apply's arithmetic) and the signature verdicts in list order; it stops at the
//                    first candidate whose verdict it needs and does not have
//   select_chunk     the candidates of the next pass of the signature check: the one the walk waits for and the checkable ones after it
//   select_finish    the cut to a power of two; select_batch compacts the selection into what plan_apply takes, unchanged
constexpr uint8_t STATUS_HELD = 8, STATUS_NOT_REACHED = 9; // cstark_ledger_reason beyond Reason
constexpr uint8_t NO_VERDICT = 0xFF;
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;
struct Candidate { uint32_t s_row, r_row; uint64_t delta, k; };
static_assert(sizeof(Candidate) == 24, "the candidate table is copied to the device as it is");

struct Selection {
    // the call
    uint32_t n = 0, want = 0;
    uint64_t size = 0; // 2^depth
    bool check_signatures = false;
    const uint64_t *s_idx = nullptr;
    // preparation
    std::vector<uint8_t> fixed;      // [n] the static status, REASON_NONE: checkable
    std::vector<uint8_t> rx_ok;      // [n] every sig_rx word is below p (all 1 without signatures)
    std::vector<Candidate> cands;    // [n] rows NO_ROW where not checkable
    std::vector<uint64_t> rows;      // [n_rows][14] the accounts as stored
    // the walk
    uint32_t at = 0, n_selected = 0;
    std::vector<uint64_t> balance;   // [n_rows] memory form, as the selected candidates so far leave it
    std::unordered_set<uint64_t> held;
    std::vector<uint8_t> status, verdict; // [n]; verdict: cstark_sig_verdict, NO_VERDICT where none came back yet
    std::vector<uint32_t> selected;  // candidate numbers, ascending
    uint32_t n_rows() const { return (uint32_t)(rows.size() / 14); }
};

inline void select_prepare(const Index &ix, uint32_t n, const uint64_t *s_idx, const uint64_t *r_idx, const uint64_t *deltas, const uint64_t *sig_rx /* or null */,
                           uint32_t want, bool check_signatures, Selection &s) {
    s.n = n; s.want = want; s.size = (uint64_t)1 << ix.depth; s.check_signatures = check_signatures; s.s_idx = s_idx;
    s.fixed.assign(n, REASON_NONE);
    s.rx_ok.assign(n, 1);
    s.cands.assign(n, Candidate{NO_ROW, NO_ROW, 0, 0});
    s.status.assign(n, STATUS_NOT_REACHED);
    s.verdict.assign(n, NO_VERDICT);
    std::unordered_map<uint64_t, uint32_t> seen, row_of; // sender index -> candidates so far; leaf -> row
    auto row = [&](uint64_t a, const Value &v) {
        const auto it = row_of.emplace(a, s.n_rows());
        if (it.second) s.rows.insert(s.rows.end(), v.begin(), v.end());
        return it.first->second;
    };
    for (uint32_t t = 0; t < n; t++) {
        const uint64_t si = s_idx[t], ri = r_idx[t];
        const uint32_t k = seen[si]++;
        if (sig_rx)
            for (int w = 0; w < 6; w++)
                if (sig_rx[(size_t)6 * t + w] >= host::P) s.rx_ok[t] = 0;
        if (si >= s.size || ri >= s.size) { s.fixed[t] = REASON_INDEX; continue; }
        if (si == ri) { s.fixed[t] = REASON_SELF; continue; }
        if (!ix.is_known(si) || !ix.is_known(ri)) { s.fixed[t] = REASON_UNKNOWN; continue; }
        const auto sv = ix.accounts.find(si), rv = ix.accounts.find(ri);
        if (sv == ix.accounts.end() || rv == ix.accounts.end()) { s.fixed[t] = REASON_ABSENT; continue; }
        const uint32_t s_row = row(si, sv->second); // two statements: the sender's row is numbered first
        const uint32_t r_row = row(ri, rv->second);
        s.cands[t] = Candidate{s_row, r_row, deltas[t], host::from_u64(k)};
    }
    s.balance.resize(s.n_rows());
    for (uint32_t i = 0; i < s.n_rows(); i++) s.balance[i] = s.rows[(size_t)14 * i + 12];
}

// the message candidate t signs, as k_select_gather builds it on the device; zeros for a candidate that is not checkable
inline void select_message(const Selection &s, uint32_t t, uint64_t *out /* [28] */) {
    memset(out, 0, 28 * 8);
    const Candidate &c = s.cands[t];
    if (c.s_row >= s.n_rows() || c.r_row >= s.n_rows()) return;
    memcpy(out, &s.rows[(size_t)14 * c.s_row], 96);
    memcpy(out + 12, &s.rows[(size_t)14 * c.r_row], 96);
    out[24] = c.delta;
    out[25] = host::add(s.rows[(size_t)14 * c.s_row + 13], c.k);
}

// true: every candidate has its status.  false: the walk stands at candidate s.at and needs s.verdict[s.at]
inline bool select_walk(Selection &s) {
    using namespace cs::host;
    for (; s.at < s.n; s.at++) {
        const uint32_t t = s.at;
        if (s.n_selected == s.want) { s.status[t] = STATUS_NOT_REACHED; continue; }
        const uint64_t si = s.s_idx[t];
        const Candidate &c = s.cands[t];
        uint8_t st = s.fixed[t];
        if (st == REASON_NONE) {
            if (s.held.count(si)) st = STATUS_HELD;
            else if (to_u64(c.delta) > to_u64(s.balance[c.s_row])) st = REASON_BALANCE;
            else if (s.check_signatures) {
                if (!s.rx_ok[t]) st = REASON_SIGNATURE; // equals no canonical x: never sent to the device
                else if (s.verdict[t] == NO_VERDICT) return false;
                else if (s.verdict[t] != 0) st = REASON_SIGNATURE;
            }
        }
        s.status[t] = st;
        if (st != REASON_NONE) {
            if (si < s.size) s.held.insert(si);
            continue;
        }
        s.balance[c.s_row] = sub(s.balance[c.s_row], c.delta);
        s.balance[c.r_row] = add(s.balance[c.r_row], c.delta);
        s.selected.push_back(t);
        s.n_selected++;
    }
    return true;
}

// the default size of a pass: the selections still missing, rounded up to a multiple of 1,024 (the count whose check costs what one
// signature's costs)
inline uint32_t select_default_chunk(const Selection &s) { return (s.want - s.n_selected + 1023) / 1024 * 1024; }

// after select_walk returned false: the candidate it waits for, then the checkable candidates after it that have no verdict yet and
// whose sender is not held by now (a hold is for the rest of the call), `chunk` at the most, in list order
inline void select_chunk(const Selection &s, uint32_t chunk, std::vector<uint32_t> &list) {
    list.clear();
    for (uint32_t t = s.at; t < s.n && list.size() < chunk; t++)
        if (s.fixed[t] == REASON_NONE && s.rx_ok[t] && s.verdict[t] == NO_VERDICT && !s.held.count(s.s_idx[t])) list.push_back(t);
}

// after select_walk returned true.  pow2: the selection is cut to the largest power of two it holds, as if `want` had been that
// number -- what precedes the cut does not depend on `want`, so everything after the last selected candidate becomes NOT_REACHED
inline void select_finish(Selection &s, bool pow2) {
    if (!pow2 || s.selected.empty()) return;
    uint32_t keep = 1;
    while (2 * keep <= s.n_selected) keep *= 2;
    if (keep == s.n_selected) return;
    for (uint32_t t = s.selected[keep - 1] + 1; t < s.n; t++) s.status[t] = STATUS_NOT_REACHED;
    s.selected.resize(keep);
    s.n_selected = keep;
}

// the selection as the batch plan_apply takes
inline void select_batch(const Selection &s, const uint64_t *s_idx, const uint64_t *r_idx, const uint64_t *deltas, std::vector<uint64_t> &bs,
                         std::vector<uint64_t> &br, std::vector<uint64_t> &bd) {
    for (const uint32_t t : s.selected) { bs.push_back(s_idx[t]); br.push_back(r_idx[t]); bd.push_back(deltas[t]); }
}

// cstark_ledger_open_accounts: the authentication paths of `count` leaves of the tree as it stands, in the witness's form (path[0] = the
// leaf, path[k + 1] = the sibling at level depth - k).  One emit list of count (depth + 1) entries, `witness`, whose word offsets count
// from the staging area [stage_slot, stage_slot + count (depth + 1)) that follows the list in the scratch: path i starts at word
// 7 (depth + 1) i.  An absent leaf and an untouched sibling read the level's empty-subtree slot (Index::slot).  Indices may repeat.
// `at`: the checkpoint position whose state is opened (Index::slot_at; HEAD = the current state, the lookup is Index::slot then).
// Nothing of the index changes and nothing is hashed.  false: an index is out of range, or the call is too large to plan.
inline uint64_t open_scratch_slots(uint32_t depth, uint64_t count) { return (count * (depth + 1) + 6) / 7 + count * (depth + 1); }
inline bool plan_open(const Index &ix, uint32_t scratch_base, uint32_t count, const uint64_t *indices, Plan &p, size_t at = HEAD) {
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
        p.witness.push_back({ix.slot_at(at, d, a), word});
        for (uint32_t k = 0; k < d; k++) p.witness.push_back({ix.slot_at(at, d - k, (a >> k) ^ 1), word + 7 * (k + 1)});
    }
    p.final_root_slot = ix.slot_at(at, 0, 0);
    detail::pack_lists(p);
    p.stage_slot = (uint32_t)p.pool_slots;
    p.pool_slots += p.witness.size();
    return p.pool_slots <= MAX_POOL_SLOTS;
}

// after the device work of a plan has been enqueued: the index follows, and the newest live checkpoint logs what it replaces
inline void commit(Index &ix, const Plan &p) {
    Checkpoint *log = ix.checkpoints.empty() ? nullptr : &ix.checkpoints.back();
    for (const NewNode &nn : p.new_nodes) {
        if (log) {
            const auto it = ix.node[nn.level].find(nn.x);
            log->node[nn.level].emplace(nn.x, it == ix.node[nn.level].end() ? ABSENT_SLOT : it->second);
        }
        ix.node[nn.level][nn.x] = nn.slot;
    }
    ix.free_slots.resize(ix.free_slots.size() - p.from_free);
    ix.n_stored += p.extended;
    for (const auto &kv : p.new_values) {
        if (log && !log->accounts.count(kv.first)) {
            const auto it = ix.accounts.find(kv.first);
            log->accounts.emplace(kv.first, it == ix.accounts.end() ? std::make_pair(false, Value{}) : std::make_pair(true, it->second));
        }
        ix.accounts[kv.first] = kv.second;
    }
}

// cstark_ledger_checkpoint: names the current state.  0: the cap of MAX_CHECKPOINTS live checkpoints is reached.
inline uint64_t checkpoint(Index &ix) {
    if (ix.checkpoints.size() >= MAX_CHECKPOINTS) return 0;
    ix.checkpoints.emplace_back(ix.next_id, ix.depth);
    return ix.next_id++;
}

// cstark_ledger_revert: the index goes back to the state at position `at`.  The logs are undone from the newest down to that one; the
// slot a node holds when its log entry is undone was written after that checkpoint and is named by nothing older, so it is freed.
// The checkpoints after `at` are dropped and `at` stays live with an empty log.  Host bookkeeping only.
inline void revert(Index &ix, size_t at) {
    for (size_t k = ix.checkpoints.size(); k-- > at;) {
        Checkpoint &c = ix.checkpoints[k];
        for (uint32_t l = 0; l <= ix.depth; l++)
            for (const auto &kv : c.node[l]) {
                const auto it = ix.node[l].find(kv.first);
                ix.free_slots.push_back(it->second);
                if (kv.second == ABSENT_SLOT) ix.node[l].erase(it);
                else it->second = kv.second;
            }
        for (const auto &kv : c.accounts) {
            if (kv.second.first) ix.accounts[kv.first] = kv.second.second;
            else ix.accounts.erase(kv.first);
        }
    }
    ix.checkpoints.erase(ix.checkpoints.begin() + at + 1, ix.checkpoints.end());
    Checkpoint &c = ix.checkpoints[at];
    for (auto &level : c.node) level.clear();
    c.accounts.clear();
}

// cstark_ledger_release: the checkpoint at position `at` ends.  Its log merges into its predecessor's, where the entries the predecessor
// already holds win (the state at the predecessor is older): the loser's slot was the node's between the two checkpoints and nothing
// names it any more.  The oldest checkpoint has no predecessor: all its slots are freed.
inline void release(Index &ix, size_t at) {
    Checkpoint &c = ix.checkpoints[at];
    Checkpoint *before = at ? &ix.checkpoints[at - 1] : nullptr;
    for (uint32_t l = 0; l <= ix.depth; l++)
        for (const auto &kv : c.node[l])
            if (!(before && before->node[l].emplace(kv.first, kv.second).second) && kv.second != ABSENT_SLOT) ix.free_slots.push_back(kv.second);
    if (before)
        for (const auto &kv : c.accounts) before->accounts.emplace(kv.first, kv.second);
    ix.checkpoints.erase(ix.checkpoints.begin() + at);
}

// the nodes of the state at checkpoint position `at`, all levels: the index with the logs from the newest down to `at` undone on a copy
inline NodeMap nodes_at(const Index &ix, size_t at) {
    NodeMap m = ix.node;
    for (size_t k = ix.checkpoints.size(); k > at; k--)
        for (uint32_t l = 0; l <= ix.depth; l++)
            for (const auto &kv : ix.checkpoints[k - 1].node[l]) {
                if (kv.second == ABSENT_SLOT) m[l].erase(kv.first);
                else m[l][kv.first] = kv.second;
            }
    return m;
}

// cstark_ledger_audit: is the state at `at` a Merkle tree?  ONE list of independent jobs (left, right, expected): the job passes iff
// merge(left, right) equals the digest STORED in slot `expected` (Job::out; nothing is written).  Every job reads stored children, never
// recomputed ones, so one launch serves all levels.  The order is fixed, and Plan::audited names the node of every job:
//   1. the empty-subtree slots, level depth - 1 down to 0: slot l against merge(slot l + 1, slot l + 1)        [depth jobs]
//   2. the leaves by ascending index: the two halves of the account's value, uploaded as a slot pair           [n_leaves jobs]
//   3. the inner nodes, level depth - 1 down to 0, ascending x within a level: the children by Index::slot_at  [n_inner jobs]
// The all-zero test of slot `depth` is no job: the caller reads that one slot back and compares it on the host.
// false: the state is too large to plan.
inline uint64_t audit_scratch_slots(uint64_t leaves, uint64_t jobs) { return 2 * leaves + (2 * jobs + 6) / 7; }
inline bool plan_audit(const Index &ix, size_t at, const NodeMap &m /* nodes_at(ix, at) */, uint32_t scratch_base, Plan &p) {
    const uint32_t d = ix.depth;
    uint64_t n_jobs = d;
    for (const auto &level : m) n_jobs += level.size();
    const uint64_t n_leaves = m[d].size();
    if (n_jobs > 0xFFFFFFF0ull || (uint64_t)scratch_base + audit_scratch_slots(n_leaves, n_jobs) > MAX_POOL_SLOTS) return false;
    p.upload_slot = scratch_base;
    p.audit_leaves = (uint32_t)n_leaves;
    p.upload.assign((size_t)14 * n_leaves, 0);
    p.jobs.reserve(n_jobs);
    p.audited.reserve(n_jobs);
    for (uint32_t l = d; l-- > 0;) {
        p.jobs.push_back({l + 1, l + 1, l, 0});
        p.audited.push_back({l, 0, l});
    }
    std::vector<std::pair<uint64_t, uint32_t>> sorted;
    for (uint32_t l = d + 1; l-- > 0;) {
        sorted.assign(m[l].begin(), m[l].end());
        std::sort(sorted.begin(), sorted.end());
        for (size_t i = 0; i < sorted.size(); i++) {
            const uint64_t x = sorted[i].first;
            if (ix.is_opaque(l, x)) continue; // a proof node of a partial ledger is not tested itself: its parent's job reads it
            if (l == d) {
                const Value *v = ix.value_at(at, x); // a stored leaf without an account fails its job against the zero value
                if (v) memcpy(&p.upload[14 * i], v->data(), sizeof *v);
                p.jobs.push_back({scratch_base + 2 * (uint32_t)i, scratch_base + 2 * (uint32_t)i + 1, sorted[i].second, 0});
            } else {
                auto child = [&](uint64_t y) -> uint32_t {
                    const auto it = m[l + 1].find(y);
                    return it == m[l + 1].end() ? l + 1 : it->second;
                };
                p.jobs.push_back({child(2 * x), child(2 * x + 1), sorted[i].second, 0});
            }
            p.audited.push_back({l, x, sorted[i].second});
        }
    }
    p.launch = {0, (uint32_t)p.jobs.size()};
    p.final_root_slot = p.audited.empty() ? 0 : ix.slot_at(at, 0, 0);
    detail::pack_lists(p);
    return p.pool_slots <= MAX_POOL_SLOTS;
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
