// The account ledger on gfx950: the Merkle work of the reference's transfer loop (TransactionMetadata::build_random,
// /root/reference/src/lib.rs:341-422) as depth + 1 dependent launches of independent Rescue merges, planned on the host
// (ledger_plan.h: balance walk, predecessor map, slot numbering) and run over one device pool of digests.
//   k_ledger_merge    one list of merge jobs (left slot, right slot, output slot): 14 lanes per hash, four hashes per wave, the
//                     lane-per-state-element permutation of the trace kernels (rescue_lane.cuh)
//   k_ledger_gather   one emit list (pool slot -> word offset): paths, roots and old values into the resident witness; the touched
//                     nodes' last versions into the stored nodes
// One launch per level, ordered by the stream: every input of a launch was written by an earlier launch or by the upload, so no
// workgroup ever waits for another one.
// cstark_ledger_apply_checked puts the signature check (trace_gen.hip, launch_signature_check) between the host plan and the first
// change: the plan's balance walk builds the message every transfer signs, the check runs in scratch of the context.
// The read side: cstark_ledger_open_accounts gathers authentication paths out of the pool (plan_open, k_ledger_gather, no hashing);
// cstark_account_check_paths, which needs no ledger, folds paths to their roots:
//   k_path_check      one path per 14 lanes: the leaf hash and all `depth` merges of a path in one launch
// Checkpoints (cstark_ledger_checkpoint, _revert, _release, _root_at, _open_accounts_at) are host bookkeeping of ledger_plan.h: old states
// are kept by not overwriting their slots, and nothing here launches for them but the gather of an opening.
// cstark_ledger_audit tests that a state is a Merkle tree, every stored node against its STORED children, in one launch:
//   k_ledger_audit    one list of jobs (left slot, right slot, expected slot) in the shape of k_ledger_merge; reads the pool only
// Multi-openings (multiproof_plan.h): cstark_ledger_open_multi gathers the de-duplicated sibling set of many leaves (plan_open_multi,
// k_ledger_gather, no hashing); cstark_account_check_multiproof, which needs no ledger, folds it level by level in a block of its own:
//   k_multi_level     one level of a multiproof's fold in the shape of k_ledger_merge: the leaf hashes, a level's job list, or the
//                     root's one job with the compare against the stated root
// cstark_account_check_update, which needs no ledger either, folds ONE multiproof over the old and the new state of its accounts:
//   k_multi_update    k_multi_level with two sides per job: the launches of one check for both folds, the new side hashing only above
//                     a changed leaf and reading the proof nodes where the old side reads them
// A partial ledger (cstark_ledger_create_partial, multiproof_plan.h: plan_seed) is a ledger built from a multi-opening: one upload puts
// the proof nodes into their final pool slots, k_ledger_merge hashes the leaves and folds the levels straight into the stored nodes, and
// the root is compared on the host before the index is committed.  It knows the opened accounts only (Index::is_known): apply refuses
// a transfer with an unknown account, the other calls refuse unknown indices (all_known), the audit skips the opaque proof nodes.
// cstark_tx_witness_check, which needs no ledger, tests a whole transaction witness, the host's or the resident one, in one launch:
//   k_witness_check     k_path_check's four chains given to ONE transfer: sender-old, sender-new, receiver-old, receiver-new, all leaves
//                       hashed from values, the four folds met in wave ballots, one verdict byte per transfer
//   k_witness_messages  the message every transfer signs, gathered from its witness row for the signature check (trace_gen.hip)
// cstark_ledger_select picks a provable batch out of a pool of candidates (ledger_plan.h: select_prepare, select_walk).  The pool goes up
// once; per pass of the signature check the host uploads candidate numbers only:
//   k_select_gather     messages, sig_rx and sig_s of the listed candidates, compacted into the signature check's block
#include <stdio.h>
#include <string.h>
#include <mutex>
#include <new>
#include <unordered_map>
#include "../../include/cstark.h"
#include "ctx.h"
#include "ledger_plan.h"
#include "multiproof_plan.h"
#include "rescue_lane.cuh"

namespace cs {
namespace {

// out = Rescue63::merge(left, right) for jobs [0, n_jobs): lanes 0..55 = (hash s, state element e), lanes 56..63 and the hashes of a
// partial last group only take part in the barriers.  A slot outside the pool (the plan never emits one) makes its hash inactive.
__global__ __launch_bounds__(64) void k_ledger_merge(fp *pool, const ledger::Job *__restrict__ jobs, uint32_t n_jobs, uint32_t pool_slots) {
    __shared__ fp st[4][14];
    const int lane = threadIdx.x;
    const bool is_state = lane < 56;
    const int s = is_state ? lane / 14 : 0, e = is_state ? lane % 14 : 0;
    const uint32_t j = 4 * blockIdx.x + s;
    bool active = is_state && j < n_jobs;
    fp mrow[14];
#pragma unroll
    for (int k = 0; k < 14; k++) mrow[k] = c_mds[e * 14 + k];
    uint32_t left = 0, right = 0, out = 0;
    if (active) {
        left = jobs[j].left; right = jobs[j].right; out = jobs[j].out;
        active = left < pool_slots && right < pool_slots && out < pool_slots;
    }
    fp v = 0;
    if (active) v = e < 7 ? pool[(size_t)7 * left + e] : pool[(size_t)7 * right + e - 7];
    for (int cyc = 0; cyc < 7; cyc++) v = rescue_round_lane(v, st[s], mrow, e, cyc, active);
    if (active && e < 7) pool[(size_t)7 * out + e] = v;
}

// cstark_ledger_audit: does merge(left, right) equal the digest stored in slot `out` (the expected slot), for jobs [0, n_jobs)?  The shape
// of k_ledger_merge with one more load and a compare: after the permutation the lanes e < 7 hold the digest, their seven verdicts meet
// in one wave ballot, and lane e = 0 of a failing hash reports it: result[0] = min(result[0], job), result[1] += 1 (the host pre-fills
// 0xFFFFFFFF and 0 on the stream).  Nothing else is written, the pool never: the result does not depend on the order of the waves.  A job
// that names a slot outside the pool fails without a load.  A workgroup without a job leaves ahead of its first barrier.
__global__ __launch_bounds__(64) void k_ledger_audit(const fp *__restrict__ pool, const ledger::Job *__restrict__ jobs, uint32_t n_jobs, uint32_t pool_slots,
                                                     uint32_t *__restrict__ result) {
    __shared__ fp st[4][14];
    if (4 * blockIdx.x >= n_jobs) return; // the whole workgroup
    const int lane = threadIdx.x;
    const bool is_state = lane < 56;
    const int s = is_state ? lane / 14 : 0, e = is_state ? lane % 14 : 0;
    const uint32_t j = 4 * blockIdx.x + s;
    const bool active = is_state && j < n_jobs;
    fp mrow[14];
#pragma unroll
    for (int k = 0; k < 14; k++) mrow[k] = c_mds[e * 14 + k];
    uint32_t left = 0, right = 0, expected = 0;
    bool hashing = false; // active and every slot inside the pool
    if (active) {
        left = jobs[j].left; right = jobs[j].right; expected = jobs[j].out;
        hashing = left < pool_slots && right < pool_slots && expected < pool_slots;
    }
    fp v = 0, want = 0;
    if (hashing) {
        v = e < 7 ? pool[(size_t)7 * left + e] : pool[(size_t)7 * right + e - 7];
        if (e < 7) want = pool[(size_t)7 * expected + e];
    }
    for (int cyc = 0; cyc < 7; cyc++) v = rescue_round_lane(v, st[s], mrow, e, cyc, hashing);
    const unsigned long long differ = __ballot(hashing && e < 7 && v != want);
    if (active && e == 0 && (!hashing || (differ & (0x7Full << (14 * s))))) {
        atomicMin(&result[0], j);
        atomicAdd(&result[1], 1u);
    }
}

// cstark_account_check_multiproof: one launch of the fold of a multiproof over its block of digest slots (multiproof_plan.h), in the shape
// of k_ledger_merge: lanes 0..55 = (hash s, state element e), lanes 56..63 and the hashes of a partial last group only attend the
// barriers; a workgroup without a job leaves ahead of its first barrier.  Three uses, told apart by uniform arguments:
//   values != null    the leaf launch: job j hashes values[j][0..14) into slot j, or writes the all-zero digest where present[j] == 0
//   jobs != null      a level: slot out = merge(slot left, slot right) for jobs [0, n_jobs)
//   result != null    with jobs, the launch of level 0 (one job): the seven words meet the stated root in one wave ballot; result word 0 =
//                     the verdict (as 64 bits), words 1..7 = the folded root, all by plain vector stores
// Every slot is tested against block_slots before it is read or written.  A job that names a slot outside the block is inactive and sets
// *fault (the host clears it in the upload; every writer stores the same 1); the last launch reads it -- the stream ordered the earlier
// launches before it -- and a set fault makes the verdict ROOT.  No launch waits for another workgroup.
static_assert((int)CSTARK_MULTI_VALID == (int)multi::VALID && (int)CSTARK_MULTI_INDEX == (int)multi::INDEX &&
                  (int)CSTARK_MULTI_NODE_COUNT == (int)multi::NODE_COUNT && (int)CSTARK_MULTI_ROOT == (int)multi::ROOT,
              "k_multi_level writes the values of cstark_multi_verdict");
__global__ __launch_bounds__(64) void k_multi_level(fp *block, uint32_t block_slots, const ledger::Job *__restrict__ jobs, const fp *__restrict__ values,
                                                    const uint8_t *__restrict__ present, uint32_t n_jobs, uint32_t *fault, const fp *__restrict__ stated,
                                                    fp *result) {
    __shared__ fp st[4][14];
    if (4 * blockIdx.x >= n_jobs) return; // the whole workgroup
    const int lane = threadIdx.x;
    const bool is_state = lane < 56;
    const int s = is_state ? lane / 14 : 0, e = is_state ? lane % 14 : 0;
    const uint32_t j = 4 * blockIdx.x + s;
    const bool active = is_state && j < n_jobs;
    fp mrow[14];
#pragma unroll
    for (int k = 0; k < 14; k++) mrow[k] = c_mds[e * 14 + k];
    uint32_t left = 0, right = 0, out = 0;
    bool inside = false, hashing = false; // inside: active and every slot in the block; hashing: and there is something to hash
    fp v = 0;
    if (values) { // uniform
        out = j;
        inside = active && j < block_slots;
        hashing = inside && (present ? present[j] != 0 : true);
        if (hashing) v = values[(size_t)14 * j + e];
    } else {
        if (active) {
            left = jobs[j].left; right = jobs[j].right; out = jobs[j].out;
            inside = left < block_slots && right < block_slots && out < block_slots;
        }
        hashing = inside;
        if (hashing) v = e < 7 ? block[(size_t)7 * left + e] : block[(size_t)7 * right + e - 7];
    }
    for (int cyc = 0; cyc < 7; cyc++) v = rescue_round_lane(v, st[s], mrow, e, cyc, hashing);
    if (!hashing) v = 0; // an absent leaf
    if (inside && e < 7) block[(size_t)7 * out + e] = v;
    if (active && !inside && e == 0) *fault = 1;
    if (result) { // uniform: one job, hash s = 0
        const unsigned long long differ = __ballot(inside && e < 7 && v != stated[e]);
        if (active && e < 7) result[1 + e] = v;
        if (active && e == 0) result[0] = (!inside || (differ & 0x7Full) || *fault != 0) ? (fp)CSTARK_MULTI_ROOT : (fp)CSTARK_MULTI_VALID;
    }
}

// cstark_account_check_update: one launch of the fold of ONE multiproof over two states of its leaves (multiproof_plan.h, plan_update), in
// the lane shape of k_multi_level.  A job has two sides and a wave carries two jobs: hash s = 2 * (job within the wave) + side, side 0 the
// old state and side 1 the new one, which sit in neighbouring groups of 14 lanes.  The new side hashes only where the job's flag says a
// changed leaf lies below; elsewhere it takes the old side's digest from the lanes 14 below by a cross-lane move that every lane executes.
// The new side's slots are the old side's through multi::update_new_slot: a proof node is read from the one slot it has.  The uses:
//   old_values != null    the leaf launch: job j hashes old_values[j] into slot j and, where state[j] says changed, new_values[j] into the
//                         new leaf slot; an absent side writes the all-zero digest
//   jobs != null          a level: out = merge(left, right) on either side, for jobs [0, n_jobs)
//   result != null        with jobs, the launch of level 0 (one job): both roots meet the stated ones (stated[0..7) old, stated[8..15) new,
//                         the latter only with have_new) in one wave ballot; result word 0 = the verdict (as 64 bits), words 1..7 = the
//                         new side's fold, all by plain vector stores
// Every slot is tested against the old side's slots before it is mapped and against block_slots before it is read or written; a job that
// names one outside is inactive on that side and sets *fault, as in k_multi_level, and a set fault makes the verdict OLD_ROOT.  No launch
// waits for another workgroup, and a workgroup without a job leaves ahead of its first barrier.
static_assert((int)CSTARK_UPDATE_VALID == (int)multi::UPDATE_VALID && (int)CSTARK_UPDATE_INDEX == (int)multi::UPDATE_INDEX &&
                  (int)CSTARK_UPDATE_NODE_COUNT == (int)multi::UPDATE_NODE_COUNT && (int)CSTARK_UPDATE_OLD_ROOT == (int)multi::UPDATE_OLD_ROOT &&
                  (int)CSTARK_UPDATE_NEW_ROOT == (int)multi::UPDATE_NEW_ROOT,
              "k_multi_update writes the values of cstark_update_verdict");
__global__ __launch_bounds__(64) void k_multi_update(fp *block, uint32_t block_slots, uint32_t count, uint32_t n_nodes, uint32_t old_slots,
                                                     const ledger::Job *__restrict__ jobs, const fp *__restrict__ old_values,
                                                     const fp *__restrict__ new_values, const uint8_t *__restrict__ state, uint32_t n_jobs, uint32_t *fault,
                                                     const fp *__restrict__ stated, uint32_t have_new, fp *result) {
    __shared__ fp st[4][14];
    if (2 * blockIdx.x >= n_jobs) return; // the whole workgroup
    const int lane = threadIdx.x;
    const bool is_state = lane < 56;
    const int s = is_state ? lane / 14 : 0, e = is_state ? lane % 14 : 0;
    const int side = s & 1;
    const uint32_t j = 2 * blockIdx.x + (s >> 1);
    const bool active = is_state && j < n_jobs;
    fp mrow[14];
#pragma unroll
    for (int k = 0; k < 14; k++) mrow[k] = c_mds[e * 14 + k];
    uint32_t left = 0, right = 0, out = 0;
    bool inside = false, hashing = false, copies = false; // inside: active and every slot in the block; copies: the new digest is the old one
    fp v = 0;
    if (old_values) { // uniform
        inside = active && j < count && j < old_slots;
        out = j;
        if (inside && side) {
            out = multi::update_new_slot(j, count, n_nodes, old_slots);
            inside = out < block_slots;
        }
        const uint8_t is = inside ? state[j] : 0;
        copies = inside && side && !(is & multi::STATE_CHANGED);
        hashing = inside && !copies && (is & (side ? multi::STATE_NEW_PRESENT : multi::STATE_OLD_PRESENT));
        if (hashing) v = (side ? new_values : old_values)[(size_t)14 * j + e];
    } else {
        if (active) {
            left = jobs[j].left; right = jobs[j].right; out = jobs[j].out;
            inside = left < old_slots && right < old_slots && out < old_slots;
            copies = inside && side && !jobs[j].reserved;
        }
        if (inside && side) {
            out = multi::update_new_slot(out, count, n_nodes, old_slots);
            if (!copies) {
                left = multi::update_new_slot(left, count, n_nodes, old_slots);
                right = multi::update_new_slot(right, count, n_nodes, old_slots);
            }
        }
        inside = inside && left < block_slots && right < block_slots && out < block_slots;
        copies = copies && inside;
        hashing = inside && !copies;
        if (hashing) v = e < 7 ? block[(size_t)7 * left + e] : block[(size_t)7 * right + e - 7];
    }
    for (int cyc = 0; cyc < 7; cyc++) v = rescue_round_lane(v, st[s], mrow, e, cyc, hashing);
    if (!hashing) v = 0; // an absent leaf
    const fp old_digest = __shfl(v, side ? lane - 14 : lane, 64); // every lane; the old side of hash s is hash s - 1
    if (copies) v = old_digest;
    if (inside && e < 7) block[(size_t)7 * out + e] = v;
    if (active && !inside && e == 0) *fault = 1;
    if (result) { // uniform: one job, hashes s = 0 (old) and s = 1 (new)
        const unsigned long long differ = __ballot(inside && e < 7 && v != stated[8 * side + e]);
        const unsigned long long outside = __ballot(active && !inside); // either side: this launch's own fault, whatever *fault shows yet
        if (active && side && e < 7) result[1 + e] = v;
        if (active && s == 0 && e == 0) {
            const bool old_bad = (differ & 0x3FFFull) || outside || *fault != 0, new_bad = ((differ >> 14) & 0x3FFFull) && have_new;
            result[0] = old_bad ? (fp)CSTARK_UPDATE_OLD_ROOT : new_bad ? (fp)CSTARK_UPDATE_NEW_ROOT : (fp)CSTARK_UPDATE_VALID;
        }
    }
}

// dst[word .. word + 7) = pool slot, for emits [0, n): one thread per word
__global__ __launch_bounds__(256) void k_ledger_gather(const fp *pool, const ledger::Emit *__restrict__ list, uint32_t n, uint32_t pool_slots,
                                                       fp *dst, size_t dst_words) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t m = (uint32_t)(i / 7), k = (uint32_t)(i % 7);
    if (m >= n) return;
    const uint32_t slot = list[m].slot;
    const size_t word = (size_t)list[m].word + k;
    if (slot < pool_slots && word < dst_words) dst[word] = pool[(size_t)7 * slot + k];
}

// cstark_account_check_paths: the leaf hash (with values) and the `depth` merges of one authentication path in ONE launch, in the shape
// of k_ledger_merge: lanes 0..55 = (path s, state element e), lanes 56..63 and the paths of a partial last group only attend the
// barriers.  After a permutation the digest sits in the lanes e < 7; the next state is (digest, sibling) or (sibling, digest) by the
// index bit of the level, so the digest goes to the lanes e >= 7 by a cross-lane move that every lane executes and the bit selects
// data only.  depth is uniform: every lane of the workgroup reaches every barrier.  The sibling of the next level is loaded ahead of
// the permutation that precedes its use.  Every read is inside [0, count) paths of depth + 1 digests.
__global__ __launch_bounds__(64) void k_path_check(const uint64_t *__restrict__ indices, const fp *__restrict__ values, const uint8_t *__restrict__ present,
                                                   const fp *__restrict__ paths, const fp *__restrict__ roots, uint32_t n_roots, uint32_t count,
                                                   uint32_t depth, uint8_t *__restrict__ verdicts, fp *__restrict__ roots_out) {
    __shared__ fp st[4][14];
    if (4 * blockIdx.x >= count) return; // the whole workgroup, ahead of its first barrier
    const int lane = threadIdx.x;
    const bool is_state = lane < 56;
    const int s = is_state ? lane / 14 : 0, e = is_state ? lane % 14 : 0;
    const bool low = e < 7;
    const int w = low ? e : e - 7;     // the digest word this lane holds in either half
    const int from = low ? lane : lane - 7;
    const uint32_t i = 4 * blockIdx.x + s;
    const bool active = is_state && i < count;
    fp mrow[14];
#pragma unroll
    for (int k = 0; k < 14; k++) mrow[k] = c_mds[e * 14 + k];
    const uint32_t bits = active ? (uint32_t)indices[i] : 0; // the fold reads bits 0 .. depth - 1 <= 30 only
    const uint32_t at = 7 * (depth + 1) * (active ? i : 0) + w; // this lane's word of entry 0: below 2^20 * 32 * 7
    fp cur = active ? paths[at] : 0;     // the stated leaf digest
    fp sib = active ? paths[at + 7] : 0; // depth >= 1
    unsigned long long leaf_bad = 0;
    if (values) { // uniform
        const bool have = active && (present ? present[i] != 0 : true);
        fp v = active ? values[(size_t)14 * i + e] : 0;
        for (int cyc = 0; cyc < 7; cyc++) v = rescue_round_lane(v, st[s], mrow, e, cyc, active);
        leaf_bad = __ballot(active && low && cur != (have ? v : (fp)0));
    }
    for (uint32_t k = 0; k < depth; k++) {
        const bool right = (bits >> k) & 1; // this node is the right child: the sibling is the left half
        const fp moved = __shfl(cur, from, 64);
        fp v = low == right ? sib : moved;
        if (active && k + 1 < depth) sib = paths[at + 7 * (k + 2)];
        for (int cyc = 0; cyc < 7; cyc++) v = rescue_round_lane(v, st[s], mrow, e, cyc, active);
        cur = v;
    }
    fp stated = 0;
    if (active && low) stated = roots[(size_t)7 * (n_roots == 1 ? 0 : i) + e];
    const unsigned long long root_bad = __ballot(active && low && cur != stated);
    if (active && low) roots_out[(size_t)7 * i + e] = cur;
    if (active && e == 0) {
        const unsigned long long mine = 0x7Full << (14 * s);
        verdicts[i] = (indices[i] >> depth) ? CSTARK_PATH_INDEX_RANGE
                      : (leaf_bad & mine) ? CSTARK_PATH_LEAF
                      : (root_bad & mine) ? CSTARK_PATH_ROOT
                                          : CSTARK_PATH_VALID;
    }
}

// cstark_tx_witness_check: the body of k_path_check with its four chains given to ONE transfer.  One 64-lane workgroup per transfer;
// lanes 0..55 = (chain s, state element e), lanes 56..63 only attend the barriers.  Chain 0 folds the sender's old leaf, 1 the sender's
// new leaf, 2 the receiver's old leaf, 3 the receiver's new leaf; chains 0/1 read the siblings of s_paths and the bits of s_index,
// chains 2/3 those of r_paths and r_index.  Every chain hashes its leaf from values: chain 1 forms balance - delta and nonce + 1,
// chain 3 balance + delta in the lane that holds the word (field arithmetic, src/lib.rs:373-375).  The stated digests s_paths[t][0]
// and r_paths[t][0] are no chain inputs: chain 0's leaf is compared with the first, chain 3's with the second, and both chains then go
// on from the STATED digest, so that the path tests are tests of the paths as stated.  The four folds meet their counterparts in one
// wave ballot: chain 0 initial_roots[t], chain 1 the fold of chain 2 (a cross-lane move that every lane executes), chain 3
// initial_roots[t + 1] or, for the last transfer, final_root (null: that test does not run).  Lane e = 0 of chain 0 stores the verdict
// byte; the lanes e < 7 of every chain store their fold.  Nothing else is written: no atomics, no flag, nothing waits for another
// workgroup.  depth is uniform, so every lane reaches every barrier.  Every read is inside transfer t < n_tx of its segment.
static_assert(CSTARK_WITNESS_VALID == 0 && CSTARK_WITNESS_INDEX_RANGE == 1 && CSTARK_WITNESS_SELF_TRANSFER == 2 && CSTARK_WITNESS_SENDER_LEAF == 3 &&
                  CSTARK_WITNESS_SENDER_PATH == 4 && CSTARK_WITNESS_BALANCE == 5 && CSTARK_WITNESS_MIDDLE_ROOT == 6 && CSTARK_WITNESS_RECEIVER_LEAF == 7 &&
                  CSTARK_WITNESS_NEXT_ROOT == 8 && CSTARK_WITNESS_SIGNATURE == 9,
              "the order of cstark_witness_verdict is the order of the tests");
__global__ __launch_bounds__(64) void k_witness_check(const fp *__restrict__ initial_roots, const fp *__restrict__ s_old, const fp *__restrict__ r_old,
                                                      const uint64_t *__restrict__ s_idx, const uint64_t *__restrict__ r_idx,
                                                      const fp *__restrict__ s_paths, const fp *__restrict__ r_paths, const fp *__restrict__ deltas,
                                                      const fp *__restrict__ final_root, uint32_t n_tx, uint32_t depth, uint8_t *__restrict__ verdicts,
                                                      fp *__restrict__ folds) {
    __shared__ fp st[4][14];
    const uint32_t t = blockIdx.x;
    if (t >= n_tx) return; // the whole workgroup, ahead of its first barrier
    const int lane = threadIdx.x;
    const bool active = lane < 56;
    const int s = active ? lane / 14 : 0, e = active ? lane % 14 : 0;
    const bool low = e < 7;
    const int w = low ? e : e - 7;
    const int from = low ? lane : lane - 7;
    const bool sender = s < 2;
    fp mrow[14];
#pragma unroll
    for (int k = 0; k < 14; k++) mrow[k] = c_mds[e * 14 + k];
    const uint64_t si = s_idx[t], ri = r_idx[t];
    const uint32_t bits = (uint32_t)(sender ? si : ri); // the fold reads bits 0 .. depth - 1 <= 30 only
    const fp *path = (sender ? s_paths : r_paths) + (size_t)7 * (depth + 1) * t + w; // this lane's word of entry 0
    const fp delta = deltas[t];
    fp v = (sender ? s_old : r_old)[(size_t)14 * t + e];
    if (s == 1 && e == 12) v = fp_sub(v, delta);
    if (s == 1 && e == 13) v = fp_add(v, FP_ONE);
    if (s == 3 && e == 12) v = fp_add(v, delta); // may wrap past p: no verdict, as in the ledger
    const fp stated_leaf = path[0];
    fp sib = path[7]; // depth >= 1
    for (int cyc = 0; cyc < 7; cyc++) v = rescue_round_lane(v, st[s], mrow, e, cyc, active);
    const unsigned long long leaf_bad = __ballot(active && low && v != stated_leaf); // read for chains 0 and 3 only
    fp cur = (s == 0 || s == 3) ? stated_leaf : v;
    for (uint32_t k = 0; k < depth; k++) {
        const bool right = (bits >> k) & 1; // this node is the right child: the sibling is the left half
        const fp moved = __shfl(cur, from, 64);
        v = low == right ? sib : moved;
        if (k + 1 < depth) sib = path[7 * (k + 2)];
        for (int cyc = 0; cyc < 7; cyc++) v = rescue_round_lane(v, st[s], mrow, e, cyc, active);
        cur = v;
    }
    const fp above = __shfl(cur, (lane + 14) & 63, 64); // chain s + 1's fold: chain 1 meets chain 2
    const bool last = t + 1 == n_tx;
    fp want = cur; // chain 2, and chain 3 of the last transfer without a stated root: no test
    if (active && low) {
        if (s == 0) want = initial_roots[(size_t)7 * t + e];
        else if (s == 1) want = above;
        else if (s == 3 && !last) want = initial_roots[(size_t)7 * (t + 1) + e];
        else if (s == 3 && final_root) want = final_root[e];
        folds[(size_t)7 * (4 * t + s) + e] = cur;
    }
    const unsigned long long fold_bad = __ballot(active && low && cur != want);
    if (lane == 0) {
        const unsigned long long chain = 0x7Full;
        const bool range = (si >> depth) || (ri >> depth);
        const bool balance = fp_to_u64(delta) > fp_to_u64(s_old[(size_t)14 * t + 12]);
        verdicts[t] = range ? CSTARK_WITNESS_INDEX_RANGE
                      : si == ri ? CSTARK_WITNESS_SELF_TRANSFER
                      : (leaf_bad & chain) ? CSTARK_WITNESS_SENDER_LEAF
                      : (fold_bad & chain) ? CSTARK_WITNESS_SENDER_PATH
                      : balance ? CSTARK_WITNESS_BALANCE
                      : (fold_bad & (chain << 14)) ? CSTARK_WITNESS_MIDDLE_ROOT
                      : (leaf_bad & (chain << 42)) ? CSTARK_WITNESS_RECEIVER_LEAF
                      : (fold_bad & (chain << 42)) ? CSTARK_WITNESS_NEXT_ROOT
                                                   : CSTARK_WITNESS_VALID;
    }
}

// The messages of cstark_tx_witness_check's signature test, one lane per word: transfer t signs build_tx_message (src/lib.rs:467-481)
// of its own witness row -- the sender's key, the receiver's key, delta, the sender's old nonce, two zeros -- into messages [n_tx][28].
__global__ __launch_bounds__(256) void k_witness_messages(const fp *__restrict__ s_old, const fp *__restrict__ r_old, const fp *__restrict__ deltas,
                                                          uint32_t n_tx, fp *__restrict__ messages) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t t = i / 28;
    const uint32_t k = (uint32_t)(i % 28);
    if (t >= n_tx) return;
    messages[i] = k < 12 ? s_old[14 * t + k] : k < 24 ? r_old[14 * t + k - 12] : k == 24 ? deltas[t] : k == 25 ? s_old[14 * t + 13] : (fp)0;
}

// One pass of cstark_ledger_select's signature check: entry j of the pass is candidate list[j] of the pool that was uploaded once
// (account table rows [n_rows][14], candidate table cands [n], sig_rx [n][6], sig_s [n][32] as four words).  One thread per 64-bit output
// word, 38 per entry, compacted into the signature check's block: the message (ledger_plan.h, select_message: the sender's key, the
// receiver's key, delta, the stored nonce + k_t, two zeros), sig_rx and sig_s.  A candidate number outside the pool or a row outside
// the table writes zeros; nothing else is written.
__global__ __launch_bounds__(256) void k_select_gather(const fp *__restrict__ rows, uint32_t n_rows, const ledger::Candidate *__restrict__ cands,
                                                       const fp *__restrict__ sig_rx, const uint64_t *__restrict__ sig_s, uint32_t n,
                                                       const uint32_t *__restrict__ list, uint32_t m, fp *__restrict__ messages, fp *__restrict__ rx_out,
                                                       uint64_t *__restrict__ s_out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t j = i / 38;
    const uint32_t k = (uint32_t)(i % 38);
    if (j >= m) return;
    const uint32_t t = list[j];
    uint64_t v = 0;
    if (t < n) {
        if (k < 28) {
            const uint32_t s_row = cands[t].s_row, r_row = cands[t].r_row;
            if (s_row < n_rows && r_row < n_rows)
                v = k < 12 ? rows[(size_t)14 * s_row + k] : k < 24 ? rows[(size_t)14 * r_row + k - 12] : k == 24 ? cands[t].delta
                  : k == 25 ? fp_add(rows[(size_t)14 * s_row + 13], cands[t].k) : (fp)0;
        } else if (k < 34) v = sig_rx[(size_t)6 * t + k - 28];
        else v = sig_s[(size_t)4 * t + k - 34];
    }
    if (k < 28) messages[28 * j + k] = v;
    else if (k < 34) rx_out[6 * j + k - 28] = v;
    else s_out[4 * j + k - 34] = v;
}

} // namespace
} // namespace cs

struct cstark_ledger {
    cstark_ctx *ctx;
    cs::ledger::Index index;
    uint64_t *pool = nullptr;    // device: EMPTY_SLOTS | stored nodes (capacity) | scratch of the call in flight
    uint32_t capacity = 0;       // stored-node slots reserved
    uint64_t pool_slots = 0;
    bool broken = false;         // a HIP call failed inside a ledger call: the pool's content is unknown
    uint32_t *audit_words = nullptr; // device: {first failing job, failing jobs} of cstark_ledger_audit, allocated by the first audit
    cstark_ledger(cstark_ctx *c, uint32_t depth) : ctx(c), index(depth) {}
};

namespace {
using namespace cs::ledger;
using cs::fail;

// room for `new_nodes` more stored nodes and `scratch` slots behind them; *scratch_base = the first scratch slot
int reserve_pool(cstark_ledger *L, uint64_t new_nodes, uint64_t scratch, uint32_t *scratch_base) {
    cstark_ctx *c = L->ctx;
    const uint64_t need_nodes = (uint64_t)L->index.n_stored + new_nodes;
    uint64_t cap = L->capacity;
    if (need_nodes > cap) {
        cap = cap ? cap : 1024;
        while (cap < need_nodes) cap *= 2;
    }
    const uint64_t slots = EMPTY_SLOTS + cap + scratch;
    if (slots > MAX_POOL_SLOTS) return fail(CSTARK_ERR_UNSUPPORTED, "ledger: the batch needs more than 2^28 digest slots");
    if (cap != L->capacity || slots > L->pool_slots) {
        uint64_t *fresh = nullptr;
        HIP_TRY(hipMalloc(&fresh, slots * 56));
        if (L->pool) {
            hipError_t e = hipMemcpyAsync(fresh, L->pool, ((size_t)EMPTY_SLOTS + L->index.n_stored) * 56, hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) { (void)hipFree(fresh); HIP_TRY(e); }
            HIP_TRY(hipFree(L->pool));
        } else {
            hipError_t e = hipMemsetAsync(fresh, 0, (size_t)EMPTY_SLOTS * 56, c->stream);
            if (e != hipSuccess) { (void)hipFree(fresh); HIP_TRY(e); }
        }
        L->pool = fresh;
        L->capacity = (uint32_t)cap;
        L->pool_slots = slots;
    }
    *scratch_base = EMPTY_SLOTS + L->capacity;
    return CSTARK_OK;
}

// upload block, merge launches, then the emit lists: `witness` into dst_witness (may be empty), `commit` back into the pool
int run_plan(cstark_ledger *L, const Plan &p, uint64_t *dst_witness, size_t witness_words) {
    cstark_ctx *c = L->ctx;
    if (p.pool_slots > L->pool_slots) return fail(CSTARK_ERR_INVALID_ARG, "ledger: plan exceeds the reserved pool");
    uint64_t *block = L->pool + (size_t)7 * p.upload_slot;
    HIP_TRY(hipMemcpyAsync(block, p.upload.data(), p.upload.size() * 8, hipMemcpyHostToDevice, c->stream));
    const uint32_t slots = (uint32_t)L->pool_slots;
    const Job *d_jobs = (const Job *)(block + p.jobs_word);
    for (size_t k = 0; k + 1 < p.launch.size(); k++) {
        const uint32_t n = p.launch[k + 1] - p.launch[k];
        if (n == 0) continue;
        hipLaunchKernelGGL(cs::k_ledger_merge, dim3((n + 3) / 4), dim3(64), 0, c->stream, L->pool, d_jobs + p.launch[k], n, slots);
        HIP_TRY(hipGetLastError());
    }
    if (!p.witness.empty()) {
        const uint32_t n = (uint32_t)p.witness.size();
        hipLaunchKernelGGL(cs::k_ledger_gather, dim3((uint32_t)(((size_t)7 * n + 255) / 256)), dim3(256), 0, c->stream, L->pool,
                           (const Emit *)(block + p.witness_word), n, slots, dst_witness, witness_words);
        HIP_TRY(hipGetLastError());
    }
    if (!p.commit.empty()) {
        const uint32_t n = (uint32_t)p.commit.size();
        hipLaunchKernelGGL(cs::k_ledger_gather, dim3((uint32_t)(((size_t)7 * n + 255) / 256)), dim3(256), 0, c->stream, L->pool,
                           (const Emit *)(block + p.commit_word), n, slots, L->pool, (size_t)7 * (EMPTY_SLOTS + L->capacity));
        HIP_TRY(hipGetLastError());
    }
    return CSTARK_OK;
}

int create_impl(cstark_ledger *L) {
    cstark_ctx *c = L->ctx;
    HIP_TRY(hipSetDevice(c->device));
    uint32_t scratch_base;
    Plan p;
    plan_empty_digests(L->index.depth, 0, p); // sizes only
    RC_TRY(reserve_pool(L, 0, (p.upload.size() + 6) / 7, &scratch_base));
    Plan q;
    plan_empty_digests(L->index.depth, scratch_base, q);
    RC_TRY(run_plan(L, q, nullptr, 0));
    HIP_TRY(cs::stream_wait(c->stream)); // the plan's host block is read by the copy
    return CSTARK_OK;
}

// cstark_ledger_create_partial behind its argument checks and host verdicts (sp is plan_seed's).  The pool is reserved with exactly the
// plan's stored slots, so the scratch follows them; the empty-subtree digests as in create_impl, then ONE upload (proof nodes into their
// final slots, values and job list into the scratch), the leaf launch and one launch per level of k_ledger_merge straight into the stored
// nodes, and the root read back.  *matches = the fold is the stated root; the caller commits the index only then.
int create_partial_impl(cstark_ledger *L, const cs::multi::SeedPlan &sp, const uint64_t *root, bool *matches) {
    cstark_ctx *c = L->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const Plan &p = sp.plan;
    Plan sizes, empty;
    plan_empty_digests(L->index.depth, 0, sizes); // sizes only
    const uint64_t scratch = std::max<uint64_t>(p.pool_slots - (EMPTY_SLOTS + p.extended), (sizes.upload.size() + 6) / 7);
    L->capacity = p.extended; // reserve_pool keeps a capacity that covers the need
    uint32_t scratch_base;
    RC_TRY(reserve_pool(L, 0, scratch, &scratch_base));
    if (scratch_base != EMPTY_SLOTS + p.extended) return fail(CSTARK_ERR_INVALID_ARG, "ledger: pool layout differs from the plan's");
    plan_empty_digests(L->index.depth, scratch_base, empty);
    RC_TRY(run_plan(L, empty, nullptr, 0));
    RC_TRY(run_plan(L, p, nullptr, 0));
    uint64_t fold[7];
    HIP_TRY(hipMemcpyAsync(fold, L->pool + (size_t)7 * p.final_root_slot, 56, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // the fold is on the host; the plans' host blocks are read by the copies
    *matches = memcmp(fold, root, 56) == 0;
    return CSTARK_OK;
}

int set_accounts_impl(cstark_ledger *L, uint32_t count, const uint64_t *indices, const uint64_t *values) {
    cstark_ctx *c = L->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t d = L->index.depth;
    // values (2 slots each), at most depth + 1 jobs per account (2 words each): an upper bound on the upload block
    const uint64_t scratch = 2ull * count + ((uint64_t)count * (d + 1) * 2 + 6) / 7 + 1;
    uint32_t scratch_base;
    RC_TRY(reserve_pool(L, max_new_nodes(d, count), scratch, &scratch_base));
    Plan p;
    if (!plan_set_accounts(L->index, scratch_base, count, indices, values, p))
        return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_set_accounts: an index is out of range or given twice, or a value word is not reduced");
    RC_TRY(run_plan(L, p, nullptr, 0));
    commit(L->index, p);
    HIP_TRY(cs::stream_wait(c->stream));
    return CSTARK_OK;
}

int root_impl(cstark_ledger *L, uint64_t *root, size_t at = HEAD) {
    cstark_ctx *c = L->ctx;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(root, L->pool + (size_t)7 * L->index.slot_at(at, 0, 0), 56, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(cs::stream_wait(c->stream));
    return CSTARK_OK;
}

int apply_impl(cstark_ledger *L, uint32_t n_tx, const uint64_t *s_indices, const uint64_t *r_indices, const uint64_t *deltas, const uint64_t *sig_rx,
               const uint8_t *sig_s, cstark_tx_witness *out, int32_t *refused_at, int32_t *reason, bool check_signatures,
               uint64_t *root_out = nullptr /* cstark_ledger_select: the root the batch leaves, read inside the call's one wait */) {
    cstark_ctx *c = L->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t d = L->index.depth, ne = 2 * n_tx;
    // the host plan first: a refused batch touches neither the pool nor the resident witness
    const uint64_t new_nodes = max_new_nodes(d, ne);
    uint64_t cap = L->capacity ? L->capacity : 1024;
    while (cap < (uint64_t)L->index.n_stored + new_nodes) cap *= 2;
    if (EMPTY_SLOTS + cap > MAX_POOL_SLOTS) return fail(CSTARK_ERR_UNSUPPORTED, "ledger: the batch needs more than 2^28 digest slots");
    Plan p;
    std::vector<uint64_t> messages;
    if (!plan_apply(L->index, (uint32_t)(EMPTY_SLOTS + cap), n_tx, s_indices, r_indices, deltas, p, check_signatures ? &messages : nullptr))
        return fail(CSTARK_ERR_UNSUPPORTED, "cstark_ledger_apply: the batch is too large to plan");
    // cstark_ledger_apply_checked: the signatures of the transfers the plan accepted, all of them or those before its refusal, in the
    // context's own scratch and ahead of every change; the first bad one refuses the batch
    const uint32_t n_signed = (uint32_t)(messages.size() / 28);
    if (n_signed) {
        std::vector<uint8_t> verdicts(n_signed);
        RC_TRY(signature_check(c, "cstark_ledger_apply_checked", n_signed, messages.data(), sig_rx, sig_s, verdicts.data(), nullptr));
        for (uint32_t t = 0; t < n_signed; t++)
            if (verdicts[t] != CSTARK_SIG_VALID) {
                *refused_at = (int32_t)t;
                *reason = REASON_SIGNATURE;
                return CSTARK_OK;
            }
    }
    *refused_at = p.refused_at;
    *reason = p.reason;
    if (p.refused_at >= 0) return CSTARK_OK;
    uint32_t scratch_base;
    RC_TRY(reserve_pool(L, new_nodes, p.pool_slots - (EMPTY_SLOTS + cap), &scratch_base));
    if (scratch_base != EMPTY_SLOTS + cap) return fail(CSTARK_ERR_INVALID_ARG, "ledger: pool layout differs from the plan's");
    size_t sz[cs::WIT_NUM_SEGMENTS], off[cs::WIT_NUM_SEGMENTS + 1];
    RC_TRY(tx_witness_reserve(c, n_tx, d, sz, off));
    char *base = (char *)c->wit_buf;
    const void *src[cs::WIT_NUM_SEGMENTS] = {};
    src[cs::WIT_S_IDX] = s_indices; src[cs::WIT_R_IDX] = r_indices; src[cs::WIT_DELTAS] = deltas; src[cs::WIT_SIG_RX] = sig_rx; src[cs::WIT_SIG_S] = sig_s;
    for (int i = 0; i < cs::WIT_NUM_SEGMENTS; i++)
        if (src[i]) HIP_TRY(hipMemcpyAsync(base + off[i], src[i], sz[i], hipMemcpyHostToDevice, c->stream));
    RC_TRY(run_plan(L, p, (uint64_t *)base, off[cs::WIT_NUM_SEGMENTS] / 8));
    tx_witness_bind(c, n_tx, d, off);
    commit(L->index, p);
    if (out) {
        const int segs[] = {cs::WIT_INITIAL_ROOTS, cs::WIT_S_OLD, cs::WIT_R_OLD, cs::WIT_S_PATHS, cs::WIT_R_PATHS};
        void *dst[] = {(void *)out->initial_roots, (void *)out->s_old_values, (void *)out->r_old_values, (void *)out->s_paths, (void *)out->r_paths};
        for (int i = 0; i < 5; i++) HIP_TRY(hipMemcpyAsync(dst[i], base + off[segs[i]], sz[segs[i]], hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync((void *)out->final_root, L->pool + (size_t)7 * L->index.root_slot(), 56, hipMemcpyDeviceToHost, c->stream));
        memcpy((void *)out->s_indices, s_indices, sz[cs::WIT_S_IDX]);
        memcpy((void *)out->r_indices, r_indices, sz[cs::WIT_R_IDX]);
        memcpy((void *)out->deltas, deltas, sz[cs::WIT_DELTAS]);
        memcpy((void *)out->sig_rx, sig_rx, sz[cs::WIT_SIG_RX]);
        memcpy((void *)out->sig_s, sig_s, sz[cs::WIT_SIG_S]);
    }
    if (root_out) HIP_TRY(hipMemcpyAsync(root_out, L->pool + (size_t)7 * L->index.root_slot(), 56, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(cs::stream_wait(c->stream)); // the caller's arrays and the plan's host block are read by the copies
    return CSTARK_OK;
}

// one upload of the emit list, one gather into the staging area behind it, the paths and the root copied out: no hashing, and neither
// the stored nodes nor the index nor the resident witness change (reserve_pool may move the pool).  `at`: the checkpoint position whose
// state is opened (HEAD: the current one); only the slots the list names and the values copied out differ
int open_impl(cstark_ledger *L, uint32_t count, const uint64_t *indices, uint64_t *values_out, uint8_t *present_out, uint64_t *paths_out, uint64_t *root_out,
              size_t at = HEAD) {
    cstark_ctx *c = L->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t d = L->index.depth;
    uint32_t scratch_base;
    RC_TRY(reserve_pool(L, 0, open_scratch_slots(d, count), &scratch_base));
    Plan p;
    if (!plan_open(L->index, scratch_base, count, indices, p, at) || p.pool_slots > L->pool_slots)
        return fail(CSTARK_ERR_INVALID_ARG, "ledger: the opening exceeds the reserved pool");
    uint64_t *block = L->pool + (size_t)7 * p.upload_slot, *stage = L->pool + (size_t)7 * p.stage_slot;
    const uint32_t n = (uint32_t)p.witness.size();
    HIP_TRY(hipMemcpyAsync(block, p.upload.data(), p.upload.size() * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(cs::k_ledger_gather, dim3((uint32_t)(((size_t)7 * n + 255) / 256)), dim3(256), 0, c->stream, L->pool,
                       (const Emit *)(block + p.witness_word), n, (uint32_t)L->pool_slots, stage, (size_t)7 * n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(paths_out, stage, (size_t)56 * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(root_out, L->pool + (size_t)7 * p.final_root_slot, 56, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(cs::stream_wait(c->stream)); // the plan's host block is read by the upload
    for (uint32_t i = 0; i < count; i++) {
        const Value *v = L->index.value_at(at, indices[i]);
        present_out[i] = v != nullptr;
        if (v) memcpy(values_out + (size_t)14 * i, v->data(), 112);
        else memset(values_out + (size_t)14 * i, 0, 112);
    }
    return CSTARK_OK;
}

// cstark_ledger_audit behind its argument checks: the job list of plan_audit in the scratch of the pool (one upload), the two result
// words pre-filled on the stream, ONE k_ledger_audit, the result words and empty-subtree slot `depth` copied back.  That slot's all-zero
// test runs here on the host; it counts as the first job of the order (kind EMPTY, level depth) when it fails.
int audit_impl(cstark_ledger *L, size_t at, cstark_ledger_audit_report *report) {
    cstark_ctx *c = L->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const Index &ix = L->index;
    const uint32_t d = ix.depth;
    const NodeMap nodes = nodes_at(ix, at);
    uint64_t n_nodes = 0;
    for (const auto &level : nodes) n_nodes += level.size();
    uint32_t scratch_base;
    RC_TRY(reserve_pool(L, 0, audit_scratch_slots(nodes[d].size(), n_nodes + d), &scratch_base));
    Plan p;
    if (!plan_audit(ix, at, nodes, scratch_base, p)) return fail(CSTARK_ERR_UNSUPPORTED, "cstark_ledger_audit: the state is too large to plan");
    if (p.pool_slots > L->pool_slots) return fail(CSTARK_ERR_INVALID_ARG, "ledger: the audit exceeds the reserved pool");
    if (!L->audit_words) HIP_TRY(hipMalloc(&L->audit_words, 8));
    const uint32_t n = (uint32_t)p.jobs.size();
    uint64_t *block = L->pool + (size_t)7 * p.upload_slot;
    uint32_t words[2] = {0xFFFFFFFFu, 0};
    uint64_t zero_slot[7];
    HIP_TRY(hipMemcpyAsync(block, p.upload.data(), p.upload.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(L->audit_words, words, 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(cs::k_ledger_audit, dim3((n + 3) / 4), dim3(64), 0, c->stream, L->pool, (const Job *)(block + p.jobs_word), n, (uint32_t)L->pool_slots,
                       L->audit_words);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(words, L->audit_words, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(zero_slot, L->pool + (size_t)7 * d, 56, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // the words above and the plan's host block are read and written by the copies
    bool zero_bad = false;
    for (int k = 0; k < 7; k++) zero_bad |= zero_slot[k] != 0;
    cstark_ledger_audit_report r = {};
    r.n_bad = words[1] + (zero_bad ? 1 : 0);
    r.consistent = r.n_bad == 0;
    if (zero_bad) {
        r.first_kind = CSTARK_LEDGER_NODE_EMPTY; r.first_level = d; r.first_index = 0;
    } else if (words[1]) {
        if (words[0] >= n) return fail(CSTARK_ERR_HIP, "cstark_ledger_audit: the kernel reported a job it was not given");
        const NewNode &node = p.audited[words[0]];
        r.first_kind = words[0] < d ? CSTARK_LEDGER_NODE_EMPTY : node.level == d ? CSTARK_LEDGER_NODE_LEAF : CSTARK_LEDGER_NODE_INNER;
        r.first_level = node.level; r.first_index = node.x;
    }
    r.n_nodes = n_nodes;
    r.slots_live = ix.live_nodes();
    r.slots_free = ix.free_slots.size();
    r.slots_held = ix.n_stored - r.slots_live - r.slots_free;
    *report = r;
    return CSTARK_OK;
}

// cstark_account_check_paths behind its argument checks.  One device block of the context, grown when needed:
//   indices [count] | values [count][14] | paths [count][depth + 1][7] | roots [n_roots][7] | roots_out [count][7] | present [count] | verdicts [count]
// (values and present only when given).  Nothing of the resident witness, tail_buf or the statement caches is read or written.
static_assert(sizeof(cstark_path_verdict) >= 1 && CSTARK_PATH_VALID == 0 && CSTARK_PATH_INDEX_RANGE == 1 && CSTARK_PATH_LEAF == 2 && CSTARK_PATH_ROOT == 3,
              "k_path_check writes the values of cstark_path_verdict");
int check_paths_impl(cstark_ctx *c, uint32_t count, uint32_t depth, const uint64_t *indices, const uint64_t *values, const uint8_t *present,
                     const uint64_t *paths, const uint64_t *roots, uint32_t n_roots, uint8_t *verdicts, uint64_t *roots_out) {
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = count, path_words = (size_t)7 * (depth + 1) * n;
    const size_t words = n + (values ? 14 * n : 0) + path_words + (size_t)7 * n_roots + 7 * n, bytes = words * 8 + 2 * n;
    if (c->path_bytes < bytes) {
        if (c->path_buf) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->path_buf)); c->path_buf = nullptr; c->path_bytes = 0; }
        HIP_TRY(hipMalloc(&c->path_buf, bytes));
        c->path_bytes = bytes;
    }
    uint64_t *d_idx = (uint64_t *)c->path_buf, *d_val = d_idx + n, *d_paths = d_val + (values ? 14 * n : 0), *d_roots = d_paths + path_words;
    uint64_t *d_out = d_roots + (size_t)7 * n_roots;
    uint8_t *d_present = (uint8_t *)(d_out + 7 * n), *d_verdicts = d_present + n;
    HIP_TRY(hipMemcpyAsync(d_idx, indices, n * 8, hipMemcpyHostToDevice, c->stream));
    if (values) HIP_TRY(hipMemcpyAsync(d_val, values, n * 112, hipMemcpyHostToDevice, c->stream));
    if (present) HIP_TRY(hipMemcpyAsync(d_present, present, n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_paths, paths, path_words * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_roots, roots, (size_t)56 * n_roots, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(cs::k_path_check, dim3((count + 3) / 4), dim3(64), 0, c->stream, d_idx, values ? d_val : nullptr, present ? d_present : nullptr, d_paths,
                       d_roots, n_roots, count, depth, d_verdicts, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(verdicts, d_verdicts, n, hipMemcpyDeviceToHost, c->stream));
    if (roots_out) HIP_TRY(hipMemcpyAsync(roots_out, d_out, n * 56, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // synchronous: the verdicts are on the host, the caller's arrays are free again
    return CSTARK_OK;
}

// cstark_ledger_open_multi behind its argument checks (the indices have a shape of n_nodes proof nodes, nodes_out holds them): one upload
// of the emit list, one gather into the staging area behind it, the nodes and the root copied out.  No hashing; stored nodes, index and
// resident witness are unchanged (reserve_pool may move the pool)
int open_multi_impl(cstark_ledger *L, size_t at, uint32_t count, const uint64_t *indices, uint32_t n_nodes, uint64_t *values_out, uint8_t *present_out,
                    uint64_t *nodes_out, uint64_t *root_out) {
    cstark_ctx *c = L->ctx;
    HIP_TRY(hipSetDevice(c->device));
    uint32_t scratch_base;
    RC_TRY(reserve_pool(L, 0, cs::multi::open_multi_scratch_slots(n_nodes), &scratch_base));
    Plan p;
    if (!cs::multi::plan_open_multi(L->index, at, scratch_base, count, indices, p) || p.pool_slots > L->pool_slots || p.witness.size() != (size_t)n_nodes + 1)
        return fail(CSTARK_ERR_INVALID_ARG, "ledger: the multi-opening exceeds the reserved pool");
    uint64_t *block = L->pool + (size_t)7 * p.upload_slot, *stage = L->pool + (size_t)7 * p.stage_slot;
    const uint32_t n = n_nodes + 1;
    HIP_TRY(hipMemcpyAsync(block, p.upload.data(), p.upload.size() * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(cs::k_ledger_gather, dim3((uint32_t)(((size_t)7 * n + 255) / 256)), dim3(256), 0, c->stream, L->pool,
                       (const Emit *)(block + p.witness_word), n, (uint32_t)L->pool_slots, stage, (size_t)7 * n);
    HIP_TRY(hipGetLastError());
    if (n_nodes) HIP_TRY(hipMemcpyAsync(nodes_out, stage, (size_t)56 * n_nodes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(root_out, stage + (size_t)7 * n_nodes, 56, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(cs::stream_wait(c->stream)); // the plan's host block is read by the upload
    for (uint32_t i = 0; i < count; i++) {
        const Value *v = L->index.value_at(at, indices[i]);
        present_out[i] = v != nullptr;
        if (v) memcpy(values_out + (size_t)14 * i, v->data(), 112);
        else memset(values_out + (size_t)14 * i, 0, 112);
    }
    return CSTARK_OK;
}

// cstark_account_check_multiproof behind its argument checks and its host verdicts (the plan exists, n_nodes is the shape's).  One
// device block of the context, grown when needed, in 64-bit words:
//   digest slots [p.slots][7] | values [count][14] (when given) | upload: stated root [7], fault word, jobs [n_merges][2], result [8] | present [count] bytes
// The upload block goes up in one copy; leaves (or values and present) and nodes are the caller's arrays and go up as they are.  Then the
// leaf launch (with values) and one launch per level, ordered by the stream.  Nothing of the resident witness, path_buf, tail_buf or the
// statement caches is read or written.
int check_multi_impl(cstark_ctx *c, uint32_t depth, uint32_t count, const uint64_t *values, const uint8_t *present, const uint64_t *leaves,
                     const uint64_t *nodes, const uint64_t *root, const cs::multi::CheckPlan &p, uint32_t *verdict, uint64_t *root_out) {
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = count, n_jobs = p.jobs.size();
    const size_t slot_words = (size_t)7 * p.slots, value_words = values ? 14 * n : 0, upload_words = 8 + 2 * n_jobs;
    const size_t bytes = (slot_words + value_words + upload_words + 8) * 8 + n;
    if (c->multi_bytes < bytes) {
        if (c->multi_buf) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->multi_buf)); c->multi_buf = nullptr; c->multi_bytes = 0; }
        HIP_TRY(hipMalloc(&c->multi_buf, bytes));
        c->multi_bytes = bytes;
    }
    uint64_t *d_slots = (uint64_t *)c->multi_buf, *d_values = d_slots + slot_words, *d_upload = d_values + value_words, *d_result = d_upload + upload_words;
    uint8_t *d_present = (uint8_t *)(d_result + 8);
    std::vector<uint64_t> upload(upload_words + 8, 0); // word 7: the fault word, cleared; the result words behind the jobs: no verdict yet
    std::fill(upload.end() - 8, upload.end(), ~(uint64_t)0);
    memcpy(upload.data(), root, 56);
    memcpy(upload.data() + 8, p.jobs.data(), 16 * n_jobs);
    if (values) HIP_TRY(hipMemcpyAsync(d_values, values, n * 112, hipMemcpyHostToDevice, c->stream));
    else HIP_TRY(hipMemcpyAsync(d_slots, leaves, n * 56, hipMemcpyHostToDevice, c->stream));
    if (present) HIP_TRY(hipMemcpyAsync(d_present, present, n, hipMemcpyHostToDevice, c->stream));
    if (p.shape.n_nodes) HIP_TRY(hipMemcpyAsync(d_slots + 7 * n, nodes, (size_t)56 * p.shape.n_nodes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_upload, upload.data(), upload.size() * 8, hipMemcpyHostToDevice, c->stream));
    uint32_t *d_fault = (uint32_t *)(d_upload + 7);
    const Job *d_jobs = (const Job *)(d_upload + 8);
    if (values) {
        hipLaunchKernelGGL(cs::k_multi_level, dim3((count + 3) / 4), dim3(64), 0, c->stream, d_slots, p.slots, (const Job *)nullptr, d_values,
                           present ? d_present : nullptr, count, d_fault, (const uint64_t *)nullptr, (uint64_t *)nullptr);
        HIP_TRY(hipGetLastError());
    }
    for (uint32_t k = 0; k < depth; k++) {
        const uint32_t m = p.launch[k + 1] - p.launch[k];
        const bool last = k + 1 == depth; // level 0: one job
        hipLaunchKernelGGL(cs::k_multi_level, dim3((m + 3) / 4), dim3(64), 0, c->stream, d_slots, p.slots, d_jobs + p.launch[k], (const uint64_t *)nullptr,
                           (const uint8_t *)nullptr, m, d_fault, last ? d_upload : nullptr, last ? d_result : nullptr);
        HIP_TRY(hipGetLastError());
    }
    uint64_t result[8];
    HIP_TRY(hipMemcpyAsync(result, d_result, 64, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // synchronous: the verdict is on the host, the caller's arrays and the upload block are free again
    if (result[0] != CSTARK_MULTI_VALID && result[0] != CSTARK_MULTI_ROOT) return fail(CSTARK_ERR_HIP, "cstark_account_check_multiproof: the kernel wrote no verdict");
    *verdict = (uint32_t)result[0];
    if (root_out) memcpy(root_out, result + 1, 56);
    return CSTARK_OK;
}

// cstark_account_check_update behind its argument checks and its host verdicts (the plan exists with its changed flags, n_nodes is the
// shape's).  The device block is the multiproof checks' (multi_buf: both calls are synchronous, upload everything they read and keep
// nothing in it between calls, so they share the one block, grown to the larger need), here in 64-bit words:
//   digest slots [update_block_slots][7] | old values [count][14] | new values [count][14] |
//   upload: old root [7], fault word, new root [7] (zeros without one), a spare word, jobs [n_merges][2], result [8] | state [count] bytes
// The upload block goes up in one copy; values, nodes and state go up as they are.  Then the leaf launch and one launch per level, as
// many as ONE cstark_account_check_multiproof takes, ordered by the stream.  Nothing of the resident witness, path_buf, tail_buf or the
// statement caches is read or written.
int check_update_impl(cstark_ctx *c, uint32_t depth, uint32_t count, const uint64_t *old_values, const uint64_t *new_values, const uint64_t *nodes,
                      const uint64_t *old_root, const uint64_t *new_root, const cs::multi::CheckPlan &p, const std::vector<uint8_t> &state, uint32_t *verdict,
                      uint64_t *fold_out) {
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = count, n_jobs = p.jobs.size();
    const uint32_t n_nodes = p.shape.n_nodes, block_slots = (uint32_t)cs::multi::update_block_slots(count, n_nodes, p.shape.n_merges); // below 2^20 * 126
    const size_t slot_words = (size_t)7 * block_slots, value_words = 14 * n, upload_words = 16 + 2 * n_jobs;
    const size_t bytes = (slot_words + 2 * value_words + upload_words + 8) * 8 + n;
    if (c->multi_bytes < bytes) {
        if (c->multi_buf) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->multi_buf)); c->multi_buf = nullptr; c->multi_bytes = 0; }
        HIP_TRY(hipMalloc(&c->multi_buf, bytes));
        c->multi_bytes = bytes;
    }
    uint64_t *d_slots = (uint64_t *)c->multi_buf, *d_old = d_slots + slot_words, *d_new = d_old + value_words, *d_upload = d_new + value_words;
    uint64_t *d_result = d_upload + upload_words;
    uint8_t *d_state = (uint8_t *)(d_result + 8);
    std::vector<uint64_t> upload(upload_words + 8, 0); // word 7: the fault word, cleared; the result words behind the jobs: no verdict yet
    std::fill(upload.end() - 8, upload.end(), ~(uint64_t)0);
    memcpy(upload.data(), old_root, 56);
    if (new_root) memcpy(upload.data() + 8, new_root, 56);
    memcpy(upload.data() + 16, p.jobs.data(), 16 * n_jobs);
    HIP_TRY(hipMemcpyAsync(d_old, old_values, n * 112, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_new, new_values, n * 112, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_state, state.data(), n, hipMemcpyHostToDevice, c->stream));
    if (n_nodes) HIP_TRY(hipMemcpyAsync(d_slots + 7 * n, nodes, (size_t)56 * n_nodes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_upload, upload.data(), upload.size() * 8, hipMemcpyHostToDevice, c->stream));
    uint32_t *d_fault = (uint32_t *)(d_upload + 7);
    const Job *d_jobs = (const Job *)(d_upload + 16);
    hipLaunchKernelGGL(cs::k_multi_update, dim3((count + 1) / 2), dim3(64), 0, c->stream, d_slots, block_slots, count, n_nodes, p.slots, (const Job *)nullptr,
                       d_old, d_new, d_state, count, d_fault, (const uint64_t *)nullptr, 0u, (uint64_t *)nullptr);
    HIP_TRY(hipGetLastError());
    for (uint32_t k = 0; k < depth; k++) {
        const uint32_t m = p.launch[k + 1] - p.launch[k];
        const bool last = k + 1 == depth; // level 0: one job
        hipLaunchKernelGGL(cs::k_multi_update, dim3((m + 1) / 2), dim3(64), 0, c->stream, d_slots, block_slots, count, n_nodes, p.slots, d_jobs + p.launch[k],
                           (const uint64_t *)nullptr, (const uint64_t *)nullptr, (const uint8_t *)nullptr, m, d_fault, last ? d_upload : nullptr,
                           new_root ? 1u : 0u, last ? d_result : nullptr);
        HIP_TRY(hipGetLastError());
    }
    uint64_t result[8];
    HIP_TRY(hipMemcpyAsync(result, d_result, 64, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // synchronous: the verdict is on the host, the caller's arrays and the upload block are free again
    if (result[0] != CSTARK_UPDATE_VALID && result[0] != CSTARK_UPDATE_OLD_ROOT && result[0] != CSTARK_UPDATE_NEW_ROOT)
        return fail(CSTARK_ERR_HIP, "cstark_account_check_update: the kernel wrote no verdict");
    *verdict = (uint32_t)result[0];
    memcpy(fold_out, result + 1, 56);
    return CSTARK_OK;
}

// the first word >= p of a [rows][per_row] array, named as `name[row][col]` (paths: `name[row][entry][word]`)
bool reduced_words(const char *who, const char *name, const uint64_t *a, size_t rows, size_t per_row, bool entries) {
    for (size_t i = 0; i < rows * per_row; i++)
        if (a[i] >= cs::host::P) {
            char where[128];
            if (entries) snprintf(where, sizeof where, "%s: %s[%zu][%zu][%zu]", who, name, i / per_row, i % per_row / 7, i % 7);
            else snprintf(where, sizeof where, "%s: %s[%zu][%zu]", who, name, i / per_row, i % per_row);
            fail(CSTARK_ERR_INVALID_ARG, "%s is not a reduced field element", where);
            return false;
        }
    return true;
}

// the misuse of the multi-opening calls that take their indices on trust: indices[i] has no place in a strictly ascending list below 2^depth
int unsorted(const char *who, uint32_t i) {
    char where[128];
    snprintf(where, sizeof where, "%s: indices[%u]", who, i);
    return fail(CSTARK_ERR_INVALID_ARG, "%s is out of range or not above its predecessor (indices are strictly ascending)", where);
}

// The device block of cstark_tx_witness_check, one per context that made such a call: grown when a larger request comes, otherwise reused
// as it is, freed by cstark_ctx_destroy (witness_check_release).  It is kept by the context's address beside struct cstark_ctx, like the
// signing table and the proof form of capi.hip: every call uploads or computes all it reads there, so nothing in it outlives a call.
struct WitnessCheckBlock {
    void *buf;
    size_t bytes;
};
std::mutex &g_wcheck_lock = *new std::mutex; // never destroyed: a context may be destroyed while the process exits
std::unordered_map<const cstark_ctx *, WitnessCheckBlock> &g_wcheck_blocks = *new std::unordered_map<const cstark_ctx *, WitnessCheckBlock>;
int witness_check_block(cstark_ctx *c, size_t bytes, void **out) {
    std::lock_guard<std::mutex> hold(g_wcheck_lock);
    WitnessCheckBlock &b = g_wcheck_blocks[c]; // a new entry is {nullptr, 0}
    if (b.bytes < bytes) {
        if (b.buf) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(b.buf)); b.buf = nullptr; b.bytes = 0; }
        HIP_TRY(hipMalloc(&b.buf, bytes));
        b.bytes = bytes;
    }
    *out = b.buf;
    return CSTARK_OK;
}

// cstark_tx_witness_check behind its argument checks.  One device block of the context, grown when needed:
//   stated final root [7] | folds [n][4][7] | verdicts [n] (padded to 256 bytes) | host form only: the witness, as witness_layout.h lays it out
// host != null: its arrays go up into the block's own witness; otherwise `dev` is the resident witness, read where it lies.  The
// signature test runs in the signature check's block (signature_block, capi.hip) on messages gathered there, with sig_rx and sig_s
// read from the witness that is being checked.  Nothing of the resident witness, tail_buf or the statement caches is written.
int witness_check_impl(cstark_ctx *c, const cstark_tx_witness *host, cs::TxWitnessDev dev, const uint64_t *final_root, bool signatures,
                       cstark_witness_report *report, uint8_t *verdicts_out, uint64_t *folds_out) {
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = dev.n_tx, d = dev.depth;
    const size_t out_bytes = (56 + n * 224 + n + 255) & ~(size_t)255;
    size_t sz[cs::WIT_NUM_SEGMENTS], off[cs::WIT_NUM_SEGMENTS + 1];
    cs::witness_segments(n, d, sz, off);
    const size_t bytes = out_bytes + (host ? off[cs::WIT_NUM_SEGMENTS] : 0);
    void *block = nullptr;
    RC_TRY(witness_check_block(c, bytes, &block));
    uint64_t *d_root = (uint64_t *)block, *d_folds = d_root + 7;
    uint8_t *d_verdicts = (uint8_t *)(d_folds + 28 * n);
    if (host) {
        char *base = (char *)block + out_bytes;
        const void *src[cs::WIT_NUM_SEGMENTS] = {host->initial_roots, host->s_old_values, host->r_old_values, host->s_indices, host->r_indices, host->s_paths,
                                                 host->r_paths, host->deltas, host->sig_rx, nullptr, host->sig_s};
        for (int i = 0; i < cs::WIT_NUM_SEGMENTS; i++)
            if (src[i]) HIP_TRY(hipMemcpyAsync(base + off[i], src[i], sz[i], hipMemcpyHostToDevice, c->stream));
        dev.initial_roots = (const uint64_t *)(base + off[cs::WIT_INITIAL_ROOTS]);
        dev.s_old = (const uint64_t *)(base + off[cs::WIT_S_OLD]);
        dev.r_old = (const uint64_t *)(base + off[cs::WIT_R_OLD]);
        dev.s_idx = (const uint64_t *)(base + off[cs::WIT_S_IDX]);
        dev.r_idx = (const uint64_t *)(base + off[cs::WIT_R_IDX]);
        dev.s_paths = (const uint64_t *)(base + off[cs::WIT_S_PATHS]);
        dev.r_paths = (const uint64_t *)(base + off[cs::WIT_R_PATHS]);
        dev.deltas = (const uint64_t *)(base + off[cs::WIT_DELTAS]);
        dev.sig_rx = (const uint64_t *)(base + off[cs::WIT_SIG_RX]);
        dev.sig_s = (const uint8_t *)(base + off[cs::WIT_SIG_S]);
    }
    if (final_root) HIP_TRY(hipMemcpyAsync(d_root, final_root, 56, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(cs::k_witness_check, dim3((uint32_t)n), dim3(64), 0, c->stream, dev.initial_roots, dev.s_old, dev.r_old, dev.s_idx, dev.r_idx, dev.s_paths,
                       dev.r_paths, dev.deltas, final_root ? d_root : nullptr, (uint32_t)n, (uint32_t)d, d_verdicts, d_folds);
    HIP_TRY(hipGetLastError());
    std::vector<uint8_t> verdicts(n), sig(signatures ? n : 0);
    cstark_witness_report r = {};
    if (signatures) {
        cstark_sig_block b;
        RC_TRY(signature_block(c, (uint32_t)n, &b));
        hipLaunchKernelGGL(cs::k_witness_messages, dim3((uint32_t)((28 * n + 255) / 256)), dim3(256), 0, c->stream, dev.s_old, dev.r_old, dev.deltas, (uint32_t)n,
                           b.messages);
        HIP_TRY(hipGetLastError());
        HIP_TRY(cs::launch_signature_check(b.messages, dev.sig_rx, dev.sig_s, b.h_limbs, b.points, b.verdicts, b.x, (uint32_t)n, c->stream));
        HIP_TRY(hipMemcpyAsync(sig.data(), b.verdicts, n, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(verdicts.data(), d_verdicts, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(r.final_root, d_folds + 28 * (n - 1) + 21, 56, hipMemcpyDeviceToHost, c->stream));
    if (folds_out) HIP_TRY(hipMemcpyAsync(folds_out, d_folds, n * 224, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // synchronous: the verdicts are on the host, the caller's arrays are free again
    r.n_tx = (uint32_t)n; r.merkle_depth = (uint32_t)d; r.first_bad = -1;
    for (size_t t = 0; t < n; t++) {
        if (signatures && verdicts[t] == CSTARK_WITNESS_VALID && sig[t] != CSTARK_SIG_VALID) verdicts[t] = CSTARK_WITNESS_SIGNATURE;
        if (verdicts[t] == CSTARK_WITNESS_VALID) continue;
        if (r.first_bad < 0) { r.first_bad = (int32_t)t; r.first_verdict = verdicts[t]; }
        r.n_bad++;
    }
    if (verdicts_out) memcpy(verdicts_out, verdicts.data(), n);
    *report = r;
    return CSTARK_OK;
}

// cstark_ledger_select behind its argument checks.  The host walk (ledger_plan.h) decides everything; the device checks signatures in
// passes.  The pool of the call lives in the context's witness-check block (both calls are synchronous and upload all they read there):
//   account table [n_rows][14] | candidate table [n][3] | sig_rx [n][6] | sig_s [n][32] | candidate numbers of the pass [<= n] (4 bytes each)
// uploaded once, the list per pass.  k_select_gather compacts the pass into the signature check's block (signature_block),
// launch_signature_check follows unchanged and one verdict byte per entry comes back.  Statically refused candidates never go up in a
// list.  Nothing of the ledger is read or written on the device unless the selection is applied, and that is apply_impl on the compacted
// selection: cstark_ledger_apply's launches, with root_after read inside apply's own wait.  The outputs are written at the very end,
// after the last step that can fail; the messages that came back are kept compact until then (224 bytes per candidate SENT, not per candidate).
int select_impl(cstark_ledger *L, uint32_t n, const uint64_t *s_indices, const uint64_t *r_indices, const uint64_t *deltas, const uint64_t *sig_rx,
                const uint8_t *sig_s, uint32_t want, uint32_t flags, uint32_t chunk, uint8_t *status_out, uint32_t *selected_out, uint64_t *messages_out,
                cstark_ledger_selection *report, cstark_tx_witness *out) {
    cstark_ctx *c = L->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const bool check = flags & CSTARK_SELECT_CHECK_SIGNATURES;
    Selection s;
    select_prepare(L->index, n, s_indices, r_indices, deltas, check ? sig_rx : nullptr, want, check, s);
    cstark_ledger_selection rep = {};
    std::vector<uint64_t> sent_messages; // [n_sig_checked][28], in the order of `sent`
    std::vector<uint32_t> list, sent;
    std::vector<uint8_t> verdicts;
    uint64_t *d_rows = nullptr, *d_cands = nullptr, *d_rx = nullptr, *d_s = nullptr;
    uint32_t *d_list = nullptr;
    while (!select_walk(s)) {
        if (!d_rows) { // the first verdict the walk needs: the pool goes up, once
            const size_t n_rows = s.n_rows(), words = 14 * n_rows + (size_t)(3 + 6 + 4) * n;
            void *block = nullptr;
            RC_TRY(witness_check_block(c, words * 8 + (size_t)4 * n, &block));
            d_rows = (uint64_t *)block; d_cands = d_rows + 14 * n_rows; d_rx = d_cands + (size_t)3 * n; d_s = d_rx + (size_t)6 * n;
            d_list = (uint32_t *)(d_s + (size_t)4 * n);
            HIP_TRY(hipMemcpyAsync(d_rows, s.rows.data(), n_rows * 112, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(d_cands, s.cands.data(), (size_t)24 * n, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(d_rx, sig_rx, (size_t)48 * n, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(d_s, sig_s, (size_t)32 * n, hipMemcpyHostToDevice, c->stream));
        }
        select_chunk(s, chunk ? chunk : select_default_chunk(s), list);
        const uint32_t m = (uint32_t)list.size();
        if (m == 0 || list[0] != s.at) return fail(CSTARK_ERR_UNSUPPORTED, "cstark_ledger_select: the walk waits for a candidate no pass can hold");
        cstark_sig_block b;
        RC_TRY(signature_block(c, m, &b));
        HIP_TRY(hipMemcpyAsync(d_list, list.data(), (size_t)4 * m, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(cs::k_select_gather, dim3((uint32_t)(((size_t)38 * m + 255) / 256)), dim3(256), 0, c->stream, d_rows, s.n_rows(),
                           (const Candidate *)d_cands, d_rx, d_s, n, d_list, m, b.messages, b.sig_rx, (uint64_t *)b.sig_s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(cs::launch_signature_check(b.messages, b.sig_rx, b.sig_s, b.h_limbs, b.points, b.verdicts, b.x, m, c->stream));
        verdicts.resize(m);
        HIP_TRY(hipMemcpyAsync(verdicts.data(), b.verdicts, m, hipMemcpyDeviceToHost, c->stream));
        if (messages_out) {
            sent_messages.resize((size_t)28 * (sent.size() + m)); // before the copy is enqueued: the vector does not move under it
            HIP_TRY(hipMemcpyAsync(&sent_messages[(size_t)28 * sent.size()], b.messages, (size_t)224 * m, hipMemcpyDeviceToHost, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream)); // the verdicts are on the host; the list and, after the first pass, the pool's host arrays are free
        for (uint32_t j = 0; j < m; j++) s.verdict[list[j]] = verdicts[j] == NO_VERDICT ? (uint8_t)CSTARK_SIG_MISMATCH : verdicts[j];
        if (messages_out) sent.insert(sent.end(), list.begin(), list.end());
        rep.n_sig_checked += m;
        rep.n_chunks++;
    }
    select_finish(s, flags & CSTARK_SELECT_POW2);
    rep.n_candidates = n;
    rep.n_selected = s.n_selected;
    for (uint32_t t = 0; t < n; t++) rep.counts[s.status[t]]++;
    if ((flags & CSTARK_SELECT_APPLY) && s.n_selected) {
        std::vector<uint64_t> bs, br, bd, brx((size_t)6 * s.n_selected);
        std::vector<uint8_t> bss((size_t)32 * s.n_selected);
        select_batch(s, s_indices, r_indices, deltas, bs, br, bd);
        for (uint32_t i = 0; i < s.n_selected; i++) {
            memcpy(&brx[(size_t)6 * i], sig_rx + (size_t)6 * s.selected[i], 48);
            memcpy(&bss[(size_t)32 * i], sig_s + (size_t)32 * s.selected[i], 32);
        }
        int32_t at = -1, why = REASON_NONE;
        RC_TRY(apply_impl(L, s.n_selected, bs.data(), br.data(), bd.data(), brx.data(), bss.data(), out, &at, &why, false, rep.root_after));
        if (at >= 0) {
            char text[96];
            snprintf(text, sizeof text, "selected candidate %u (reason %d)", s.selected[at], why);
            return fail(CSTARK_ERR_UNSUPPORTED, "cstark_ledger_select: the plan refuses %s", text);
        }
    }
    memcpy(status_out, s.status.data(), n);
    if (selected_out && s.n_selected) memcpy(selected_out, s.selected.data(), (size_t)4 * s.n_selected);
    if (messages_out) {
        memset(messages_out, 0, (size_t)224 * n);
        for (size_t j = 0; j < sent.size(); j++) memcpy(messages_out + (size_t)28 * sent[j], &sent_messages[(size_t)28 * j], 224);
    }
    *report = rep;
    return CSTARK_OK;
}

// a HIP failure inside a ledger call leaves the pool in an unknown state: every later call fails
int guard(cstark_ledger *L, int rc) {
    if (rc == CSTARK_ERR_HIP || rc == CSTARK_ERR_OOM) L->broken = true;
    return rc;
}
int usable(cstark_ctx *c, cstark_ledger *L, const char *who) {
    if (!c || !L) return fail(CSTARK_ERR_INVALID_ARG, "%s: null argument", who);
    if (L->ctx != c) return fail(CSTARK_ERR_INVALID_ARG, "%s: the ledger belongs to another context", who);
    if (L->broken) return fail(CSTARK_ERR_HIP, "%s: an earlier HIP failure left this ledger unusable", who);
    return CSTARK_OK;
}

// a partial ledger refuses every index it does not know (a full one knows every leaf): the first such position is named, nothing is done
int all_known(cstark_ledger *L, const char *who, uint32_t count, const uint64_t *indices) {
    if (!L->index.partial) return CSTARK_OK;
    for (uint32_t i = 0; i < count; i++)
        if (!L->index.is_known(indices[i])) {
            char where[96];
            snprintf(where, sizeof where, "%s: indices[%u]", who, i);
            return fail(CSTARK_ERR_INVALID_ARG, "%s is not among the accounts this partial ledger knows", where);
        }
    return CSTARK_OK;
}

static_assert(MAX_CHECKPOINTS == CSTARK_LEDGER_MAX_CHECKPOINTS, "the documented cap is the plan's");
// the position of checkpoint `id` (0: the current state) for the calls that take one; -1 with the error set
ptrdiff_t checkpoint_position(cstark_ledger *L, uint64_t id, const char *who) {
    const ptrdiff_t at = L->index.position(id);
    if (at < 0) fail(CSTARK_ERR_INVALID_ARG, "%s: no live checkpoint of this ledger has that id (never taken, released, or dropped by a revert)", who);
    return at;
}

} // namespace

void witness_check_release(const cstark_ctx *c) {
    std::lock_guard<std::mutex> hold(g_wcheck_lock);
    const auto it = g_wcheck_blocks.find(c);
    if (it == g_wcheck_blocks.end()) return;
    (void)hipFree(it->second.buf);
    g_wcheck_blocks.erase(it);
}

// internal, for the test-only library (include/cstark_debug_ledger.h): XORs `mask` into word `word` of the digest that the lookup at
// checkpoint `id` finds for node (level, index), or, with level == 0xFFFFFFFF, of empty-subtree slot `index`.  One word down, one word
// up, no launch.  1: refused (an unknown id, a node the state does not store, a word or slot out of range), nothing written.
int ledger_xor_word(cstark_ledger *L, uint64_t id, uint32_t level, uint64_t index, uint32_t word, uint64_t mask) {
    if (!L || L->broken || word >= 7) return 1;
    const Index &ix = L->index;
    const ptrdiff_t at = ix.position(id);
    if (at < 0) return 1;
    uint32_t slot;
    if (level == 0xFFFFFFFFu) {
        if (index > ix.depth) return 1;
        slot = (uint32_t)index;
    } else {
        if (level > ix.depth || (index >> level)) return 1;
        slot = ix.slot_at((size_t)at, level, index);
        if (slot < EMPTY_SLOTS) return 1; // the state stores no such node: it reads an empty-subtree slot
    }
    if (slot >= L->pool_slots) return 1;
    cstark_ctx *c = L->ctx;
    if (hipSetDevice(c->device) != hipSuccess) return (int)hipErrorInvalidDevice;
    uint64_t *at_word = L->pool + (size_t)7 * slot + word, w = 0;
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(&w, at_word, 8, hipMemcpyDeviceToHost);
    w ^= mask;
    if (e == hipSuccess) e = hipMemcpy(at_word, &w, 8, hipMemcpyHostToDevice);
    return (int)e;
}

extern "C" {

int cstark_ledger_create(cstark_ctx *c, uint32_t merkle_depth, cstark_ledger **out) {
    if (!c || !out) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_create: null argument");
    *out = nullptr;
    const uint32_t d = merkle_depth;
    if (d == 0 || ((d + 1) & d) != 0 || d > MAX_DEPTH) return fail(CSTARK_ERR_INVALID_ARG, "tree depth must be one less than a power of 2 and at most 31");
    cstark_ledger *L = new (std::nothrow) cstark_ledger(c, d);
    if (!L) return fail(CSTARK_ERR_OOM, "cstark_ledger_create: out of host memory");
    const int rc = create_impl(L);
    if (rc) { cstark_ledger_destroy(L); return rc; }
    *out = L;
    return CSTARK_OK;
}

int cstark_ledger_create_partial(cstark_ctx *c, uint32_t merkle_depth, uint32_t count, const uint64_t *indices, const uint64_t *values, const uint8_t *present,
                                 const uint64_t *nodes, uint32_t n_nodes, const uint64_t root[7], cstark_ledger **out, uint32_t *verdict, uint32_t *at) {
    const char *who = "cstark_ledger_create_partial";
    if (!c || !indices || !values || !root || !out || !verdict || !at) return fail(CSTARK_ERR_INVALID_ARG, "%s: null argument", who);
    const uint32_t d = merkle_depth;
    if (d == 0 || ((d + 1) & d) != 0 || d > MAX_DEPTH) return fail(CSTARK_ERR_INVALID_ARG, "%s: tree depth must be one less than a power of 2 and at most 31", who);
    if (count == 0 || count > cs::multi::MAX_COUNT) return fail(CSTARK_ERR_INVALID_ARG, "%s: count must be 1 .. 2^20", who);
    if (!nodes != !n_nodes) return fail(CSTARK_ERR_INVALID_ARG, "%s: nodes is null iff n_nodes is 0", who);
    if (n_nodes > cs::multi::MAX_COUNT * MAX_DEPTH) return fail(CSTARK_ERR_INVALID_ARG, "%s: n_nodes is beyond any multiproof", who);
    if (!reduced_words(who, "values", values, count, 14, false)) return CSTARK_ERR_INVALID_ARG;
    if (nodes && !reduced_words(who, "nodes", nodes, n_nodes, 7, false)) return CSTARK_ERR_INVALID_ARG;
    if (!reduced_words(who, "root", root, 1, 7, false)) return CSTARK_ERR_INVALID_ARG;
    // the shape of an untrusted opening is data: these two are verdicts, and nothing is launched for them
    const cs::multi::Shape s = cs::multi::multiproof_shape(d, count, indices);
    if (!s.ok || n_nodes != s.n_nodes) {
        *out = nullptr;
        *verdict = s.ok ? CSTARK_MULTI_NODE_COUNT : CSTARK_MULTI_INDEX;
        *at = s.ok ? s.n_nodes : s.bad_at;
        return CSTARK_OK;
    }
    cs::multi::SeedPlan sp;
    if (!cs::multi::plan_seed(d, count, indices, values, present, nodes, sp)) return fail(CSTARK_ERR_UNSUPPORTED, "%s: the opening is too large to plan", who);
    cstark_ledger *L = new (std::nothrow) cstark_ledger(c, d);
    if (!L) return fail(CSTARK_ERR_OOM, "%s: out of host memory", who);
    bool matches = false;
    const int rc = create_partial_impl(L, sp, root, &matches);
    if (rc || !matches) cstark_ledger_destroy(L); // nothing stays allocated; the index was never committed
    if (rc) return rc;
    if (matches) cs::multi::commit_seed(L->index, sp, count, indices);
    *out = matches ? L : nullptr;
    *verdict = matches ? CSTARK_MULTI_VALID : CSTARK_MULTI_ROOT;
    *at = 0;
    return CSTARK_OK;
}

int cstark_ledger_known(cstark_ctx *c, cstark_ledger *L, uint32_t count, const uint64_t *indices, uint8_t *known_out) {
    RC_TRY(usable(c, L, "cstark_ledger_known"));
    if (count && (!indices || !known_out)) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_known: null argument");
    for (uint32_t i = 0; i < count; i++) known_out[i] = L->index.is_known(indices[i]);
    return CSTARK_OK;
}

int cstark_ledger_partial_info(cstark_ctx *c, cstark_ledger *L, uint32_t *is_partial, uint64_t *n_known, uint64_t *n_opaque) {
    RC_TRY(usable(c, L, "cstark_ledger_partial_info"));
    if (!is_partial || !n_known || !n_opaque) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_partial_info: null argument");
    *is_partial = L->index.partial;
    *n_known = L->index.partial ? L->index.known.size() : L->index.accounts.size();
    *n_opaque = L->index.n_opaque;
    return CSTARK_OK;
}

void cstark_ledger_destroy(cstark_ledger *L) {
    if (!L) return;
    (void)hipSetDevice(L->ctx->device);
    (void)hipStreamSynchronize(L->ctx->stream);
    if (L->pool) (void)hipFree(L->pool);
    if (L->audit_words) (void)hipFree(L->audit_words);
    delete L;
}

int cstark_ledger_set_accounts(cstark_ctx *c, cstark_ledger *L, uint32_t count, const uint64_t *indices, const uint64_t *values) {
    RC_TRY(usable(c, L, "cstark_ledger_set_accounts"));
    if (count == 0 || count > MAX_TRANSFERS || !indices || !values) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_set_accounts: bad argument");
    RC_TRY(all_known(L, "cstark_ledger_set_accounts", count, indices));
    return guard(L, set_accounts_impl(L, count, indices, values));
}

int cstark_ledger_get_accounts(cstark_ctx *c, cstark_ledger *L, uint32_t count, const uint64_t *indices, uint64_t *values_out, uint8_t *present_out) {
    RC_TRY(usable(c, L, "cstark_ledger_get_accounts"));
    if (count && (!indices || !values_out || !present_out)) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_get_accounts: null argument");
    RC_TRY(all_known(L, "cstark_ledger_get_accounts", count, indices));
    for (uint32_t i = 0; i < count; i++) {
        const auto it = L->index.accounts.find(indices[i]);
        present_out[i] = it != L->index.accounts.end();
        if (present_out[i]) memcpy(values_out + (size_t)14 * i, it->second.data(), 112);
        else memset(values_out + (size_t)14 * i, 0, 112);
    }
    return CSTARK_OK;
}

int cstark_ledger_open_accounts(cstark_ctx *c, cstark_ledger *L, uint32_t count, const uint64_t *indices, uint64_t *values_out, uint8_t *present_out,
                                uint64_t *paths_out, uint64_t root_out[7]) {
    RC_TRY(usable(c, L, "cstark_ledger_open_accounts"));
    if (count == 0 || count > MAX_TRANSFERS || !indices || !values_out || !present_out || !paths_out || !root_out)
        return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_open_accounts: bad argument");
    for (uint32_t i = 0; i < count; i++)
        if (indices[i] >> L->index.depth) {
            char where[32];
            snprintf(where, sizeof where, "indices[%u]", i);
            return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_open_accounts: %s is out of range", where);
        }
    RC_TRY(all_known(L, "cstark_ledger_open_accounts", count, indices));
    return guard(L, open_impl(L, count, indices, values_out, present_out, paths_out, root_out));
}

int cstark_ledger_checkpoint(cstark_ctx *c, cstark_ledger *L, uint64_t *id_out) {
    RC_TRY(usable(c, L, "cstark_ledger_checkpoint"));
    if (!id_out) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_checkpoint: null argument");
    const uint64_t id = checkpoint(L->index);
    if (!id) return fail(CSTARK_ERR_UNSUPPORTED, "cstark_ledger_checkpoint: 16 checkpoints are live already (release one)");
    *id_out = id;
    return CSTARK_OK;
}

int cstark_ledger_revert(cstark_ctx *c, cstark_ledger *L, uint64_t id) {
    RC_TRY(usable(c, L, "cstark_ledger_revert"));
    if (id == 0) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_revert: id 0 is the current state");
    const ptrdiff_t at = checkpoint_position(L, id, "cstark_ledger_revert");
    if (at < 0) return CSTARK_ERR_INVALID_ARG;
    revert(L->index, (size_t)at);
    return CSTARK_OK;
}

int cstark_ledger_release(cstark_ctx *c, cstark_ledger *L, uint64_t id) {
    RC_TRY(usable(c, L, "cstark_ledger_release"));
    if (id == 0) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_release: id 0 is the current state");
    const ptrdiff_t at = checkpoint_position(L, id, "cstark_ledger_release");
    if (at < 0) return CSTARK_ERR_INVALID_ARG;
    release(L->index, (size_t)at);
    return CSTARK_OK;
}

int cstark_ledger_root_at(cstark_ctx *c, cstark_ledger *L, uint64_t id, uint64_t root[7]) {
    RC_TRY(usable(c, L, "cstark_ledger_root_at"));
    if (!root) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_root_at: null argument");
    const ptrdiff_t at = checkpoint_position(L, id, "cstark_ledger_root_at");
    if (at < 0) return CSTARK_ERR_INVALID_ARG;
    return guard(L, root_impl(L, root, (size_t)at));
}

int cstark_ledger_open_accounts_at(cstark_ctx *c, cstark_ledger *L, uint64_t id, uint32_t count, const uint64_t *indices, uint64_t *values_out,
                                   uint8_t *present_out, uint64_t *paths_out, uint64_t root_out[7]) {
    RC_TRY(usable(c, L, "cstark_ledger_open_accounts_at"));
    if (count == 0 || count > MAX_TRANSFERS || !indices || !values_out || !present_out || !paths_out || !root_out)
        return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_open_accounts_at: bad argument");
    const ptrdiff_t at = checkpoint_position(L, id, "cstark_ledger_open_accounts_at");
    if (at < 0) return CSTARK_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < count; i++)
        if (indices[i] >> L->index.depth) {
            char where[32];
            snprintf(where, sizeof where, "indices[%u]", i);
            return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_open_accounts_at: %s is out of range", where);
        }
    RC_TRY(all_known(L, "cstark_ledger_open_accounts_at", count, indices));
    return guard(L, open_impl(L, count, indices, values_out, present_out, paths_out, root_out, (size_t)at));
}

int cstark_ledger_audit(cstark_ctx *c, cstark_ledger *L, uint64_t id, cstark_ledger_audit_report *report) {
    RC_TRY(usable(c, L, "cstark_ledger_audit"));
    if (!report) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_audit: null argument");
    const ptrdiff_t at = checkpoint_position(L, id, "cstark_ledger_audit");
    if (at < 0) return CSTARK_ERR_INVALID_ARG;
    return guard(L, audit_impl(L, (size_t)at, report));
}

int cstark_account_check_paths(cstark_ctx *c, uint32_t count, uint32_t depth, const uint64_t *indices, const uint64_t *values, const uint8_t *present,
                               const uint64_t *paths, const uint64_t *roots, uint32_t n_roots, uint8_t *verdicts, uint64_t *roots_out) {
    const char *who = "cstark_account_check_paths";
    if (!c || !indices || !paths || !roots || !verdicts) return fail(CSTARK_ERR_INVALID_ARG, "%s: null argument", who);
    if (count == 0 || count > MAX_TRANSFERS) return fail(CSTARK_ERR_INVALID_ARG, "%s: count must be 1 .. 2^20", who);
    if (depth == 0 || depth > MAX_DEPTH) return fail(CSTARK_ERR_INVALID_ARG, "%s: depth must be 1 .. 31", who);
    if (n_roots != 1 && n_roots != count) return fail(CSTARK_ERR_INVALID_ARG, "%s: n_roots must be 1 or count", who);
    if (present && !values) return fail(CSTARK_ERR_INVALID_ARG, "%s: present without values", who);
    if (values && !reduced_words(who, "values", values, count, 14, false)) return CSTARK_ERR_INVALID_ARG;
    if (!reduced_words(who, "paths", paths, count, (size_t)7 * (depth + 1), true)) return CSTARK_ERR_INVALID_ARG;
    if (!reduced_words(who, "roots", roots, n_roots, 7, false)) return CSTARK_ERR_INVALID_ARG;
    return check_paths_impl(c, count, depth, indices, values, present, paths, roots, n_roots, verdicts, roots_out);
}

int cstark_tx_witness_check(cstark_ctx *c, const cstark_tx_witness *w, const uint64_t *final_root, uint32_t flags, cstark_witness_report *report,
                            uint8_t *verdicts_out, uint64_t *folds_out) {
    const char *who = "cstark_tx_witness_check";
    if (!c || !report) return fail(CSTARK_ERR_INVALID_ARG, "%s: null argument", who);
    if (flags & ~CSTARK_WITNESS_CHECK_SIGNATURES) return fail(CSTARK_ERR_INVALID_ARG, "%s: unknown flag", who);
    const bool signatures = flags & CSTARK_WITNESS_CHECK_SIGNATURES;
    if (!w) {
        if (!c->wit_buf || c->wit.n_tx == 0 || c->wit.msg_tail) return fail(CSTARK_ERR_INVALID_ARG, "%s: no transaction witness uploaded", who);
        if (c->wit.n_tx > MAX_TRANSFERS) return fail(CSTARK_ERR_INVALID_ARG, "%s: the resident witness has more than 2^20 transfers", who);
        if (final_root && !reduced_words(who, "final_root", final_root, 1, 7, false)) return CSTARK_ERR_INVALID_ARG;
        return witness_check_impl(c, nullptr, c->wit, final_root, signatures, report, verdicts_out, folds_out);
    }
    if (final_root) return fail(CSTARK_ERR_INVALID_ARG, "%s: final_root is for the resident form; a host witness states its own", who);
    const size_t n = w->n_tx, d = w->merkle_depth;
    if (n == 0 || n > MAX_TRANSFERS) return fail(CSTARK_ERR_INVALID_ARG, "%s: n_tx must be 1 .. 2^20", who);
    if (d == 0 || ((d + 1) & d) != 0 || d > MAX_DEPTH) return fail(CSTARK_ERR_INVALID_ARG, "%s: tree depth must be one less than a power of 2 and at most 31", who);
    if (!w->initial_roots || !w->final_root || !w->s_old_values || !w->r_old_values || !w->s_indices || !w->r_indices || !w->s_paths || !w->r_paths ||
        !w->deltas || !w->sig_rx || !w->sig_s)
        return fail(CSTARK_ERR_INVALID_ARG, "%s: witness array pointer is null", who);
    if (!reduced_words(who, "initial_roots", w->initial_roots, n, 7, false) || !reduced_words(who, "final_root", w->final_root, 1, 7, false) ||
        !reduced_words(who, "s_old_values", w->s_old_values, n, 14, false) || !reduced_words(who, "r_old_values", w->r_old_values, n, 14, false) ||
        !reduced_words(who, "s_paths", w->s_paths, n, 7 * (d + 1), true) || !reduced_words(who, "r_paths", w->r_paths, n, 7 * (d + 1), true) ||
        !reduced_words(who, "deltas", w->deltas, n, 1, false) || !reduced_words(who, "sig_rx", w->sig_rx, n, 6, false))
        return CSTARK_ERR_INVALID_ARG;
    cs::TxWitnessDev view{};
    view.n_tx = (uint32_t)n; view.depth = (uint32_t)d;
    return witness_check_impl(c, w, view, w->final_root, signatures, report, verdicts_out, folds_out);
}

int cstark_account_multiproof_shape(uint32_t depth, uint32_t count, const uint64_t *indices, uint32_t *n_nodes, uint32_t *n_merges) {
    const char *who = "cstark_account_multiproof_shape";
    if (!indices || !n_nodes || !n_merges) return fail(CSTARK_ERR_INVALID_ARG, "%s: null argument", who);
    if (depth == 0 || depth > MAX_DEPTH) return fail(CSTARK_ERR_INVALID_ARG, "%s: depth must be 1 .. 31", who);
    if (count == 0 || count > cs::multi::MAX_COUNT) return fail(CSTARK_ERR_INVALID_ARG, "%s: count must be 1 .. 2^20", who);
    const cs::multi::Shape s = cs::multi::multiproof_shape(depth, count, indices);
    if (!s.ok) return unsorted(who, s.bad_at);
    *n_nodes = s.n_nodes;
    *n_merges = s.n_merges;
    return CSTARK_OK;
}

int cstark_ledger_open_multi(cstark_ctx *c, cstark_ledger *L, uint64_t id, uint32_t count, const uint64_t *indices, uint64_t *values_out, uint8_t *present_out,
                             uint64_t *nodes_out, uint32_t nodes_capacity, uint32_t *n_nodes, uint64_t root_out[7]) {
    const char *who = "cstark_ledger_open_multi";
    RC_TRY(usable(c, L, who));
    if (count == 0 || count > cs::multi::MAX_COUNT || !indices || !values_out || !present_out || (!nodes_out && nodes_capacity) || !n_nodes || !root_out)
        return fail(CSTARK_ERR_INVALID_ARG, "%s: bad argument", who);
    const ptrdiff_t at = checkpoint_position(L, id, who);
    if (at < 0) return CSTARK_ERR_INVALID_ARG;
    const cs::multi::Shape s = cs::multi::multiproof_shape(L->index.depth, count, indices);
    if (!s.ok) return unsorted(who, s.bad_at);
    RC_TRY(all_known(L, who, count, indices)); // an opening through an opaque node would read empty digests beneath it
    if (nodes_capacity < s.n_nodes) {
        *n_nodes = s.n_nodes;
        char need[96];
        snprintf(need, sizeof need, "%s: nodes_capacity %u is below the %u proof nodes of this opening", who, nodes_capacity, s.n_nodes);
        return fail(CSTARK_ERR_INVALID_ARG, "%s", need);
    }
    RC_TRY(guard(L, open_multi_impl(L, (size_t)at, count, indices, s.n_nodes, values_out, present_out, nodes_out, root_out)));
    *n_nodes = s.n_nodes;
    return CSTARK_OK;
}

int cstark_account_check_multiproof(cstark_ctx *c, uint32_t depth, uint32_t count, const uint64_t *indices, const uint64_t *values, const uint8_t *present,
                                    const uint64_t *leaves, const uint64_t *nodes, uint32_t n_nodes, const uint64_t root[7], uint32_t *verdict, uint32_t *at,
                                    uint64_t *root_out, uint32_t *n_merges) {
    const char *who = "cstark_account_check_multiproof";
    if (!c || !indices || !root || !verdict || !at) return fail(CSTARK_ERR_INVALID_ARG, "%s: null argument", who);
    if (depth == 0 || depth > MAX_DEPTH) return fail(CSTARK_ERR_INVALID_ARG, "%s: depth must be 1 .. 31", who);
    if (count == 0 || count > cs::multi::MAX_COUNT) return fail(CSTARK_ERR_INVALID_ARG, "%s: count must be 1 .. 2^20", who);
    if (!values == !leaves) return fail(CSTARK_ERR_INVALID_ARG, "%s: exactly one of values and leaves is given", who);
    if (present && !values) return fail(CSTARK_ERR_INVALID_ARG, "%s: present without values", who);
    if (!nodes != !n_nodes) return fail(CSTARK_ERR_INVALID_ARG, "%s: nodes is null iff n_nodes is 0", who);
    if (n_nodes > cs::multi::MAX_COUNT * MAX_DEPTH) return fail(CSTARK_ERR_INVALID_ARG, "%s: n_nodes is beyond any multiproof", who);
    if (values && !reduced_words(who, "values", values, count, 14, false)) return CSTARK_ERR_INVALID_ARG;
    if (leaves && !reduced_words(who, "leaves", leaves, count, 7, false)) return CSTARK_ERR_INVALID_ARG;
    if (nodes && !reduced_words(who, "nodes", nodes, n_nodes, 7, false)) return CSTARK_ERR_INVALID_ARG;
    if (!reduced_words(who, "root", root, 1, 7, false)) return CSTARK_ERR_INVALID_ARG;
    // the shape of an untrusted proof is data: these two are verdicts, and nothing is launched for them
    cs::multi::CheckPlan p;
    if (!cs::multi::plan_check(depth, count, indices, p)) {
        *verdict = CSTARK_MULTI_INDEX;
        *at = p.shape.bad_at;
        return CSTARK_OK;
    }
    if (n_merges) *n_merges = p.shape.n_merges;
    if (n_nodes != p.shape.n_nodes) {
        *verdict = CSTARK_MULTI_NODE_COUNT;
        *at = p.shape.n_nodes;
        return CSTARK_OK;
    }
    uint32_t v = 0;
    RC_TRY(check_multi_impl(c, depth, count, values, present, leaves, nodes, root, p, &v, root_out));
    *verdict = v;
    *at = 0;
    return CSTARK_OK;
}

int cstark_account_check_update(cstark_ctx *c, uint32_t depth, uint32_t count, const uint64_t *indices, const uint64_t *old_values, const uint8_t *old_present,
                                const uint64_t *new_values, const uint8_t *new_present, const uint64_t *nodes, uint32_t n_nodes, const uint64_t old_root[7],
                                const uint64_t *new_root, uint32_t *verdict, uint32_t *at, uint64_t *new_root_out, uint32_t *n_changed) {
    const char *who = "cstark_account_check_update";
    if (!c || !indices || !old_values || !new_values || !old_root || !verdict || !at) return fail(CSTARK_ERR_INVALID_ARG, "%s: null argument", who);
    if (depth == 0 || depth > MAX_DEPTH) return fail(CSTARK_ERR_INVALID_ARG, "%s: depth must be 1 .. 31", who);
    if (count == 0 || count > cs::multi::MAX_COUNT) return fail(CSTARK_ERR_INVALID_ARG, "%s: count must be 1 .. 2^20", who);
    if (!nodes != !n_nodes) return fail(CSTARK_ERR_INVALID_ARG, "%s: nodes is null iff n_nodes is 0", who);
    if (n_nodes > cs::multi::MAX_COUNT * MAX_DEPTH) return fail(CSTARK_ERR_INVALID_ARG, "%s: n_nodes is beyond any multiproof", who);
    if (!reduced_words(who, "old_values", old_values, count, 14, false)) return CSTARK_ERR_INVALID_ARG;
    if (!reduced_words(who, "new_values", new_values, count, 14, false)) return CSTARK_ERR_INVALID_ARG;
    if (nodes && !reduced_words(who, "nodes", nodes, n_nodes, 7, false)) return CSTARK_ERR_INVALID_ARG;
    if (!reduced_words(who, "old_root", old_root, 1, 7, false)) return CSTARK_ERR_INVALID_ARG;
    if (new_root && !reduced_words(who, "new_root", new_root, 1, 7, false)) return CSTARK_ERR_INVALID_ARG;
    // the shape of an untrusted opening is data: these two are verdicts, and nothing is launched for them
    const cs::multi::Shape s = cs::multi::multiproof_shape(depth, count, indices);
    if (!s.ok) {
        *verdict = CSTARK_UPDATE_INDEX;
        *at = s.bad_at;
        return CSTARK_OK;
    }
    if (n_nodes != s.n_nodes) {
        *verdict = CSTARK_UPDATE_NODE_COUNT;
        *at = s.n_nodes;
        return CSTARK_OK;
    }
    std::vector<uint8_t> state;
    const uint32_t changed = cs::multi::update_states(count, old_values, old_present, new_values, new_present, state);
    cs::multi::CheckPlan p;
    if (!cs::multi::plan_update(depth, count, indices, state.data(), p)) return fail(CSTARK_ERR_INVALID_ARG, "%s: the indices lost their shape", who);
    uint32_t v = 0;
    uint64_t fold[7];
    RC_TRY(check_update_impl(c, depth, count, old_values, new_values, nodes, old_root, new_root, p, state, &v, fold));
    *verdict = v;
    *at = 0;
    if (new_root_out && v != CSTARK_UPDATE_OLD_ROOT) memcpy(new_root_out, fold, 56);
    if (n_changed) *n_changed = changed;
    return CSTARK_OK;
}

int cstark_ledger_root(cstark_ctx *c, cstark_ledger *L, uint64_t root[7]) {
    RC_TRY(usable(c, L, "cstark_ledger_root"));
    if (!root) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_root: null argument");
    return guard(L, root_impl(L, root));
}

// cstark_ledger_apply and cstark_ledger_apply_checked: one argument contract
static int apply_entry(cstark_ctx *c, cstark_ledger *L, uint32_t n_tx, const uint64_t *s_indices, const uint64_t *r_indices, const uint64_t *deltas,
                       const uint64_t *sig_rx, const uint8_t *sig_s, cstark_tx_witness *out, int32_t *refused_at, int32_t *reason, bool check_signatures) {
    RC_TRY(usable(c, L, "cstark_ledger_apply"));
    if (n_tx == 0 || n_tx > MAX_TRANSFERS || !s_indices || !r_indices || !deltas || !sig_rx || !sig_s || !refused_at || !reason)
        return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_apply: bad argument");
    if (out) {
        if (out->n_tx != n_tx || out->merkle_depth != L->index.depth) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_apply: the output witness has another shape");
        if (!out->initial_roots || !out->final_root || !out->s_old_values || !out->r_old_values || !out->s_indices || !out->r_indices || !out->s_paths ||
            !out->r_paths || !out->deltas || !out->sig_rx || !out->sig_s)
            return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_apply: output witness array pointer is null (the caller allocates every array)");
    }
    for (uint32_t t = 0; t < n_tx; t++)
        if (deltas[t] >= cs::host::P) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_apply: a delta is not a reduced field element");
    return guard(L, apply_impl(L, n_tx, s_indices, r_indices, deltas, sig_rx, sig_s, out, refused_at, reason, check_signatures));
}

int cstark_ledger_apply(cstark_ctx *c, cstark_ledger *L, uint32_t n_tx, const uint64_t *s_indices, const uint64_t *r_indices, const uint64_t *deltas,
                        const uint64_t *sig_rx, const uint8_t *sig_s, cstark_tx_witness *out, int32_t *refused_at, int32_t *reason) {
    return apply_entry(c, L, n_tx, s_indices, r_indices, deltas, sig_rx, sig_s, out, refused_at, reason, false);
}

int cstark_ledger_apply_checked(cstark_ctx *c, cstark_ledger *L, uint32_t n_tx, const uint64_t *s_indices, const uint64_t *r_indices, const uint64_t *deltas,
                                const uint64_t *sig_rx, const uint8_t *sig_s, cstark_tx_witness *out, int32_t *refused_at, int32_t *reason) {
    return apply_entry(c, L, n_tx, s_indices, r_indices, deltas, sig_rx, sig_s, out, refused_at, reason, true);
}

// cstark_ledger_messages and cstark_ledger_sign: the walk of plan_apply on the index as it stands, for its messages and its refusal.  The
// plan itself is dropped: nothing is reserved, launched or committed.
static int messages_entry(cstark_ledger *L, const char *who, uint32_t n_tx, const uint64_t *s_indices, const uint64_t *r_indices, const uint64_t *deltas,
                          std::vector<uint64_t> &messages, int32_t *refused_at, int32_t *reason) {
    for (uint32_t t = 0; t < n_tx; t++)
        if (deltas[t] >= cs::host::P) return fail(CSTARK_ERR_INVALID_ARG, "%s: a delta is not a reduced field element", who);
    uint64_t cap = L->capacity ? L->capacity : 1024;
    while (cap < (uint64_t)L->index.n_stored + max_new_nodes(L->index.depth, 2 * (uint64_t)n_tx)) cap *= 2;
    if (EMPTY_SLOTS + cap > MAX_POOL_SLOTS) return fail(CSTARK_ERR_UNSUPPORTED, "ledger: the batch needs more than 2^28 digest slots");
    Plan p;
    if (!plan_apply(L->index, (uint32_t)(EMPTY_SLOTS + cap), n_tx, s_indices, r_indices, deltas, p, &messages))
        return fail(CSTARK_ERR_UNSUPPORTED, "%s: the batch is too large to plan", who);
    *refused_at = p.refused_at;
    *reason = p.reason;
    return CSTARK_OK;
}

int cstark_ledger_messages(cstark_ctx *c, cstark_ledger *L, uint32_t n_tx, const uint64_t *s_indices, const uint64_t *r_indices, const uint64_t *deltas,
                           uint64_t *messages_out, int32_t *refused_at, int32_t *reason) {
    RC_TRY(usable(c, L, "cstark_ledger_messages"));
    if (n_tx == 0 || n_tx > MAX_TRANSFERS || !s_indices || !r_indices || !deltas || !messages_out || !refused_at || !reason)
        return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_messages: bad argument");
    std::vector<uint64_t> messages;
    int32_t at, why;
    RC_TRY(messages_entry(L, "cstark_ledger_messages", n_tx, s_indices, r_indices, deltas, messages, &at, &why));
    *refused_at = at;
    *reason = why;
    if (at < 0) memcpy(messages_out, messages.data(), messages.size() * 8);
    return CSTARK_OK;
}

int cstark_ledger_sign(cstark_ctx *c, cstark_ledger *L, uint32_t n_tx, const uint64_t *s_indices, const uint64_t *r_indices, const uint64_t *deltas,
                       const uint64_t *secrets, uint64_t seed, uint32_t max_attempts, uint64_t *sig_rx_out, uint8_t *sig_s_out, uint32_t *attempts_out,
                       int32_t *refused_at, int32_t *reason) {
    RC_TRY(usable(c, L, "cstark_ledger_sign"));
    if (n_tx == 0 || n_tx > MAX_TRANSFERS || !s_indices || !r_indices || !deltas || !secrets || !sig_rx_out || !sig_s_out || !refused_at || !reason)
        return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_sign: bad argument");
    char text[96];
    for (uint32_t t = 0; t < n_tx; t++)
        if (secrets[t] == 0 || secrets[t] > CSTARK_SIG_MAX_SECRET) {
            snprintf(text, sizeof text, "cstark_ledger_sign: secrets[%u] is not in 1 .. %u", t, CSTARK_SIG_MAX_SECRET);
            return fail(CSTARK_ERR_INVALID_ARG, "%s", text);
        }
    if (max_attempts == 0 || max_attempts > 4096) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_sign: max_attempts must be 1 .. 4096");
    std::vector<uint64_t> messages;
    int32_t at, why;
    RC_TRY(messages_entry(L, "cstark_ledger_sign", n_tx, s_indices, r_indices, deltas, messages, &at, &why));
    // the secrets of the transfers the plan accepted against the senders' keys, all of them or those before its refusal
    const uint32_t n_msg = (uint32_t)(messages.size() / 28);
    if (n_msg) {
        std::vector<uint64_t> keys((size_t)12 * n_msg);
        RC_TRY(sign_public_keys(c, n_msg, secrets, keys.data()));
        for (uint32_t t = 0; t < n_msg; t++)
            if (memcmp(&keys[(size_t)12 * t], &messages[(size_t)28 * t], 96) != 0) {
                *refused_at = (int32_t)t;
                *reason = REASON_KEY;
                return CSTARK_OK;
            }
    }
    *refused_at = at;
    *reason = why;
    if (at >= 0) return CSTARK_OK;
    std::vector<uint64_t> rx((size_t)6 * n_tx);
    std::vector<uint8_t> s((size_t)32 * n_tx), status(n_tx);
    std::vector<uint32_t> attempts(n_tx);
    RC_TRY(sign_seeded(c, n_tx, messages.data(), secrets, seed, max_attempts, rx.data(), s.data(), attempts.data(), status.data()));
    for (uint32_t t = 0; t < n_tx; t++)
        if (status[t] != CSTARK_SIGN_OK) {
            snprintf(text, sizeof text, "cstark_ledger_sign: transfer %u has no accepted attempt among %u", t, max_attempts);
            return fail(CSTARK_ERR_UNSUPPORTED, "%s", text);
        }
    memcpy(sig_rx_out, rx.data(), rx.size() * 8);
    memcpy(sig_s_out, s.data(), s.size());
    if (attempts_out) memcpy(attempts_out, attempts.data(), attempts.size() * 4);
    return CSTARK_OK;
}

static_assert(CSTARK_LEDGER_HELD == STATUS_HELD && CSTARK_LEDGER_NOT_REACHED == STATUS_NOT_REACHED, "select_walk writes the values of cstark_ledger_reason");
int cstark_ledger_select(cstark_ctx *c, cstark_ledger *L, uint32_t n, const uint64_t *s_indices, const uint64_t *r_indices, const uint64_t *deltas,
                         const uint64_t *sig_rx, const uint8_t *sig_s, uint32_t want, uint32_t flags, uint32_t chunk, uint8_t *status_out,
                         uint32_t *selected_out, uint64_t *messages_out, cstark_ledger_selection *report, cstark_tx_witness *out) {
    RC_TRY(usable(c, L, "cstark_ledger_select"));
    const uint32_t all = CSTARK_SELECT_CHECK_SIGNATURES | CSTARK_SELECT_POW2 | CSTARK_SELECT_APPLY;
    if (n == 0 || n > MAX_TRANSFERS || want == 0 || want > MAX_TRANSFERS || chunk > MAX_TRANSFERS || (flags & ~all))
        return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_select: n and want are 1 .. 2^20, chunk is at most 2^20, flags are CSTARK_SELECT_*");
    if (!s_indices || !r_indices || !deltas || !status_out || !report) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_select: null argument");
    if ((flags & (CSTARK_SELECT_CHECK_SIGNATURES | CSTARK_SELECT_APPLY)) && (!sig_rx || !sig_s))
        return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_select: sig_rx and sig_s may be null only without CHECK_SIGNATURES and APPLY");
    if (out) {
        if (!(flags & CSTARK_SELECT_APPLY)) return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_select: an output witness needs CSTARK_SELECT_APPLY");
        if (out->n_tx < std::min(want, n) || out->merkle_depth != L->index.depth)
            return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_select: the output witness has another depth or holds fewer than min(want, n) transfers");
        if (!out->initial_roots || !out->final_root || !out->s_old_values || !out->r_old_values || !out->s_indices || !out->r_indices || !out->s_paths ||
            !out->r_paths || !out->deltas || !out->sig_rx || !out->sig_s)
            return fail(CSTARK_ERR_INVALID_ARG, "cstark_ledger_select: output witness array pointer is null (the caller allocates every array)");
    }
    for (uint32_t t = 0; t < n; t++)
        if (deltas[t] >= cs::host::P) {
            char where[64];
            snprintf(where, sizeof where, "cstark_ledger_select: deltas[%u]", t);
            return fail(CSTARK_ERR_INVALID_ARG, "%s is not a reduced field element", where);
        }
    return guard(L, select_impl(L, n, s_indices, r_indices, deltas, sig_rx, sig_s, want, flags, chunk, status_out, selected_out, messages_out, report, out));
}

} // extern "C"
