// cstark.hpp -- C++ host-side mirror of the reference's prover interface over the C ABI of cstark.h.
//
// The reference is a Rust crate; no Rust toolchain exists in the build environment, so the host layer a Rust maintainer would
// write is provided in C++ with the reference's names, argument meaning and error behaviour:
//   ProofOptions            winterfell::ProofOptions::new(...) as used at /root/reference/src/lib.rs:78-86
//   TransactionMetadata     src/lib.rs:183-232 (field for field), ::build_random src/lib.rs:235-465 (seeded)
//   TransactionProver       src/prover.rs:20-134: new(options), build_trace, get_pub_inputs, prove
//   TransactionExample      src/lib.rs:92-150: new(options, num_transactions), prove(), verify()
//   get_example             src/lib.rs:75-89
//   MerkleExample / SchnorrExample / RangeProofExample    the sub-AIR examples (src/merkle/update/mod.rs, src/schnorr/mod.rs,
//                                                         src/range/mod.rs)
// Failures are exceptions (cstark::Error) where the reference returns Err / panics.  Header-only; link libcstark_hip.so.
#ifndef CSTARK_HPP
#define CSTARK_HPP
#include <algorithm>
#include <array>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <future>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>
#include "cstark.h"

namespace cstark {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error("cstark error " + std::to_string(c) + ": " + m), code(c) {}
};
inline void check(int rc) {
    if (rc != CSTARK_OK) throw Error(rc, cstark_last_error());
}

using BaseElement = uint64_t; // memory form of f63::BaseElement (Montgomery, reduced)
using Hash = std::array<BaseElement, 7>;

enum class HashFunction : uint32_t { Blake3_256 = 0, Sha3_256 = 1 };
enum class FieldExtension : uint32_t { None = 0, Quadratic = 1, Cubic = 2 };

struct ProofOptions {
    uint32_t num_queries = 42, blowup_factor = 8, grinding_factor = 0;
    HashFunction hash_fn = HashFunction::Blake3_256;
    FieldExtension field_extension = FieldExtension::None;
    uint32_t fri_folding_factor = 4, fri_max_remainder = 256;
    ProofOptions() = default;
    ProofOptions(uint32_t q, uint32_t b, uint32_t g, HashFunction h, FieldExtension e, uint32_t f, uint32_t r)
        : num_queries(q), blowup_factor(b), grinding_factor(g), hash_fn(h), field_extension(e), fri_folding_factor(f), fri_max_remainder(r) {}
    cstark_options raw() const {
        return {num_queries, blowup_factor, grinding_factor, (uint32_t)hash_fn, (uint32_t)field_extension, fri_folding_factor, fri_max_remainder};
    }
};

struct PublicInputs { // src/air.rs:52-62
    Hash initial_root{}, final_root{};
};

// One GPU context (device, stream).  Not copyable; one per host thread.
class Context {
  public:
    explicit Context(int device = -1, void *stream = nullptr) { check(cstark_ctx_create(device, stream, &ctx_)); }
    struct OwnStream {}; // Context(OwnStream{}, device): a stream of the context's own (several contexts side by side: ProverPool)
    explicit Context(OwnStream, int device = -1) { check(cstark_ctx_create_own_stream(device, &ctx_)); }
    ~Context() { cstark_ctx_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    cstark_ctx *raw() const { return ctx_; }
    void synchronize() const { check(cstark_ctx_synchronize(ctx_)); }
    std::array<float, CSTARK_PROVE_NUM_STAGES> prove_stage_ms() const {
        std::array<float, CSTARK_PROVE_NUM_STAGES> ms{};
        check(cstark_prove_stage_ms(ctx_, ms.data()));
        return ms;
    }
    // CSTARK_CHANNEL_HOST / CSTARK_CHANNEL_DEVICE: the Fiat-Shamir channel of the last proof on this context
    uint32_t prove_channel() const {
        uint32_t channel = CSTARK_CHANNEL_HOST;
        check(cstark_prove_channel(ctx_, &channel));
        return channel;
    }
    // CSTARK_FORM_PLAIN (the default) / CSTARK_FORM_COMPACT: the form of the proofs every single-GPU prover of this context writes
    void set_proof_form(uint32_t form) { check(cstark_ctx_set_proof_form(ctx_, form)); }
    uint32_t proof_form() const {
        uint32_t form = CSTARK_FORM_PLAIN;
        check(cstark_ctx_proof_form(ctx_, &form));
        return form;
    }

  private:
    cstark_ctx *ctx_ = nullptr;
};

// CSTARK_FORM_PLAIN / CSTARK_FORM_COMPACT by the proof's magic (host only); throws when the bytes carry neither
inline uint32_t proof_form(const std::vector<uint8_t> &proof) {
    uint32_t form = CSTARK_FORM_PLAIN;
    check(cstark_proof_form(proof.data(), proof.size(), &form));
    return form;
}

// Series of transfers in the account tree (src/lib.rs:183-194).  Paths are [leaf, sibling_0 .. sibling_{depth-1}].
struct TransactionMetadata {
    unsigned merkle_depth = 15;
    std::vector<Hash> initial_roots;
    Hash final_root{};
    std::vector<std::array<BaseElement, 14>> s_old_values, r_old_values;
    std::vector<uint64_t> s_indices, r_indices;
    std::vector<BaseElement> s_paths, r_paths; // [n][depth + 1][7]
    std::vector<BaseElement> deltas;
    std::vector<std::array<BaseElement, 6>> sig_rx;
    std::vector<std::array<uint8_t, 32>> sig_s;

    size_t len() const { return initial_roots.size(); }
    // "Enforce that all vectors are of equal length" (src/lib.rs:211-218)
    void validate() const {
        const size_t n = len();
        if (n == 0 || s_old_values.size() != n || r_old_values.size() != n || s_indices.size() != n || r_indices.size() != n || deltas.size() != n ||
            sig_rx.size() != n || sig_s.size() != n || s_paths.size() != n * (merkle_depth + 1) * 7 || r_paths.size() != s_paths.size())
            throw Error(CSTARK_ERR_INVALID_ARG, "transaction metadata vectors are not of equal length");
        if ((merkle_depth + 1) & merkle_depth) throw Error(CSTARK_ERR_INVALID_ARG, "tree depth must be one less than a power of 2"); // src/lib.rs:102-105
    }
    cstark_tx_witness view() const {
        cstark_tx_witness w{};
        w.n_tx = (uint32_t)len(); w.merkle_depth = merkle_depth;
        w.initial_roots = initial_roots[0].data(); w.final_root = final_root.data();
        w.s_old_values = s_old_values[0].data(); w.r_old_values = r_old_values[0].data();
        w.s_indices = s_indices.data(); w.r_indices = r_indices.data();
        w.s_paths = s_paths.data(); w.r_paths = r_paths.data();
        w.deltas = deltas.data(); w.sig_rx = sig_rx[0].data(); w.sig_s = sig_s[0].data();
        return w;
    }
    // TransactionMetadata::build_random (src/lib.rs:235-465), deterministic in `seed`
    static TransactionMetadata build_random(size_t num_transactions, unsigned depth = 15, uint64_t seed = 0x5EED) {
        TransactionMetadata m;
        const size_t n = num_transactions;
        m.merkle_depth = depth;
        m.initial_roots.resize(n); m.s_old_values.resize(n); m.r_old_values.resize(n); m.s_indices.resize(n); m.r_indices.resize(n);
        m.s_paths.resize(n * (depth + 1) * 7); m.r_paths.resize(n * (depth + 1) * 7); m.deltas.resize(n); m.sig_rx.resize(n); m.sig_s.resize(n);
        if (n == 0) throw Error(CSTARK_ERR_INVALID_ARG, "no transactions");
        cstark_tx_witness w = m.view();
        check(cstark_tx_witness_generate(&w, seed));
        return m;
    }
};

// What check_witness found: the report of cstark_tx_witness_check (first_bad -1: consistent; final_root: the root the batch leaves,
// folded on the device whatever the verdicts), one cstark_witness_verdict per transfer, and the four folds of every transfer
// ([n_tx][4][7] words: sender-old, sender-new, receiver-old, receiver-new) when they were asked for
struct WitnessCheck {
    cstark_witness_report report{};
    std::vector<uint8_t> verdicts;
    std::vector<BaseElement> folds;
    bool ok() const { return report.first_bad < 0; }
};
// cstark_tx_witness_check of a host witness: every transfer's indices, leaves, paths, balance and roots (with check_signatures its
// signature too) tested on the device in one launch, before any trace is built.  The number of transfers need not be a power of two.
// The witness resident in the context is neither replaced nor touched.
inline WitnessCheck check_witness(Context &ctx, const TransactionMetadata &m, bool check_signatures = false, bool want_folds = false) {
    m.validate();
    WitnessCheck out;
    out.verdicts.resize(m.len());
    if (want_folds) out.folds.resize(m.len() * 28);
    const cstark_tx_witness w = m.view();
    check(cstark_tx_witness_check(ctx.raw(), &w, nullptr, check_signatures ? CSTARK_WITNESS_CHECK_SIGNATURES : 0u, &out.report, out.verdicts.data(),
                                  want_folds ? out.folds.data() : nullptr));
    return out;
}
// ... and of the witness RESIDENT in the context (TransactionProver::load, Ledger::apply), checked where it lies: n_tx its number of
// transfers; final_root (optional) the root it must lead to -- without it the last transfer's NEXT_ROOT test does not run and
// report.final_root is where that root is read
inline WitnessCheck check_resident_witness(Context &ctx, size_t n_tx, const Hash *final_root = nullptr, bool check_signatures = false, bool want_folds = false) {
    WitnessCheck out;
    out.verdicts.resize(n_tx);
    if (want_folds) out.folds.resize(n_tx * 28);
    check(cstark_tx_witness_check(ctx.raw(), nullptr, final_root ? final_root->data() : nullptr, check_signatures ? CSTARK_WITNESS_CHECK_SIGNATURES : 0u,
                                  &out.report, out.verdicts.data(), want_folds ? out.folds.data() : nullptr));
    return out;
}

// src/prover.rs:20-134.  The trace lives in device memory (the reference's TraceTable is a host object); prove() is the
// whole of Prover::prove including trace generation.
class TransactionProver {
  public:
    TransactionProver(const ProofOptions &options, Context &ctx) : options_(options), ctx_(ctx) {}
    const ProofOptions &options() const { return options_; }

    // uploads the witness; the trace itself is built inside prove() / build_trace()
    void load(const TransactionMetadata &m) {
        m.validate();
        if (m.len() & (m.len() - 1)) throw Error(CSTARK_ERR_INVALID_ARG, "the number of transactions must be a power of two");
        const cstark_tx_witness w = m.view();
        check(cstark_tx_witness_upload(ctx_.raw(), &w));
        n_tx_ = m.len();
    }
    // 94 x (1024 n) column-major trace into caller-provided device memory (cstark_malloc)
    void build_trace(const TransactionMetadata &m, uint64_t *d_trace) {
        load(m);
        check(cstark_tx_build_trace(ctx_.raw(), d_trace));
    }
    std::vector<uint8_t> prove(const TransactionMetadata &m) {
        load(m);
        const cstark_options o = options_.raw();
        std::vector<uint8_t> proof(cstark_tx_proof_size_bound((uint32_t)n_tx_, &o));
        size_t len = 0;
        check(cstark_tx_prove(ctx_.raw(), &o, proof.data(), proof.size(), &len));
        proof.resize(len);
        return proof;
    }
    // proves the witness that is resident in the context: the batch Ledger::apply just left there (n_tx: its number of transfers)
    std::vector<uint8_t> prove_resident(size_t n_tx) {
        const cstark_options o = options_.raw();
        std::vector<uint8_t> proof(cstark_tx_proof_size_bound((uint32_t)n_tx, &o));
        size_t len = 0;
        check(cstark_tx_prove(ctx_.raw(), &o, proof.data(), proof.size(), &len));
        proof.resize(len);
        return proof;
    }
    // src/prover.rs:106-129 (from the metadata: the first initial root and the final root)
    static PublicInputs get_pub_inputs(const TransactionMetadata &m) { return {m.initial_roots.at(0), m.final_root}; }

  private:
    ProofOptions options_;
    Context &ctx_;
    size_t n_tx_ = 0;
};

// Ledger::apply refused the batch at transfer `index` (reason: cstark_ledger_reason); ledger and resident witness are unchanged
struct TransferRefused : std::runtime_error {
    int32_t index, reason;
    TransferRefused(int32_t i, int32_t r) : std::runtime_error("transfer " + std::to_string(i) + " refused (reason " + std::to_string(r) + ")"), index(i), reason(r) {}
};
// A batch of signed transfers as an operator receives them
struct Transfers {
    std::vector<uint64_t> s_indices, r_indices;
    std::vector<BaseElement> deltas;
    std::vector<std::array<BaseElement, 6>> sig_rx;
    std::vector<std::array<uint8_t, 32>> sig_s;
};
// What Ledger::open returns: the accounts at `indices` with their authentication paths ([count][depth + 1][7] words, the witness's path
// form; an absent account's leaf is the all-zero digest) under `root`
struct AccountOpening {
    unsigned depth = 0;
    std::vector<uint64_t> indices;
    std::vector<std::array<BaseElement, 14>> values;
    std::vector<uint8_t> present;
    std::vector<BaseElement> paths;
    Hash root{};
};
// cstark_account_check_paths: one cstark_path_verdict per path (CSTARK_PATH_VALID = 0).  paths [count][depth + 1][7]; roots: one root or
// one per path; values / present (optional): the leaf test, without values the paths are paths of digests; roots_out (optional): what
// every path folds to, [count][7].  No ledger is needed and a resident witness is not touched.
inline std::vector<uint8_t> check_account_paths(Context &ctx, unsigned depth, const std::vector<uint64_t> &indices, const std::vector<BaseElement> &paths,
                                                const std::vector<Hash> &roots, const std::vector<std::array<BaseElement, 14>> *values = nullptr,
                                                const std::vector<uint8_t> *present = nullptr, std::vector<BaseElement> *roots_out = nullptr) {
    const size_t n = indices.size();
    if (n == 0 || paths.size() != n * (depth + 1) * 7 || roots.empty() || (values && values->size() != n) || (present && present->size() != n))
        throw Error(CSTARK_ERR_INVALID_ARG, "path vectors are not of equal length");
    std::vector<uint8_t> verdicts(n);
    if (roots_out) roots_out->resize(7 * n);
    check(cstark_account_check_paths(ctx.raw(), (uint32_t)n, depth, indices.data(), values ? (*values)[0].data() : nullptr, present ? present->data() : nullptr,
                                     paths.data(), roots[0].data(), (uint32_t)roots.size(), verdicts.data(), roots_out ? roots_out->data() : nullptr));
    return verdicts;
}
// What Ledger::open_multi returns: the accounts at the strictly ascending `indices` and ONE multiproof for all of them under `root`:
// nodes [n_nodes][7] words, the siblings no opened leaf accounts for, level `depth` first and ascending within a level (cstark.h)
struct AccountMultiOpening {
    unsigned depth = 0;
    std::vector<uint64_t> indices;
    std::vector<std::array<BaseElement, 14>> values;
    std::vector<uint8_t> present;
    std::vector<BaseElement> nodes;
    Hash root{};
};
// cstark_account_check_multiproof
struct MultiproofCheck {
    uint32_t verdict = 0; // cstark_multi_verdict (CSTARK_MULTI_VALID = 0)
    uint32_t at = 0;      // INDEX: the offending position; NODE_COUNT: the needed number of nodes
    uint32_t n_merges = 0;
    Hash root{};          // the fold, for VALID and ROOT
};
// One multiproof against the root it states.  Exactly one of values (with present, optional) and leaves ([count][7] words, digest mode);
// nodes [n_nodes][7] words.  A wrong order of the indices or a wrong number of nodes is a verdict, not an Error.  No ledger is needed and
// a resident witness is not touched.
inline MultiproofCheck check_account_multiproof(Context &ctx, unsigned depth, const std::vector<uint64_t> &indices, const std::vector<BaseElement> &nodes,
                                                const Hash &root, const std::vector<std::array<BaseElement, 14>> *values = nullptr,
                                                const std::vector<uint8_t> *present = nullptr, const std::vector<BaseElement> *leaves = nullptr) {
    const size_t n = indices.size();
    if (n == 0 || nodes.size() % 7 || (values && values->size() != n) || (present && present->size() != n) || (leaves && leaves->size() != 7 * n))
        throw Error(CSTARK_ERR_INVALID_ARG, "multiproof vectors are not of matching length");
    MultiproofCheck r;
    check(cstark_account_check_multiproof(ctx.raw(), depth, (uint32_t)n, indices.data(), values ? (*values)[0].data() : nullptr,
                                          present ? present->data() : nullptr, leaves ? leaves->data() : nullptr, nodes.empty() ? nullptr : nodes.data(),
                                          (uint32_t)(nodes.size() / 7), root.data(), &r.verdict, &r.at, r.root.data(), &r.n_merges));
    return r;
}
// cstark_account_check_update
struct UpdateCheck {
    uint32_t verdict = 0;   // cstark_update_verdict (CSTARK_UPDATE_VALID = 0)
    uint32_t at = 0;        // INDEX: the offending position; NODE_COUNT: the needed number of nodes
    uint32_t n_changed = 0; // positions whose (value, presence) differ; for VALID, OLD_ROOT and NEW_ROOT
    Hash new_root{};        // the fold of the new state, for VALID and NEW_ROOT
};
// The opening `old` under old.root against the new state of the same accounts (new_values in the order of old.indices; new_present
// optional: all present), both folded in one pass: with new_root the transition old.root -> *new_root is checked, without it the answer's
// new_root is the root the change leads to.  A wrong order of the indices or a wrong number of nodes is a verdict, not an Error.  No
// ledger is needed and a resident witness is not touched.
inline UpdateCheck check_account_update(Context &ctx, const AccountMultiOpening &old, const std::vector<std::array<BaseElement, 14>> &new_values,
                                        const std::vector<uint8_t> *new_present = nullptr, const Hash *new_root = nullptr) {
    const size_t n = old.indices.size();
    if (n == 0 || old.values.size() != n || (!old.present.empty() && old.present.size() != n) || new_values.size() != n || old.nodes.size() % 7 ||
        (new_present && new_present->size() != n))
        throw Error(CSTARK_ERR_INVALID_ARG, "update vectors are not of matching length");
    UpdateCheck r;
    check(cstark_account_check_update(ctx.raw(), old.depth, (uint32_t)n, old.indices.data(), old.values[0].data(),
                                      old.present.empty() ? nullptr : old.present.data(), new_values[0].data(), new_present ? new_present->data() : nullptr,
                                      old.nodes.empty() ? nullptr : old.nodes.data(), (uint32_t)(old.nodes.size() / 7), old.root.data(),
                                      new_root ? new_root->data() : nullptr, &r.verdict, &r.at, r.new_root.data(), &r.n_changed));
    return r;
}
// The account tree an operator holds, resident on the GPU (cstark_ledger_*): what replaces the sequential loop of
// TransactionMetadata::build_random (src/lib.rs:341-422) on real accounts.  apply() leaves the batch's witness resident in the context:
// TransactionProver::prove_resident follows without an upload.
class Ledger {
  public:
    Ledger(Context &ctx, unsigned depth = 15) : ctx_(ctx), depth_(depth) { check(cstark_ledger_create(ctx.raw(), depth, &led_)); }
    ~Ledger() { cstark_ledger_destroy(led_); }
    Ledger(const Ledger &) = delete;
    Ledger &operator=(const Ledger &) = delete;
    // A PARTIAL ledger (cstark_ledger_create_partial) built from a multi-opening under the root it states: it knows exactly the opened
    // accounts, present or absent, and for them behaves as the full ledger does (apply, set_accounts, root, open, open_multi,
    // checkpoints, audit; apply() leaves the witness resident).  A transfer that names an unknown account is refused with
    // CSTARK_LEDGER_UNKNOWN, every other call with an unknown index throws.  Throws Error(CSTARK_ERR_INVALID_ARG) naming the verdict when
    // the opening has no shape or does not fold to its root; *verdict (optional) receives the cstark_multi_verdict either way.  Returned
    // by value: the class cannot be copied or moved, the caller binds the result (`cstark::Ledger p = cstark::Ledger::from_multiproof(..)`)
    static Ledger from_multiproof(Context &ctx, const AccountMultiOpening &o, uint32_t *verdict = nullptr) {
        const size_t n = o.indices.size();
        if (n == 0 || o.values.size() != n || (!o.present.empty() && o.present.size() != n) || o.nodes.size() % 7)
            throw Error(CSTARK_ERR_INVALID_ARG, "multiproof vectors are not of matching length");
        cstark_ledger *led = nullptr;
        uint32_t v = 0, at = 0;
        check(cstark_ledger_create_partial(ctx.raw(), o.depth, (uint32_t)n, o.indices.data(), o.values[0].data(), o.present.empty() ? nullptr : o.present.data(),
                                           o.nodes.empty() ? nullptr : o.nodes.data(), (uint32_t)(o.nodes.size() / 7), o.root.data(), &led, &v, &at));
        if (verdict) *verdict = v;
        if (!led) throw Error(CSTARK_ERR_INVALID_ARG, "the opening gives no ledger: cstark_multi_verdict " + std::to_string(v) + " at " + std::to_string(at));
        return Ledger(ctx, o.depth, led);
    }
    // which of the given leaves the ledger knows (a full ledger: every index below 2^depth)
    std::vector<uint8_t> known(const std::vector<uint64_t> &indices) const {
        std::vector<uint8_t> k(indices.size());
        if (!indices.empty()) check(cstark_ledger_known(ctx_.raw(), led_, (uint32_t)indices.size(), indices.data(), k.data()));
        return k;
    }
    struct PartialInfo { bool is_partial; uint64_t n_known, n_opaque; };
    // partial: opened indices and proof nodes; full: {false, number of accounts, 0}
    PartialInfo partial_info() const {
        uint32_t partial = 0;
        PartialInfo r{};
        check(cstark_ledger_partial_info(ctx_.raw(), led_, &partial, &r.n_known, &r.n_opaque));
        r.is_partial = partial != 0;
        return r;
    }
    void set_accounts(const std::vector<uint64_t> &indices, const std::vector<std::array<BaseElement, 14>> &values) {
        if (indices.size() != values.size() || indices.empty()) throw Error(CSTARK_ERR_INVALID_ARG, "one value per account index");
        check(cstark_ledger_set_accounts(ctx_.raw(), led_, (uint32_t)indices.size(), indices.data(), values[0].data()));
    }
    Hash root() const {
        Hash r{};
        check(cstark_ledger_root(ctx_.raw(), led_, r.data()));
        return r;
    }
    // values of the given accounts; present[i] = 0 where there is none (its value reads as zeros)
    std::vector<std::array<BaseElement, 14>> accounts(const std::vector<uint64_t> &indices, std::vector<uint8_t> *present = nullptr) const {
        std::vector<std::array<BaseElement, 14>> values(indices.size());
        std::vector<uint8_t> have(indices.size());
        if (!indices.empty()) check(cstark_ledger_get_accounts(ctx_.raw(), led_, (uint32_t)indices.size(), indices.data(), values[0].data(), have.data()));
        if (present) *present = have;
        return values;
    }
    // values, presence and authentication paths of the given leaves under the current root (cstark_ledger_open_accounts); indices may
    // repeat and may name absent accounts.  Read-only.  check_account_paths(ctx, o.depth, o.indices, o.paths, {o.root}, &o.values,
    // &o.present) is all CSTARK_PATH_VALID for what this returns
    AccountOpening open(const std::vector<uint64_t> &indices) const {
        if (indices.empty()) throw Error(CSTARK_ERR_INVALID_ARG, "no account index to open");
        AccountOpening o;
        o.depth = depth_;
        o.indices = indices;
        o.values.resize(indices.size());
        o.present.resize(indices.size());
        o.paths.resize(indices.size() * (depth_ + 1) * 7);
        check(cstark_ledger_open_accounts(ctx_.raw(), led_, (uint32_t)indices.size(), indices.data(), o.values[0].data(), o.present.data(), o.paths.data(),
                                          o.root.data()));
        return o;
    }
    // ---- checkpoints (cstark_ledger_checkpoint ...): ids are integers >= 1, never reused; 0 names the current state where an id is read
    // names the state as it is now; no device work, and apply() costs what it costs without one.  At most
    // CSTARK_LEDGER_MAX_CHECKPOINTS are live at once (Error CSTARK_ERR_UNSUPPORTED beyond)
    uint64_t checkpoint() {
        uint64_t id = 0;
        check(cstark_ledger_checkpoint(ctx_.raw(), led_, &id));
        return id;
    }
    // the ledger goes back to the checkpoint: later checkpoints are dropped, this one stays live.  The resident witness is left alone
    void revert(uint64_t id) { check(cstark_ledger_revert(ctx_.raw(), led_, id)); }
    void release(uint64_t id) { check(cstark_ledger_release(ctx_.raw(), led_, id)); }
    Hash root(uint64_t at) const {
        Hash r{};
        check(cstark_ledger_root_at(ctx_.raw(), led_, at, r.data()));
        return r;
    }
    // open() as the ledger was at checkpoint `at`: under the root a proof of that moment binds
    AccountOpening open(const std::vector<uint64_t> &indices, uint64_t at) const {
        if (indices.empty()) throw Error(CSTARK_ERR_INVALID_ARG, "no account index to open");
        AccountOpening o;
        o.depth = depth_;
        o.indices = indices;
        o.values.resize(indices.size());
        o.present.resize(indices.size());
        o.paths.resize(indices.size() * (depth_ + 1) * 7);
        check(cstark_ledger_open_accounts_at(ctx_.raw(), led_, at, (uint32_t)indices.size(), indices.data(), o.values[0].data(), o.present.data(),
                                             o.paths.data(), o.root.data()));
        return o;
    }
    // the given leaves (any order, repeats allowed: sorted and de-duplicated here) with ONE multiproof for all of them
    // (cstark_ledger_open_multi), under the current root or the root of checkpoint `at`.  Read-only: one gather, no hashing.
    // check_account_multiproof(ctx, o.depth, o.indices, o.nodes, o.root, &o.values, &o.present).verdict is CSTARK_MULTI_VALID
    AccountMultiOpening open_multi(std::vector<uint64_t> indices, uint64_t at = 0) const {
        if (indices.empty()) throw Error(CSTARK_ERR_INVALID_ARG, "no account index to open");
        std::sort(indices.begin(), indices.end());
        indices.erase(std::unique(indices.begin(), indices.end()), indices.end());
        AccountMultiOpening o;
        o.depth = depth_;
        uint32_t n_nodes = 0, n_merges = 0;
        check(cstark_account_multiproof_shape(depth_, (uint32_t)indices.size(), indices.data(), &n_nodes, &n_merges));
        o.values.resize(indices.size());
        o.present.resize(indices.size());
        o.nodes.resize((size_t)7 * n_nodes);
        check(cstark_ledger_open_multi(ctx_.raw(), led_, at, (uint32_t)indices.size(), indices.data(), o.values[0].data(), o.present.data(),
                                       n_nodes ? o.nodes.data() : nullptr, n_nodes, &n_nodes, o.root.data()));
        o.indices = std::move(indices);
        return o;
    }
    // every stored node of the state at `at` (0: the current one) against its stored children, on the GPU in one launch.  Read-only; an
    // inconsistency is reported (consistent == 0, the first failing node named), not thrown
    cstark_ledger_audit_report audit(uint64_t at = 0) const {
        cstark_ledger_audit_report r{};
        check(cstark_ledger_audit(ctx_.raw(), led_, at, &r));
        return r;
    }
    // applies the transfers in order; throws TransferRefused (nothing changed) at the first one that cannot be applied.  Signatures are
    // copied through unchecked, and TransactionAir does not bind them: a forged one still proves and verifies (apply_checked)
    TransactionMetadata apply(const Transfers &t) { return apply(t, false); }
    // the same with every transfer's signature checked on the device first (cstark_ledger_apply_checked): TransferRefused with reason
    // CSTARK_LEDGER_SIGNATURE at the first transfer whose signature does not verify
    TransactionMetadata apply_checked(const Transfers &t) { return apply(t, true); }
    // the message each transfer of the batch has to sign, [n][28] (cstark_ledger_messages; sig_rx and sig_s of `t` are not read): throws
    // TransferRefused where apply would, with its reason.  Read-only
    std::vector<std::array<BaseElement, 28>> messages(const Transfers &t) const {
        const size_t n = t.s_indices.size();
        if (n == 0 || t.r_indices.size() != n || t.deltas.size() != n) throw Error(CSTARK_ERR_INVALID_ARG, "transfer vectors are not of equal length");
        std::vector<std::array<BaseElement, 28>> out(n);
        int32_t at = -1, reason = 0;
        check(cstark_ledger_messages(ctx_.raw(), led_, (uint32_t)n, t.s_indices.data(), t.r_indices.data(), t.deltas.data(), out[0].data(), &at, &reason));
        if (at >= 0) throw TransferRefused(at, reason);
        return out;
    }
    // the batch signed on the device with the senders' secret keys (cstark_ledger_sign; secrets[t] signs transfer t, 1 .. 255): what
    // apply_checked takes.  Throws TransferRefused where apply would, or with CSTARK_LEDGER_KEY at the first transfer whose secret is not
    // its sender's key.  Read-only.  A signer for building batches, tests and benchmarks.  It is not a wallet.
    Transfers sign(const Transfers &t, const std::vector<uint64_t> &secrets, uint64_t seed = 0, uint32_t max_attempts = 256) const {
        const size_t n = t.s_indices.size();
        if (n == 0 || t.r_indices.size() != n || t.deltas.size() != n || secrets.size() != n)
            throw Error(CSTARK_ERR_INVALID_ARG, "transfer vectors are not of equal length");
        Transfers out{t.s_indices, t.r_indices, t.deltas, {}, {}};
        out.sig_rx.resize(n);
        out.sig_s.resize(n);
        int32_t at = -1, reason = 0;
        check(cstark_ledger_sign(ctx_.raw(), led_, (uint32_t)n, t.s_indices.data(), t.r_indices.data(), t.deltas.data(), secrets.data(), seed, max_attempts,
                                 out.sig_rx[0].data(), out.sig_s[0].data(), nullptr, &at, &reason));
        if (at >= 0) throw TransferRefused(at, reason);
        return out;
    }
    // What select returns: one cstark_ledger_reason per candidate (CSTARK_LEDGER_APPLIED: selected), the selected candidate numbers in
    // ascending order, their transfers (what apply takes), the report, and with apply_selection the witness of the applied selection
    struct Selection {
        std::vector<uint8_t> status;
        std::vector<uint32_t> selected;
        Transfers transfers;
        cstark_ledger_selection report{};
        std::vector<std::array<BaseElement, 28>> messages; // with want_messages: the message of every candidate sent to the device, zeros elsewhere
        TransactionMetadata witness;                        // with apply_selection and something selected
    };
    // A provable batch out of a pool of candidates in arrival order (cstark_ledger_select): every candidate gets a status, up to `want`
    // are selected, nothing is refused as a whole.  A refused candidate holds its sender for the rest of the call (CSTARK_LEDGER_HELD for
    // the sender's later candidates; the account still receives), so the signatures are checked on the device in passes of `chunk`
    // candidates (0: the library's choice) whatever the bad ones do.  flags: CSTARK_SELECT_CHECK_SIGNATURES, CSTARK_SELECT_POW2 (the
    // selection cut to a power of two, what prove needs), CSTARK_SELECT_APPLY (the selection applied as apply would apply it, its witness
    // resident for prove_resident; otherwise the call is read-only).  The pool's signatures may be empty without CHECK and APPLY.
    Selection select(const Transfers &pool, uint32_t want, uint32_t flags = CSTARK_SELECT_CHECK_SIGNATURES | CSTARK_SELECT_POW2, uint32_t chunk = 0,
                     bool want_messages = false) {
        const size_t n = pool.s_indices.size();
        const bool signatures = !pool.sig_rx.empty() || !pool.sig_s.empty();
        if (n == 0 || pool.r_indices.size() != n || pool.deltas.size() != n || (signatures && (pool.sig_rx.size() != n || pool.sig_s.size() != n)))
            throw Error(CSTARK_ERR_INVALID_ARG, "candidate vectors are not of equal length");
        const size_t cap = std::max<size_t>(1, std::min<size_t>(want, n));
        Selection r;
        r.status.resize(n);
        r.selected.resize(cap);
        if (want_messages) r.messages.resize(n);
        TransactionMetadata &m = r.witness;
        cstark_tx_witness w{};
        const bool apply_selection = flags & CSTARK_SELECT_APPLY;
        if (apply_selection) {
            m.merkle_depth = depth_;
            m.initial_roots.resize(cap); m.s_old_values.resize(cap); m.r_old_values.resize(cap); m.s_indices.resize(cap); m.r_indices.resize(cap);
            m.s_paths.resize(cap * (depth_ + 1) * 7); m.r_paths.resize(cap * (depth_ + 1) * 7); m.deltas.resize(cap); m.sig_rx.resize(cap); m.sig_s.resize(cap);
            w = m.view();
        }
        check(cstark_ledger_select(ctx_.raw(), led_, (uint32_t)n, pool.s_indices.data(), pool.r_indices.data(), pool.deltas.data(),
                                   signatures ? pool.sig_rx[0].data() : nullptr, signatures ? pool.sig_s[0].data() : nullptr, want, flags, chunk, r.status.data(),
                                   r.selected.data(), want_messages ? r.messages[0].data() : nullptr, &r.report, apply_selection ? &w : nullptr));
        const size_t k = r.report.n_selected;
        r.selected.resize(k);
        for (const uint32_t t : r.selected) {
            r.transfers.s_indices.push_back(pool.s_indices[t]); r.transfers.r_indices.push_back(pool.r_indices[t]); r.transfers.deltas.push_back(pool.deltas[t]);
            if (signatures) { r.transfers.sig_rx.push_back(pool.sig_rx[t]); r.transfers.sig_s.push_back(pool.sig_s[t]); }
        }
        if (apply_selection) {
            m.initial_roots.resize(k); m.s_old_values.resize(k); m.r_old_values.resize(k); m.s_indices.resize(k); m.r_indices.resize(k);
            m.s_paths.resize(k * (depth_ + 1) * 7); m.r_paths.resize(k * (depth_ + 1) * 7); m.deltas.resize(k); m.sig_rx.resize(k); m.sig_s.resize(k);
        }
        return r;
    }

  private:
    Ledger(Context &ctx, unsigned depth, cstark_ledger *led) : ctx_(ctx), depth_(depth), led_(led) {}
    TransactionMetadata apply(const Transfers &t, bool check_signatures) {
        const size_t n = t.s_indices.size();
        if (n == 0 || t.r_indices.size() != n || t.deltas.size() != n || t.sig_rx.size() != n || t.sig_s.size() != n)
            throw Error(CSTARK_ERR_INVALID_ARG, "transfer vectors are not of equal length");
        TransactionMetadata m;
        m.merkle_depth = depth_;
        m.initial_roots.resize(n); m.s_old_values.resize(n); m.r_old_values.resize(n); m.s_indices.resize(n); m.r_indices.resize(n);
        m.s_paths.resize(n * (depth_ + 1) * 7); m.r_paths.resize(n * (depth_ + 1) * 7); m.deltas.resize(n); m.sig_rx.resize(n); m.sig_s.resize(n);
        cstark_tx_witness w = m.view();
        int32_t at = -1, reason = 0;
        check((check_signatures ? cstark_ledger_apply_checked : cstark_ledger_apply)(ctx_.raw(), led_, (uint32_t)n, t.s_indices.data(), t.r_indices.data(),
                                                                                     t.deltas.data(), t.sig_rx[0].data(), t.sig_s[0].data(), &w, &at, &reason));
        if (at >= 0) throw TransferRefused(at, reason);
        return m;
    }
    Context &ctx_;
    unsigned depth_;
    cstark_ledger *led_ = nullptr;
};

// Several proofs in flight on ONE GPU.  A proof is a chain of launches with a dozen host round trips (the Fiat-Shamir channel) during
// which the GPU idles (~0.6 ms of a 28 ms proof); a second proof on a context and host thread of its own fills those gaps: 36.7
// instead of 35.2 proofs/s at 2^20 steps (bench.py --inflight 2).  Every worker owns a Context with its own stream; submit() hands a
// witness to the next free worker and returns a future of the proof bytes (exceptions travel through the future).
class ProverPool {
  public:
    explicit ProverPool(const ProofOptions &options, unsigned workers = 2, int device = -1) : options_(options) {
        if (workers == 0) throw Error(CSTARK_ERR_INVALID_ARG, "ProverPool: at least one worker");
        for (unsigned w = 0; w < workers; w++) ctx_.emplace_back(new Context(Context::OwnStream{}, device));
        try {
            for (unsigned w = 0; w < workers; w++) threads_.emplace_back([this, w] { run(w); });
        } catch (...) { // a thread could not be created: stop and join the ones already running (a joinable std::thread must not be destroyed)
            { std::lock_guard<std::mutex> g(m_); stop_ = true; }
            cv_.notify_all();
            for (std::thread &t : threads_) t.join();
            throw;
        }
    }
    ~ProverPool() {
        { std::lock_guard<std::mutex> g(m_); stop_ = true; }
        cv_.notify_all();
        for (std::thread &t : threads_) t.join();
    }
    ProverPool(const ProverPool &) = delete;
    ProverPool &operator=(const ProverPool &) = delete;
    std::future<std::vector<uint8_t>> submit(TransactionMetadata m) {
        std::packaged_task<std::vector<uint8_t>(Context &)> task(
            [opt = options_, m = std::move(m)](Context &c) { return TransactionProver(opt, c).prove(m); });
        std::future<std::vector<uint8_t>> f = task.get_future();
        { std::lock_guard<std::mutex> g(m_); q_.push_back(std::move(task)); }
        cv_.notify_one();
        return f;
    }
    unsigned workers() const { return (unsigned)threads_.size(); }

  private:
    void run(unsigned w) {
        for (;;) {
            std::packaged_task<std::vector<uint8_t>(Context &)> task;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [this] { return stop_ || !q_.empty(); });
                if (q_.empty()) return; // stop_ and nothing left
                task = std::move(q_.front());
                q_.pop_front();
            }
            task(*ctx_[w]);
        }
    }
    ProofOptions options_;
    std::vector<std::unique_ptr<Context>> ctx_;
    std::vector<std::thread> threads_;
    std::deque<std::packaged_task<std::vector<uint8_t>(Context &)>> q_;
    std::mutex m_;
    std::condition_variable cv_;
    bool stop_ = false;
};

// winterfell::VerifierError: a rejected proof; verdict = the cstark_verdict of the first failing check (include/cstark.h)
struct VerifierError : std::runtime_error {
    int verdict;
    explicit VerifierError(int v) : std::runtime_error("proof rejected (verdict " + std::to_string(v) + ")"), verdict(v) {}
};

// cstark_tx_verify for many proofs in one call: one verdict per proof (CSTARK_PROOF_OK = accepted).  expected = nullptr: each proof's own
// options; otherwise every proof must state exactly these.
inline std::vector<int32_t> verify_batch(Context &ctx, const std::vector<std::vector<uint8_t>> &proofs, const std::vector<PublicInputs> &pub,
                                         const ProofOptions *expected = nullptr) {
    if (pub.size() != proofs.size()) throw Error(CSTARK_ERR_INVALID_ARG, "one PublicInputs per proof");
    std::vector<const uint8_t *> ptrs(proofs.size());
    std::vector<size_t> lens(proofs.size());
    std::vector<uint64_t> r0(7 * proofs.size()), r1(7 * proofs.size());
    for (size_t i = 0; i < proofs.size(); i++) {
        ptrs[i] = proofs[i].data();
        lens[i] = proofs[i].size();
        for (int k = 0; k < 7; k++) { r0[7 * i + k] = pub[i].initial_root[k]; r1[7 * i + k] = pub[i].final_root[k]; }
    }
    std::vector<int32_t> verdicts(proofs.size());
    cstark_options o{};
    if (expected) o = expected->raw();
    check(cstark_tx_verify(ctx.raw(), (uint32_t)proofs.size(), ptrs.data(), lens.data(), r0.data(), r1.data(), expected ? &o : nullptr,
                           verdicts.data()));
    return verdicts;
}

// ---- conversion between the proof forms (cstark_*_convert: the verify call that also writes every accepted proof in `form`) ----
// cstark_proof_convert_bound (host only): a capacity that holds `proof` in `form` whatever its positions; throws when it does not parse
inline size_t convert_bound(const std::vector<uint8_t> &proof, uint32_t form) {
    size_t bound = 0;
    check(cstark_proof_convert_bound(proof.data(), proof.size(), form, &bound));
    return bound;
}
// what a convert call returns: verdicts[i] as the verify call gives it, proofs[i] the proof in the target form (empty unless accepted)
struct Converted {
    std::vector<std::vector<uint8_t>> proofs;
    std::vector<int32_t> verdicts;
};
namespace detail {
// the output arguments of one convert call: a buffer per proof sized by its bound (a proof that does not parse is never converted)
struct ConvertBuffers {
    Converted result;
    std::vector<uint8_t *> out;
    std::vector<size_t> capacities, lens;
    ConvertBuffers(const std::vector<const uint8_t *> &ptrs, const std::vector<size_t> &in_lens, uint32_t form)
        : out(ptrs.size()), capacities(ptrs.size()), lens(ptrs.size(), 0) {
        result.proofs.resize(ptrs.size());
        result.verdicts.assign(ptrs.size(), -1);
        for (size_t i = 0; i < ptrs.size(); i++) {
            size_t bound = 1;
            if (cstark_proof_convert_bound(ptrs[i], in_lens[i], form, &bound) != CSTARK_OK) bound = 1;
            result.proofs[i].resize(bound);
            out[i] = result.proofs[i].data();
            capacities[i] = bound;
        }
    }
    Converted finish() {
        for (size_t i = 0; i < out.size(); i++) result.proofs[i].resize(result.verdicts[i] == CSTARK_PROOF_OK ? lens[i] : 0);
        return std::move(result);
    }
};
// one proof: its bytes in `form`, or VerifierError with the verdict
inline std::vector<uint8_t> converted_or_throw(Converted c) {
    if (c.verdicts.at(0) != CSTARK_PROOF_OK) throw VerifierError(c.verdicts[0]);
    return std::move(c.proofs[0]);
}
} // namespace detail
// cstark_tx_convert for many proofs in one call, as verify_batch
inline Converted convert_batch(Context &ctx, const std::vector<std::vector<uint8_t>> &proofs, const std::vector<PublicInputs> &pub, uint32_t form,
                               const ProofOptions *expected = nullptr) {
    if (pub.size() != proofs.size()) throw Error(CSTARK_ERR_INVALID_ARG, "one PublicInputs per proof");
    std::vector<const uint8_t *> ptrs(proofs.size());
    std::vector<size_t> lens(proofs.size());
    std::vector<uint64_t> r0(7 * proofs.size()), r1(7 * proofs.size());
    for (size_t i = 0; i < proofs.size(); i++) {
        ptrs[i] = proofs[i].data();
        lens[i] = proofs[i].size();
        for (int k = 0; k < 7; k++) { r0[7 * i + k] = pub[i].initial_root[k]; r1[7 * i + k] = pub[i].final_root[k]; }
    }
    detail::ConvertBuffers b(ptrs, lens, form);
    cstark_options o{};
    if (expected) o = expected->raw();
    check(cstark_tx_convert(ctx.raw(), (uint32_t)proofs.size(), ptrs.data(), lens.data(), r0.data(), r1.data(), expected ? &o : nullptr, form,
                            b.out.data(), b.capacities.data(), b.lens.data(), b.result.verdicts.data()));
    return b.finish();
}
// cstark_air_convert: proofs[i] is stated to be of airs[i], with the 14 public words pub[i]
inline Converted air_convert_batch(Context &ctx, const std::vector<std::vector<uint8_t>> &proofs, const std::vector<int32_t> &airs,
                                   const std::vector<std::array<uint64_t, 14>> &pub, uint32_t form, const ProofOptions *expected = nullptr) {
    if (pub.size() != proofs.size() || airs.size() != proofs.size()) throw Error(CSTARK_ERR_INVALID_ARG, "one AIR id and 14 public words per proof");
    std::vector<const uint8_t *> ptrs(proofs.size());
    std::vector<size_t> lens(proofs.size());
    for (size_t i = 0; i < proofs.size(); i++) { ptrs[i] = proofs[i].data(); lens[i] = proofs[i].size(); }
    detail::ConvertBuffers b(ptrs, lens, form);
    cstark_options o{};
    if (expected) o = expected->raw();
    check(cstark_air_convert(ctx.raw(), (uint32_t)proofs.size(), ptrs.data(), lens.data(), airs.data(), pub.empty() ? nullptr : pub[0].data(),
                             expected ? &o : nullptr, form, b.out.data(), b.capacities.data(), b.lens.data(), b.result.verdicts.data()));
    return b.finish();
}
// cstark_schnorr_convert: proofs[i] against statements[i]
inline Converted schnorr_convert_batch(Context &ctx, const std::vector<std::vector<uint8_t>> &proofs, const std::vector<cstark_schnorr_statement> &statements,
                                       uint32_t form, const ProofOptions *expected = nullptr) {
    if (statements.size() != proofs.size()) throw Error(CSTARK_ERR_INVALID_ARG, "one statement per proof");
    std::vector<const uint8_t *> ptrs(proofs.size());
    std::vector<size_t> lens(proofs.size());
    for (size_t i = 0; i < proofs.size(); i++) { ptrs[i] = proofs[i].data(); lens[i] = proofs[i].size(); }
    detail::ConvertBuffers b(ptrs, lens, form);
    cstark_options o{};
    if (expected) o = expected->raw();
    check(cstark_schnorr_convert(ctx.raw(), (uint32_t)proofs.size(), ptrs.data(), lens.data(), statements.data(), expected ? &o : nullptr, form,
                                 b.out.data(), b.capacities.data(), b.lens.data(), b.result.verdicts.data()));
    return b.finish();
}

// ---- trace validation (cstark_air_validate_trace) ----
// What the validation of a device trace found: step < 0 and boundary < 0 is a clean trace.  cycle = step / cycle length (one transfer,
// signature or link; the whole trace for RangeProofAir), row_in_cycle = step % cycle length.
struct TraceReport {
    int air = 0;
    int64_t step = -1;
    uint64_t cycle = 0;
    uint32_t row_in_cycle = 0, constraint = CSTARK_TRACE_CLEAN, bad_cycles = 0;
    int32_t boundary = -1;
    uint32_t boundary_register = 0;
    uint64_t boundary_step = 0;
    std::vector<uint32_t> cycle_codes;     // with want_cycles: one code per cycle (CSTARK_TRACE_CLEAN, or row * n_constraints + constraint)
    std::vector<BaseElement> frame_values; // with want_frame and a violated frame: every constraint value of the first violated frame
    bool ok() const { return step < 0 && boundary < 0; }
    // "transfer 3, row 126, constraint 99", "boundary entry 8: register 59 at step 2047", both joined by "; ", or "clean"
    std::string str() const {
        static const char *unit[5] = {"transfer", "transfer", "signature", "trace", "link"};
        std::string s;
        if (step >= 0) s = std::string(unit[air]) + " " + std::to_string(cycle) + ", row " + std::to_string(row_in_cycle) + ", constraint " + std::to_string(constraint);
        if (boundary >= 0)
            s += std::string(s.empty() ? "" : "; ") + "boundary entry " + std::to_string(boundary) + ": register " + std::to_string(boundary_register) + " at step " +
                 std::to_string(boundary_step);
        return s.empty() ? "clean" : s;
    }
};
// d_trace: [width][2^log_n] device memory; item: the Merkle depth (TransactionAir, MerkleAir); public_inputs: 14 words as for
// cstark_air_verify, or null for no boundary check (SchnorrAir: any non-null pointer checks the resident statement)
inline TraceReport validate_trace(Context &ctx, int air, const uint64_t *d_trace, uint32_t log_n, uint32_t item, const uint64_t *public_inputs,
                                  bool want_cycles = false, bool want_frame = false) {
    uint32_t width = 0, nc = 0, lc = 0;
    check(cstark_air_trace_shape(air, log_n, &width, &nc, &lc)); // an unknown AIR or an impossible trace length throws here
    TraceReport r;
    r.air = air;
    if (want_cycles) r.cycle_codes.assign((size_t)1 << (log_n - lc), CSTARK_TRACE_CLEAN);
    if (want_frame) r.frame_values.assign(nc, 0);
    cstark_trace_report rep{};
    check(cstark_air_validate_trace(ctx.raw(), air, d_trace, log_n, item, public_inputs, &rep, r.cycle_codes.empty() ? nullptr : r.cycle_codes.data(),
                                    want_frame ? r.frame_values.data() : nullptr));
    r.step = rep.step; r.constraint = rep.constraint; r.bad_cycles = rep.bad_cycles;
    r.boundary = rep.boundary; r.boundary_register = rep.boundary_register; r.boundary_step = rep.boundary_step;
    if (rep.step >= 0) { r.cycle = (uint64_t)rep.step >> lc; r.row_in_cycle = (uint32_t)((uint64_t)rep.step & (((uint64_t)1 << lc) - 1)); }
    else r.frame_values.clear();
    return r;
}
namespace detail {
// a device trace of width x 2^log_n filled by `build`, validated, freed
template <class Build>
inline TraceReport validate_built(Context &ctx, int air, uint32_t width, size_t rows, uint32_t item, const uint64_t *public_inputs, bool want_cycles,
                                  bool want_frame, Build build) {
    uint32_t log_n = 0;
    while (((size_t)1 << log_n) < rows) log_n++;
    if (((size_t)1 << log_n) != rows) throw Error(CSTARK_ERR_INVALID_ARG, "the trace length must be a power of two");
    void *d_trace = nullptr;
    check(cstark_malloc(ctx.raw(), (size_t)width * rows * 8, &d_trace));
    try {
        check(build((uint64_t *)d_trace));
        TraceReport r = validate_trace(ctx, air, (const uint64_t *)d_trace, log_n, item, public_inputs, want_cycles, want_frame);
        cstark_free(ctx.raw(), d_trace);
        return r;
    } catch (...) {
        cstark_free(ctx.raw(), d_trace);
        throw;
    }
}
inline void root_words(const PublicInputs &p, uint64_t (&pub)[14]) {
    for (int k = 0; k < 7; k++) { pub[k] = p.initial_root[k]; pub[7 + k] = p.final_root[k]; }
}
} // namespace detail

// src/lib.rs:92-150
class TransactionExample {
  public:
    TransactionExample(const ProofOptions &options, size_t num_transactions, Context &ctx, unsigned depth = 15, uint64_t seed = 0x5EED)
        : options_(options), tx_metadata_(TransactionMetadata::build_random(num_transactions, depth, seed)), ctx_(ctx) {}
    std::vector<uint8_t> prove() { return TransactionProver(options_, ctx_).prove(tx_metadata_); }
    PublicInputs pub_inputs() const { return TransactionProver::get_pub_inputs(tx_metadata_); }
    const TransactionMetadata &metadata() const { return tx_metadata_; }
    // winterfell::verify::<TransactionAir>(proof, pub_inputs) (src/lib.rs:144-150): throws VerifierError on rejection
    void verify(const std::vector<uint8_t> &proof) const {
        const int32_t v = verify_batch(ctx_, {proof}, {pub_inputs()})[0];
        if (v != CSTARK_PROOF_OK) throw VerifierError(v);
    }
    // Trace::validate of the reference's debug builds, on the device: the trace of this witness against every transition constraint and
    // the accepted proof in `form` (cstark_tx_convert): the bytes a prover set to that form writes; throws VerifierError as verify() does
    std::vector<uint8_t> convert(const std::vector<uint8_t> &proof, uint32_t form = CSTARK_FORM_COMPACT) const {
        return detail::converted_or_throw(convert_batch(ctx_, {proof}, {pub_inputs()}, form));
    }
    // the statement verify() is given
    TraceReport validate(bool want_cycles = false, bool want_frame = false) const {
        uint64_t pub[14];
        detail::root_words(pub_inputs(), pub);
        const cstark_tx_witness w = tx_metadata_.view();
        check(cstark_tx_witness_upload(ctx_.raw(), &w));
        return detail::validate_built(ctx_, CSTARK_AIR_STATE_TRANSITION, 94, tx_metadata_.len() * 1024, w.merkle_depth, pub, want_cycles, want_frame,
                                      [&](uint64_t *d) { return cstark_tx_build_trace(ctx_.raw(), d); });
    }

  private:
    ProofOptions options_;
    TransactionMetadata tx_metadata_;
    Context &ctx_;
};
inline TransactionExample get_example(size_t num_transactions, Context &ctx) { // src/lib.rs:75-89
    return TransactionExample(ProofOptions(42, 8, 0, HashFunction::Blake3_256, FieldExtension::None, 4, 256), num_transactions, ctx);
}

namespace detail {
// cstark_air_verify for one proof of `air` against its 14 public words: throws VerifierError on rejection
inline void air_verify(Context &ctx, int32_t air, const std::vector<uint8_t> &proof, const uint64_t (&pub)[14]) {
    const uint8_t *ptr = proof.data();
    const size_t len = proof.size();
    int32_t v = -1;
    check(cstark_air_verify(ctx.raw(), 1, &ptr, &len, &air, pub, nullptr, &v));
    if (v != CSTARK_PROOF_OK) throw VerifierError(v);
}
// cstark_air_convert for one proof: its bytes in `form`; throws VerifierError on rejection
inline std::vector<uint8_t> air_convert(Context &ctx, int32_t air, const std::vector<uint8_t> &proof, const uint64_t (&pub)[14], uint32_t form) {
    std::array<uint64_t, 14> words;
    for (int k = 0; k < 14; k++) words[k] = pub[k];
    return converted_or_throw(air_convert_batch(ctx, {proof}, {air}, {words}, form));
}
inline std::vector<uint8_t> air_prove(Context &ctx, int air, const ProofOptions &options, uint64_t number, size_t rows) {
    const cstark_options o = options.raw();
    std::vector<uint8_t> proof(2 * cstark_tx_proof_size_bound((uint32_t)((rows + 1023) / 1024), &o));
    size_t len = 0;
    check(cstark_air_prove(ctx.raw(), air, &o, number, proof.data(), proof.size(), &len));
    proof.resize(len);
    return proof;
}
} // namespace detail

// merkle::update::MerkleExample (src/merkle/update/mod.rs:36-127)
class MerkleExample {
  public:
    MerkleExample(const ProofOptions &options, TransactionMetadata m, Context &ctx) : options_(options), m_(std::move(m)), ctx_(ctx) { m_.validate(); }
    std::vector<uint8_t> prove() {
        const cstark_tx_witness w = m_.view();
        check(cstark_tx_witness_upload(ctx_.raw(), &w));
        return detail::air_prove(ctx_, CSTARK_AIR_MERKLE_UPDATE, options_, 0, m_.len() * 512);
    }
    PublicInputs pub_inputs() const { return {m_.initial_roots.at(0), m_.final_root}; }
    // src/merkle/update/mod.rs:109-127: throws VerifierError on rejection
    void verify(const std::vector<uint8_t> &proof) const {
        const PublicInputs p = pub_inputs();
        uint64_t pub[14];
        for (int k = 0; k < 7; k++) { pub[k] = p.initial_root[k]; pub[7 + k] = p.final_root[k]; }
        detail::air_verify(ctx_, CSTARK_AIR_MERKLE_UPDATE, proof, pub);
    }
    std::vector<uint8_t> convert(const std::vector<uint8_t> &proof, uint32_t form = CSTARK_FORM_COMPACT) const {
        uint64_t pub[14];
        detail::root_words(pub_inputs(), pub);
        return detail::air_convert(ctx_, CSTARK_AIR_MERKLE_UPDATE, proof, pub, form);
    }
    TraceReport validate(bool want_cycles = false, bool want_frame = false) const {
        uint64_t pub[14];
        detail::root_words(pub_inputs(), pub);
        const cstark_tx_witness w = m_.view();
        check(cstark_tx_witness_upload(ctx_.raw(), &w));
        return detail::validate_built(ctx_, CSTARK_AIR_MERKLE_UPDATE, 65, m_.len() * 512, w.merkle_depth, pub, want_cycles, want_frame,
                                      [&](uint64_t *d) { return cstark_merkle_build_trace(ctx_.raw(), d); });
    }

  private:
    ProofOptions options_;
    TransactionMetadata m_;
    Context &ctx_;
};
// range::RangeProofExample (src/range/mod.rs:28-110)
class RangeProofExample {
  public:
    RangeProofExample(const ProofOptions &options, BaseElement number, Context &ctx) : options_(options), number_(number), ctx_(ctx) {}
    std::vector<uint8_t> prove() { return detail::air_prove(ctx_, CSTARK_AIR_RANGE, options_, number_, 64); }
    // src/range/mod.rs:103-110: throws VerifierError on rejection
    void verify(const std::vector<uint8_t> &proof) const {
        const uint64_t pub[14] = {number_};
        detail::air_verify(ctx_, CSTARK_AIR_RANGE, proof, pub);
    }
    std::vector<uint8_t> convert(const std::vector<uint8_t> &proof, uint32_t form = CSTARK_FORM_COMPACT) const {
        const uint64_t pub[14] = {number_};
        return detail::air_convert(ctx_, CSTARK_AIR_RANGE, proof, pub, form);
    }
    TraceReport validate(bool want_cycles = false, bool want_frame = false) const {
        const uint64_t pub[14] = {number_};
        return detail::validate_built(ctx_, CSTARK_AIR_RANGE, 2, 64, 0, pub, want_cycles, want_frame,
                                      [&](uint64_t *d) { return cstark_range_build_trace(ctx_.raw(), number_, d); });
    }

  private:
    ProofOptions options_;
    BaseElement number_;
    Context &ctx_;
};
// The loop of benches/range.rs:15-37 in one call: one 64-row range proof per number (cstark_range_prove_batch), each byte-identical to
// RangeProofExample(options, number, ctx).prove()
inline std::vector<std::vector<uint8_t>> prove_range_batch(const ProofOptions &options, const std::vector<BaseElement> &numbers, Context &ctx) {
    const cstark_options o = options.raw();
    const size_t stride = cstark_tx_proof_size_bound(1, &o);
    std::vector<uint8_t> buf(stride * numbers.size());
    std::vector<size_t> lens(numbers.size());
    check(cstark_range_prove_batch(ctx.raw(), &o, numbers.data(), (uint32_t)numbers.size(), buf.data(), stride, lens.data()));
    std::vector<std::vector<uint8_t>> out(numbers.size());
    for (size_t t = 0; t < numbers.size(); t++) out[t].assign(buf.begin() + t * stride, buf.begin() + t * stride + lens[t]);
    return out;
}
// RescueExample of benches/rescue.rs:25-102: a chain of chain_length Rescue hashes from the bench's seed 42..48; the public inputs (seed
// and result) are read from the trace inside the prover, as RescueProver::get_pub_inputs does (:331-354)
class RescueExample {
  public:
    RescueExample(size_t chain_length, const ProofOptions &options, Context &ctx) : options_(options), chain_length_(chain_length), ctx_(ctx) {
        if (chain_length < 8 || (chain_length & (chain_length - 1))) throw Error(CSTARK_ERR_INVALID_ARG, "chain length must a power of 2"); // :34-37
        const unsigned __int128 p = ((unsigned __int128)1 << 62) + ((unsigned __int128)1 << 56) + ((unsigned __int128)1 << 55) + 1;
        for (int i = 0; i < 7; i++) seed[i] = (BaseElement)((((unsigned __int128)(42 + i)) << 64) % p); // BaseElement::from(42u8 + i): memory form, R = 2^64
    }
    std::vector<uint8_t> prove() {
        const cstark_options o = options_.raw();
        std::vector<uint8_t> proof(2 * cstark_tx_proof_size_bound((uint32_t)((chain_length_ + 127) / 128), &o));
        size_t len = 0;
        check(cstark_rescue_prove(ctx_.raw(), &o, seed, (uint32_t)chain_length_, proof.data(), proof.size(), &len));
        proof.resize(len);
        return proof;
    }
    // the chain's result: the rate half of the last row of its trace (RescueProver::get_pub_inputs :331-354), built on the device the
    // first time it is asked for
    std::array<BaseElement, 7> result() const {
        if (have_result_) return result_;
        const size_t n = 8 * chain_length_;
        void *d_trace = nullptr;
        check(cstark_malloc(ctx_.raw(), 14 * n * 8, &d_trace));
        std::array<BaseElement, 7> r{};
        int rc = cstark_rescue_chain_build_trace(ctx_.raw(), seed, (uint32_t)chain_length_, (uint64_t *)d_trace);
        for (int i = 0; i < 7 && rc == CSTARK_OK; i++) rc = cstark_memcpy_d2h(ctx_.raw(), &r[i], (const uint64_t *)d_trace + (size_t)i * n + n - 1, 8);
        cstark_free(ctx_.raw(), d_trace);
        check(rc);
        result_ = r;
        have_result_ = true;
        return r;
    }
    // benches/rescue.rs:88-94: throws VerifierError on rejection
    void verify(const std::vector<uint8_t> &proof) const {
        const std::array<BaseElement, 7> r = result();
        uint64_t pub[14];
        for (int k = 0; k < 7; k++) { pub[k] = seed[k]; pub[7 + k] = r[k]; }
        detail::air_verify(ctx_, CSTARK_AIR_RESCUE_CHAIN, proof, pub);
    }
    std::vector<uint8_t> convert(const std::vector<uint8_t> &proof, uint32_t form = CSTARK_FORM_COMPACT) const {
        const std::array<BaseElement, 7> r = result();
        uint64_t pub[14];
        for (int k = 0; k < 7; k++) { pub[k] = seed[k]; pub[7 + k] = r[k]; }
        return detail::air_convert(ctx_, CSTARK_AIR_RESCUE_CHAIN, proof, pub, form);
    }
    TraceReport validate(bool want_cycles = false, bool want_frame = false) const {
        const std::array<BaseElement, 7> r = result();
        uint64_t pub[14];
        for (int k = 0; k < 7; k++) { pub[k] = seed[k]; pub[7 + k] = r[k]; }
        return detail::validate_built(ctx_, CSTARK_AIR_RESCUE_CHAIN, 14, 8 * chain_length_, 0, pub, want_cycles, want_frame,
                                      [&](uint64_t *d) { return cstark_rescue_chain_build_trace(ctx_.raw(), seed, (uint32_t)chain_length_, d); });
    }
    BaseElement seed[7];

  private:
    ProofOptions options_;
    size_t chain_length_;
    mutable std::array<BaseElement, 7> result_{};
    mutable bool have_result_ = false;
    Context &ctx_;
};
// verify_signature (src/schnorr/mod.rs:220-245) on the device for every signature: messages [n][28], sig_rx [n][6], sig_s [n][32] ->
// one cstark_sig_verdict each (CSTARK_SIG_VALID = 0); rx_out (optional): the affine x of s*G + h*P, [n][6].  A resident witness is
// not touched.
inline std::vector<uint8_t> schnorr_check(Context &ctx, const std::vector<BaseElement> &messages, const std::vector<BaseElement> &sig_rx,
                                          const std::vector<uint8_t> &sig_s, std::vector<BaseElement> *rx_out = nullptr) {
    const size_t n = messages.size() / 28;
    if (n == 0 || messages.size() != 28 * n || sig_rx.size() != 6 * n || sig_s.size() != 32 * n)
        throw Error(CSTARK_ERR_INVALID_ARG, "signature vectors are not of equal length");
    std::vector<uint8_t> verdicts(n);
    if (rx_out) rx_out->resize(6 * n);
    check(cstark_schnorr_check_signatures(ctx.raw(), (uint32_t)n, messages.data(), sig_rx.data(), sig_s.data(), verdicts.data(),
                                          rx_out ? rx_out->data() : nullptr));
    return verdicts;
}
// ---- signing with small integer keys, 1 .. CSTARK_SIG_MAX_SECRET (see "signing" in cstark.h): a signer for building batches, tests and
// benchmarks.  It is not a wallet.
// secrets[i] * G -> [n][12] affine (x, y): words 0..11 of an account and of a Schnorr message
inline std::vector<std::array<BaseElement, 12>> schnorr_public_keys(Context &ctx, const std::vector<uint64_t> &secrets) {
    if (secrets.empty()) throw Error(CSTARK_ERR_INVALID_ARG, "no secret");
    std::vector<std::array<BaseElement, 12>> keys(secrets.size());
    check(cstark_schnorr_public_keys(ctx.raw(), (uint32_t)secrets.size(), secrets.data(), keys[0].data()));
    return keys;
}
struct Signatures {
    std::vector<BaseElement> sig_rx;  // [n][6]
    std::vector<uint8_t> sig_s;       // [n][32]
    std::vector<uint8_t> status;      // [n] cstark_sign_status
    std::vector<uint32_t> attempts;   // [n], schnorr_sign only: index of the accepted attempt + 1
};
// one attempt per message with the caller's nonce ([n][5] little-endian limbs, below 2^264); every output is defined whatever the status
inline Signatures schnorr_sign_nonces(Context &ctx, const std::vector<BaseElement> &messages, const std::vector<uint64_t> &secrets,
                                      const std::vector<uint64_t> &nonces) {
    const size_t n = secrets.size();
    if (n == 0 || messages.size() != 28 * n || nonces.size() != 5 * n) throw Error(CSTARK_ERR_INVALID_ARG, "signing vectors are not of equal length");
    Signatures s{std::vector<BaseElement>(6 * n), std::vector<uint8_t>(32 * n), std::vector<uint8_t>(n), {}};
    check(cstark_schnorr_sign_nonces(ctx.raw(), (uint32_t)n, messages.data(), secrets.data(), nonces.data(), s.sig_rx.data(), s.sig_s.data(), s.status.data()));
    return s;
}
// the seeded signer: the first accepted attempt of every signature's own nonce stream; status CSTARK_SIGN_EXHAUSTED (zero outputs)
// where none of max_attempts is accepted
inline Signatures schnorr_sign(Context &ctx, const std::vector<BaseElement> &messages, const std::vector<uint64_t> &secrets, uint64_t seed = 0,
                               uint32_t max_attempts = 256) {
    const size_t n = secrets.size();
    if (n == 0 || messages.size() != 28 * n) throw Error(CSTARK_ERR_INVALID_ARG, "signing vectors are not of equal length");
    Signatures s{std::vector<BaseElement>(6 * n), std::vector<uint8_t>(32 * n), std::vector<uint8_t>(n), std::vector<uint32_t>(n)};
    check(cstark_schnorr_sign(ctx.raw(), (uint32_t)n, messages.data(), secrets.data(), seed, max_attempts, s.sig_rx.data(), s.sig_s.data(), s.attempts.data(),
                              s.status.data()));
    return s;
}
// schnorr::SchnorrExample (src/schnorr/mod.rs:52-186)
class SchnorrExample {
  public:
    SchnorrExample(const ProofOptions &options, size_t num_signatures, Context &ctx, uint64_t seed = 0x5EED)
        : options_(options), messages(num_signatures * 28), sig_rx(num_signatures * 6), sig_s(num_signatures * 32), ctx_(ctx) {
        check(cstark_schnorr_witness_generate((uint32_t)num_signatures, seed, messages.data(), sig_rx.data(), sig_s.data()));
    }
    std::vector<uint8_t> prove() {
        const uint32_t n = (uint32_t)(messages.size() / 28);
        check(cstark_schnorr_witness_upload(ctx_.raw(), n, messages.data(), sig_rx.data(), sig_s.data()));
        return detail::air_prove(ctx_, CSTARK_AIR_SCHNORR, options_, 0, (size_t)n * 512);
    }
    // verify_signature for every signature held here: one cstark_sig_verdict each
    std::vector<uint8_t> check_signatures() const { return schnorr_check(ctx_, messages, sig_rx, sig_s); }
    // src/schnorr/mod.rs:175-186 through cstark_schnorr_verify: the statement is every message and signature held here; throws
    // VerifierError on rejection
    void verify(const std::vector<uint8_t> &proof) const {
        const cstark_schnorr_statement st{(uint32_t)(messages.size() / 28), messages.data(), sig_rx.data(), sig_s.data()};
        const uint8_t *ptr = proof.data();
        const size_t len = proof.size();
        int32_t v = -1;
        check(cstark_schnorr_verify(ctx_.raw(), 1, &ptr, &len, &st, nullptr, &v));
        if (v != CSTARK_PROOF_OK) throw VerifierError(v);
    }
    std::vector<uint8_t> convert(const std::vector<uint8_t> &proof, uint32_t form = CSTARK_FORM_COMPACT) const {
        const cstark_schnorr_statement st{(uint32_t)(messages.size() / 28), messages.data(), sig_rx.data(), sig_s.data()};
        return detail::converted_or_throw(schnorr_convert_batch(ctx_, {proof}, {st}, form));
    }
    // the trace of the signatures held here against the transitions and the 61 assertions: a forged signature is the failing boundary
    // entry at the last row of its block
    TraceReport validate(bool want_cycles = false, bool want_frame = false) const {
        const uint32_t n = (uint32_t)(messages.size() / 28);
        check(cstark_schnorr_witness_upload(ctx_.raw(), n, messages.data(), sig_rx.data(), sig_s.data()));
        return detail::validate_built(ctx_, CSTARK_AIR_SCHNORR, 56, (size_t)n * 512, 0, sig_rx.data(), want_cycles, want_frame,
                                      [&](uint64_t *d) { return cstark_schnorr_build_trace(ctx_.raw(), d); });
    }
    ProofOptions options_;
    std::vector<BaseElement> messages, sig_rx;
    std::vector<uint8_t> sig_s;

  private:
    Context &ctx_;
};

} // namespace cstark
#endif // CSTARK_HPP
