// Whole-proof orchestrator: cstark_tx_prove = TransactionExample::prove (/root/reference/src/lib.rs:116-141), i.e.
// TransactionProver::build_trace followed by the engine's Prover::prove, as one C call.  Every stage runs on the GPU through
// the stage entry points of capi.hip; the host side here is only the Fiat-Shamir channel (a few hundred BLAKE3 calls), the
// FRI layer loop, and the serialisation of the openings.
//
// Protocol [UPSTREAM-RECALL winterfell v0.3, parity unpinned -- the engine is absent from the reference tree]:
//   coin      seed = H(context || public inputs); reseed(d) = H(seed || d); reseed_int(v) = H(seed || v_le64);
//             draw: counter += 1, H(seed || counter_le64), first 8 bytes LE as integer, rejected unless < p
//   order     what enters the coin and what is drawn after it, step by step: transcript.h (the host channel calls those steps;
//             channel.hip states the same order for the device-side channel)
//   FRI       folding factor f = 4, 8 or 16, layers while the domain exceeds fri_max_remainder; layer rows are the f evaluations
//             { e[i + t N/f] } that fold into position i
//   domains   blowup factor b = 2, 4, 8 or 16, at least the AIR's constraint-evaluation blowup ce (8 / 4 / 8 / 2).  b > ce: the trace
//             table is kept in BLOCK ORDER (blake3.h, lde_coset_slot) -- b / ce blocks of ce cosets, block 0 = the constraint-
//             evaluation domain -- so the evaluators always read a plain [ce][width][n] table; commitment leaves, query positions and
//             the proof bytes are in natural order (leaf b j + k)
// The byte layout of the proof is this library's own (documented in include/cstark.h, written and parsed by proof_layout.h); the tests
// check it with a restated verifier.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <new>
#include <chrono>
#include <thread>
#include <vector>
#include "../../include/cstark.h"
#include "ctx.h"
#include "blake3.h"
#include "channel.h"
#include "deep.h"
#include "ext.h"
#include "range_batch.h"
#include "hostblake3.h"
#include "keccak.cuh"
#include "air_tx_host.h"
#include "hostfield.h"
#include "coin.h"
#include "proof_layout.h"
#include "transcript.h"

namespace cs {

enum { PROVE_EVENTS = CSTARK_PROVE_NUM_STAGES + 1 };

struct ProveArena {
    int air = -1;
    unsigned log_n = 0, log_b = 0, log_f = 0;
    uint64_t *trace = nullptr, *coeffs = nullptr, *lde = nullptr, *combined = nullptr, *ccoef = nullptr, *clde = nullptr, *deep = nullptr;
    std::vector<void *> extra; // per-AIR buffers (materialised transition evaluations, SchnorrAir's public columns)
    std::vector<size_t> extra_bytes; // allocated size of every slot of `extra`
    uint8_t *tnodes = nullptr, *cnodes = nullptr;
    std::vector<uint64_t *> layer;   // FRI layer evaluations (layer[0] = DEEP composition in natural order), last = remainder
    std::vector<uint8_t *> lnodes;   // FRI layer trees
    uint32_t *d_pos = nullptr;
    uint64_t *d_pub = nullptr;    // [16] the public inputs read from the trace (first / last row of seven registers)
    uint64_t *d_shifts = nullptr; // [b] g w_(b n)^k: the coset offsets of the LDE domain (k_deep)
    uint8_t *d_open = nullptr;
    uint64_t *h_pub = nullptr; // pinned
    uint8_t *h_open = nullptr; // pinned: the openings land here (a pageable destination is staged by the runtime: ~60 us for 0.5 MB)
    size_t h_open_bytes = 0;
    size_t open_bytes = 0;
    hipEvent_t ev[PROVE_EVENTS] = {};
    bool timed = false;
    uint32_t channel = CSTARK_CHANNEL_HOST; // which Fiat-Shamir channel the last proof used (valid with `timed`: cstark_prove_channel)
    std::vector<void *> owned;
    struct ProofRun *run = nullptr; // a proof in progress between the phases of the sharded entry points (cstark_tx_shard_*)
};
void proof_run_free(struct ProofRun *r);

void prove_arena_free(ProveArena *a) {
    if (!a) return;
    proof_run_free(a->run);
    for (void *p : a->owned) (void)hipFree(p);
    if (a->h_pub) (void)hipHostFree(a->h_pub);
    if (a->h_open) (void)hipHostFree(a->h_open);
    for (hipEvent_t e : a->ev) if (e) (void)hipEventDestroy(e);
    delete a;
}
int grind_nonce(cstark_ctx *c, ProveArena *a, const Coin &coin, unsigned bits, uint64_t *nonce_out);

namespace {

__global__ void k_gather_rows(const uint64_t *__restrict__ lde, uint32_t width, uint32_t log_n, uint32_t log_b, const uint32_t *__restrict__ pos,
                              uint64_t *__restrict__ out) {
    const uint32_t q = blockIdx.x, i = pos[q], k = i & ((1u << log_b) - 1), j = i >> log_b;
    for (uint32_t c = threadIdx.x; c < width; c += blockDim.x) out[(size_t)q * width + c] = lde[(((size_t)k * width + c) << log_n) + j];
}
// the same for a table that holds cosets [k0, k0 + nk) only, each row followed by the bottom log2(nk) siblings of its authentication path
// from the rank's own subtree heap `sub` (leaf nk j + (k - k0) at nk n + ...; phase_commit): [nq][width + 4 log_nk] words.  Rows of
// other cosets are written as zeros (the owners' rows are summed in).
__global__ void k_gather_rows_window(const uint64_t *__restrict__ lde, uint32_t width, uint32_t log_n, uint32_t log_b, uint32_t k0, uint32_t nk,
                                     const uint32_t *__restrict__ pos, uint64_t *__restrict__ out, const uint64_t *__restrict__ sub, uint32_t log_nk) {
    const uint32_t q = blockIdx.x, i = pos[q], k = i & ((1u << log_b) - 1), j = i >> log_b, stride = width + 4 * log_nk;
    const bool mine = k >= k0 && k < k0 + nk;
    for (uint32_t c = threadIdx.x; c < width; c += blockDim.x)
        out[(size_t)q * stride + c] = mine ? lde[(((size_t)(k - k0) * width + c) << log_n) + j] : 0;
    const size_t leaf = ((size_t)nk << log_n) + ((size_t)j << log_nk) + (k - k0);
    for (uint32_t t = threadIdx.x; t < 4 * log_nk; t += blockDim.x)
        out[(size_t)q * stride + width + t] = mine ? sub[4 * ((leaf >> (t >> 2)) ^ 1) + (t & 3)] : 0;
}
// the summed rows of the ranks [nq][width + 4 log_nk] -> the opened rows [nq][width] and levels [0, log_nk) of the authentication paths
// [nq][log_leaves][32 bytes] (the levels above come from the upper tree: GatherJob::lvl0)
__global__ void k_split_shard_rows(const uint64_t *__restrict__ rows, uint32_t width, uint32_t log_nk, uint32_t log_leaves, uint64_t *__restrict__ out_rows,
                                   uint64_t *__restrict__ out_paths) {
    const uint32_t q = blockIdx.x, stride = width + 4 * log_nk;
    for (uint32_t c = threadIdx.x; c < width; c += blockDim.x) out_rows[(size_t)q * width + c] = rows[(size_t)q * stride + c];
    for (uint32_t t = threadIdx.x; t < 4 * log_nk; t += blockDim.x) out_paths[(size_t)q * log_leaves * 4 + t] = rows[(size_t)q * stride + width + t];
}
// leaf digests [b][n] (coset-major, as the ranks' all-gather delivers them) -> natural order: leaf b*j + k = digest (k, j)
__global__ void k_interleave_leaves(const uint4 *__restrict__ in, uint4 *__restrict__ out, size_t n, uint32_t log_b) {
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; // one 16-byte half of a digest
    if (t >= (n << (log_b + 1))) return;
    const size_t i = t >> 1, half = t & 1, k = i & ((1u << log_b) - 1), j = i >> log_b;
    out[t] = in[2 * (k * n + j) + half];
}
// authentication path of leaf pos[q]: siblings from the leaf level upwards
__global__ void k_gather_paths(const uint4 *__restrict__ nodes, uint32_t log_leaves, const uint32_t *__restrict__ pos, uint4 *__restrict__ out) {
    const uint32_t q = blockIdx.x;
    for (uint32_t t = threadIdx.x; t < 2 * log_leaves; t += blockDim.x) {
        const uint32_t lvl = t >> 1, half = t & 1;
        const size_t node = ((((size_t)1 << log_leaves) + pos[q]) >> lvl) ^ 1;
        out[((size_t)q * log_leaves + lvl) * 2 + half] = nodes[2 * node + half];
    }
}
// All opening gathers of a proof in ONE launch (they were twenty launches of a few microseconds each, 0.14 ms of launch latency):
// job = blockIdx.y, query = blockIdx.x.  kind 0: row pos[q] of a coset-major table (as k_gather_rows); kind 1: authentication path
// of leaf pos[q] (as k_gather_paths; a = log2 of the leaf count).
struct GatherJob { const void *src; void *out; const uint32_t *pos; uint32_t kind, a, log_n, log_b, count, log_s; const uint32_t *dcount; uint32_t lvl0; };
// log_s: block order of the table's cosets (blake3.h); dcount != null: the number of positions is read from the device (at most `count`:
// the device-side channel folds the query positions itself, channel.hip); lvl0 (paths): the levels below it are left alone (sharded
// proofs: they come from the rank that owns the leaf)
constexpr int MAX_GATHER_JOBS = 32;
struct GatherBatch { GatherJob job[MAX_GATHER_JOBS]; };
__global__ void k_gather_batch(GatherBatch b) {
    const GatherJob g = b.job[blockIdx.y];
    const uint32_t q = blockIdx.x;
    if (q >= (g.dcount ? *g.dcount : g.count)) return;
    if (g.kind == 0) {
        const uint64_t *lde = (const uint64_t *)g.src;
        uint64_t *out = (uint64_t *)g.out;
        const uint32_t width = g.a, i = g.pos[q], k = lde_coset_slot(i & ((1u << g.log_b) - 1), g.log_b, g.log_s), j = i >> g.log_b;
        for (uint32_t c = threadIdx.x; c < width; c += blockDim.x) out[(size_t)q * width + c] = lde[(((size_t)k * width + c) << g.log_n) + j];
    } else {
        const uint4 *nodes = (const uint4 *)g.src;
        uint4 *out = (uint4 *)g.out;
        const uint32_t log_leaves = g.a;
        for (uint32_t t = threadIdx.x + 2 * g.lvl0; t < 2 * log_leaves; t += blockDim.x) {
            const uint32_t lvl = t >> 1, half = t & 1;
            const size_t node = ((((size_t)1 << log_leaves) + g.pos[q]) >> lvl) ^ 1;
            out[((size_t)q * log_leaves + lvl) * 2 + half] = nodes[2 * node + half];
        }
    }
}
struct GatherList {
    GatherBatch b{};
    int n = 0;
    uint32_t max_count = 0;
    void rows(const uint64_t *lde, uint32_t width, uint32_t log_n, uint32_t log_b, const uint32_t *pos, void *out, uint32_t count, uint32_t log_s = 0,
              const uint32_t *dcount = nullptr) {
        b.job[n++] = GatherJob{lde, out, pos, 0u, width, log_n, log_b, count, log_s, dcount, 0u};
        if (count > max_count) max_count = count;
    }
    void paths(const uint8_t *nodes, uint32_t log_leaves, const uint32_t *pos, void *out, uint32_t count, const uint32_t *dcount = nullptr, uint32_t lvl0 = 0) {
        b.job[n++] = GatherJob{nodes, out, pos, 1u, log_leaves, 0u, 0u, count, 0u, dcount, lvl0};
        if (count > max_count) max_count = count;
    }
    hipError_t launch(hipStream_t st) {
        if (n == 0 || max_count == 0) return hipSuccess;
        k_gather_batch<<<dim3(max_count, (unsigned)n), 128, 0, st>>>(b);
        return hipGetLastError();
    }
};
// first / last row of seven registers from reg0: 58 = PREV_TREE_ROOT_POS (src/prover.rs:106-129), 0 = the hash chain (benches/rescue.rs:331-354)
__global__ void k_gather_pub(const uint64_t *__restrict__ trace, size_t n, uint64_t *__restrict__ out, uint32_t reg0) {
    const uint32_t t = threadIdx.x;
    if (t < 14) out[t] = trace[(size_t)(reg0 + (t % 7)) * n + (t < 7 ? 0 : n - 1)];
}

template <class T>
int dev_alloc(ProveArena *a, T **p, size_t bytes) {
    HIP_TRY(hipMalloc((void **)p, bytes));
    a->owned.push_back(*p);
    return CSTARK_OK;
}

// Slot `slot` of the arena's per-AIR buffers with at least `bytes` bytes.  A slot outlives the proof that created it (the arena is
// reused across proofs with other query counts, field extensions or AIR options), so its size is recorded and a larger request
// replaces the allocation once the stream has drained.
template <class T>
int arena_extra(cstark_ctx *c, ProveArena *a, size_t slot, T **p, size_t bytes) {
    if (a->extra.size() <= slot) { a->extra.resize(slot + 1, nullptr); a->extra_bytes.resize(slot + 1, 0); }
    if (a->extra[slot] && a->extra_bytes[slot] < bytes) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        void *old = a->extra[slot];
        a->extra[slot] = nullptr; a->extra_bytes[slot] = 0;
        a->owned.erase(std::find(a->owned.begin(), a->owned.end(), old));
        HIP_TRY(hipFree(old));
    }
    if (!a->extra[slot]) {
        void *q;
        HIP_TRY(hipMalloc(&q, bytes));
        a->owned.push_back(q); a->extra[slot] = q; a->extra_bytes[slot] = bytes;
    }
    *p = (T *)a->extra[slot];
    return CSTARK_OK;
}

unsigned ceil_log2(uint64_t x) { unsigned l = 0; while ((1ull << l) < x) l++; return l; }

// What differs between the AIRs: how the trace is built, what goes into the channel seed, and how the combined constraint
// evaluations are produced from the extended trace and the drawn coefficients.
struct AirJob {
    int air = 0;
    uint32_t width = 0, log_n = 0, log_ce = 0, n_constraints = 0, n_assertions = 0, item = 0; // item: Merkle depth / signature count / 0
    std::vector<uint64_t> pub;      // public-input elements (memory form), appended to the seed in canonical form
    std::vector<uint8_t> pub_bytes; // further public material appended verbatim (Schnorr: the s halves of the signatures)
    int (*build)(cstark_ctx *, ProveArena *, AirJob &) = nullptr;
    // merged constraint evaluations [b][n] for ONE set of (base-field) coefficients -> out
    int (*combine)(cstark_ctx *, ProveArena *, AirJob &, const uint64_t *ta, const uint64_t *tb, const uint64_t *ba, const uint64_t *bb, uint64_t *out) = nullptr;
    // optional: the merged evaluations of m coefficient sets in one pass over the frame (extension proofs); falls back to m calls
    int (*combine_sets)(cstark_ctx *, ProveArena *, AirJob &, unsigned m, const uint64_t *const *ta, const uint64_t *const *tb, const uint64_t *const *ba,
                        const uint64_t *const *bb, uint64_t *const *outs) = nullptr;
    // Optional: the order in which the trace columns become complete when build() returns with parts of the trace still being
    // written on internal streams (TransactionAir).  The prover interpolates and extends batch after batch, waiting for a batch's
    // events first; empty = all columns at once.
    // block != 0: a step batch -- every column is constant over blocks of `block` rows (taken to cstark_step_columns where the proof's shape allows),
    // or, with split != 0, over rows [0, split) and [split, block) of every block (cstark_step2_columns)
    struct ColumnBatch { uint32_t col0, ncols; hipEvent_t wait[2]; uint32_t block = 0, split = 0; };
    std::vector<ColumnBatch> batches;
    const uint64_t *pub_staging = nullptr; // pinned host copy of the public inputs, valid once every batch has been waited for
    bool public_ready = false;      // SchnorrAir: the extended public-input columns of this proof are in the arena
    bool evals_ready = false;       // sub-AIRs: the materialised transition evaluations of this proof are already in the arena
    uint32_t k0 = 0, nk = 8;        // sharded proofs (blowup 8): the LDE cosets this GPU owns
    bool sharded = false;
    bool dev_channel = false;       // the Fiat-Shamir channel runs on the device (prove_core_dev): the host never reads the public inputs
    const uint64_t *d_coefs = nullptr;   // ... and the coefficients are drawn there: alpha[115] | beta[115] | b_alpha[na] | b_beta[na] (device)
    const uint64_t *d_avalues = nullptr; // the assertion values on the device (null: the AIR's built-in constants)
    uint32_t log_b = 3;             // log2 of the blowup factor; the trace table holds its cosets in block order when log_b > log_ce
    uint64_t seed[7] = {};          // RescueAir
    uint64_t number = 0;            // RangeProofAir
    const uint64_t *bits = nullptr; // RangeProofAir, long form: the n/64 words of the value (host)
};

// A sharded proof in progress (cstark_tx_shard_*) lives in the arena's buffers between its phases.  Anything else that takes the arena --
// a whole proof on the same context, a new sharded proof, a replacement of the arena -- ends it: the later phases then fail with "phase
// called out of order" instead of building a proof from foreign buffers.
void drop_run(ProveArena *a) {
    if (a && a->run) { proof_run_free(a->run); a->run = nullptr; }
}

int get_arena(cstark_ctx *c, const AirJob &job, unsigned log_b, unsigned log_f, unsigned n_layers, size_t nq, ProveArena **out) {
    drop_run(c->arena);
    if (c->arena && c->arena->air == job.air && c->arena->log_n == job.log_n && c->arena->log_b == log_b && c->arena->log_f == log_f &&
        c->arena->layer.size() == n_layers + 1 && c->arena->open_bytes >= nq) { *out = c->arena; return CSTARK_OK; }
    if (c->arena) { HIP_TRY(hipStreamSynchronize(c->stream)); prove_arena_free(c->arena); c->arena = nullptr; }
    ProveArena *a = new (std::nothrow) ProveArena();
    if (!a) return fail(CSTARK_ERR_OOM, "host allocation failed");
    c->arena = a; // owned by the context from here on (freed with it, also after a partial failure)
    a->air = job.air; a->log_n = job.log_n; a->log_b = log_b; a->log_f = log_f;
    const size_t n = (size_t)1 << job.log_n, b = (size_t)1 << log_b, N = n * b, W = job.width, ce = (size_t)1 << job.log_ce, f = (size_t)1 << log_f;
    RC_TRY(dev_alloc(a, &a->trace, W * n * 8));
    RC_TRY(dev_alloc(a, &a->coeffs, W * n * 8));
    RC_TRY(dev_alloc(a, &a->lde, W * N * 8));
    RC_TRY(dev_alloc(a, &a->tnodes, 2 * N * 32));
    RC_TRY(dev_alloc(a, &a->combined, N * 8)); // merged evaluations on the constraint-evaluation domain, [ce][n]
    RC_TRY(dev_alloc(a, &a->ccoef, ce * n * 8));
    RC_TRY(dev_alloc(a, &a->clde, b * ce * n * 8)); // [b cosets][ce columns][n]
    RC_TRY(dev_alloc(a, &a->cnodes, 2 * N * 32));
    RC_TRY(dev_alloc(a, &a->deep, N * 8));
    size_t sz = N;
    for (unsigned l = 0; l <= n_layers; l++) {
        uint64_t *e; uint8_t *t = nullptr;
        RC_TRY(dev_alloc(a, &e, sz * 8));
        if (l < n_layers) RC_TRY(dev_alloc(a, &t, 2 * (sz / f) * 32));
        a->layer.push_back(e); a->lnodes.push_back(t);
        sz /= f;
    }
    RC_TRY(dev_alloc(a, &a->d_pos, 4 * 256 * (n_layers + 2)));
    RC_TRY(dev_alloc(a, &a->d_pub, 16 * 8));
    RC_TRY(dev_alloc(a, &a->d_shifts, b * 8));
    {
        std::vector<uint64_t> sh(b);
        const uint64_t wbn = host::root_of_unity(job.log_n + log_b);
        uint64_t v = host::lde_offset();
        for (size_t k = 0; k < b; k++) { sh[k] = v; v = host::mul(v, wbn); }
        HIP_TRY(hipMemcpy(a->d_shifts, sh.data(), b * 8, hipMemcpyHostToDevice)); // once per arena
    }
    // openings: per query a trace row + path, a composition row + path, per layer a row of f + path
    a->open_bytes = nq;
    const size_t log_N = job.log_n + log_b;
    const size_t per_q = W * 8 + ce * 8 + 2 * log_N * 32 + (size_t)n_layers * (f * 8 + log_N * 32);
    RC_TRY(dev_alloc(a, &a->d_open, per_q * nq + 256));
    for (hipEvent_t &e : a->ev) HIP_TRY(hipEventCreate(&e));
    *out = a;
    return CSTARK_OK;
}

// The option values the reference passes (src/lib.rs:78-86; blowup 4 in src/merkle/update/tests.rs:41-52, src/range/tests.rs:87-98 and
// benches/rescue.rs:370-378; -b / -f on the command line, examples/state-transition.rs:33-34, :46-47).  log_ce: the AIR's
// constraint-evaluation blowup -- a blowup factor below it cannot hold the composition polynomial (the engine refuses it too).
int check_options(const cstark_options *opt, unsigned log_ce, unsigned *log_rem_out, unsigned *log_b_out, unsigned *log_f_out) {
    const uint32_t b = opt->blowup_factor, f = opt->fri_folding_factor;
    if (b != 2 && b != 4 && b != 8 && b != 16) return fail(CSTARK_ERR_UNSUPPORTED, "blowup_factor must be 2, 4, 8 or 16");
    if (b < (1u << log_ce)) return fail(CSTARK_ERR_INVALID_ARG, "blowup_factor below the AIR's constraint-evaluation blowup (TransactionAir / SchnorrAir 8, MerkleAir 4, RangeProofAir 2)");
    if (opt->hash_fn > 1) return fail(CSTARK_ERR_UNSUPPORTED, "hash_fn must be Blake3_256 (0) or Sha3_256 (1)");
    if (opt->field_extension > 2) return fail(CSTARK_ERR_INVALID_ARG, "field_extension must be None (0), Quadratic (1) or Cubic (2)");
    if (f != 4 && f != 8 && f != 16) return fail(CSTARK_ERR_UNSUPPORTED, "fri_folding_factor must be 4, 8 or 16");
    *log_b_out = b == 2 ? 1 : b == 4 ? 2 : b == 8 ? 3 : 4;
    *log_f_out = f == 4 ? 2 : f == 8 ? 3 : 4;
    if (opt->num_queries == 0 || opt->num_queries > 128) return fail(CSTARK_ERR_INVALID_ARG, "num_queries must be 1..128");
    if (opt->grinding_factor > 32) return fail(CSTARK_ERR_INVALID_ARG, "grinding_factor must be at most 32");
    unsigned log_rem = 0;
    while ((1u << log_rem) < opt->fri_max_remainder) log_rem++;
    if ((1u << log_rem) != opt->fri_max_remainder || log_rem < 7 || log_rem > 10) return fail(CSTARK_ERR_INVALID_ARG, "fri_max_remainder must be a power of two in 128..1024");
    *log_rem_out = log_rem;
    return CSTARK_OK;
}

// the channel seed (transcript.h), and a job's
using transcript::channel_seed;
using transcript::SEED_PREFIX;
std::vector<uint8_t> channel_seed(const AirJob &job, const cstark_options &opt, unsigned log_rem) {
    return channel_seed(job.width, job.log_n, opt, job.log_b, log_rem, job.pub.data(), job.pub.size(), job.pub_bytes.data(), job.pub_bytes.size());
}

// ---- query stage (host channel): proof of work, the query positions and their folded forms, on the device at a->d_pos --------------------
struct Queries {
    uint64_t nonce = 1;
    uint32_t counts[VMAX_LAYERS] = {}; // distinct folded positions per FRI layer
    std::vector<uint32_t> hpos;        // [1 + n_layers][256]: the drawn positions, then every layer's folded positions
};
// `coin`: after the reseed with the remainder commitment
int query_stage(cstark_ctx *c, ProveArena *a, Coin &coin, const ProofShape &S, Queries &Q) {
    RC_TRY(grind_nonce(c, a, coin, S.opt[2], &Q.nonce));
    Q.hpos.assign(256 * (S.n_layers + 1), 0);
    transcript::draw_queries(coin, S, Q.nonce, Q.hpos.data(), Q.hpos.data() + 256, 256, Q.counts);
    HIP_TRY(hipMemcpyAsync(a->d_pos, Q.hpos.data(), Q.hpos.size() * 4, hipMemcpyHostToDevice, c->stream));
    return CSTARK_OK;
}

// ---- opening stage: every opened row and authentication path gathered into one device block, one copy to the pinned a->h_open ----------
// The block's offsets: the sections in proof order.  counts = null: room for nq positions in every layer (the device-side channel
// knows the counts only on the device).  start / align: the device channel's result block holds more in front and aligns its pieces.
struct OpenBlock { size_t trows, tpaths, crows, cpaths, lrows[VMAX_LAYERS], lpaths[VMAX_LAYERS], bytes; };
OpenBlock open_block(const ProofShape &S, const uint32_t *counts, size_t start = 0, size_t align = 1) {
    OpenBlock O;
    size_t off = start;
    auto take = [&off, align](size_t bytes) { const size_t o = off; off += (bytes + align - 1) / align * align; return o; };
    O.trows = take(trace_row_bytes(S)); O.tpaths = take(path_bytes(S)); O.crows = take(comp_row_bytes(S)); O.cpaths = take(path_bytes(S));
    for (unsigned l = 0; l < S.n_layers; l++) {
        const uint32_t np = counts ? counts[l] : S.nq;
        O.lrows[l] = take(layer_row_bytes(S, np)); O.lpaths[l] = take(layer_path_bytes(S, l, np));
    }
    O.bytes = off;
    return O;
}
int host_open_block(ProveArena *a, size_t bytes) {
    if (a->h_open_bytes < bytes) {
        if (a->h_open) { HIP_TRY(hipHostFree(a->h_open)); a->h_open = nullptr; a->h_open_bytes = 0; }
        HIP_TRY(hipHostMalloc((void **)&a->h_open, bytes, hipHostMallocDefault));
        a->h_open_bytes = bytes;
    }
    return CSTARK_OK;
}
// What the callers' openings differ in: the composition table (S.ce S.m base columns) and the FRI layers (rows of S.f S.m words), the
// block order of the trace table's cosets, trace rows that arrive from the ranks of a sharded proof (with the bottom shard_lvl0 levels
// of their paths), and where the per-layer counts are: host numbers, or device counters dcount[l] with nq slots per layer.
struct OpenSrc {
    const uint64_t *clde; uint64_t *const *layer; unsigned log_s;
    const uint32_t *counts, *dcount;
    const uint64_t *shard_rows; uint32_t shard_lvl0;
    const uint32_t *pos = nullptr; // the positions, 256 slots per layer (null: a->d_pos)
};
// Gathers into d_block at the offsets O (positions: a->d_pos, 256 slots per layer) and enqueues the copy of d_block[0, O.bytes) to a->h_open.
int open_stage(cstark_ctx *c, ProveArena *a, const ProofShape &S, const OpenSrc &src, uint8_t *d_block, const OpenBlock &O) {
    hipStream_t st = c->stream;
    const uint32_t nq = S.nq, W = S.width, *d_pos = src.pos ? src.pos : a->d_pos;
    GatherList gl;
    uint32_t trace_lvl0 = 0;
    if (src.shard_rows) { // sharded: rows and the bottom levels of the paths come from the owning ranks
        trace_lvl0 = src.shard_lvl0;
        k_split_shard_rows<<<nq, 128, 0, st>>>(src.shard_rows, W, trace_lvl0, S.log_N, (uint64_t *)(d_block + O.trows), (uint64_t *)(d_block + O.tpaths));
        HIP_TRY(hipGetLastError());
    } else gl.rows(a->lde, W, S.log_n, S.log_b, d_pos, d_block + O.trows, nq, src.log_s);
    gl.paths(a->tnodes, S.log_N, d_pos, d_block + O.tpaths, nq, nullptr, trace_lvl0);
    gl.rows(src.clde, S.ce * S.m, S.log_n, S.log_b, d_pos, d_block + O.crows, nq);
    gl.paths(a->cnodes, S.log_N, d_pos, d_block + O.cpaths, nq);
    for (unsigned l = 0; l < S.n_layers; l++) {
        const uint32_t np = src.counts ? src.counts[l] : nq, lr = layer_log_rows(S, l), *pos = d_pos + 256 * (l + 1), *dc = src.dcount ? src.dcount + l : nullptr;
        gl.rows(src.layer[l], S.f * S.m, lr, 0, pos, d_block + O.lrows[l], np, 0, dc);
        gl.paths(a->lnodes[l], lr, pos, d_block + O.lpaths[l], np, dc);
    }
    HIP_TRY(gl.launch(st));
    RC_TRY(host_open_block(a, O.bytes));
    HIP_TRY(hipMemcpyAsync(a->h_open, d_block, O.bytes, hipMemcpyDeviceToHost, st));
    return CSTARK_OK;
}

// Extension of columns [col0, col0 + ncols) of the trace: the cosets [k0, k0 + nk) of a sharded proof, or all of them -- in block
// order when the blowup factor exceeds the AIR's constraint-evaluation blowup: block r = the blowup-ce extension with offset g w_(b n)^r
int lde_trace(cstark_ctx *c, ProveArena *a, const AirJob &job, uint32_t col0, uint32_t ncols) {
    const uint32_t W = job.width, log_n = job.log_n, log_b = job.log_b;
    if (job.sharded || log_b <= job.log_ce) return lde_column_range(c, a->coeffs, a->lde, W, col0, ncols, log_n, log_b, host::lde_offset(), job.k0, job.nk);
    const size_t n = (size_t)1 << log_n, ce = (size_t)1 << job.log_ce;
    const uint64_t wbn = host::root_of_unity(log_n + log_b);
    uint64_t offset = host::lde_offset();
    for (uint32_t r = 0; r < (1u << (log_b - job.log_ce)); r++) {
        RC_TRY(lde_column_range(c, a->coeffs, a->lde + (size_t)r * ce * W * n, W, col0, ncols, log_n, job.log_ce, offset, 0, (uint32_t)ce));
        offset = host::mul(offset, wbn);
    }
    return CSTARK_OK;
}
// Interpolation and extension of the trace columns (cosets [job.k0, job.k0 + job.nk)); records the two stage events (after the
// interpolation, after the extension).  With column batches (AirJob::batches) the complete columns go first -- interpolated AND
// extended while the internal streams still write the later ones -- so the "interpolate" stage time then also holds the extension
// of the earlier batches.
int commit_columns(cstark_ctx *c, ProveArena *a, AirJob &job, hipStream_t st, int &evi) {
    const uint32_t W = job.width, log_n = job.log_n;
    const size_t n = (size_t)1 << log_n;
    if (job.batches.empty()) {
        RC_TRY(cstark_interpolate_columns(c, a->trace, a->coeffs, W, log_n));
        HIP_TRY(hipEventRecord(a->ev[evi++], st));
        RC_TRY(lde_trace(c, a, job, 0, W));
        HIP_TRY(hipEventRecord(a->ev[evi++], st));
        return CSTARK_OK;
    }
    for (size_t i = 0; i < job.batches.size(); i++) {
        const AirJob::ColumnBatch &cb = job.batches[i];
        for (hipEvent_t e : cb.wait)
            if (e) HIP_TRY(hipStreamWaitEvent(st, e, 0));
        // a step batch of an unsharded proof whose extension is the single-offset form: coefficients and cosets without full-length transforms
        const bool step = cb.block != 0 && !job.sharded && job.log_b <= job.log_ce;
        if (!step) RC_TRY(cstark_interpolate_columns(c, a->trace + (size_t)cb.col0 * n, a->coeffs + (size_t)cb.col0 * n, cb.ncols, log_n));
        if (i + 1 == job.batches.size()) HIP_TRY(hipEventRecord(a->ev[evi++], st));
        if (step) RC_TRY(step_column_range(c, a->trace, a->coeffs, a->lde, W, cb.col0, cb.ncols, log_n, cb.block, cb.split, job.log_b, host::lde_offset(), job.k0, job.nk));
        else RC_TRY(lde_trace(c, a, job, cb.col0, cb.ncols));
    }
    HIP_TRY(hipEventRecord(a->ev[evi++], st));
    return CSTARK_OK;
}

} // namespace

// Proof of work: the smallest nonce >= 1 whose digest with the seed has `bits` low zero bits (0 bits: nonce 1).  A search of 2^bits
// hashes in sequence on the host (transcript::host_nonce) costs 10 ms at 16 bits (43 ms with the Sha3 coin); from 12 bits on the GPU searches 2^22 nonces per launch --
// chunks in increasing order and an atomic minimum inside a chunk, so the nonce is the one the sequential search finds.
// CSTARK_GRIND_DEVICE=0: always on the host.
int grind_nonce(cstark_ctx *c, ProveArena *a, const Coin &coin, unsigned bits, uint64_t *nonce_out) {
    static const bool dev_env = [] { const char *e = getenv("CSTARK_GRIND_DEVICE"); return !e || atoi(e) != 0; }();
    if (bits == 0 || !dev_env || bits < 12) {
        *nonce_out = transcript::host_nonce(coin, bits);
        return CSTARK_OK;
    }
    unsigned long long *d_found; // [found | seed (Sha3 coin: read from device memory)]
    RC_TRY(arena_extra(c, a, 42, &d_found, 64));
    return grind_search(c->stream, d_found, coin.seed, coin.hash_fn, bits, (uint64_t)1 << 22, nonce_out);
}
// the device search of grind_nonce: chunks of `chunk` nonces from 1 on until one holds a hit (ctx.h)
int grind_search(hipStream_t stream, unsigned long long *d_found, const uint8_t seed[32], uint32_t hash_fn, unsigned bits, uint64_t chunk, uint64_t *nonce_out) {
    if (chunk == 0) return fail(CSTARK_ERR_INVALID_ARG, "proof of work: empty chunk");
    if (hash_fn == 1) {
        HIP_TRY(hipMemcpyAsync(d_found + 1, seed, 32, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(d_found, 0xFF, 8, stream));
    }
    for (uint64_t base = 1;; base += chunk) {
        if (hash_fn == 1) HIP_TRY(cs::grind_batch_chunk_sha3((const uint64_t *)(d_found + 1), 1, base, chunk, bits, d_found, stream));
        else HIP_TRY(cs::grind_chunk(seed, base, chunk, bits, d_found, stream));
        unsigned long long found = 0;
        HIP_TRY(hipMemcpyAsync(&found, d_found, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(cs::stream_wait(stream));
        if (found != ~0ull) { *nonce_out = found; return CSTARK_OK; }
        if (base > ((uint64_t)1 << 44)) return fail(CSTARK_ERR_HIP, "proof of work: no nonce found"); // 2^-(2^12) to get here at 32 bits
    }
}

// Prover::prove for any of the AIRs, as a sequence of phases.  On one GPU (prove_core) they run back to back; the sharded entry points
// (cstark_tx_shard_*: one proof across several GPUs by LDE coset) run them with the ranks' all-gathers in between -- leaf digests after
// `commit`, merged evaluations after `evaluate`, the opened trace rows after `compose`.
// FieldExtension::Quadratic / Cubic (m = 2, 3): base-field trace; everything the coin draws lives in the degree-m extension (ext.hip).
// Coefficients multiply base-field constraint values, so the merged evaluations are the AIR's evaluator applied with m coefficient sets
// (one per component): TransactionAir merges all sets in one pass over the frame, the sub-AIRs merge their materialised evaluations m
// times.  Layout differences of the proof: out-of-domain values are m-tuples, composition rows hold ce m-tuples, FRI rows and the
// remainder are component-major.
struct ProofRun {
    cstark_options opt{};
    AirJob job;
    unsigned log_rem = 0, n_layers = 0, log_b = 3, log_f = 2, m = 1; // m: base-field words of a drawn element (field_extension + 1)
    ProofShape shape{};
    Coin coin;
    uint8_t trace_root[32] = {}, cons_root[32] = {}, rem_commit[32] = {};
    std::vector<uint64_t> ta[3], tb[3], ba[3], bb[3], ood_trace, ood_comp, remainder; // ta .. bb: one coefficient set per component
    std::vector<uint8_t> layer_roots;
    // device buffers (run_buffers): the arena's own for m = 1, slots of its per-AIR list sized for three components otherwise
    uint64_t *comb[3] = {}, *cco[3] = {}; // per component: merged evaluations [ce][n], their column coefficients
    uint64_t *ccoefs = nullptr;           // the m ce coefficient columns of the composition table: column m i + q = component q of column i
    uint64_t *clde = nullptr, *deep = nullptr; // its extension [b][m ce][n]; the DEEP composition [m][b n], coset-major
    std::vector<uint64_t *> layer;        // FRI layer evaluations, rows of m f words (component-major), last = remainder
    uint8_t *d_open = nullptr;
    Queries q;
    int evi = 0, phase = 0; // phase: 1 commit, 2 evaluate, 3 compose done
    bool sharded() const { return job.sharded; }
    unsigned log_s() const { return job.sharded ? 0 : log_b - job.log_ce; } // block order of the trace table's cosets
};
void proof_run_free(ProofRun *r) { delete r; }

namespace {

int run_buffers(cstark_ctx *c, ProveArena *a, ProofRun &R) {
    const unsigned m = R.m, n_layers = R.n_layers, log_N = R.job.log_n + R.log_b;
    if (m == 1) {
        R.comb[0] = a->combined; R.cco[0] = R.ccoefs = a->ccoef; R.clde = a->clde; R.deep = a->deep; R.layer = a->layer; R.d_open = a->d_open;
        return CSTARK_OK;
    }
    const size_t b = (size_t)1 << R.log_b, N = b << R.job.log_n, W = R.job.width, CN = (size_t)1 << (R.job.log_ce + R.job.log_n), nq = R.opt.num_queries;
    const uint32_t fold = 1u << R.log_f;
    uint64_t *combined_x, *ccoef_x;
    RC_TRY(arena_extra(c, a, 16, &combined_x, 2 * CN * 8)); // components 1, 2 of the merged evaluations
    RC_TRY(arena_extra(c, a, 17, &ccoef_x, 2 * CN * 8));    // their column coefficients
    RC_TRY(arena_extra(c, a, 18, &R.ccoefs, 3 * CN * 8));
    RC_TRY(arena_extra(c, a, 19, &R.clde, 3 * b * CN * 8));
    RC_TRY(arena_extra(c, a, 20, &R.deep, 3 * N * 8));
    RC_TRY(arena_extra(c, a, 21, &R.d_open, nq * (W * 8 + 192 + 2 * log_N * 32 + (size_t)n_layers * (fold * 24 + log_N * 32)) + 256));
    R.layer.resize(n_layers + 1);
    size_t sz = N;
    for (unsigned l = 0; l <= n_layers; l++) { RC_TRY(arena_extra(c, a, 22 + l, &R.layer[l], 3 * sz * 8)); sz >>= R.log_f; }
    for (unsigned q = 0; q < 3; q++) { R.comb[q] = q ? combined_x + (q - 1) * CN : a->combined; R.cco[q] = q ? ccoef_x + (q - 1) * CN : a->ccoef; }
    return CSTARK_OK;
}

// options / sizes of a run, its arena and buffers
int run_setup(cstark_ctx *c, const cstark_options *opt, const AirJob &job, ProofRun &R, ProveArena **a) {
    RC_TRY(check_options(opt, job.log_ce, &R.log_rem, &R.log_b, &R.log_f));
    const unsigned log_N = job.log_n + R.log_b;
    if (log_N > 24) return fail(CSTARK_ERR_UNSUPPORTED, "the LDE domain holds at most 2^24 points (2^21 trace rows at blowup 8)");
    if (job.sharded && R.log_b != 3) return fail(CSTARK_ERR_UNSUPPORTED, "sharded proofs use blowup factor 8 (one to four of its eight cosets per rank)");
    R.opt = *opt; R.job = job;
    R.job.log_b = R.log_b;
    R.m = opt->field_extension + 1;
    if (!job.sharded) { R.job.k0 = 0; R.job.nk = 1u << R.log_b; }
    R.shape = proof_shape((uint32_t)job.air, job.width, job.log_n, job.item, *opt);
    R.n_layers = R.shape.n_layers;
    if (opt->num_queries > ((size_t)1 << log_N) / 2) return fail(CSTARK_ERR_INVALID_ARG, "more queries than the domain supports"); // (distinct positions are drawn)
    // all openings are one launch (GatherBatch); no accepted option set reaches this (folding >= 4, 2^24 points: at most 9 layers)
    static_assert((MAX_GATHER_JOBS - 4) / 2 <= (int)VMAX_LAYERS, "a proof that fits one opening launch fits the layout's per-layer tables");
    if (2 * (size_t)R.n_layers + 4 > MAX_GATHER_JOBS) return fail(CSTARK_ERR_UNSUPPORTED, "too many FRI layers for one opening launch");
    HIP_TRY(hipSetDevice(c->device));
    RC_TRY(get_arena(c, R.job, R.log_b, R.log_f, R.n_layers, opt->num_queries, a));
    return run_buffers(c, *a, R);
}

// ---- host steps of a proof -----------------------------------------------------------------------------------------------------------
// What the host-channel phases below and the device-channel prover (prove_core_dev) share: every step enqueues on the context's stream
// and reads its buffers from the run.  What differs between the two -- who absorbs a root and draws -- stays with the callers.

// the end of a stage: the next of the arena's events, in stream order (cstark_prove_stage_ms reads the times between them)
#define STAGE() HIP_TRY(hipEventRecord(a->ev[R.evi++], c->stream))

// The first step of every run.  Trace, interpolation and extension (three stages), then the row hashes of the whole table straight into
// the trace tree's leaf level; a sharded run hashes its own cosets instead (phase_commit).
int commit_trace_leaves(cstark_ctx *c, ProveArena *a, ProofRun &R) {
    AirJob &job = R.job;
    a->timed = false;
    R.evi = 0;
    STAGE();
    RC_TRY(job.build(c, a, job));
    STAGE();
    RC_TRY(commit_columns(c, a, job, c->stream, R.evi));
    if (R.sharded()) return CSTARK_OK;
    return hash_rows_slots(c, R.opt.hash_fn, a->lde, a->tnodes + ((size_t)32 << (job.log_n + R.log_b)), job.width, job.log_n, R.log_b, R.log_s());
}

// The host coin after the trace commitment, and the coefficient sets drawn from it.  Call after the wait for the root, which also
// completes the public-input copy of job.build.
void open_host_channel(ProofRun &R) {
    AirJob &job = R.job;
    const size_t nc = job.n_constraints, na = job.n_assertions;
    if (job.pub_staging) job.pub.assign(job.pub_staging, job.pub_staging + 14);
    const std::vector<uint8_t> seed = channel_seed(job, R.opt, R.log_rem);
    transcript::open(R.coin, R.opt.hash_fn, seed.data(), seed.size(), R.trace_root);
    transcript::CoefficientSets cs{};
    for (unsigned q = 0; q < R.m; q++) {
        R.ta[q].resize(nc); R.tb[q].resize(nc); R.ba[q].resize(na); R.bb[q].resize(na);
        cs.ta[q] = R.ta[q].data(); cs.tb[q] = R.tb[q].data(); cs.ba[q] = R.ba[q].data(); cs.bb[q] = R.bb[q].data();
    }
    std::vector<uint64_t> dr(R.m * transcript::coefficient_draws(nc, na));
    transcript::draw_coefficients(R.coin, R.m, nc, na, dr.data(), cs);
}

// Merged evaluations [ce][n] per component (R.comb) -> the composition table and its tree: column coefficients per component, one
// extension of the m ce columns, row hashes, tree.  The committed table is R.clde (rows of ce m-tuples).
int commit_composition(cstark_ctx *c, ProveArena *a, ProofRun &R) {
    const unsigned m = R.m, log_n = R.job.log_n, log_ce = R.job.log_ce, log_b = R.log_b;
    const uint32_t hf = R.opt.hash_fn, b = 1u << log_b, cw = m << log_ce;
    for (unsigned q = 0; q < m; q++) RC_TRY(cstark_composition_columns(c, R.comb[q], R.cco[q], log_n, log_ce));
    if (m > 1) HIP_TRY(cs::interleave_set_columns(R.ccoefs, R.cco, m, 1u << log_ce, (size_t)1 << log_n, c->stream));
    RC_TRY(cstark_lde_columns(c, R.ccoefs, R.clde, cw, log_n, log_b, host::lde_offset(), 0, b));
    RC_TRY(cstark_hash_rows_fn(c, hf, R.clde, a->cnodes + ((size_t)32 << (log_n + log_b)), cw, log_n, log_b, 0, b));
    return cstark_merkle_build_fn(c, hf, a->cnodes, log_n + log_b);
}

// The DEEP composition polynomial has degree < n in every component (quotients of degree n - 2 times the linear degree adjustment): its
// values on ONE coset determine it.  The callers evaluate the quotient sums on coset 0 only (1/8 of the extended trace read) into `sums`
// [m][n]; here they are interpolated (the coefficients of P(g y), dcoef [m][n]) and extended to all cosets with offset 1 -- the same
// values as evaluating the sums at every point -- then put in natural order: FRI layer 0.
int deep_extend(cstark_ctx *c, ProofRun &R, uint64_t *sums, uint64_t *dcoef) {
    const unsigned log_n = R.job.log_n, log_b = R.log_b;
    const size_t n = (size_t)1 << log_n, N = n << log_b;
    RC_TRY(cstark_interpolate_columns(c, sums, dcoef, R.m, log_n));
    for (unsigned q = 0; q < R.m; q++) {
        RC_TRY(cstark_lde_columns(c, dcoef + q * n, R.deep + q * N, 1, log_n, log_b, host::from_u64(1), 0, 1u << log_b));
        RC_TRY(cstark_interleave_cosets(c, R.deep + q * N, R.layer[0] + q * N, log_n, log_b));
    }
    return CSTARK_OK;
}

// FRI commit phase: per layer the row hashes, the tree, and the fold at the point the coin draws after the layer's root.  `last`: where
// the last fold lands (the remainder).  The coin is the run's:
//   d_fri != null  a coin block on the device, [seed 8 words][alpha: m elements (2 m words) per layer x 32]: k_fri_coin / k_fri_coin_ext
//                  reseeds with the layer's root, draws the folding point and copies the root to d_roots + 8 l, so all layers are
//                  enqueued at once and nothing waits (Blake3);
//   d_fri == null  the host coin R.coin: one wait per layer for the root (-> R.layer_roots), the point drawn between two launches.
int fri_commit(cstark_ctx *c, ProveArena *a, ProofRun &R, uint32_t *d_fri, uint32_t *d_roots, uint64_t *last) {
    const unsigned m = R.m, log_f = R.log_f;
    const uint32_t hf = R.opt.hash_fn, fold = 1u << log_f;
    uint64_t offset = host::lde_offset();
    unsigned lg = R.job.log_n + R.log_b;
    for (unsigned l = 0; l < R.n_layers; l++) {
        const size_t rows = (size_t)1 << (lg - log_f);
        uint64_t *next = l + 1 == R.n_layers ? last : R.layer[l + 1];
        RC_TRY(cstark_hash_rows_fn(c, hf, R.layer[l], a->lnodes[l] + 32 * rows, fold * m, lg - log_f, 0, 0, 1));
        RC_TRY(cstark_merkle_build_fn(c, hf, a->lnodes[l], lg - log_f));
        if (d_fri) {
            RC_TRY(fri_coin_fold_dev(c, d_fri, a->lnodes[l] + 32, (uint64_t *)(d_fri + 8) + m * l, d_roots + 8 * l, R.layer[l], next, lg, log_f, offset, m));
        } else {
            HIP_TRY(hipMemcpyAsync(&R.layer_roots[32 * l], a->lnodes[l] + 32, 32, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(cs::stream_wait(c->stream));
            host::EX alpha = host::ex_zero();
            transcript::fri_layer(R.coin, &R.layer_roots[32 * l], m, alpha.c);
            if (m == 1) RC_TRY(cstark_fri_fold(c, R.layer[l], next, lg, fold, offset, alpha.c[0]));
            else RC_TRY(cstark_fri_fold_ext(c, R.layer[l], next, lg, fold, offset, m, alpha.c));
        }
        offset = host::pow(offset, fold);
        lg -= log_f;
    }
    return CSTARK_OK;
}

// The proof bytes (proof_layout.h), straight into the caller's buffer.  `p`: roots, frame, nonce and remainder; the openings are the
// sections O of the host copy `h` of an opening block, `counts` positions per layer.  form: the context's (CSTARK_FORM_*); the compact
// form is selected from the same block and needs the positions on the host: pos [nq], then layer l's at pos + lstride * (l + 1).
int finish_proof(const ProofShape &S, ProofParts p, const uint8_t *h, const OpenBlock &O, const uint32_t *counts, uint32_t form, const uint32_t *pos,
                 size_t lstride, uint8_t *proof, size_t capacity, size_t *proof_len) {
    p.trows = h + O.trows; p.tpaths = h + O.tpaths; p.crows = h + O.crows; p.cpaths = h + O.cpaths;
    p.counts = counts;
    p.form = form; p.pos = pos;
    for (unsigned l = 0; l < S.n_layers; l++) { p.lrows[l] = h + O.lrows[l]; p.lpaths[l] = h + O.lpaths[l]; p.lpos[l] = pos + lstride * (l + 1); }
    if (write_proof(S, p, proof, capacity, proof_len)) return fail(CSTARK_ERR_INVALID_ARG, "proof buffer too small (required size returned in *proof_len)");
    return CSTARK_OK;
}

// ---- phase 1: trace, its interpolation and extension, row hashes of the owned cosets ---------------------------------------------
// d_leaves_local (sharded only): [n][32], the roots of the rank's subtrees -- the nk leaves 8 j + k0 .. 8 j + k0 + nk - 1 of row j are a
// complete subtree of the trace tree, so the rank hashes the bottom log2(nk) levels itself (its own heap `sub`, kept for the openings)
// and the all-gather moves 32 n bytes per rank at every world size.  Otherwise the leaves go straight into the tree.
int phase_commit(cstark_ctx *c, ProveArena *a, ProofRun &R, uint8_t *d_leaves_local) {
    AirJob &job = R.job;
    const unsigned log_n = job.log_n;
    const size_t n = (size_t)1 << log_n, W = job.width;
    const uint32_t hf = R.opt.hash_fn;
    RC_TRY(commit_trace_leaves(c, a, R));
    if (R.sharded()) {
        const unsigned log_nk = ceil_log2(job.nk);
        if (log_nk == 0) { // one coset: its row digests are the subtree roots
            RC_TRY(cstark_hash_rows_fn(c, hf, a->lde, d_leaves_local, (uint32_t)W, log_n, 0, 0, 1));
        } else {           // the rank's cosets as a tree of their own: leaf nk j + (k - k0); the level with n nodes = the subtree roots
            uint8_t *sub;
            RC_TRY(arena_extra(c, a, 45, &sub, 2 * ((size_t)job.nk << log_n) * 32));
            RC_TRY(cstark_hash_rows_fn(c, hf, a->lde, sub + 32 * ((size_t)job.nk << log_n), (uint32_t)W, log_n, log_nk, 0, job.nk));
            RC_TRY(cstark_merkle_build_fn(c, hf, sub, log_n + log_nk));
            HIP_TRY(hipMemcpyAsync(d_leaves_local, sub + 32 * n, n * 32, hipMemcpyDeviceToDevice, c->stream));
        }
    }
    R.phase = 1;
    return CSTARK_OK;
}

// ---- phase 2: trace tree, channel, coefficients, merged constraint evaluations of the owned cosets -----------------------------------
// d_leaves_all (sharded only): the all-gathered subtree roots [W][n][32], rank-major (W = 8 / nk).  d_out: [nk][n], component 0 of the
// merged evaluations (the further components of an extension proof: R.comb).
int phase_evaluate(cstark_ctx *c, ProveArena *a, ProofRun &R, const uint8_t *d_leaves_all, uint64_t *d_out) {
    AirJob &job = R.job;
    const unsigned m = R.m, log_n = job.log_n, log_b = R.log_b, log_N = log_n + log_b;
    const size_t n = (size_t)1 << log_n;
    hipStream_t st = c->stream;
    unsigned log_top = log_N; // leaves of the tree that is built here
    if (R.sharded()) { // node W j + r of the level with W n nodes = rank r's subtree root of row j; the levels from there up
        const unsigned log_w = log_b - ceil_log2(job.nk);
        log_top = log_n + log_w;
        k_interleave_leaves<<<(unsigned)(((2 * n << log_w) + 255) / 256), 256, 0, st>>>((const uint4 *)d_leaves_all, (uint4 *)(a->tnodes + 32 * (n << log_w)), n, log_w);
        HIP_TRY(hipGetLastError());
    }
    RC_TRY(cstark_merkle_build_fn(c, R.opt.hash_fn, a->tnodes, log_top));
    HIP_TRY(hipMemcpyAsync(R.trace_root, a->tnodes + 32, 32, hipMemcpyDeviceToHost, st));
    STAGE();
    HIP_TRY(cs::stream_wait(st));
    static const bool hostprof = getenv("CSTARK_HOSTPROF") != nullptr; // debugging: host time between the root and the evaluation launches
    const auto hp0 = std::chrono::steady_clock::now();
    open_host_channel(R);
    const auto hp1 = std::chrono::steady_clock::now();
    uint64_t *outs[3] = {d_out, R.comb[1], R.comb[2]};
    if (job.combine_sets) {
        const uint64_t *pa[3], *pb[3], *qa[3], *qb[3];
        for (unsigned q = 0; q < m; q++) { pa[q] = R.ta[q].data(); pb[q] = R.tb[q].data(); qa[q] = R.ba[q].data(); qb[q] = R.bb[q].data(); }
        RC_TRY(job.combine_sets(c, a, job, m, pa, pb, qa, qb, outs));
    } else {
        for (unsigned q = 0; q < m; q++) RC_TRY(job.combine(c, a, job, R.ta[q].data(), R.tb[q].data(), R.ba[q].data(), R.bb[q].data(), outs[q]));
    }
    if (hostprof) {
        const auto hp2 = std::chrono::steady_clock::now();
        fprintf(stderr, "[cstark hostprof] coefficients drawn in %.1f us, evaluation enqueued in %.1f us\n",
                std::chrono::duration<double, std::micro>(hp1 - hp0).count(), std::chrono::duration<double, std::micro>(hp2 - hp1).count());
    }
    STAGE();
    R.phase = 2;
    return CSTARK_OK;
}

// ---- phase 3: composition polynomial and its commitment, out-of-domain frame, DEEP composition, FRI, query positions -----------------
// Needs the merged evaluations on the constraint-evaluation domain, [ce][n] per component, in R.comb and coset 0 of the extended trace at
// a->lde (the owner of coset 0).
int phase_compose(cstark_ctx *c, ProveArena *a, ProofRun &R) {
    using host::EX;
    AirJob &job = R.job;
    const unsigned m = R.m, log_n = job.log_n, log_b = R.log_b, log_N = log_n + log_b, n_layers = R.n_layers;
    const size_t n = (size_t)1 << log_n, W = job.width, ce = (size_t)1 << job.log_ce;
    hipStream_t st = c->stream;
    const uint32_t hf = R.opt.hash_fn;
    Coin &coin = R.coin;
    if (job.k0 != 0) return fail(CSTARK_ERR_INVALID_ARG, "the composition phase runs on the rank that owns coset 0");
    RC_TRY(commit_composition(c, a, R));
    HIP_TRY(hipMemcpyAsync(R.cons_root, a->cnodes + 32, 32, hipMemcpyDeviceToHost, st));
    STAGE();
    HIP_TRY(cs::stream_wait(st));

    // ---- out-of-domain frame: T(z) | T(z w), then H_i(z^ce) -----------------------------------------------------------------
    EX z = host::ex_zero();
    transcript::draw_ood_point(coin, R.cons_root, m, z.c);
    std::vector<uint64_t> &ood_trace = R.ood_trace, &ood_comp = R.ood_comp;
    ood_trace.assign(2 * m * W, 0); ood_comp.assign(m * ce, 0);
    if (m == 1) {
        const uint64_t zpts[2] = {z.c[0], host::mul(z.c[0], host::root_of_unity(log_n))};
        RC_TRY(evaluate_ood_frames(c, a->coeffs, (uint32_t)W, R.ccoefs, (uint32_t)ce, log_n, zpts, host::pow(z.c[0], ce), ood_trace.data(), ood_comp.data()));
    } else {
        const EX zw = host::ex_scale(z, host::root_of_unity(log_n)), zb = host::ex_pow(z, ce, m);
        std::vector<uint64_t> raw(m * m * ce);
        RC_TRY(cstark_evaluate_polys_at_ext(c, a->coeffs, (uint32_t)W, log_n, m, z.c, ood_trace.data()));
        RC_TRY(cstark_evaluate_polys_at_ext(c, a->coeffs, (uint32_t)W, log_n, m, zw.c, ood_trace.data() + m * W));
        RC_TRY(cstark_evaluate_polys_at_ext(c, R.ccoefs, (uint32_t)(m * ce), log_n, m, zb.c, raw.data()));
        EX gen = host::ex_zero();
        gen.c[1] = host::ONE; // the adjoined root
        for (size_t i = 0; i < ce; i++) { // H_i = sum_q root^q H_i,q, each component polynomial evaluated at z^ce
            EX h = host::ex_zero(), gq = host::ex_one();
            for (unsigned q = 0; q < m; q++) {
                h = host::ex_add(h, host::ex_mul(gq, host::ex_load(raw.data() + m * (m * i + q), m), m));
                gq = host::ex_mul(gq, gen, m);
            }
            for (unsigned q = 0; q < m; q++) ood_comp[m * i + q] = h.c[q];
        }
    }
    transcript::absorb_frame(coin, m, W, ce, ood_trace.data(), ood_comp.data());
    STAGE();

    // ---- DEEP composition -------------------------------------------------------------------------------------------------
    std::vector<uint64_t> d_alpha(m * W), d_beta(m * W), d_delta(m * ce), dr(m * transcript::deep_draws(W, ce));
    EX deg_a = host::ex_zero(), deg_b = host::ex_zero();
    transcript::draw_deep(coin, m, W, ce, dr.data(), d_alpha.data(), d_beta.data(), d_delta.data(), deg_a.c, deg_b.c);
    uint64_t *sums, *dcoef; // the quotient sums on coset 0 and their coefficients (deep_extend)
    if (m == 1) {
        sums = R.deep;
        RC_TRY(arena_extra(c, a, 40, &dcoef, n * 8));
        RC_TRY(cstark_deep_composition(c, a->lde, R.clde, (uint32_t)W, (uint32_t)ce, z.c[0], ood_trace.data(), ood_comp.data(), d_alpha.data(),
                                       d_beta.data(), d_delta.data(), deg_a.c[0], deg_b.c[0], sums, log_n, log_b, 0, 1));
    } else {
        RC_TRY(arena_extra(c, a, 40, &sums, 3 * n * 8));
        RC_TRY(arena_extra(c, a, 41, &dcoef, 3 * n * 8));
        RC_TRY(deep_composition_ext_cosets(c, a->lde, R.clde, (uint32_t)W, (uint32_t)ce, m, z.c, ood_trace.data(), ood_comp.data(), d_alpha.data(),
                                           d_beta.data(), d_delta.data(), deg_a.c, deg_b.c, sums, log_n, log_b, 1));
    }
    RC_TRY(deep_extend(c, R, sums, dcoef));
    STAGE();

    // ---- FRI commit phase -----------------------------------------------------------------------------------------------------
    // Base field, Blake3 coin: the layers' coin lives on the device (fri_commit), so the host enqueues all layers at once and collects the
    // roots with the remainder -- one wait instead of one per layer (8 x ~20 us of GPU idle time at 2^20 steps); it then replays the
    // reseeds on its own coin.  CSTARK_FRI_DEVICE_COIN=0, the Sha3 coin and extension fields: the host draws every folding point.
    static const bool dev_coin_env = [] { const char *e = getenv("CSTARK_FRI_DEVICE_COIN"); return !e || atoi(e) != 0; }();
    const bool dev_coin = dev_coin_env && hf == 0 && m == 1 && n_layers > 0;
    uint32_t *d_fri = nullptr, *d_roots = nullptr; // [seed 8 words][alpha: 2 words per layer x 32][roots: 8 words per layer]
    R.layer_roots.assign(32 * (size_t)n_layers, 0);
    if (dev_coin) {
        RC_TRY(arena_extra(c, a, 41, &d_fri, (size_t)(8 + 10 * 32) * 4));
        HIP_TRY(hipMemcpyAsync(d_fri, coin.seed, 32, hipMemcpyHostToDevice, st));
        d_roots = d_fri + 8 + 2 * 32;
    }
    RC_TRY(fri_commit(c, a, R, d_fri, d_roots, R.layer[n_layers]));
    R.remainder.assign((size_t)m << (log_N - n_layers * R.log_f), 0);
    if (dev_coin) HIP_TRY(hipMemcpyAsync(R.layer_roots.data(), d_roots, 32 * (size_t)n_layers, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(R.remainder.data(), R.layer[n_layers], R.remainder.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(cs::stream_wait(st));
    if (dev_coin) // the layers' points were drawn on the device: the same steps without their draws
        for (unsigned l = 0; l < n_layers; l++) transcript::fri_layer(coin, &R.layer_roots[32 * l], m, nullptr);
    transcript::commit_remainder(coin, R.remainder.data(), R.remainder.size(), R.rem_commit);
    STAGE();

    // ---- proof of work, query positions -------------------------------------------------------------------------------------
    RC_TRY(query_stage(c, a, coin, R.shape, R.q));
    R.phase = 3;
    return CSTARK_OK;
}

// ---- phase 4: openings (gathered on the device, one copy back) and the proof bytes ---------------------------------------------------
// d_trace_rows (sharded only): the opened rows of the extended trace [nq][W], complete (summed over the ranks).
int phase_open(cstark_ctx *c, ProveArena *a, ProofRun &R, const uint64_t *d_trace_rows, uint8_t *proof, size_t capacity, size_t *proof_len) {
    const ProofShape &S = R.shape;
    const OpenBlock O = open_block(S, R.q.counts);
    RC_TRY(open_stage(c, a, S, {R.clde, R.layer.data(), R.log_s(), R.q.counts, nullptr, d_trace_rows, ceil_log2(R.job.nk)}, R.d_open, O));
    STAGE();
    HIP_TRY(cs::stream_wait(c->stream));
    a->timed = true; a->channel = CSTARK_CHANNEL_HOST;

    ProofParts p{};
    p.trace_root = R.trace_root; p.cons_root = R.cons_root; p.layer_roots = R.layer_roots.data(); p.rem_commit = R.rem_commit;
    p.ood_trace = R.ood_trace.data(); p.ood_comp = R.ood_comp.data(); p.nonce = R.q.nonce; p.remainder = R.remainder.data();
    return finish_proof(S, p, a->h_open, O, R.q.counts, R.sharded() ? (uint32_t)CSTARK_FORM_PLAIN : ctx_proof_form(c), R.q.hpos.data(), 256, proof, capacity, proof_len);
}

// every host-channel proof on one GPU
int prove_core(cstark_ctx *c, const cstark_options *opt, AirJob &job, uint8_t *proof, size_t capacity, size_t *proof_len) {
    ProofRun R;
    ProveArena *a;
    RC_TRY(run_setup(c, opt, job, R, &a));
    RC_TRY(phase_commit(c, a, R, nullptr));
    RC_TRY(phase_evaluate(c, a, R, nullptr, a->combined));
    RC_TRY(phase_compose(c, a, R));
    return phase_open(c, a, R, nullptr, proof, capacity, proof_len);
}
// ---- the same proof with the Fiat-Shamir channel on the device (channel.hip) ---------------------------------------------------------
// Any of the AIRs, any field extension, Blake3 coin, no proof of work, one GPU: every channel step -- seed, reseeds, the 238 coefficient
// draws, the out-of-domain point, the DEEP coefficients, the FRI layers' folding points (k_fri_coin), the remainder commitment, the query
// positions and their folded forms -- is a launch on the context's stream, the kernels read what was drawn from device memory, and the
// host waits ONCE, for the block that holds everything the proof bytes are written from.  Every buffer is sized before the first launch:
// nothing is allocated, freed or uploaded in between.  The Sha3 coin, proof of work and sharded proofs take the host channel (prove_core /
// the cstark_tx_shard_* phases).  Same bytes as prove_core (the tests compare both with the CPU prover); CSTARK_HOST_CHANNEL=1 keeps the
// host channel for the A/B.  One-at-a-time proving on the host channel leaves the GPU idle for 0.6 ms of a 28.4 ms base-field proof,
// 0.39 ms of it in the five waits (profiles/r04_timeline_host_channel.txt); an extension-field proof waits more often (three frame
// evaluations, an upload before the DEEP stage, every FRI layer) and recombines the frame on the host.
// Extension fields (m = 2, 3 words per drawn element): the channel draws m-tuples (ChanStep::m); the m coefficient sets lie one block
// apart; the frame, the DEEP constants and the folds read their points where the channel wrote them (ext.hip).
// The stages between the four channel steps are the host steps above.
int prove_core_dev(cstark_ctx *c, const cstark_options *opt, AirJob &job0, uint8_t *proof, size_t capacity, size_t *proof_len) {
    const auto hp0 = std::chrono::steady_clock::now();
    ProofRun R;
    ProveArena *a;
    job0.dev_channel = true;
    RC_TRY(run_setup(c, opt, job0, R, &a));
    AirJob &job = R.job;
    const unsigned m = R.m, log_n = job.log_n, log_b = R.log_b, log_N = log_n + log_b, n_layers = R.n_layers;
    const size_t n = (size_t)1 << log_n, W = job.width, ce = (size_t)1 << job.log_ce, nq = opt->num_queries;
    const size_t rem_len = (size_t)m << (log_N - n_layers * R.log_f), n_ood = m * (2 * W + ce); // words
    hipStream_t st = c->stream;
    // ---- the result block: everything the proof bytes are written from, one copy to the host at the end ------------------------------------
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_troot = take(32), o_croot = take(32), o_rem = take(32), o_cnt = take(4 * 64), o_ood = take(n_ood * 8), o_lroots = take(32 * (size_t)n_layers),
                 o_remainder = take(rem_len * 8);
    const ProofShape &S = R.shape;
    // the compact form is selected on the host and needs the positions there: the channel then draws them into the result block, where
    // the gathers read them and the one copy takes them along (the plain form keeps a->d_pos and a block without them)
    const bool compact = ctx_proof_form(c) == CSTARK_FORM_COMPACT;
    const size_t o_pos = compact ? take(4 * 256 * ((size_t)n_layers + 1)) : 0;
    const OpenBlock O = open_block(S, nullptr, off, 256); // the openings: the tail of the block, nq slots in every layer
    off = O.bytes;
    uint8_t *d_res;
    uint32_t *d_fri;   // [seed 8 words][alpha: m elements per layer x 32]: the coin and the layers' folding points
    uint64_t *d_chan;  // [pts 4 m][scal 8 m][deep coefficients m (2 W + ce)]: m-tuples
    uint64_t *sums, *dcoef; // the quotient sums on coset 0 [m][n] and their coefficients (deep_extend)
    RC_TRY(arena_extra(c, a, 44, &d_res, off));
    RC_TRY(arena_extra(c, a, 43, &d_chan, 12 * m * 8 + n_ood * 8));
    // (slots 40, 41 also serve the host channel: dcoef and the coin block for m = 1, sums and dcoef otherwise; an extension proof on
    // this channel keeps its own, so a context that alternates between the channels never replaces a slot back and forth)
    if (m == 1) {
        RC_TRY(arena_extra(c, a, 41, &d_fri, (size_t)(8 + 10 * 32) * 4));
        RC_TRY(arena_extra(c, a, 40, &dcoef, n * 8));
        sums = R.deep;
    } else {
        RC_TRY(arena_extra(c, a, 47, &d_fri, (size_t)(8 + 2 * 3 * 32) * 4));
        RC_TRY(arena_extra(c, a, 48, &sums, 3 * n * 8));
        RC_TRY(arena_extra(c, a, 49, &dcoef, 3 * n * 8));
    }
    uint64_t *d_pts = d_chan, *d_scal = d_chan + 4 * m, *d_deepc = d_chan + 12 * m, *d_ood = (uint64_t *)(d_res + o_ood);
    uint32_t *d_cnt = (uint32_t *)(d_res + o_cnt), *d_qpos = compact ? (uint32_t *)(d_res + o_pos) : a->d_pos;
    RC_TRY(host_open_block(a, off)); // before the first launch: replacing a pinned block waits for the device
    RC_TRY(desc_reserve(c, ood_frames_dev_scratch_bytes((uint32_t)W, (uint32_t)ce, log_n, m))); // the frame's scratch, likewise
    // the coefficient blocks the channel draws into, one per component: TransactionAir's evaluator reads the context's cstark_tx_coeffs
    // blocks; the sub-AIRs' merge takes alpha[115] | beta[115] | b_alpha[na] | b_beta[na]
    uint64_t *d_coef_block;
    const bool is_tx = job.air == CSTARK_AIR_STATE_TRANSITION;
    const size_t coef_stride = is_tx ? (size_t)CE_COEF_WORDS : 230 + 2 * (size_t)job.n_assertions;
    if (is_tx) RC_TRY(tx_coef_device_block(c, &d_coef_block));
    else RC_TRY(arena_extra(c, a, 46, &d_coef_block, m * coef_stride * 8));
    const uint64_t *pw, *pwinv;
    RC_TRY(plan_tables(c, log_n, &pw, &pwinv));

    RC_TRY(commit_trace_leaves(c, a, R));
    RC_TRY(cstark_merkle_build_fn(c, R.opt.hash_fn, a->tnodes, log_N));
    STAGE();
    {   // the coin: context || public inputs (read from the trace, on the device), the trace root, the coefficient pairs
        ChanStep s{};
        s.seed = d_fri; s.m = m;
        const std::vector<uint8_t> prefix = channel_seed(job.width, log_n, *opt, log_b, R.log_rem); // the seed up to the public inputs
        if (job.air == CSTARK_AIR_SCHNORR) {
            // SchnorrAir's public inputs -- every message, R.x and s half: 304 bytes per signature -- are host data: the seed is hashed
            // here (once per uploaded witness and option set: c->schnorr_seed) and uploaded
            uint8_t key[12] = {}; // width, log n, the seven option bytes, 0, 0, 1 (valid)
            memcpy(key, prefix.data(), 2); memcpy(key + 2, prefix.data() + 10, 7); key[11] = 1;
            if (memcmp(key, c->schnorr_seed_key, sizeof key) != 0) {
                const std::vector<uint8_t> seed = channel_seed(job, *opt, R.log_rem);
                hostb3::hash(seed.data(), seed.size(), c->schnorr_seed);
                memcpy(c->schnorr_seed_key, key, sizeof key);
            }
            HIP_TRY(hipMemcpyAsync(d_fri, c->schnorr_seed, 32, hipMemcpyHostToDevice, st));
        } else {
            s.init = 1; s.pub = a->d_pub; s.npub = job.air == CSTARK_AIR_RANGE ? 1 : 14;
        }
        memcpy(s.prefix, prefix.data(), SEED_PREFIX); s.prefix_len = SEED_PREFIX;
        s.absorb[0].kind = CHAN_DIGEST; s.absorb[0].ptr = a->tnodes + 32; s.absorb[0].copy_out = d_res + o_troot;
        s.draw = CHAN_DRAW_COEFFS; s.a = job.n_constraints; s.b = job.n_assertions; s.stride = CSTARK_TX_NUM_CONSTRAINTS;
        s.set_stride = (uint32_t)coef_stride;
        s.count = (uint32_t)transcript::coefficient_draws(job.n_constraints, job.n_assertions); s.out = d_coef_block;
        HIP_TRY(channel_step(s, st));
    }
    if (is_tx) {
        RC_TRY(tx_evaluate_constraints_sets(c, a->lde, nullptr, m, nullptr, R.comb, job.item, log_n, 3, 0, 8, true, a->d_pub));
    } else { // the sub-AIRs: the assertion values are the public inputs (MerkleAir, RescueAir), (0, number) (RangeProofAir) or built in (SchnorrAir)
        job.d_avalues = job.air == CSTARK_AIR_RANGE ? a->d_pub + 1 : job.air == CSTARK_AIR_SCHNORR ? nullptr : a->d_pub;
        for (unsigned q = 0; q < m; q++) { // one merge per component's coefficient set
            job.d_coefs = d_coef_block + q * coef_stride;
            RC_TRY(job.combine(c, a, job, nullptr, nullptr, nullptr, nullptr, R.comb[q]));
        }
    }
    STAGE();
    RC_TRY(commit_composition(c, a, R));
    STAGE();
    {   // the constraint root -> the out-of-domain point z; z w and z^ce beside it
        ChanStep s{};
        s.seed = d_fri; s.m = m;
        s.absorb[0].kind = CHAN_DIGEST; s.absorb[0].ptr = a->cnodes + 32; s.absorb[0].copy_out = d_res + o_croot;
        s.draw = CHAN_DRAW_POINT; s.count = 1; s.b = (uint32_t)ce; s.w = host::root_of_unity(log_n); s.out = d_pts; s.out2 = d_scal;
        HIP_TRY(channel_step(s, st));
    }
    if (m == 1) RC_TRY(ood_frames_dev(c, a->coeffs, (uint32_t)W, R.ccoefs, (uint32_t)ce, log_n, d_pts, d_ood));
    else RC_TRY(ood_frames_dev_ext(c, a->coeffs, (uint32_t)W, R.ccoefs, (uint32_t)ce, log_n, m, d_pts, d_ood));
    STAGE();
    {   // the two halves of the frame -> the DEEP coefficients
        ChanStep s{};
        s.seed = d_fri; s.m = m;
        s.absorb[0].kind = CHAN_ELEMS; s.absorb[0].ptr = d_ood; s.absorb[0].count = (uint32_t)(2 * m * W);
        s.absorb[1].kind = CHAN_ELEMS; s.absorb[1].ptr = d_ood + 2 * m * W; s.absorb[1].count = (uint32_t)(m * ce);
        s.draw = CHAN_DRAW_DEEP; s.a = (uint32_t)W; s.b = (uint32_t)ce; s.per = CSTARK_CONV_DEEP_DRAWS_PER_REGISTER;
        s.count = (uint32_t)transcript::deep_draws(W, ce); s.out = d_deepc; s.out2 = d_scal;
        HIP_TRY(channel_step(s, st));
    }
    if (m == 1) { // the quotient sums on coset 0, read from the channel's blocks
        cs::DeepParams p{};
        p.trace_lde = a->lde; p.comp_lde = R.clde; p.w = pw; p.coef = d_deepc; p.ood = d_ood; p.shifts = a->d_shifts; p.out = sums;
        p.width = (uint32_t)W; p.nb = (uint32_t)ce; p.log_n = log_n; p.k0 = 0; p.scal = d_scal;
        HIP_TRY(cs::deep_composition(p, 1, st));
    } else {
        RC_TRY(deep_composition_ext_dev(c, a->lde, R.clde, (uint32_t)W, (uint32_t)ce, m, d_deepc, d_ood, d_scal, a->d_shifts, sums, log_n, log_b, 1));
    }
    RC_TRY(deep_extend(c, R, sums, dcoef));
    const hipEvent_t deep_done = a->ev[R.evi]; // the end of the DEEP stage: what the tail wait below sleeps on
    STAGE();
    // the layers' roots and the remainder land in the result block
    RC_TRY(fri_commit(c, a, R, d_fri, (uint32_t *)(d_res + o_lroots), (uint64_t *)(d_res + o_remainder)));
    STAGE();
    {   // remainder commitment, proof of work (none: nonce 1), query positions and their folded forms
        ChanStep s{};
        s.seed = d_fri; s.m = m;
        s.absorb[0].kind = CHAN_ELEMS; s.absorb[0].ptr = d_res + o_remainder; s.absorb[0].count = (uint32_t)rem_len; s.absorb[0].copy_out = d_res + o_rem;
        s.absorb[1].kind = CHAN_INT; s.absorb[1].value = 1;
        s.draw = CHAN_DRAW_QUERIES; s.count = (uint32_t)nq; s.log_domain = log_N; s.log_f = R.log_f; s.n_layers = n_layers; s.slot = 256;
        s.pos = d_qpos; s.cnt = d_cnt;
        HIP_TRY(channel_step(s, st));
    }
    // at most nq rows per layer; how many: cnt[l + 1], on the device.  The copy takes the whole result block.
    RC_TRY(open_stage(c, a, S, {R.clde, R.layer.data(), R.log_s(), nullptr, d_cnt + 1, nullptr, 0, d_qpos}, d_res, O));
    STAGE();
    static const bool hostprof = getenv("CSTARK_HOSTPROF") != nullptr; // debugging: where the host's time goes
    const auto hp1 = std::chrono::steady_clock::now();
    HIP_TRY(cs::stream_wait_tail(st, deep_done)); // the only wait of the proof: sleep until the DEEP stage is done, poll through the FRI tail
    const auto hp2 = std::chrono::steady_clock::now();
    a->timed = true; a->channel = CSTARK_CHANNEL_DEVICE;
    const uint8_t *h = a->h_open;
    const uint32_t *cnt = (const uint32_t *)(h + o_cnt);
    if (cnt[0] != nq) return fail(CSTARK_ERR_HIP, "device channel: the query positions could not be drawn");
    for (unsigned l = 0; l < n_layers; l++)
        if (cnt[l + 1] == 0 || cnt[l + 1] > nq) return fail(CSTARK_ERR_HIP, "device channel: bad folded position count");
    ProofParts p{};
    p.trace_root = h + o_troot; p.cons_root = h + o_croot; p.layer_roots = h + o_lroots; p.rem_commit = h + o_rem;
    p.ood_trace = h + o_ood; p.ood_comp = h + o_ood + ood_trace_bytes(S); p.remainder = h + o_remainder;
    p.nonce = 1; // grinding_factor 0
    RC_TRY(finish_proof(S, p, h, O, cnt + 1, ctx_proof_form(c), (const uint32_t *)(h + o_pos), 256, proof, capacity, proof_len));
    if (hostprof) {
        const auto hp3 = std::chrono::steady_clock::now();
        auto us = [](auto d) { return std::chrono::duration<double, std::micro>(d).count(); };
        fprintf(stderr, "[cstark hostprof] device channel: enqueued in %.0f us, waited %.0f us, proof written in %.0f us\n", us(hp1 - hp0), us(hp2 - hp1), us(hp3 - hp2));
    }
    return CSTARK_OK;
}
#undef STAGE
// which channel: the device's for what prove_core_dev covers, unless CSTARK_HOST_CHANNEL=1
bool use_dev_channel(const cstark_options *opt, const AirJob &job) {
    static const bool host_env = [] { const char *e = getenv("CSTARK_HOST_CHANNEL"); return e && atoi(e) != 0; }();
    if (host_env || job.sharded || job.n_constraints > CSTARK_TX_NUM_CONSTRAINTS) return false;
    if (opt->hash_fn != 0 || opt->field_extension > 2 || opt->grinding_factor != 0) return false;
    uint32_t lb = 0, lf = 0, lr = 0;
    while ((1u << lb) < opt->blowup_factor && lb < 8) lb++;
    while ((1u << lf) < opt->fri_folding_factor && lf < 8) lf++;
    while ((1u << lr) < opt->fri_max_remainder && lr < 12) lr++;
    return lf >= 2 && job.log_n + lb > lr; // at least one FRI layer (always, but for a 64-row range proof with a large remainder)
}

// Sharded proofs: a rank that holds 2 or 4 cosets evaluates its share of the degree-split form (CSTARK_SHARD_SPLIT=0, tuning /
// debugging: every point of its cosets directly, as a rank with a single coset always does).  shard_rows = rows of n merged
// evaluations the rank hands to the all-gather: its nk cosets, or its nk / 2 even cosets + its share of the four odd ones.
bool shard_split(uint32_t nk) {
    static const bool on = [] { const char *e = getenv("CSTARK_SHARD_SPLIT"); return !e || atoi(e) != 0; }();
    return on && (nk == 2 || nk == 4);
}
uint32_t shard_rows(uint32_t nk) { return shard_split(nk) ? nk / 2 + 4 : nk; }

// first / last row of registers 58..64 -> job.pub (TransactionProver::get_pub_inputs src/prover.rs:106-129; MerkleProver alike)
int gather_roots(cstark_ctx *c, ProveArena *a, AirJob &job, uint32_t reg0 = 58) {
    const size_t n = (size_t)1 << job.log_n;
    k_gather_pub<<<1, 64, 0, c->stream>>>(a->trace, n, a->d_pub, reg0);
    HIP_TRY(hipGetLastError());
    if (job.dev_channel) return CSTARK_OK; // the device-side channel reads them where they are
    job.pub.assign(14, 0);
    HIP_TRY(hipMemcpyAsync(job.pub.data(), a->d_pub, 14 * 8, hipMemcpyDeviceToHost, c->stream)); // complete at the commitment sync
    return CSTARK_OK;
}


// ---- TransactionAir ---------------------------------------------------------------------------------------------------------------
int tx_build(cstark_ctx *c, ProveArena *a, AirJob &job) {
    // the curve ladders are latency-bound (two waves per SIMD for ~2.8 ms): they run beside the interpolation and extension of
    // the 57 registers that do not depend on them
    static const int mode = [] { const char *e = getenv("CSTARK_TRACE_OVERLAP"); return e ? atoi(e) : 1; }(); // tuning / debugging: 0 = no overlap, 2 = split launch joined at once
    if (mode == 0) {
        RC_TRY(cstark_tx_build_trace(c, a->trace));
        return gather_roots(c, a, job);
    }
    RC_TRY(tx_build_trace_split(c, a->trace));
    if (mode == 2) {
        for (hipEvent_t e : {c->ev_join, c->ev_mid, c->ev_join2}) HIP_TRY(hipStreamWaitEvent(c->stream, e, 0));
        return gather_roots(c, a, job);
    }
    // public inputs (tree roots in registers 58..64, written by the Merkle recurrence): gathered on its stream, before the event the
    // second batch waits for, into pinned memory; collected after the commitment sync
    const size_t n = (size_t)1 << job.log_n;
    if (!a->h_pub) HIP_TRY(hipHostMalloc((void **)&a->h_pub, 14 * 8, hipHostMallocDefault));
    k_gather_pub<<<1, 64, 0, c->side>>>(a->trace, n, a->d_pub, 58u);
    HIP_TRY(hipGetLastError());
    if (!job.dev_channel) HIP_TRY(hipMemcpyAsync(a->h_pub, a->d_pub, 14 * 8, hipMemcpyDeviceToHost, c->side));
    HIP_TRY(hipEventRecord(c->ev_join, c->side));
    job.pub_staging = a->h_pub;
    if (mode == 3) // two batches: everything but the curve registers once the Merkle recurrence and the message hash are done
        job.batches = {{TX_LATE_COLS, job.width - TX_LATE_COLS, {c->ev_join, c->ev_mid}}, {0, TX_LATE_COLS, {c->ev_join2, nullptr}}};
    else
        // registers 65..91 are constant over a transaction (k_trace_aux): a step batch; the sigma range accumulator behind them is not
        job.batches = {{TX_COPY_COLS, TX_STEP_COLS, {nullptr, nullptr}, 1024},
                       {TX_COPY_COLS + TX_STEP_COLS, job.width - TX_COPY_COLS - TX_STEP_COLS, {nullptr, nullptr}},
                       {TX_LATE_COLS, TX_ROOT_COLS - TX_LATE_COLS, {c->ev_join, c->ev_mid}},
                       // the tree roots 58..64 hold one value up to the root copy of the Merkle recurrence (row 8 depth + 7 of a
                       // transaction) and another behind it: a two-level step batch
                       {TX_ROOT_COLS, TX_COPY_COLS - TX_ROOT_COLS, {c->ev_join, c->ev_mid}, 1024, 8 * job.item + 7},
                       {0, TX_LATE_COLS, {c->ev_join2, nullptr}}};
    return CSTARK_OK;
}
int tx_combine(cstark_ctx *c, ProveArena *a, AirJob &job, const uint64_t *ta, const uint64_t *tb, const uint64_t *ba, const uint64_t *bb, uint64_t *out) {
    cstark_tx_coeffs cf;
    memcpy(cf.t_alpha, ta, sizeof cf.t_alpha); memcpy(cf.t_beta, tb, sizeof cf.t_beta);
    memcpy(cf.b_alpha, ba, sizeof cf.b_alpha); memcpy(cf.b_beta, bb, sizeof cf.b_beta);
    const uint64_t pub4[4] = {job.pub[0], job.pub[1], job.pub[7], job.pub[8]}; // get_assertions, src/air.rs:175-184
    uint64_t *outs[1] = {out};
    // all cosets on this GPU: the degree-split evaluation (the table is this prover's own extension); a window of 2 or 4 cosets of a
    // sharded proof: the rank's share of the split evaluation (rows: shard_rows); a single coset (8 ranks): every point directly
    // (blowup 16: block 0 of the trace table is the eight cosets of the constraint-evaluation domain)
    if (!job.sharded) return tx_evaluate_constraints_sets(c, a->lde, &cf, 1, pub4, outs, job.item, job.log_n, 3, 0, 8, true);
    if (shard_split(job.nk)) return tx_evaluate_constraints_shard(c, a->lde, a->coeffs, &cf, pub4, out, job.item, job.log_n, job.k0, job.nk);
    return tx_evaluate_constraints_sets(c, a->lde, &cf, 1, pub4, outs, job.item, job.log_n, 3, job.k0, job.nk, false);
}
int tx_combine_sets(cstark_ctx *c, ProveArena *a, AirJob &job, unsigned m, const uint64_t *const *ta, const uint64_t *const *tb, const uint64_t *const *ba,
                    const uint64_t *const *bb, uint64_t *const *outs) {
    cstark_tx_coeffs cf[3];
    for (unsigned q = 0; q < m; q++) {
        memcpy(cf[q].t_alpha, ta[q], sizeof cf[q].t_alpha); memcpy(cf[q].t_beta, tb[q], sizeof cf[q].t_beta);
        memcpy(cf[q].b_alpha, ba[q], sizeof cf[q].b_alpha); memcpy(cf[q].b_beta, bb[q], sizeof cf[q].b_beta);
    }
    const uint64_t pub4[4] = {job.pub[0], job.pub[1], job.pub[7], job.pub[8]};
    return tx_evaluate_constraints_sets(c, a->lde, cf, m, pub4, outs, job.item, job.log_n, 3, 0, 8, true);
}
// The sub-AIRs are evaluated on their constraint-evaluation domain -- blowup 2^log_ce: MerkleAir 4, RangeProofAir 2 -- which is block 0 of
// the trace table whatever the blowup factor of the proof: a plain [ce][width][n] extension with the domain offset.
// The request to the sub-AIR stage (ctx.h) for this proof's table, with the coefficients where the channel drew them: on the device
// (job.d_coefs, job.d_avalues) or the host's four arrays and the AIR's assertion values.  The caller adds the source of the transition sum.
cs::AirStageRequest air_request(ProveArena *a, const AirJob &job, const uint64_t *ta, const uint64_t *tb, const uint64_t *ba, const uint64_t *bb,
                                const uint64_t *assertion_values, uint64_t *out) {
    cs::AirStageRequest rq;
    rq.air = job.air; rq.n_items = job.air == CSTARK_AIR_SCHNORR ? job.item : 0;
    rq.log_n = job.log_n; rq.log_blowup = job.log_ce; rq.k0 = 0; rq.nk = 1u << job.log_ce;
    rq.d_lde = a->lde; rq.d_out = out;
    // (job.d_avalues is null for SchnorrAir, whose assertion constants are built in: prove_core_dev sets it beside job.d_coefs)
    if (job.d_coefs) { rq.d_coefs = job.d_coefs; rq.d_avalues = job.d_avalues; }
    else { rq.t_alpha = ta; rq.t_beta = tb; rq.b_alpha = ba; rq.b_beta = bb; rq.assertion_values = assertion_values; }
    return rq;
}
// RangeProofAir and RescueAir: the transition values are materialised once per proof (an extension proof merges them with each of its m
// coefficient sets), then merged
int materialise_and_merge(cstark_ctx *c, ProveArena *a, AirJob &job, cs::AirStageRequest rq) {
    uint64_t *evals;
    RC_TRY(arena_extra(c, a, 0, &evals, ((size_t)rq.nk * job.n_constraints << job.log_n) * 8));
    if (!job.evals_ready) RC_TRY(cstark_air_evaluate_transitions(c, job.air, a->lde, evals, 0, job.log_n, rq.log_blowup, 0, rq.nk));
    job.evals_ready = true;
    rq.source = cs::AirTransitions::Materialised; rq.d_evals = evals;
    return air_stage(c, rq);
}
// ---- MerkleAir (src/merkle/update) ---------------------------------------------------------------------------------------------
int merkle_build(cstark_ctx *c, ProveArena *a, AirJob &job) {
    RC_TRY(cstark_merkle_build_trace(c, a->trace));
    return gather_roots(c, a, job);
}
int merkle_combine(cstark_ctx *c, ProveArena *a, AirJob &job, const uint64_t *ta, const uint64_t *tb, const uint64_t *ba, const uint64_t *bb, uint64_t *out) {
    cs::AirStageRequest rq = air_request(a, job, ta, tb, ba, bb, job.pub.data(), out);
    rq.source = cs::AirTransitions::MerkleFused; rq.merkle_depth = job.item;
    return air_stage(c, rq);
}
// ---- RangeProofAir (src/range) -------------------------------------------------------------------------------------------------------
int range_build(cstark_ctx *c, ProveArena *a, AirJob &job) {
    if (job.dev_channel) { // the public input (the number) and the two assertion values (0, the number: src/range/air.rs:79-86) for the device-side channel
        const uint64_t v[3] = {job.number, 0, job.number};
        HIP_TRY(hipMemcpyAsync(a->d_pub, v, sizeof v, hipMemcpyHostToDevice, c->stream)); // (a small pageable source is staged by the runtime before the call returns)
    }
    if (job.bits) return cstark_range_build_trace_bits(c, job.bits, job.log_n, a->trace, nullptr);
    return cstark_range_build_trace(c, job.number, a->trace);
}
int range_combine(cstark_ctx *c, ProveArena *a, AirJob &job, const uint64_t *ta, const uint64_t *tb, const uint64_t *ba, const uint64_t *bb, uint64_t *out) {
    const uint64_t vals[2] = {0, job.number}; // get_assertions, src/range/air.rs:79-86
    return materialise_and_merge(c, a, job, air_request(a, job, ta, tb, ba, bb, vals, out));
}
// ---- RescueAir (benches/rescue.rs:145-356) ---------------------------------------------------------------------------------------------
int rescue_build(cstark_ctx *c, ProveArena *a, AirJob &job) {
    RC_TRY(cstark_rescue_chain_build_trace(c, job.seed, job.item, a->trace));
    return gather_roots(c, a, job, 0); // get_pub_inputs :331-354: seed and result are the first / last row of registers 0..6
}
int rescue_combine(cstark_ctx *c, ProveArena *a, AirJob &job, const uint64_t *ta, const uint64_t *tb, const uint64_t *ba, const uint64_t *bb, uint64_t *out) {
    return materialise_and_merge(c, a, job, air_request(a, job, ta, tb, ba, bb, job.pub.data(), out));
}
// ---- SchnorrAir (src/schnorr) ---------------------------------------------------------------------------------------------------------
// the public-input columns (src/schnorr/air.rs:228-290; not committed: both sides derive them from the messages) and the sequence
// polynomials of the assertions, extended over the constraint-evaluation domain (blowup 8, whatever the proof's blowup factor): they
// depend on the public inputs only
int schnorr_public_columns(cstark_ctx *c, ProveArena *a, AirJob &job, uint64_t **aux_lde_out, uint64_t **av_lde_out, bool compute) {
    const size_t n = (size_t)1 << job.log_n;
    uint64_t *aux, *aux_co, *aux_lde, *av_co, *av_lde;
    RC_TRY(arena_extra(c, a, 1, &aux, 19 * n * 8));
    RC_TRY(arena_extra(c, a, 2, &aux_co, 19 * n * 8));
    RC_TRY(arena_extra(c, a, 3, &aux_lde, 8 * 19 * n * 8));
    RC_TRY(arena_extra(c, a, 4, &av_co, 12 * n * 8));
    RC_TRY(arena_extra(c, a, 5, &av_lde, 8 * 12 * n * 8));
    if (compute) {
        RC_TRY(cstark_schnorr_aux_columns(c, aux));
        RC_TRY(cstark_interpolate_columns(c, aux, aux_co, 19, job.log_n));
        RC_TRY(cstark_lde_columns(c, aux_co, aux_lde, 19, job.log_n, 3, host::lde_offset(), 0, 8));
        RC_TRY(cstark_schnorr_assertion_polys(c, av_co, job.log_n));
        RC_TRY(cstark_lde_columns(c, av_co, av_lde, 12, job.log_n, 3, host::lde_offset(), 0, 8));
    }
    *aux_lde_out = aux_lde; *av_lde_out = av_lde;
    return CSTARK_OK;
}
// The ladders are latency-bound (two waves per signature, one per SIMD at 512 signatures): they run on an internal stream beside the
// work that does not need them -- the public-input columns above, then the interpolation and extension of registers 37..55 (message
// hash, bit registers, limb accumulators).  CSTARK_SCHNORR_OVERLAP=0 (tuning / debugging): one stream, one thing after the other.
int schnorr_build(cstark_ctx *c, ProveArena *a, AirJob &job) {
    static const bool overlap = [] { const char *e = getenv("CSTARK_SCHNORR_OVERLAP"); return !e || atoi(e) != 0; }();
    if (!overlap) return cstark_schnorr_build_trace(c, a->trace);
    if (!c->wit_buf || c->wit.n_tx == 0 || !c->wit.msg_tail) return fail(CSTARK_ERR_INVALID_ARG, "no Schnorr witness uploaded");
    uint64_t *aux_lde, *av_lde;
    RC_TRY(schnorr_public_columns(c, a, job, &aux_lde, &av_lde, false)); // allocations (they may synchronise) before the fork
    HIP_TRY(cs::launch_schnorr_trace_split(c->wit, a->trace, c->stream, c->side, c->ev_fork, c->ev_join, c->ev_join2));
    RC_TRY(schnorr_public_columns(c, a, job, &aux_lde, &av_lde, true));
    job.public_ready = true;
    job.batches = {{37, job.width - 37, {c->ev_join, nullptr}}, {0, 37, {c->ev_join2, nullptr}}};
    return CSTARK_OK;
}
int schnorr_combine(cstark_ctx *c, ProveArena *a, AirJob &job, const uint64_t *ta, const uint64_t *tb, const uint64_t *ba, const uint64_t *bb, uint64_t *out) {
    uint64_t *aux_lde, *av_lde;
    RC_TRY(schnorr_public_columns(c, a, job, &aux_lde, &av_lde, !job.public_ready)); // once per proof, in schnorr_build when it overlaps
    job.public_ready = true;
    cs::AirStageRequest rq = air_request(a, job, ta, tb, ba, bb, nullptr, out); // (built-in assertion constants)
    rq.source = cs::AirTransitions::SchnorrFused; rq.d_aux_lde = aux_lde; rq.own_extension = true; // own extensions: split form
    rq.d_avals_lde = av_lde; rq.n_avals = 12;
    return air_stage(c, rq);
}

// one proof on this GPU, on the channel its options allow
int prove(cstark_ctx *c, const cstark_options *opt, AirJob &job, uint8_t *proof, size_t capacity, size_t *proof_len) {
    return use_dev_channel(opt, job) ? prove_core_dev(c, opt, job, proof, capacity, proof_len) : prove_core(c, opt, job, proof, capacity, proof_len);
}


// ---- host steps of the batched range prover (cstark_range_prove_batch) ---------------------------------------------------------------------
// B proofs of the reference's 64-row shape (range_batch.h: RB_N rows, RB_LDE points, W = RB_CE = 2 columns, base field): every device
// stage is one launch over the batch, every channel step a walk over the B coins on a few host threads (transcript.h with m = 1).

// f(i) for every i < count on up to eight host threads.  Nothing escapes: an exception inside a worker (the channel code allocates) or a
// thread that cannot be created ends in CSTARK_ERR_OOM -- these lambdas run inside extern "C" functions, where an escaping exception
// would be std::terminate.
template <class F>
int parallel_for(size_t count, F f) {
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 1 : nt > 8 ? 8 : nt;
    std::atomic<bool> failed{false};
    auto guarded = [&](size_t first, size_t step) {
        try { for (size_t i = first; i < count && !failed.load(std::memory_order_relaxed); i += step) f(i); }
        catch (...) { failed.store(true); }
    };
    if (count < 64 || nt == 1) {
        guarded(0, 1);
    } else {
        std::vector<std::thread> th;
        try {
            th.reserve(nt);
            for (unsigned w = 0; w < nt; w++) th.emplace_back(guarded, (size_t)w, (size_t)nt);
        } catch (...) { failed.store(true); }
        for (std::thread &t : th) t.join();
    }
    return failed.load() ? cs::fail(CSTARK_ERR_OOM, "host allocation or thread creation failed inside a batched channel step") : CSTARK_OK;
}
struct Carver { // consecutive 256-byte aligned pieces of one block; base = null: only the offsets advance (off = the bytes a block needs)
    uint8_t *base; size_t off = 0;
    template <class T> T *take(size_t bytes) { T *q = base ? (T *)(base + off) : nullptr; off += (bytes + 255) & ~(size_t)255; return q; }
};

constexpr size_t RB_W = 2, RB_NC = 2, RB_NA = 2;                   // registers, transition constraints, assertions (src/range/air.rs:60-105)
constexpr size_t RB_COEFS = transcript::coefficient_draws(RB_NC, RB_NA); // t_alpha[2] t_beta[2] b_alpha[2] b_beta[2]
constexpr size_t RB_FRAME = 2 * RB_W + RB_CE;                      // T(z) | T(z w) | H_i(z^2)
constexpr size_t RB_DEEP = RB_FRAME + 2;                           // alpha[2] beta[2] delta[2] deg_a deg_b

struct RangeBatch {
    cstark_ctx *c; const cstark_options *opt; const uint64_t *numbers; size_t B;
    ProofShape S; OpenBlock O; // O: one proof's slot of the opening block, room for nq positions in the layer
    unsigned log_rem;
    hipStream_t st;
    RangeBatchConsts K{};
    std::vector<Coin> coins;
    std::vector<uint64_t> nonces;
    std::vector<uint8_t> rem_commit;
    // the device block: per proof the tables, trees and channel values of range_batch.h
    uint64_t *d_canon, *d_num, *d_trace, *d_coeffs, *d_lde, *d_coefs, *d_comb, *d_ccoef, *d_clde, *d_z, *d_ood, *d_dcoef, *d_layer, *d_alpha, *d_rem;
    uint8_t *d_tnodes, *d_cnodes, *d_lnodes, *d_open;
    uint32_t *d_pos, *d_lpos, *d_lcount, *d_gseed;
    unsigned long long *d_gfound;
    // the pinned host block: what the channel reads and the proof bytes are written from
    uint8_t *h_troot, *h_croot, *h_lroot, *h_open;
    uint64_t *h_coefs, *h_ood, *h_dcoef, *h_z, *h_alpha, *h_rem;
    uint32_t *h_pos, *h_lpos, *h_lcount, *h_gseed;
    unsigned long long *h_gfound;
    size_t dev_bytes, host_bytes;


    // every piece of both blocks, once: over null bases this measures them, over the blocks it places the pointers
    void carve(uint8_t *dev, uint8_t *host) {
        Carver D{dev}, H{host};
        const size_t col = RB_N * 8, ext = RB_LDE * 8, tree = 2 * RB_LDE * 32, nq = S.nq; // bytes: a column, its extension, a tree over RB_LDE leaves
        d_canon = D.take<uint64_t>(B * 8); d_num = D.take<uint64_t>(B * 8);
        d_trace = D.take<uint64_t>(B * RB_W * col); d_coeffs = D.take<uint64_t>(B * RB_W * col); d_lde = D.take<uint64_t>(B * RB_W * ext);
        d_coefs = D.take<uint64_t>(B * RB_COEFS * 8);
        d_comb = D.take<uint64_t>(B * RB_CE * col); d_ccoef = D.take<uint64_t>(B * RB_CE * col); d_clde = D.take<uint64_t>(B * RB_CE * ext);
        d_z = D.take<uint64_t>(B * 8); d_ood = D.take<uint64_t>(B * RB_FRAME * 8); d_dcoef = D.take<uint64_t>(B * RB_DEEP * 8);
        d_layer = D.take<uint64_t>(B * ext); d_alpha = D.take<uint64_t>(B * 8); d_rem = D.take<uint64_t>(B * remainder_bytes(S));
        d_tnodes = D.take<uint8_t>(B * tree); d_cnodes = D.take<uint8_t>(B * tree); d_lnodes = D.take<uint8_t>(B * ((size_t)64 << layer_log_rows(S, 0)));
        d_pos = D.take<uint32_t>(B * nq * 4); d_lpos = D.take<uint32_t>(B * nq * 4); d_lcount = D.take<uint32_t>(B * 4);
        d_open = D.take<uint8_t>(B * O.bytes);
        d_gseed = D.take<uint32_t>(B * 32); d_gfound = D.take<unsigned long long>(B * 8);
        h_troot = H.take<uint8_t>(B * 32); h_croot = H.take<uint8_t>(B * 32); h_lroot = H.take<uint8_t>(B * 32);
        h_coefs = H.take<uint64_t>(B * RB_COEFS * 8); h_ood = H.take<uint64_t>(B * RB_FRAME * 8); h_dcoef = H.take<uint64_t>(B * RB_DEEP * 8);
        h_z = H.take<uint64_t>(B * 8); h_alpha = H.take<uint64_t>(B * 8); h_rem = H.take<uint64_t>(B * remainder_bytes(S));
        h_pos = H.take<uint32_t>(B * nq * 4); h_lpos = H.take<uint32_t>(B * nq * 4); h_lcount = H.take<uint32_t>(B * 4);
        h_open = H.take<uint8_t>(B * O.bytes);
        h_gseed = H.take<uint32_t>(B * 32); h_gfound = H.take<unsigned long long>(B * 8);
        dev_bytes = D.off; host_bytes = H.off;
    }
    // one device block and one pinned host block of the context, kept across calls and replaced when a call needs more; the constants
    int buffers() {
        carve(nullptr, nullptr);
        if (c->rb_dev_bytes < dev_bytes) {
            HIP_TRY(hipStreamSynchronize(st));
            if (c->rb_dev) { HIP_TRY(hipFree(c->rb_dev)); c->rb_dev = nullptr; c->rb_dev_bytes = 0; }
            HIP_TRY(hipMalloc(&c->rb_dev, dev_bytes));
            c->rb_dev_bytes = dev_bytes;
        }
        if (c->rb_host_bytes < host_bytes) {
            HIP_TRY(hipStreamSynchronize(st));
            if (c->rb_host) { HIP_TRY(hipHostFree(c->rb_host)); c->rb_host = nullptr; c->rb_host_bytes = 0; }
            HIP_TRY(hipHostMalloc(&c->rb_host, host_bytes, hipHostMallocDefault));
            c->rb_host_bytes = host_bytes;
        }
        carve((uint8_t *)c->rb_dev, (uint8_t *)c->rb_host);
        coins.resize(B); nonces.resize(B); rem_commit.resize(32 * B);

        using namespace cs::host;
        const uint64_t n = RB_N, cen = n * RB_CE, wN = root_of_unity(S.log_N), g = lde_offset();
        uint64_t sh = g;
        for (int k = 0; k < 8; k++) { K.shift[k] = sh; K.zinv[k] = inv(sub(pow(sh, n), ONE)); sh = mul(sh, wN); }
        K.w_last = inv(root_of_unity(RB_LOG_N));
        K.adj[0] = CSTARK_CONV_TRANSITION_ADJUSTMENT(cen, n, 2 * (n - 1)); // degrees (2), (1): src/range/air.rs:100-105
        K.adj[1] = CSTARK_CONV_TRANSITION_ADJUSTMENT(cen, n, 1 * (n - 1));
        K.badj = CSTARK_CONV_BOUNDARY_ADJUSTMENT(cen, n, 1);
        K.inv128 = inv(from_u64(cen)); K.ginv = inv(g); K.offset_inv = inv(g); K.inv4 = inv(from_u64(4));
        const uint64_t *unused;
        RC_TRY(plan_tables(c, RB_LOG_N, &K.w64, &unused));
        RC_TRY(plan_tables(c, RB_LOG_N + 1, &unused, &K.winv128));
        return plan_tables(c, S.log_N, &unused, &K.winv512);
    }
    // the rows of B tables [2^lb cosets][gw columns][2^ln] hashed into the leaves of B trees, the trees, their roots to the host
    int commit_rows(const uint64_t *tab, unsigned gw, unsigned ln, unsigned lb, uint8_t *nodes, uint8_t *h_root) {
        const size_t leaves = (size_t)1 << (ln + lb), tree = 2 * leaves * 32;
        const unsigned nb = (unsigned)B;
        if (opt->hash_fn == 1) {
            HIP_TRY(hash_rows_batch_sha3(tab, nodes + 32 * leaves, gw, gw * nb, ln, lb, nb, tree, st));
            HIP_TRY(merkle_build_batch_sha3(nodes, ln + lb, nb, tree, st));
        } else {
            HIP_TRY(hash_rows_batch(tab, nodes + 32 * leaves, gw, gw * nb, ln, lb, nb, tree, st));
            HIP_TRY(merkle_build_batch(nodes, ln + lb, nb, tree, st));
        }
        HIP_TRY(hipMemcpy2DAsync(h_root, 32, nodes + 32, tree, 32, B, hipMemcpyDeviceToHost, st));
        return CSTARK_OK;
    }
    int extend(const uint64_t *coef, uint64_t *lde) {
        return cstark_lde_columns(c, coef, lde, (uint32_t)(2 * B), RB_LOG_N, RB_LOG_B, host::lde_offset(), 0, 1u << RB_LOG_B);
    }

    // trace, interpolation, extension, commitment; returns once the roots are on the host (`canon` and the caller's numbers have been read)
    int trace_to_root(const uint64_t *canon) {
        HIP_TRY(hipMemcpyAsync(d_canon, canon, B * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_num, numbers, B * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(rb_trace(d_canon, d_trace, (unsigned)B, st));
        RC_TRY(cstark_interpolate_columns(c, d_trace, d_coeffs, (uint32_t)(RB_W * B), RB_LOG_N));
        RC_TRY(extend(d_coeffs, d_lde));
        RC_TRY(commit_rows(d_lde, RB_W, RB_LOG_N, RB_LOG_B, d_tnodes, h_troot));
        HIP_TRY(cs::stream_wait(st));
        return CSTARK_OK;
    }
    int coefficients() {
        return parallel_for(B, [&](size_t t) {
            const std::vector<uint8_t> seed = channel_seed(S.width, S.log_n, *opt, S.log_b, log_rem, &numbers[t], 1); // PublicInputs: the number (src/range/air.rs:26-36)
            transcript::open(coins[t], opt->hash_fn, seed.data(), seed.size(), h_troot + 32 * t);
            uint64_t dr[RB_COEFS], *cf = h_coefs + RB_COEFS * t;
            transcript::draw_coefficients(coins[t], 1, RB_NC, RB_NA, dr, {{cf}, {cf + RB_NC}, {cf + 2 * RB_NC}, {cf + 2 * RB_NC + RB_NA}});
        });
    }
    // constraint evaluation, composition polynomial and its commitment; returns once the roots are on the host
    int constraints_to_root() {
        HIP_TRY(hipMemcpyAsync(d_coefs, h_coefs, B * RB_COEFS * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(rb_combine(K, d_lde, d_coefs, d_num, d_comb, (unsigned)B, st));
        HIP_TRY(rb_composition(K, d_comb, d_ccoef, (unsigned)B, st));
        RC_TRY(extend(d_ccoef, d_clde));
        RC_TRY(commit_rows(d_clde, RB_CE, RB_LOG_N, RB_LOG_B, d_cnodes, h_croot));
        HIP_TRY(cs::stream_wait(st));
        return CSTARK_OK;
    }
    // the out-of-domain points, the frames, and the DEEP coefficients drawn after them
    int frame() {
        RC_TRY(parallel_for(B, [&](size_t t) { transcript::draw_ood_point(coins[t], h_croot + 32 * t, 1, h_z + t); }));
        HIP_TRY(hipMemcpyAsync(d_z, h_z, B * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(rb_ood(K, d_coeffs, d_ccoef, d_z, d_ood, (unsigned)B, st));
        HIP_TRY(hipMemcpyAsync(h_ood, d_ood, B * RB_FRAME * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(cs::stream_wait(st));
        return parallel_for(B, [&](size_t t) {
            const uint64_t *f = h_ood + RB_FRAME * t;
            transcript::absorb_frame(coins[t], 1, RB_W, RB_CE, f, f + 2 * RB_W);
            uint64_t dr[transcript::deep_draws(RB_W, RB_CE)], *cf = h_dcoef + RB_DEEP * t;
            transcript::draw_deep(coins[t], 1, RB_W, RB_CE, dr, cf, cf + RB_W, cf + 2 * RB_W, cf + RB_FRAME, cf + RB_FRAME + 1);
        });
    }
    int deep() {
        HIP_TRY(hipMemcpyAsync(d_dcoef, h_dcoef, B * RB_DEEP * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(rb_deep(K, d_lde, d_clde, d_z, d_ood, d_dcoef, d_layer, (unsigned)B, st));
        return CSTARK_OK;
    }
    // at most one layer for a 512-point domain (remainder 128 .. 1024); returns once the remainders are on the host
    int fri() {
        if (S.n_layers) { // rows { e[i + t rows] }: table t = [f][rows] inside its 512 words
            RC_TRY(commit_rows(d_layer, S.f, layer_log_rows(S, 0), 0, d_lnodes, h_lroot));
            HIP_TRY(cs::stream_wait(st));
            RC_TRY(parallel_for(B, [&](size_t t) { transcript::fri_layer(coins[t], h_lroot + 32 * t, 1, h_alpha + t); }));
            HIP_TRY(hipMemcpyAsync(d_alpha, h_alpha, B * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(rb_fold(K, d_layer, d_alpha, d_rem, (unsigned)B, st));
        }
        HIP_TRY(hipMemcpyAsync(h_rem, S.n_layers ? d_rem : d_layer, B * remainder_bytes(S), hipMemcpyDeviceToHost, st));
        HIP_TRY(cs::stream_wait(st));
        return CSTARK_OK;
    }
    // Remainder commitments, proof of work, query positions.  From 12 bits on all B searches run on the device, chunk after chunk in
    // increasing order, until every proof has its smallest nonce (grind_nonce above: the single-proof form); below, each proof's
    // sequential search on its host thread.
    int queries() {
        static const bool grind_dev_env = [] { const char *e = getenv("CSTARK_GRIND_DEVICE"); return !e || atoi(e) != 0; }();
        const unsigned bits = opt->grinding_factor;
        const bool grind_dev = grind_dev_env && bits >= 12;
        auto commit = [&](size_t t) { transcript::commit_remainder(coins[t], h_rem + S.R * t, S.R, &rem_commit[32 * t]); };
        if (grind_dev) {
            RC_TRY(parallel_for(B, [&](size_t t) {
                commit(t);
                memcpy(h_gseed + 8 * t, coins[t].seed, 32);
                h_gfound[t] = ~0ull;
            }));
            HIP_TRY(hipMemcpyAsync(d_gseed, h_gseed, B * 32, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_gfound, h_gfound, B * 8, hipMemcpyHostToDevice, st));
            uint64_t chunk = (uint64_t)4 << bits;                // four expected hits per proof and chunk
            while (chunk * B > ((uint64_t)1 << 28)) chunk >>= 1; // at most 2^28 nonces per launch
            if (chunk < 256) chunk = 256;
            for (uint64_t base = 1;; base += chunk) {
                if (opt->hash_fn == 1) HIP_TRY(cs::grind_batch_chunk_sha3((const uint64_t *)d_gseed, (unsigned)B, base, chunk, bits, d_gfound, st));
                else HIP_TRY(cs::grind_batch_chunk(d_gseed, (unsigned)B, base, chunk, bits, d_gfound, st));
                HIP_TRY(hipMemcpyAsync(h_gfound, d_gfound, B * 8, hipMemcpyDeviceToHost, st));
                HIP_TRY(cs::stream_wait(st));
                bool all = true;
                for (size_t t = 0; t < B; t++) all = all && h_gfound[t] != ~0ull;
                if (all) break;
                if (base > ((uint64_t)1 << 44)) return fail(CSTARK_ERR_HIP, "proof of work: no nonce found");
            }
        }
        return parallel_for(B, [&](size_t t) {
            if (grind_dev) nonces[t] = h_gfound[t];
            else { commit(t); nonces[t] = transcript::host_nonce(coins[t], bits); }
            h_lcount[t] = 0;
            transcript::draw_queries(coins[t], S, nonces[t], h_pos + S.nq * t, h_lpos + S.nq * t, 0, h_lcount + t);
        });
    }
    // the openings of every proof into its slot of the block, the block to the host
    int open() {
        const size_t nq = S.nq;
        HIP_TRY(hipMemcpyAsync(d_pos, h_pos, B * nq * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_lpos, h_lpos, B * nq * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_lcount, h_lcount, B * 4, hipMemcpyHostToDevice, st));
        const RangeBatchOpen o{d_lde, d_clde, d_layer, d_tnodes, d_cnodes, d_lnodes, d_pos, d_lpos, d_lcount, d_open, (uint32_t)nq, (uint32_t)B, S.n_layers,
                               O.bytes, O.trows, O.tpaths, O.crows, O.cpaths, O.lrows[0], O.lpaths[0]};
        HIP_TRY(rb_open(o, st));
        HIP_TRY(hipMemcpyAsync(h_open, d_open, B * O.bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(cs::stream_wait(st));
        return CSTARK_OK;
    }
    // the proof bytes, proof t at proofs + stride t (the caller has checked that any proof of this shape fits a stride)
    int write(uint8_t *proofs, size_t stride, size_t *lens) {
        const uint32_t form = ctx_proof_form(c);
        return parallel_for(B, [&](size_t t) {
            const uint64_t *f = h_ood + RB_FRAME * t;
            ProofParts p{};
            p.trace_root = h_troot + 32 * t; p.cons_root = h_croot + 32 * t; p.layer_roots = h_lroot + 32 * t; p.rem_commit = &rem_commit[32 * t];
            p.ood_trace = f; p.ood_comp = f + 2 * RB_W; p.nonce = nonces[t]; p.remainder = h_rem + S.R * t;
            // the positions of proof t and, B * nq words behind them, its folded ones: h_lpos follows h_pos in the block
            (void)finish_proof(S, p, h_open + O.bytes * t, O, h_lcount + t, form, h_pos + S.nq * t, (size_t)(h_lpos - h_pos), proofs + stride * t, stride, &lens[t]);
        });
    }
};

} // namespace
} // namespace cs

using namespace cs;

int gather_jobs_launch(cstark_ctx *c, const cstark_gather_desc *jobs, uint32_t n_jobs) {
    if (!c || !jobs || n_jobs == 0 || n_jobs > (uint32_t)MAX_GATHER_JOBS) return fail(CSTARK_ERR_INVALID_ARG, "gather_jobs_launch: 1 .. 32 jobs");
    GatherList gl;
    for (uint32_t i = 0; i < n_jobs; i++) {
        const cstark_gather_desc &j = jobs[i];
        if (j.paths) gl.paths((const uint8_t *)j.src, j.a, j.d_pos, j.out, j.count, j.d_count, j.lvl0);
        else gl.rows((const uint64_t *)j.src, j.a, j.log_n, j.log_b, j.d_pos, j.out, j.count, j.log_s, j.d_count);
    }
    HIP_TRY(gl.launch(c->stream));
    return CSTARK_OK;
}

extern "C" {

int cstark_tx_prove(cstark_ctx *c, const cstark_options *opt, uint8_t *proof, size_t capacity, size_t *proof_len) {
    if (!c || !opt || !proof_len) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_prove: null argument");
    if (!c->wit_buf || c->wit.n_tx == 0 || c->wit.msg_tail) return fail(CSTARK_ERR_INVALID_ARG, "no transaction witness uploaded");
    if (c->wit.n_tx & (c->wit.n_tx - 1)) return fail(CSTARK_ERR_INVALID_ARG, "the number of transactions must be a power of two");
    AirJob job;
    job.air = CSTARK_AIR_STATE_TRANSITION; job.width = CSTARK_TX_TRACE_WIDTH; job.log_n = 10 + ceil_log2(c->wit.n_tx); job.log_ce = 3;
    job.n_constraints = CSTARK_TX_NUM_CONSTRAINTS; job.n_assertions = 4; job.item = c->wit.depth;
    job.build = tx_build; job.combine = tx_combine; job.combine_sets = tx_combine_sets;
    return prove(c, opt, job, proof, capacity, proof_len);
}

int cstark_air_prove(cstark_ctx *c, int air, const cstark_options *opt, uint64_t number, uint8_t *proof, size_t capacity, size_t *proof_len) {
    if (!c || !opt || !proof_len) return fail(CSTARK_ERR_INVALID_ARG, "cstark_air_prove: null argument");
    if (air == CSTARK_AIR_STATE_TRANSITION) return cstark_tx_prove(c, opt, proof, capacity, proof_len);
    AirJob job;
    job.air = air;
    host::AirShape s;
    if (air == CSTARK_AIR_MERKLE_UPDATE) {
        if (!c->wit_buf || c->wit.n_tx == 0 || c->wit.msg_tail) return fail(CSTARK_ERR_INVALID_ARG, "no transaction witness uploaded");
        if (c->wit.n_tx & (c->wit.n_tx - 1)) return fail(CSTARK_ERR_INVALID_ARG, "the number of transactions must be a power of two");
        host::air_shape(air, s, 0);
        job.log_n = 9 + ceil_log2(c->wit.n_tx); job.item = c->wit.depth;
        job.build = merkle_build; job.combine = merkle_combine;
    } else if (air == CSTARK_AIR_RANGE) {
        if (number >= host::P || (host::to_u64(number) >> 63)) return fail(CSTARK_ERR_INVALID_ARG, "range proofs cover 63-bit field elements (src/range/tests.rs:54-62)");
        // One 64-row proof is host-API bound either way.  The batch prover with a batch of one makes the same bytes from ~25 launches
        // instead of ~150 (CSTARK_RANGE_VIA_BATCH=1): 0.30 against 0.36 ms in a process that does nothing else, but 0.48 against 0.38 ms
        // inside bench.py's process (other contexts alive) -- so the generic path stays the default (profiles/r03_range_single.txt).
        static const bool via_batch = [] { const char *e = getenv("CSTARK_RANGE_VIA_BATCH"); return e && atoi(e) != 0; }();
        if (via_batch && opt->field_extension == 0 && opt->blowup_factor == 8 && opt->fri_folding_factor == 4 && proof && capacity >= cstark_tx_proof_size_bound(1, opt))
            return cstark_range_prove_batch(c, opt, &number, 1, proof, capacity, proof_len);
        host::air_shape(air, s, 0);
        job.log_n = 6; job.item = 0; job.number = number; // RANGE_LOG = 64 rows, src/range/mod.rs:34
        job.pub = {number};
        job.build = range_build; job.combine = range_combine;
    } else if (air == CSTARK_AIR_SCHNORR) {
        if (!c->wit_buf || c->wit.n_tx == 0 || !c->wit.msg_tail) return fail(CSTARK_ERR_INVALID_ARG, "no Schnorr witness uploaded");
        const uint32_t ns = c->wit.n_tx;
        if (ns & (ns - 1)) return fail(CSTARK_ERR_INVALID_ARG, "the number of signatures must be a power of two");
        host::air_shape(air, s, ns);
        job.log_n = 9 + ceil_log2(ns); job.item = ns;
        job.pub = c->schnorr_pub; // messages [ns][28] then R.x [ns][6] (src/schnorr/air.rs:29-38)
        job.pub_bytes = c->schnorr_s;
        job.build = schnorr_build; job.combine = schnorr_combine;
    } else {
        return fail(CSTARK_ERR_UNSUPPORTED, "no prover for this AIR");
    }
    job.width = s.width; job.n_constraints = s.n_constraints; job.n_assertions = (uint32_t)s.a_reg.size(); job.log_ce = s.log_ce_blowup();
    return prove(c, opt, job, proof, capacity, proof_len);
}

// ---- one proof across several GPUs by LDE coset -------------------------------------------------------------------------
// Every rank holds the witness and calls the phases in the same order; the caller moves the three exchanged buffers between the
// ranks (RCCL all-gather / all-reduce through torch.distributed in sharding.py).  Trace generation and interpolation are replicated
// (every rank needs all coefficient columns for its cosets), extension / row hashing / constraint evaluation run on the rank's cosets,
// everything after the merged evaluations on the rank that owns coset 0.
static int shard_run(cstark_ctx *c, int min_phase, ProofRun **out) {
    if (!c || !c->arena || !c->arena->run || c->arena->run->phase < min_phase) return fail(CSTARK_ERR_INVALID_ARG, "sharded proof: phase called out of order");
    *out = c->arena->run;
    return CSTARK_OK;
}
int cstark_tx_shard_commit(cstark_ctx *c, const cstark_options *opt, uint32_t k0, uint32_t nk, uint8_t *d_leaves_local) {
    if (!c || !opt || !d_leaves_local) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_shard_commit: null argument");
    if (ctx_proof_form(c) != CSTARK_FORM_PLAIN) return fail(CSTARK_ERR_UNSUPPORTED, "sharded proofs are written in the plain form only");
    if (!c->wit_buf || c->wit.n_tx == 0 || c->wit.msg_tail) return fail(CSTARK_ERR_INVALID_ARG, "no transaction witness uploaded");
    if (c->wit.n_tx & (c->wit.n_tx - 1)) return fail(CSTARK_ERR_INVALID_ARG, "the number of transactions must be a power of two");
    if (nk == 0 || nk >= 8 || (nk & (nk - 1)) || k0 % nk || k0 + nk > 8) return fail(CSTARK_ERR_INVALID_ARG, "a rank owns 1, 2 or 4 consecutive cosets of the 8 (world size 8, 4 or 2)");
    if (opt->field_extension != 0) return fail(CSTARK_ERR_UNSUPPORTED, "sharded proofs use FieldExtension::None");
    AirJob job;
    job.air = CSTARK_AIR_STATE_TRANSITION; job.width = CSTARK_TX_TRACE_WIDTH; job.log_n = 10 + ceil_log2(c->wit.n_tx); job.log_ce = 3;
    job.n_constraints = CSTARK_TX_NUM_CONSTRAINTS; job.n_assertions = 4; job.item = c->wit.depth;
    job.build = tx_build; job.combine = tx_combine;
    job.k0 = k0; job.nk = nk; job.sharded = true;
    ProofRun *R = new (std::nothrow) ProofRun();
    if (!R) return fail(CSTARK_ERR_OOM, "host allocation failed");
    ProveArena *a = nullptr;
    int rc = run_setup(c, opt, job, *R, &a); // ends any earlier run on this context (get_arena)
    if (rc) { delete R; return rc; }
    a->run = R;
    rc = phase_commit(c, a, *R, d_leaves_local);
    if (rc) { proof_run_free(a->run); a->run = nullptr; }
    return rc;
}
uint32_t cstark_tx_shard_rows(uint32_t nk) { return (nk == 1 || nk == 2 || nk == 4) ? shard_rows(nk) : 0; }
uint32_t cstark_tx_shard_open_words(uint32_t nk) { return (nk == 1 || nk == 2 || nk == 4) ? CSTARK_TX_TRACE_WIDTH + 4 * ceil_log2(nk) : 0; }
int cstark_tx_shard_evaluate(cstark_ctx *c, const uint8_t *d_leaves_all, uint64_t *d_combined_local, uint32_t rows) {
    ProofRun *R;
    RC_TRY(shard_run(c, 1, &R));
    if (!d_leaves_all || !d_combined_local) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_shard_evaluate: null argument");
    // the caller sized d_combined_local [rows][n]: the count depends on nk AND on the evaluation mode of this process (shard_rows)
    if (rows != shard_rows(R->job.nk)) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_shard_evaluate: rows differs from cstark_tx_shard_rows(nk)");
    return phase_evaluate(c, c->arena, *R, d_leaves_all, d_combined_local);
}
int cstark_tx_shard_compose(cstark_ctx *c, const uint64_t *d_combined_all, uint32_t total_rows, uint32_t *positions /* host [num_queries] */) {
    ProofRun *R;
    RC_TRY(shard_run(c, 2, &R));
    if (!d_combined_all || !positions) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_shard_compose: null argument");
    // every rank must have handed over the same number of rows (ranks whose CSTARK_SHARD_SPLIT differs would not)
    if (total_rows != (8 / R->job.nk) * shard_rows(R->job.nk)) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_shard_compose: total_rows differs from W * cstark_tx_shard_rows(nk)");
    ProveArena *a = c->arena;
    const size_t N = (size_t)8 << R->job.log_n;
    if (shard_split(R->job.nk)) RC_TRY(tx_shard_combine(c, d_combined_all, a->combined, R->job.log_n, R->job.nk)); // the ranks' shares -> [8][n]
    else if (d_combined_all != a->combined) HIP_TRY(hipMemcpyAsync(a->combined, d_combined_all, N * 8, hipMemcpyDeviceToDevice, c->stream));
    RC_TRY(phase_compose(c, a, *R));
    memcpy(positions, R->q.hpos.data(), R->opt.num_queries * 4);
    return CSTARK_OK;
}
int cstark_tx_shard_open_rows(cstark_ctx *c, const uint32_t *positions, uint32_t nq, uint64_t *d_rows) {
    ProofRun *R;
    RC_TRY(shard_run(c, 2, &R));
    if (!positions || !d_rows) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_shard_open_rows: null argument");
    // d_rows is sized by the caller's nq and read back as num_queries rows by cstark_tx_shard_finish: they must agree
    if (nq != R->opt.num_queries) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_shard_open_rows: nq differs from the proof's num_queries");
    const uint32_t N = 8u << R->job.log_n;
    for (uint32_t q = 0; q < nq; q++)
        if (positions[q] >= N) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_shard_open_rows: position outside the LDE domain");
    ProveArena *a = c->arena;
    HIP_TRY(hipMemcpyAsync(a->d_pos, positions, nq * 4, hipMemcpyHostToDevice, c->stream));
    const uint32_t log_nk = ceil_log2(R->job.nk);
    const uint64_t *sub = log_nk ? (const uint64_t *)a->extra[45] : nullptr; // the rank's subtree heap (phase_commit)
    k_gather_rows_window<<<nq, 128, 0, c->stream>>>(a->lde, R->job.width, R->job.log_n, 3, R->job.k0, R->job.nk, a->d_pos, d_rows, sub, log_nk);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream)); // the caller's positions may be transient
    return CSTARK_OK;
}
int cstark_tx_shard_finish(cstark_ctx *c, const uint64_t *d_rows, uint8_t *proof, size_t capacity, size_t *proof_len) {
    if (c && ctx_proof_form(c) != CSTARK_FORM_PLAIN) return fail(CSTARK_ERR_UNSUPPORTED, "sharded proofs are written in the plain form only");
    ProofRun *R;
    RC_TRY(shard_run(c, 3, &R));
    if (!d_rows || !proof_len) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_shard_finish: null argument");
    if (R->job.k0 != 0) return fail(CSTARK_ERR_INVALID_ARG, "cstark_tx_shard_finish runs on the rank that owns coset 0");
    const int rc = phase_open(c, c->arena, *R, d_rows, proof, capacity, proof_len);
    if (rc == CSTARK_OK) { proof_run_free(c->arena->run); c->arena->run = nullptr; }
    return rc;
}

// RescueExample::prove (benches/rescue.rs:66-86): a chain of `chain_length` Rescue hashes from `seed` (7 elements, memory form)
int cstark_rescue_prove(cstark_ctx *c, const cstark_options *opt, const uint64_t seed[7], uint32_t chain_length, uint8_t *proof, size_t capacity,
                        size_t *proof_len) {
    if (!c || !opt || !seed || !proof_len) return fail(CSTARK_ERR_INVALID_ARG, "cstark_rescue_prove: null argument");
    if (chain_length < 8 || (chain_length & (chain_length - 1)) || chain_length > (1u << 21))
        return fail(CSTARK_ERR_INVALID_ARG, "chain length must be a power of two, 8 .. 2^21 (benches/rescue.rs:34-37)");
    for (int i = 0; i < 7; i++) if (seed[i] >= host::P) return fail(CSTARK_ERR_INVALID_ARG, "seed is not a field element");
    AirJob job;
    job.air = CSTARK_AIR_RESCUE_CHAIN;
    host::AirShape s;
    host::air_shape(CSTARK_AIR_RESCUE_CHAIN, s, 0);
    job.log_n = 3 + ceil_log2(chain_length); job.item = chain_length;
    memcpy(job.seed, seed, sizeof job.seed);
    job.build = rescue_build; job.combine = rescue_combine;
    job.width = s.width; job.n_constraints = s.n_constraints; job.n_assertions = (uint32_t)s.a_reg.size(); job.log_ce = s.log_ce_blowup();
    return prove(c, opt, job, proof, capacity, proof_len);
}

// RangeProofAir over 2^log_n rows (synthetic long form; log_n = 6 with a one-word value is cstark_air_prove(CSTARK_AIR_RANGE))
int cstark_range_prove_bits(cstark_ctx *c, const cstark_options *opt, const uint64_t *words, uint32_t log_n, uint8_t *proof, size_t capacity,
                            size_t *proof_len) {
    if (!c || !opt || !words || !proof_len) return fail(CSTARK_ERR_INVALID_ARG, "cstark_range_prove_bits: null argument");
    if (log_n < 6 || log_n > 21) return fail(CSTARK_ERR_INVALID_ARG, "trace length must be 2^6 .. 2^21");
    const size_t nw = (size_t)1 << (log_n - 6);
    if (words[nw - 1] >> 63) return fail(CSTARK_ERR_INVALID_ARG, "the value must have at most n - 1 bits");
    uint64_t number = 0; // V mod p, memory form: Horner in base 2^64
    for (size_t i = nw; i-- > 0;) number = host::add(host::mul(number, host::R2), host::from_u64(words[i] % host::P));
    AirJob job;
    job.air = CSTARK_AIR_RANGE;
    host::AirShape s;
    host::air_shape(CSTARK_AIR_RANGE, s, 0);
    job.log_n = log_n; job.item = 0; job.number = number; job.bits = words;
    job.pub = {number};
    job.build = range_build; job.combine = range_combine;
    job.width = s.width; job.n_constraints = s.n_constraints; job.n_assertions = (uint32_t)s.a_reg.size(); job.log_ce = s.log_ce_blowup();
    return prove(c, opt, job, proof, capacity, proof_len);
}

// ---- B reference-shaped range proofs in one call (RangeProofExample::prove, src/range/mod.rs:75-100, benches/range.rs:15-37) ---------
// Every stage is one launch over the batch (range_batch.hip; interpolation and extension of the 2 B columns through the generic
// transform kernels), the host walks the B Fiat-Shamir channels between the stages on a few threads.  Same protocol, same bytes as
// prove_core for CSTARK_AIR_RANGE, from the same pieces: the channel steps are transcript.h's, the sizes proof_layout.h's, the opening
// slot an OpenBlock, the bytes finish_proof's.  The stages (RangeBatch above): buffers; trace to root; coefficients; constraints to
// root; frame and DEEP coefficients; DEEP composition; FRI; remainder, nonce and positions; openings; bytes.
int cstark_range_prove_batch(cstark_ctx *c, const cstark_options *opt, const uint64_t *numbers, uint32_t count, uint8_t *proofs, size_t stride, size_t *lens) {
    if (!c || !opt || !numbers || !proofs || !lens || count == 0) return fail(CSTARK_ERR_INVALID_ARG, "cstark_range_prove_batch: null argument");
    // the transforms of the 2 * count columns are one launch with the column index in grid.y (at most 65535): 32768 proofs per call
    if (count > 32768) return fail(CSTARK_ERR_INVALID_ARG, "cstark_range_prove_batch: at most 32768 proofs per call");
    if (opt->field_extension != 0) return fail(CSTARK_ERR_UNSUPPORTED, "cstark_range_prove_batch: FieldExtension::None only (use cstark_air_prove)");
    unsigned log_rem = 0, log_b_opt = 3, log_f_opt = 2;
    RC_TRY(check_options(opt, 1, &log_rem, &log_b_opt, &log_f_opt));
    if (log_b_opt != RB_LOG_B || log_f_opt != 2) {
        // the one-launch-per-stage kernels (range_batch.hip) are laid out for the reference's get_example options (blowup 8, folding 4,
        // src/range/mod.rs:44-50); other option values go through the generic prover one proof at a time -- same bytes
        for (uint32_t t = 0; t < count; t++)
            RC_TRY(cstark_air_prove(c, CSTARK_AIR_RANGE, opt, numbers[t], proofs + stride * t, stride, &lens[t]));
        return CSTARK_OK;
    }
    const ProofShape S = proof_shape(CSTARK_AIR_RANGE, AIR_WIDTH[CSTARK_AIR_RANGE], RB_LOG_N, 0, *opt);
    if (S.nq > RB_LDE / 4) return fail(CSTARK_ERR_INVALID_ARG, "more queries than the domain supports");
    std::vector<uint64_t> canon(count);
    for (size_t t = 0; t < count; t++) {
        if (numbers[t] >= host::P) return fail(CSTARK_ERR_INVALID_ARG, "number is not a field element");
        canon[t] = host::to_u64(numbers[t]);
        if (canon[t] >> 63) return fail(CSTARK_ERR_INVALID_ARG, "range proofs cover 63-bit field elements (src/range/tests.rs:54-62)");
    }
    // the longest proof of this shape and form: nq distinct positions in every layer
    if (stride < proof_size_bound(S, ctx_proof_form(c))) return fail(CSTARK_ERR_INVALID_ARG, "cstark_range_prove_batch: stride too small (cstark_tx_proof_size_bound(1, opt) is sufficient)");
    HIP_TRY(hipSetDevice(c->device));
    if (c->arena) c->arena->timed = false; // cstark_prove_stage_ms describes the generic prover's last proof: none after a batch

    static const bool rb_prof = getenv("CSTARK_RB_PROF") != nullptr; // debugging: host wall-clock of the phases on stderr
    auto t_prev = std::chrono::steady_clock::now();
    auto mark = [&](const char *what) {
        if (!rb_prof) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[cstark range batch] %-28s %8.1f us\n", what, std::chrono::duration<double, std::micro>(now - t_prev).count());
        t_prev = now;
    };
    RangeBatch R{c, opt, numbers, count, S, open_block(S, nullptr), log_rem, c->stream};
    RC_TRY(R.buffers());
    mark("setup");
    RC_TRY(R.trace_to_root(canon.data()));
    mark("trace..trace roots (gpu)");
    RC_TRY(R.coefficients());
    mark("coefficients (host)");
    RC_TRY(R.constraints_to_root());
    mark("constraints..comp roots (gpu)");
    RC_TRY(R.frame());
    mark("ood + deep coefficients");
    RC_TRY(R.deep());
    RC_TRY(R.fri());
    mark("deep + fri (gpu + host)");
    RC_TRY(R.queries());
    mark("remainder, positions (host)");
    RC_TRY(R.open());
    RC_TRY(R.write(proofs, stride, lens));
    mark("openings + serialise");
    return CSTARK_OK;
}

size_t cstark_tx_proof_size_bound(uint32_t n_tx, const cstark_options *opt) {
    if (!opt || n_tx == 0) return 0;
    unsigned log_b = 0, log_f = 2;
    while ((1u << log_b) < opt->blowup_factor && log_b < 6) log_b++;
    while ((1u << log_f) < opt->fri_folding_factor && log_f < 4) log_f++;
    unsigned log_N = 10 + log_b;
    while ((1u << (log_N - 10 - log_b)) < n_tx) log_N++;
    const size_t nq = opt->num_queries, layers = log_N / log_f + 1, em = opt->field_extension + 1; // em: words per drawn-field element
    return 4096 + 32 * layers + (2 * 94 + 8) * 8 * em + nq * (94 * 8 + 8 * 8 * em + 2 * log_N * 32) +
           layers * (4 + nq * (((size_t)8 << log_f) * em + log_N * 32)) + 8 * em * (size_t)opt->fri_max_remainder;
}

int cstark_prove_channel(cstark_ctx *c, uint32_t *channel) {
    if (!c || !channel) return fail(CSTARK_ERR_INVALID_ARG, "null argument");
    if (!c->arena || !c->arena->timed) return fail(CSTARK_ERR_INVALID_ARG, "no proof has been generated on this context");
    *channel = c->arena->channel;
    return CSTARK_OK;
}

int cstark_prove_stage_ms(cstark_ctx *c, float *ms /* [CSTARK_PROVE_NUM_STAGES] */) {
    if (!c || !ms) return fail(CSTARK_ERR_INVALID_ARG, "null argument");
    if (!c->arena || !c->arena->timed) return fail(CSTARK_ERR_INVALID_ARG, "no proof has been generated on this context");
    for (int i = 0; i < CSTARK_PROVE_NUM_STAGES; i++) HIP_TRY(hipEventElapsedTime(&ms[i], c->arena->ev[i], c->arena->ev[i + 1]));
    return CSTARK_OK;
}

} // extern "C"
