/* cstark.h -- C ABI of the MI355X-native prover backend for the Topos state-transition AIR.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference (a Rust crate) has no
 * FFI of its own; these entry points are what a Rust shim bound at
 *     impl Prover for TransactionProver            /root/reference/src/prover.rs:101-134
 *     TransactionProver::build_trace               /root/reference/src/prover.rs:37-98
 *     TransactionExample::prove                    /root/reference/src/lib.rs:116-141
 * would call (the binding a maintainer adds is shown in INTEGRATION.md).
 *
 * NOT winterfell-compatible: the reference's engine (winterfell fork, Cargo.toml:20) is absent from its tree.  Field conventions, the
 * Fiat-Shamir coin and the extension polynomials are recalled / assumed (every one a macro in cstark_conventions.h), the channel
 * order and the proof byte layout are this library's own (documented at cstark_tx_prove).  "Bit-exact" in this header always means:
 * against the CPU restatement under oracle/, which is pinned by algebraic known answers and hash test vectors, not by a Rust run.
 * The stage entry points (K1..K6) hand an engine its own objects (LDE values, digests, merged evaluations) and depend on two
 * conventions only (domain offset / root of unity, byte form of hashed elements).
 *
 * Conventions
 *  - Field elements cross the ABI as uint64_t holding the in-memory representation of the
 *    reference's `f63::BaseElement`: Montgomery form, R = 2^64, p = 2^62+2^56+2^55+1, reduced to
 *    [0,p).  A Rust `&[BaseElement]` can therefore be passed without conversion.
 *  - Matrices of field elements are column-major ("one Vec per register", as TraceTable stores
 *    them): element (column c, row r) of a W x N table lives at  base[c * N + r].
 *  - `d_*` pointers are device (HBM) addresses, everything else is host memory.
 *  - All functions return CSTARK_OK (0) or a negative cstark_status; they never abort.  The
 *    reference reports failure through Result / panics (src/lib.rs:140, :212-218).
 *  - The library is re-entrant per context: one cstark_ctx owns one HIP stream and its workspace.
 */
#ifndef CSTARK_H
#define CSTARK_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum cstark_status {
    CSTARK_OK = 0,
    CSTARK_ERR_INVALID_ARG = -1,   /* malformed sizes / null pointers (reference: assert! panics) */
    CSTARK_ERR_NO_DEVICE = -2,     /* no HIP device / kernel image missing: fail loudly, no CPU fallback */
    CSTARK_ERR_HIP = -3,           /* a HIP runtime call failed; see cstark_last_error() */
    CSTARK_ERR_OOM = -4,
    CSTARK_ERR_UNSUPPORTED = -5
} cstark_status;

/* which AIR program (BASELINE.json configs; reference benches/{rescue,range,merkle,schnorr,state_transition}.rs) */
typedef enum cstark_air_id {
    CSTARK_AIR_STATE_TRANSITION = 0, /* TransactionAir, src/air.rs:64-189; 94 registers, 1024 rows / tx */
    CSTARK_AIR_MERKLE_UPDATE = 1,    /* MerkleAir, src/merkle/update/air.rs:36-177; 65 registers, 512 rows / tx */
    CSTARK_AIR_SCHNORR = 2,          /* SchnorrAir, src/schnorr/air.rs:41-300; 56 registers, 512 rows / sig */
    CSTARK_AIR_RANGE = 3,            /* RangeProofAir, src/range/air.rs:23-105; 2 registers, 64 rows */
    CSTARK_AIR_RESCUE_CHAIN = 4      /* RescueAir, benches/rescue.rs:128-360; 14 registers, 8 rows / link (cstark_rescue_prove) */
} cstark_air_id;

#define CSTARK_TX_TRACE_WIDTH 94      /* src/constants.rs:35 */
#define CSTARK_TX_CYCLE_LENGTH 1024   /* src/constants.rs:83 */
#define CSTARK_TX_NUM_CONSTRAINTS 115 /* src/air.rs:76-100 */
#define CSTARK_TX_NUM_PERIODIC 48     /* src/air.rs:195, src/constants.rs:116 */
#define CSTARK_DIGEST_BYTES 32        /* Blake3_256, src/lib.rs:82 */

/* Witness for a batch of transfers: field-for-field the reference's TransactionMetadata
 * (src/lib.rs:183-194).  Field elements in BaseElement memory form (see Conventions). */
typedef struct cstark_tx_witness {
    uint32_t n_tx;                /* number of transactions; a power of two for proving */
    uint32_t merkle_depth;        /* MERKLE_TREE_DEPTH: 15 (src/merkle/constants.rs:25), 3 under cfg(test) (:22) */
    const uint64_t *initial_roots; /* [n_tx][7]   root before each transaction */
    const uint64_t *final_root;    /* [7] */
    const uint64_t *s_old_values;  /* [n_tx][14]  sender leaf: pk.x(6) pk.y(6) balance nonce */
    const uint64_t *r_old_values;  /* [n_tx][14]  receiver leaf */
    const uint64_t *s_indices;     /* [n_tx] */
    const uint64_t *r_indices;     /* [n_tx] */
    const uint64_t *s_paths;       /* [n_tx][merkle_depth+1][7]  [leaf, sibling_0 .. sibling_{d-1}] */
    const uint64_t *r_paths;       /* [n_tx][merkle_depth+1][7]  (after the sender update) */
    const uint64_t *deltas;        /* [n_tx] */
    const uint64_t *sig_rx;        /* [n_tx][6]   signature.0 = R.x */
    const uint8_t *sig_s;          /* [n_tx][32]  signature.1.to_bytes(), little-endian (src/schnorr/trace.rs:133) */
} cstark_tx_witness;

/* Mirror of the 7 ProofOptions fields (src/lib.rs:78-86). */
typedef struct cstark_options {
    uint32_t num_queries;      /* 42; 1..128 */
    uint32_t blowup_factor;    /* 8; 2, 4, 8 or 16 and at least the AIR's constraint-evaluation blowup (see cstark_tx_prove) */
    uint32_t grinding_factor;  /* 0; up to 32 bits of proof of work (Blake3 coin, 12 bits and more: searched on the device) */
    uint32_t hash_fn;          /* 0 = Blake3_256, 1 = Sha3_256 */
    uint32_t field_extension;  /* 0 = None, 1 = Quadratic, 2 = Cubic */
    uint32_t fri_folding_factor; /* 4; 4, 8 or 16 */
    uint32_t fri_max_remainder;  /* 256; 128, 256, 512 or 1024 */
} cstark_options;

/* Composition coefficients for the constraint-evaluation driver (what the engine draws from the
 * public coin after the trace commitment; inputs here so the stage can be tested in isolation). */
typedef struct cstark_tx_coeffs {
    uint64_t t_alpha[CSTARK_TX_NUM_CONSTRAINTS]; /* per transition constraint: (alpha, beta) */
    uint64_t t_beta[CSTARK_TX_NUM_CONSTRAINTS];
    uint64_t b_alpha[4];                         /* boundary assertions in get_assertions order, src/air.rs:175-184 */
    uint64_t b_beta[4];
} cstark_tx_coeffs;

typedef struct cstark_ctx cstark_ctx;

/* ---- context ------------------------------------------------------------------------------- */
/* device < 0: current HIP device.  stream: the hipStream_t every launch of this context goes to
 * (NULL = HIP's default stream).  Work is asynchronous; cstark_ctx_synchronize() waits for it. */
int cstark_ctx_create(int device, void *stream, cstark_ctx **out);
/* The same with a stream of the context's own (non-blocking, destroyed with the context): for callers that do not link HIP, and
 * for several contexts working side by side -- contexts that share a stream (e.g. the default one) serialise their work on it. */
int cstark_ctx_create_own_stream(int device, cstark_ctx **out);
void cstark_ctx_destroy(cstark_ctx *ctx);
const char *cstark_last_error(void);
const char *cstark_version(void);
int cstark_ctx_synchronize(cstark_ctx *ctx);

/* ---- K1: execution trace (replaces TransactionProver::build_trace, src/prover.rs:37-98) ---- */
/* Copies the witness to device memory owned by the context (host -> HBM, ~2.3 KB / tx). */
int cstark_tx_witness_upload(cstark_ctx *ctx, const cstark_tx_witness *w);
/* Fills the 94 x (1024*n_tx) column-major trace at d_trace from the uploaded witness. */
int cstark_tx_build_trace(cstark_ctx *ctx, uint64_t *d_trace);

/* ---- K2/K3: low-degree extension (engine: trace.extend) ------------------------------------- */
/* Field conventions of the engine [UPSTREAM-RECALL]: multiplicative generator (domain offset) and
 * the primitive 2^log_n-th root of unity, in memory form. */
uint64_t cstark_field_generator(void);   /* multiplicative generator of the field (CSTARK_CONV_GENERATOR) */
uint64_t cstark_field_lde_offset(void);  /* domain offset of the STARK's LDE domain (CSTARK_CONV_LDE_OFFSET; the generator unless flipped) */
uint64_t cstark_field_root_of_unity(uint32_t log_n);
/* d_evals: width x n evaluations over the trace domain <w_n> (natural order); it is used as scratch
 * and destroyed.  d_coeffs (distinct buffer): width x n polynomial coefficients, natural order. */
int cstark_interpolate_columns(cstark_ctx *ctx, uint64_t *d_evals, uint64_t *d_coeffs, uint32_t width, uint32_t log_n);
/* d_coeffs: width x n coefficients.  d_lde: cosets [k0, k0+nk) of the blowup-times larger domain,
 * coset-major:  d_lde[((k - k0) * width + c) * n + j] = f_c(offset * w_{bn}^k * w_n^j),
 * i.e. natural LDE-domain index i = b*j + k.  offset = cstark_field_lde_offset() for the STARK domain.
 * Sharding by coset is what distributes one proof over several GPUs. */
int cstark_lde_columns(cstark_ctx *ctx, const uint64_t *d_coeffs, uint64_t *d_lde, uint32_t width, uint32_t log_n,
                       uint32_t log_blowup, uint64_t domain_offset, uint32_t k0, uint32_t nk);
/* Both stages for columns [col0, col0 + ncols) of a table of `width` columns whose values are constant over blocks of block_len rows
 * (a power of two): d_coeffs and d_lde receive what cstark_interpolate_columns and cstark_lde_columns write for these columns, other
 * columns are not touched.  At trace lengths 2^16, 2^18 and 2^20 with block_len >= the square root of the length only the first row of
 * every block is read, d_evals stays intact and no full-length transform of the column is run; at every other shape the columns go
 * through the two calls above (and their part of d_evals is destroyed). */
int cstark_step_columns(cstark_ctx *ctx, uint64_t *d_evals, uint64_t *d_coeffs, uint64_t *d_lde, uint32_t width, uint32_t col0, uint32_t ncols,
                        uint32_t log_n, uint32_t block_len, uint32_t log_blowup, uint64_t domain_offset, uint32_t k0, uint32_t nk);
/* The same for columns with two values per block: one on rows [0, split) of every block and another on rows [split, block_len),
 * 0 < split < block_len.  On the shapes named above rows 0 and split of every block are read. */
int cstark_step2_columns(cstark_ctx *ctx, uint64_t *d_evals, uint64_t *d_coeffs, uint64_t *d_lde, uint32_t width, uint32_t col0, uint32_t ncols,
                         uint32_t log_n, uint32_t block_len, uint32_t split, uint32_t log_blowup, uint64_t domain_offset, uint32_t k0, uint32_t nk);

/* FieldExtension::Quadratic / Cubic: the same three stages over the degree-m extension, m = 2: F_p[u]/(u^2 - 2u - 2), m = 3:
 * F_p[v]/(v^3 + v + 1) [assumption: the two polynomials of the reference's own curve tower, src/utils/ecc.rs:407-648; the fork's
 * choices for f63 are not in the tree].  An element is m consecutive base elements (coefficients of 1, x, x^2).  The trace stays
 * in the base field.
 *   cstark_evaluate_polys_at_ext: base-coefficient columns at one point; out[c][m] on the host.
 *   cstark_deep_composition_ext: all cosets; d_comp_lde holds m n_comp base columns per coset (column m i + k = component k of
 *     composition column i); coefficient / OOD arrays are host arrays of m-tuples; d_out = [m][b][n], component-major.
 *   cstark_fri_fold4_ext / cstark_fri_fold_ext: d_evals = [m][N] component-major -> d_out = [m][N/4] / [m][N/folding_factor]. */
int cstark_evaluate_polys_at_ext(cstark_ctx *ctx, const uint64_t *d_coeffs, uint32_t width, uint32_t log_n, uint32_t m, const uint64_t *z, uint64_t *out);
int cstark_deep_composition_ext(cstark_ctx *ctx, const uint64_t *d_trace_lde, const uint64_t *d_comp_lde, uint32_t width, uint32_t n_comp, uint32_t m,
                                const uint64_t *z, const uint64_t *ood_trace, const uint64_t *ood_comp, const uint64_t *alpha,
                                const uint64_t *beta, const uint64_t *delta, const uint64_t *deg_a, const uint64_t *deg_b, uint64_t *d_out,
                                uint32_t log_n, uint32_t log_blowup);
int cstark_fri_fold4_ext(cstark_ctx *ctx, const uint64_t *d_evals, uint64_t *d_out, uint32_t log_n, uint64_t domain_offset, uint32_t m,
                         const uint64_t *alpha);
int cstark_fri_fold_ext(cstark_ctx *ctx, const uint64_t *d_evals, uint64_t *d_out, uint32_t log_n, uint32_t folding_factor, uint64_t domain_offset,
                        uint32_t m, const uint64_t *alpha);

/* ---- K4/K5: Blake3 row hashing + Merkle tree (engine: build_commitment) ---------------------- */
/* Hash row j of coset k (width elements, 8 bytes LE each, memory form) into leaf i = b*j + k:
 *   d_leaves[32 * i .. 32 * i + 32]. */
int cstark_hash_rows(cstark_ctx *ctx, const uint64_t *d_lde, uint8_t *d_leaves, uint32_t width,
                     uint32_t log_n, uint32_t log_blowup, uint32_t k0, uint32_t nk);
/* d_nodes: 2 * n_leaves digests; nodes[n_leaves + i] = leaf i on input; on return nodes[1] is the
 * root and nodes[i] = Blake3(nodes[2i] || nodes[2i+1]). nodes[0] is zero. */
int cstark_merkle_build(cstark_ctx *ctx, uint8_t *d_nodes, uint32_t log_leaves);
/* The same two stages with the hash function chosen as in cstark_options::hash_fn: 0 = Blake3_256 (identical to the calls above),
 * 1 = Sha3_256 (FIPS 202; a row is absorbed as its 8-byte little-endian words, a parent is SHA3-256 of its two 32-byte children). */
int cstark_hash_rows_fn(cstark_ctx *ctx, uint32_t hash_fn, const uint64_t *d_lde, uint8_t *d_leaves, uint32_t width, uint32_t log_n,
                        uint32_t log_blowup, uint32_t k0, uint32_t nk);
int cstark_merkle_build_fn(cstark_ctx *ctx, uint32_t hash_fn, uint8_t *d_nodes, uint32_t log_leaves);

/* ---- K6/K7: constraint evaluation (Air::evaluate_transition, src/air.rs:114-173, + driver) --- */
/* d_lde: cosets [k0,k0+nk) of the extended 94-column trace, coset-major as cstark_lde_columns writes them; 16-byte aligned.
 * merkle_depth selects the mask columns (src/merkle/constants.rs:21-27).  log_blowup must be 3.
 *
 * All 115 transition-constraint values at every point:  d_out[((k - k0) * 115 + i) * n + j].
 * Parity / debugging entry point (the production path never materialises them). */
int cstark_tx_evaluate_transitions(cstark_ctx *ctx, const uint64_t *d_lde, uint64_t *d_out, uint32_t merkle_depth,
                                   uint32_t log_n, uint32_t log_blowup, uint32_t k0, uint32_t nk);
/* Fused production path: combined constraint evaluations
 *   d_out[(k - k0) * n + j] = sum_i (alpha_i + beta_i x^adj_i) C_i(x) / Z(x) + boundary terms,
 * x = g * w_{bn}^k * w_n^j.  pub_inputs = initial_root[0..2], final_root[0..2] (src/air.rs:175-184). */
int cstark_tx_evaluate_constraints(cstark_ctx *ctx, const uint64_t *d_lde, const cstark_tx_coeffs *coeffs,
                                   const uint64_t pub_inputs[4], uint64_t *d_out, uint32_t merkle_depth,
                                   uint32_t log_n, uint32_t log_blowup, uint32_t k0, uint32_t nk);
/* The same result for a table that IS the low-degree extension of 94 columns of degree < n over all 8 cosets (k0 = 0, nk = 8), e.g.
 * the output of cstark_lde_columns: allows the degree-split evaluation the prover uses (every part except the final
 * addition on the even cosets only, their merged polynomials extended to the odd cosets).  On such a table the output equals
 * cstark_tx_evaluate_constraints bit for bit; on any other table it is undefined (use cstark_tx_evaluate_constraints). */
int cstark_tx_evaluate_constraints_lde(cstark_ctx *ctx, const uint64_t *d_lde, const cstark_tx_coeffs *coeffs,
                                       const uint64_t pub_inputs[4], uint64_t *d_out, uint32_t merkle_depth, uint32_t log_n);
/* The same for m = 1..3 coefficient sets in ONE pass over the frame (the components of a FieldExtension::Quadratic / Cubic
 * proof: extension coefficients multiply base-field constraint values, so the values are computed once and merged m times).
 * coeffs: m consecutive blocks; d_out[(q * nk + (k - k0)) * n + j] = the merged evaluations for block q. */
int cstark_tx_evaluate_constraints_ext(cstark_ctx *ctx, const uint64_t *d_lde, const cstark_tx_coeffs *coeffs, uint32_t m,
                                       const uint64_t pub_inputs[4], uint64_t *d_out, uint32_t merkle_depth,
                                       uint32_t log_n, uint32_t log_blowup, uint32_t k0, uint32_t nk);
/* Both at once: m = 1..3 coefficient sets on a table that IS the low-degree extension over all 8 cosets (the precondition of
 * cstark_tx_evaluate_constraints_lde), evaluated by the degree-split path of an extension-field proof; d_out[(q * 8 + k) * n + j]. */
int cstark_tx_evaluate_constraints_ext_lde(cstark_ctx *ctx, const uint64_t *d_lde, const cstark_tx_coeffs *coeffs, uint32_t m,
                                           const uint64_t pub_inputs[4], uint64_t *d_out, uint32_t merkle_depth, uint32_t log_n);
/* Measurement aid: when enabled, cstark_tx_evaluate_constraints records HIP events around each of its 9 launches
 * (Rescue windows; doubling / mixed addition of s*G; of h*P; final addition; three linear groups) on the context's
 * stream; cstark_tx_constraint_part_ms waits for the last one and returns the 9 durations in milliseconds. */
/* Inside cstark_tx_prove (base field) the parts run as the degree-split evaluation: every part except the final
 * addition on the even cosets only; the last figure (third linear group) then also holds the extension of the 13 merged
 * polynomials (11 + the final addition's 2) to the odd cosets and the recombination over all cosets. */
int cstark_ctx_set_part_timing(cstark_ctx *ctx, int enable);
int cstark_tx_constraint_part_ms(cstark_ctx *ctx, float *ms /* [9] */);
/* With part timing enabled every low-degree extension on this context (cstark_lde_columns and the prover's own extensions: trace,
 * composition columns, split polynomials, DEEP) is bracketed by a HIP event pair on the context's stream.  Returns the summed
 * duration and the number of evaluations written (columns x cosets x n) since the previous call, and resets both. */
int cstark_lde_timing_ms(cstark_ctx *ctx, float *total_ms, uint64_t *elements);
/* Host-side AIR description (no GPU needed): degree (base; number of 1024-row cycles) of transition constraint i
 * (TransactionAir::new, src/air.rs:76-108) and the 48 periodic columns (src/air.rs:194-380), [48][1024]. */
int cstark_tx_constraint_degree(uint32_t i, uint32_t *base, uint32_t *cycles);  /* CSTARK_AIR_STATE_TRANSITION */
int cstark_tx_periodic_columns(uint32_t merkle_depth, uint64_t *out);

/* ---- composition polynomial (engine: evaluations -> H(x) -> column split; first of the "next" rows) ----------
 * d_combined: [b][n] combined constraint evaluations, coset-major (output of cstark_tx_evaluate_constraints with all b
 * cosets).  d_cols: [b][n] coefficients of the column polynomials H_i, H(x) = sum_i x^i H_i(x^b); extend and commit
 * them with cstark_lde_columns / cstark_hash_rows (width b) / cstark_merkle_build. */
int cstark_composition_columns(cstark_ctx *ctx, const uint64_t *d_combined, uint64_t *d_cols, uint32_t log_n, uint32_t log_blowup);

/* Out-of-domain frame: values of `width` coefficient columns (device) at up to 16 points (host); out[p][c] on the host. */
int cstark_evaluate_polys_at(cstark_ctx *ctx, const uint64_t *d_coeffs, uint32_t width, uint32_t log_n, const uint64_t *points,
                             uint32_t npts, uint64_t *out);
/* DEEP composition over LDE cosets [k0,k0+nk):
 *   d_out[(k-k0)*n + j] = [ sum_c alpha_c (T_c(x)-T_c(z))/(x-z) + beta_c (T_c(x)-T_c(z w))/(x-z w)
 *                         + sum_i delta_i (H_i(x)-H_i(z^n_comp))/(x-z^n_comp) ] * (deg_a + deg_b x).
 * ood_trace = T(z)[width] | T(z w)[width], ood_comp = H_i(z^n_comp); all coefficient / OOD arrays are host memory. */
int cstark_deep_composition(cstark_ctx *ctx, const uint64_t *d_trace_lde, const uint64_t *d_comp_lde, uint32_t width, uint32_t n_comp,
                            uint64_t z, const uint64_t *ood_trace, const uint64_t *ood_comp, const uint64_t *alpha,
                            const uint64_t *beta, const uint64_t *delta, uint64_t deg_a, uint64_t deg_b, uint64_t *d_out,
                            uint32_t log_n, uint32_t log_blowup, uint32_t k0, uint32_t nk);

/* FRI (FriOptions::folding_factor f = 4, 8 or 16; the reference's examples pass -f, examples/state-transition.rs:46-47).
 * cstark_interleave_cosets: [b][n] coset-major -> natural LDE order (i = b*j + k).
 * cstark_fri_fold: N = 2^log_n evaluations over domain_offset * <w_N> (natural order) -> N/f evaluations of the
 * alpha-folded polynomial over domain_offset^f * <w_{N/f}>.  A layer is committed by viewing its N evaluations as the
 * f x (N/f) column-major table of rows { e[i + t N/f] } and calling cstark_hash_rows (width f, log_blowup 0) and
 * cstark_merkle_build.  cstark_fri_fold4 = cstark_fri_fold with f = 4. */
int cstark_interleave_cosets(cstark_ctx *ctx, const uint64_t *d_coset_major, uint64_t *d_natural, uint32_t log_n, uint32_t log_blowup);
int cstark_fri_fold4(cstark_ctx *ctx, const uint64_t *d_evals, uint64_t *d_out, uint32_t log_n, uint64_t domain_offset, uint64_t alpha);
int cstark_fri_fold(cstark_ctx *ctx, const uint64_t *d_evals, uint64_t *d_out, uint32_t log_n, uint32_t folding_factor, uint64_t domain_offset,
                    uint64_t alpha);

/* ---- whole proof (replaces TransactionExample::prove, src/lib.rs:116-141 = build_trace + Prover::prove) ------------
 * Proves the uploaded witness (cstark_tx_witness_upload) under `opt` and writes the serialised proof to `proof`
 * (host, `capacity` bytes; cstark_tx_proof_size_bound gives a sufficient capacity).  *proof_len receives the length; if the
 * buffer is too small the call fails with CSTARK_ERR_INVALID_ARG and *proof_len still holds the required size.
 * The public inputs are read from the trace as TransactionProver::get_pub_inputs does (src/prover.rs:106-129).
 * Supported options (the values the reference's own tests, benches and command line pass: src/lib.rs:78-86, src/merkle/update/tests.rs:41-52,
 * src/range/tests.rs:87-98, benches/rescue.rs:370-378, examples/state-transition.rs:33-34, :46-47): blowup_factor 2, 4, 8 or 16 and at least
 * the AIR's constraint-evaluation blowup (TransactionAir / SchnorrAir 8, MerkleAir 4, RangeProofAir 2 -- below it the engine refuses the
 * options too); Blake3_256 or Sha3_256; FieldExtension::None / Quadratic / Cubic; fri_folding_factor 4, 8 or 16; fri_max_remainder 128..1024;
 * num_queries 1..128; grinding_factor 0..32.  The sharded entry points and cstark_range_prove_batch's one-launch-per-stage path take
 * blowup 8 / folding 4 (the batch call falls back to one proof at a time for other values).
 *
 * Proof layout (little-endian; field elements as 8-byte memory form; this library's own format, the engine's
 * StarkProof::to_bytes layout is not available in the reference tree):
 *   "CSTK" u32 version | u32 air, trace_width, log2(trace_length), merkle_depth | u32 x 7 options
 *   trace_root[32] constraint_root[32] | u32 n_layers, layer_root[n_layers][32], remainder_commitment[32]
 *   T(z)[94] T(z w)[94] H_i(z^8)[8] | u64 pow_nonce                                 (8 = the AIR's composition columns: 8 / 4 / 8 / 2)
 *   trace rows [q][94], paths [q][log N][32] | composition rows [q][8], paths [q][log N][32]      (q = num_queries, N = blowup * n)
 *   per layer: u32 n_positions, rows [n_positions][f], paths [n_positions][log rows][32]          (f = fri_folding_factor, rows = N_layer / f)
 *   u32 remainder_len, remainder[remainder_len]
 * Query positions are not stored: the verifier re-derives them from the channel.  Paths list siblings leaf-upwards.
 *
 * The compact form (CSTARK_FORM_COMPACT; cstark_ctx_set_proof_form) has the magic "CSTC" (same version) and replaces each of the
 * 2 + n_layers path sections by
 *   u32 n_nodes, nodes[n_nodes][32]
 * the Merkle multiproof of that tree for the sorted distinct positions opened in it: with K_d those positions at the leaf level d, for
 * l = d .. 1 every x of K_l, ascending, contributes the node (l, x ^ 1) iff x ^ 1 is not in K_l, and K_(l-1) is the set of parents
 * (the order of cstark_ledger_open_multi).  A leaf is the hash of its row and a parent the hash of its two children, as in the plain
 * form.  Every other byte -- header words, roots, frame, nonce, all rows in the same order (rows keep their multiplicity when positions
 * repeat), remainder -- is the plain form's: the channel seed does not contain the form, so both forms of one statement under one
 * option set open the same positions.  n_nodes <= n_positions * depth is a layout matter (MALFORMED); whether it is the count the
 * re-derived positions ask for is part of that tree's opening check. */
#define CSTARK_PROOF_VERSION 1
#define CSTARK_FORM_PLAIN   0
#define CSTARK_FORM_COMPACT 1
/* The form of the proofs the context's provers write: cstark_tx_prove, cstark_air_prove, cstark_rescue_prove, cstark_range_prove_bits and
 * cstark_range_prove_batch, on either Fiat-Shamir channel.  CSTARK_FORM_PLAIN is the default and any other value than the two is
 * CSTARK_ERR_INVALID_ARG.  The compact form is selected on the host from the same gathered openings: no launch, copy or wait is added
 * (the device channel's result block carries the positions too).  cstark_tx_proof_size_bound is a sufficient capacity for both
 * forms.  The sharded phases write the plain form only: cstark_tx_shard_commit and cstark_tx_shard_finish return
 * CSTARK_ERR_UNSUPPORTED while the compact form is set. */
int cstark_ctx_set_proof_form(cstark_ctx *ctx, uint32_t form);
int cstark_ctx_proof_form(cstark_ctx *ctx, uint32_t *form);
#define CSTARK_PROVE_NUM_STAGES 10
int cstark_tx_prove(cstark_ctx *ctx, const cstark_options *opt, uint8_t *proof, size_t capacity, size_t *proof_len);
/* The same for the standalone AIRs (MerkleExample / SchnorrExample / RangeProofExample ::prove, src/merkle/update/mod.rs:84-107,
 * src/schnorr/mod.rs:150-173, src/range/mod.rs:78-101): CSTARK_AIR_MERKLE_UPDATE proves the uploaded transaction witness with the
 * 65-register MerkleAir, CSTARK_AIR_SCHNORR the uploaded Schnorr witness, CSTARK_AIR_RANGE the field element `number` (ignored
 * otherwise).  Same proof layout with the AIR's width and its number of composition columns (4 / 8 / 2); the header's 4th word
 * holds the Merkle depth / the number of signatures / 0.  Use cstark_tx_proof_size_bound(rows / 1024 rounded up, opt) * 2 as capacity. */
int cstark_air_prove(cstark_ctx *ctx, int air, const cstark_options *opt, uint64_t number, uint8_t *proof, size_t capacity, size_t *proof_len);
size_t cstark_tx_proof_size_bound(uint32_t n_tx, const cstark_options *opt);
/* RescueExample::prove (benches/rescue.rs:66-86, options :370-378: blowup 4): a chain of chain_length Rescue hashes from `seed` (7
 * elements, memory form; the bench uses 42..48); chain_length a power of two, 8 .. 2^21; the trace is 14 x 8 chain_length.  Same proof
 * layout (4 composition columns; the header's 4th word holds chain_length); public inputs = seed and result, read from the trace as
 * RescueProver::get_pub_inputs does (:331-354).  cstark_tx_proof_size_bound(chain_length / 128 rounded up, opt) is a sufficient capacity. */
int cstark_rescue_prove(cstark_ctx *ctx, const cstark_options *opt, const uint64_t seed[7], uint32_t chain_length, uint8_t *proof, size_t capacity,
                        size_t *proof_len);
/* RescueProver::build_trace (benches/rescue.rs:277-322) and the AIR's 29 periodic columns [29][8] (host; :245-249) */
int cstark_rescue_chain_build_trace(cstark_ctx *ctx, const uint64_t seed[7], uint32_t chain_length, uint64_t *d_trace);
int cstark_rescue_chain_periodic_columns(uint64_t *out);

/* ---- one proof across several GPUs, sharded by LDE coset (the reference's only parallel axis is the rayon loop
 * over trace fragments, src/prover.rs:50-52) -------------------------------------------------------------------------------------
 * Every rank (one process per GPU, one cstark_ctx each) uploads the same witness and calls the phases in this order; the caller
 * moves three device buffers between the ranks -- RCCL collectives, see certificate-stark_amd/sharding.py.  Rank r of W in {2, 4, 8}
 * owns the nk = 8 / W cosets [k0, k0 + nk), k0 = r nk.  The proof bytes equal cstark_tx_prove's bit for bit.
 *   1 cstark_tx_shard_commit     trace + interpolation (replicated), extension and row hashes of the rank's cosets.  The rank's nk leaves
 *                                of a row are a complete subtree of the trace tree: it hashes the bottom log2(nk) levels itself and hands
 *                                over the subtree roots, d_leaves_local [n][32] -> all-gather -> d_leaves_all [W][n][32] (rank-major):
 *                                32 n bytes per rank at every world size (34 MB at 2^20 steps)
 *   2 cstark_tx_shard_evaluate   trace tree + root (every rank: the channel is replayed everywhere), coefficients, the rank's share of the
 *                                merged constraint evaluations: d_combined_local [R][n], R = cstark_tx_shard_rows(nk)
 *                                -> all-gather -> d_combined_all [W][R][n].  W = 8: R = 1, the rank's coset evaluated point by point.
 *                                W = 2, 4: the degree-split evaluation, sharded -- R = nk / 2 + 4: the rank's nk / 2 even cosets
 *                                (complete), then ITS SHARE of each of the four odd cosets (the split polynomials are evaluated on the
 *                                rank's even cosets only; their extension to the odd cosets is linear, so the ranks' shares add up)
 *   3 cstark_tx_shard_compose    rank 0 only (it owns coset 0, which the DEEP composition reads): sums the shares into the merged
 *                                evaluations of all cosets, composition polynomial and its commitment, out-of-domain frame, DEEP, FRI;
 *                                positions[num_queries] (host) -> broadcast
 *   4 cstark_tx_shard_open_rows  every rank: the opened rows of the extended trace that lie in its cosets, each followed by the bottom
 *                                log2(nk) siblings of its authentication path (the levels only the owner holds), zeros elsewhere;
 *                                d_rows [nq][cstark_tx_shard_open_words(nk)] -> all-reduce (sum) -> complete rows and path bottoms
 *   5 cstark_tx_shard_finish     rank 0: paths, remaining openings, proof bytes. */
uint32_t cstark_tx_shard_rows(uint32_t nk); /* rows of n evaluations a rank with nk cosets contributes in phase 2 (0: invalid nk) */
uint32_t cstark_tx_shard_open_words(uint32_t nk); /* 64-bit words per query in phase 4: 94 + 4 log2(nk) (0: invalid nk) */
int cstark_tx_shard_commit(cstark_ctx *ctx, const cstark_options *opt, uint32_t k0, uint32_t nk, uint8_t *d_leaves_local);
/* rows / total_rows: the row counts the caller sized d_combined_local ([rows][n]) and d_combined_all ([total_rows][n]) by; a value other
 * than cstark_tx_shard_rows(nk) / W * cstark_tx_shard_rows(nk) is refused before anything is written (version 0.2 of this library). */
int cstark_tx_shard_evaluate(cstark_ctx *ctx, const uint8_t *d_leaves_all, uint64_t *d_combined_local, uint32_t rows);
int cstark_tx_shard_compose(cstark_ctx *ctx, const uint64_t *d_combined_all, uint32_t total_rows, uint32_t *positions);
int cstark_tx_shard_open_rows(cstark_ctx *ctx, const uint32_t *positions, uint32_t nq, uint64_t *d_rows);
int cstark_tx_shard_finish(cstark_ctx *ctx, const uint64_t *d_rows, uint8_t *proof, size_t capacity, size_t *proof_len);
/* Wall-clock of the stages of the last cstark_tx_prove on this context (HIP events on its stream), milliseconds:
 * trace, interpolate, LDE, row hashes + tree, constraint evaluation, composition polynomial + commitment,
 * out-of-domain frame, DEEP composition, FRI layers, query openings.
 * cstark_tx_prove runs the curve ladders of the trace (registers 0..36) on an internal stream beside the interpolation AND
 * extension of the other 57 registers; its first three figures are therefore: trace = the rest of the trace on the context's
 * stream; interpolate = registers 37..93 interpolated and extended, the wait for the ladders, registers 0..36 interpolated;
 * LDE = extension of registers 0..36.  Their sum is the time from the start of the proof to the complete extended trace. */
int cstark_prove_stage_ms(cstark_ctx *ctx, float *ms /* [CSTARK_PROVE_NUM_STAGES] */);
/* Which Fiat-Shamir channel the last proof of the generic prover on this context used (cstark_tx_prove, cstark_air_prove and the
 * other single-proof entry points; the phases of a sharded proof count as CSTARK_CHANNEL_HOST).  DEVICE: every channel step ran as a
 * kernel on the context's stream and the host waited once, for the finished proof -- Blake3 coin, grinding_factor 0, any field
 * extension, at least one FRI layer.  HOST: the host absorbed every commitment and drew between the stages -- Sha3 coin, proof of work,
 * sharded proofs, or CSTARK_HOST_CHANNEL=1 in the environment.  The proof bytes are the same either way.  Fails like
 * cstark_prove_stage_ms when no proof has been generated on the context. */
#define CSTARK_CHANNEL_HOST   0
#define CSTARK_CHANNEL_DEVICE 1
int cstark_prove_channel(cstark_ctx *ctx, uint32_t *channel);

/* ---- standalone sub-AIRs (reference src/merkle/update, src/range; BASELINE configs 1-2) ---------- */
/* MerkleProver::build_trace (src/merkle/update/prover.rs:28-80): 65 x (512*n_tx) from the uploaded witness. */
int cstark_merkle_build_trace(cstark_ctx *ctx, uint64_t *d_trace);
/* RangeProver::build_trace (src/range/prover.rs:24-43): 2 x 64; `number` is a field element in memory form
 * whose canonical value must be below 2^63. */
int cstark_range_build_trace(cstark_ctx *ctx, uint64_t number, uint64_t *d_trace);
/* SYNTHETIC long form of the same accumulator for BASELINE.json's config "range-proof AIR, 2^16 steps" (the reference's range trace
 * is fixed at 64 rows, src/range/mod.rs:34, so this size has no reference counterpart): 2 x 2^log_n rows of the (n-1)-bit integer V
 * whose n/64 little-endian words are `words` (host; top bit of the last word clear).  Row q >= 1 holds bit (n-1-q) of V and
 * acc_q = 2 acc_(q-1) + bit (src/range/prover.rs:74-84), the AIR is RangeProofAir unchanged (src/range/air.rs:60-105) with the
 * assertion acc[n-1] = V mod p.  log_n = 6 with words[0] = number reproduces cstark_range_build_trace / cstark_air_prove exactly.
 * *number_out (optional): V mod p in memory form. */
int cstark_range_build_trace_bits(cstark_ctx *ctx, const uint64_t *words, uint32_t log_n, uint64_t *d_trace, uint64_t *number_out);
int cstark_range_prove_bits(cstark_ctx *ctx, const cstark_options *opt, const uint64_t *words, uint32_t log_n, uint8_t *proof, size_t capacity,
                            size_t *proof_len);
/* `count` reference-shaped range proofs (RangeProofExample::prove, src/range/mod.rs:75-100; the loop of benches/range.rs:15-37) in ONE
 * call: every stage is one launch over the batch, the host walks the `count` Fiat-Shamir channels between the stages.  numbers[count]:
 * field elements in memory form, canonical value below 2^63.  Proof t is written to proofs + t * stride (host memory;
 * cstark_tx_proof_size_bound(1, opt) is a sufficient stride), its length to lens[t]; it equals
 * cstark_air_prove(ctx, CSTARK_AIR_RANGE, opt, numbers[t], ...) byte for byte.  FieldExtension::None; both hash functions. */
int cstark_range_prove_batch(cstark_ctx *ctx, const cstark_options *opt, const uint64_t *numbers, uint32_t count, uint8_t *proofs, size_t stride,
                             size_t *lens);
/* SchnorrAir (src/schnorr/air.rs:41-300, src/schnorr/prover.rs:21-67): n signatures over 28-element messages
 * (message[0..12] = public key).  Trace 56 x (512*n); the 19 public-input columns (pkey x12, message chunks x7;
 * src/schnorr/air.rs:228-290) as a 19 x (512*n) table that the caller extends like trace columns; the 8 mask + 28
 * round-constant periodic columns [36][512] (host).  The 61 periodic / sequence assertions (:111-226) are merged by
 * cstark_air_combine. */
int cstark_schnorr_witness_upload(cstark_ctx *ctx, uint32_t n_sig, const uint64_t *messages, const uint64_t *sig_rx, const uint8_t *sig_s);
int cstark_schnorr_build_trace(cstark_ctx *ctx, uint64_t *d_trace);
int cstark_schnorr_aux_columns(cstark_ctx *ctx, uint64_t *d_out);
int cstark_schnorr_mask_columns(uint64_t *out /* [36][512] host */);
int cstark_schnorr_evaluate_transitions(cstark_ctx *ctx, const uint64_t *d_lde, const uint64_t *d_aux_lde, uint64_t *d_out,
                                        uint32_t log_n, uint32_t log_blowup, uint32_t k0, uint32_t nk);
/* Coefficient columns [12][n] of the value polynomials of SchnorrAir's sequence assertions (R.x asserted at step 0 and at
 * step 511 of every block, src/schnorr/air.rs:172-224); extend them with cstark_lde_columns and pass them to
 * cstark_air_combine. */
int cstark_schnorr_assertion_polys(cstark_ctx *ctx, uint64_t *d_out, uint32_t log_n);
/* Shape of an AIR as the engine sees it (host side): trace width, number of transition constraints and of
 * assertions, log2 of the constraint-evaluation blowup; degree (base; cycles) of constraint i.  n_items = number of
 * signatures for CSTARK_AIR_SCHNORR (its degrees depend on it, src/schnorr/air.rs:537), ignored otherwise. */
int cstark_air_shape(int air, uint32_t n_items, uint32_t *width, uint32_t *n_constraints, uint32_t *n_assertions, uint32_t *log_ce_blowup);
int cstark_air_constraint_degree(int air, uint32_t n_items, uint32_t i, uint32_t *base, uint32_t *cycles);
int cstark_merkle_periodic_columns(uint32_t merkle_depth, uint64_t *out /* [33][512] host */);
/* All transition constraints of AIR `air` (CSTARK_AIR_MERKLE_UPDATE, CSTARK_AIR_RANGE) on LDE cosets [k0,k0+nk):
 *   d_out[((k - k0) * n_constraints + i) * n + j].  (SchnorrAir: cstark_schnorr_evaluate_transitions.) */
int cstark_air_evaluate_transitions(cstark_ctx *ctx, int air, const uint64_t *d_lde, uint64_t *d_out, uint32_t merkle_depth,
                                    uint32_t log_n, uint32_t log_blowup, uint32_t k0, uint32_t nk);
/* Generic merge of materialised transition evaluations with the AIR's assertions (single, periodic and sequence) into
 * the combined constraint evaluations d_out[(k - k0) * n + j].  Coefficient arrays (per transition constraint / per
 * assertion in get_assertions order) are host memory.  assertion_values: host, one per assertion, for Merkle (7+7 roots)
 * and Range (0, number); NULL for Schnorr whose constants are built in and whose sequence values arrive as
 * d_avals_lde = [nk][n_avals][n] (extension of cstark_schnorr_assertion_polys).  The constraint-evaluation domain may be
 * smaller than the LDE domain (MerkleAir: blowup 4); cosets outside it are written as 0. */
int cstark_air_combine(cstark_ctx *ctx, int air, uint32_t n_items, const uint64_t *d_lde, const uint64_t *d_evals,
                       const uint64_t *t_alpha, const uint64_t *t_beta, const uint64_t *b_alpha, const uint64_t *b_beta,
                       const uint64_t *assertion_values, const uint64_t *d_avals_lde, uint32_t n_avals, uint64_t *d_out,
                       uint32_t log_n, uint32_t log_blowup, uint32_t k0, uint32_t nk);

/* SchnorrAir's combined constraint evaluations WITHOUT the 56 materialised transition values: the transition sum
 * sum_i (alpha_i + beta_i x^adj_i) C_i(x) is accumulated per point by the fused gadget evaluators (the ones behind
 * cstark_tx_evaluate_constraints) and merged with the 61 assertions like cstark_air_combine does.  Same values as
 * cstark_schnorr_evaluate_transitions followed by cstark_air_combine (exact arithmetic); what cstark_air_prove uses for
 * CSTARK_AIR_SCHNORR.  Replaces the evaluation loop of winterfell's ConstraintEvaluator for SchnorrAir
 * (/root/reference/src/schnorr/air.rs:72-109, :394-531) [UPSTREAM-RECALL for the driver]. */
/* MerkleAir likewise (one launch over the cosets of its constraint-evaluation domain, blowup 4; src/merkle/update/air.rs:64-141,
 * :215-369): same values as cstark_air_evaluate_transitions + cstark_air_combine; what cstark_air_prove uses for
 * CSTARK_AIR_MERKLE_UPDATE.  assertion_values: the 7 + 7 root elements (host). */
int cstark_merkle_evaluate_constraints(cstark_ctx *ctx, uint32_t merkle_depth, const uint64_t *d_lde, const uint64_t *t_alpha,
                                       const uint64_t *t_beta, const uint64_t *b_alpha, const uint64_t *b_beta,
                                       const uint64_t *assertion_values, uint64_t *d_out, uint32_t log_n, uint32_t log_blowup,
                                       uint32_t k0, uint32_t nk);
int cstark_schnorr_evaluate_constraints(cstark_ctx *ctx, uint32_t n_sig, const uint64_t *d_lde, const uint64_t *d_aux_lde,
                                        const uint64_t *t_alpha, const uint64_t *t_beta, const uint64_t *b_alpha, const uint64_t *b_beta,
                                        const uint64_t *d_avals_lde, uint32_t n_avals, uint64_t *d_out, uint32_t log_n,
                                        uint32_t log_blowup, uint32_t k0, uint32_t nk);
/* The same result for tables that ARE low-degree extensions over all 8 cosets (d_lde: 56 columns of degree < n, d_aux_lde: the 19
 * public-input columns; e.g. outputs of cstark_lde_columns): allows the degree-split evaluation of the doubling / addition gadgets that
 * cstark_air_prove uses (on the even cosets only, their eight merged polynomials extended to the odd cosets).  On such tables
 * the output equals cstark_schnorr_evaluate_constraints bit for bit; on any other table it is undefined. */
int cstark_schnorr_evaluate_constraints_lde(cstark_ctx *ctx, uint32_t n_sig, const uint64_t *d_lde, const uint64_t *d_aux_lde,
                                            const uint64_t *t_alpha, const uint64_t *t_beta, const uint64_t *b_alpha, const uint64_t *b_beta,
                                            const uint64_t *d_avals_lde, uint32_t n_avals, uint64_t *d_out, uint32_t log_n);

/* ---- witness synthesis (host; counterpart of TransactionMetadata::build_random, src/lib.rs:235-465, and of
 * SchnorrExample::new + schnorr::sign, src/schnorr/mod.rs:86-141, :197-217; seeded and deterministic) -----------------
 * cstark_tx_witness_generate fills the arrays of `w` (every pointer caller-allocated with the sizes documented on
 * cstark_tx_witness; n_tx and merkle_depth set by the caller).  Like the reference this is CPU work outside the timed
 * region.  Signatures are produced with integer arithmetic and small secret keys (see csrc/witness_gen.hip). */
int cstark_tx_witness_generate(cstark_tx_witness *w, uint64_t seed);
/* n_sig messages [n][28] (public key || 16 elements) with their signatures (R.x [n][6], s [n][32]). */
int cstark_schnorr_witness_generate(uint32_t n_sig, uint64_t seed, uint64_t *messages, uint64_t *sig_rx, uint8_t *sig_s);

/* ---- signature check: verify_signature (src/schnorr/mod.rs:220-245) on the device, for its verdict ---------------------------------
 * Where several verdicts apply, the verdict is the first of SCALAR_RANGE, KEY_NOT_ON_CURVE, MISMATCH.  The order of the curve's scalar
 * field is stated nowhere in the reference tree (csrc/witness_gen.hip), so s < 2^255 is the ONLY range rule: a scalar at or above the
 * group order is not refused for that, it is used by its bits 254..0 exactly as the SchnorrAir trace uses it. */
typedef enum cstark_sig_verdict {
    CSTARK_SIG_VALID = 0,
    CSTARK_SIG_MISMATCH = 1,          /* x(s*G + h*P) != R.x, or the sum is the point at infinity */
    CSTARK_SIG_KEY_NOT_ON_CURVE = 2,  /* message[0..12] is no affine point of the curve (the reference asserts this, mod.rs:228) */
    CSTARK_SIG_SCALAR_RANGE = 3       /* bit 255 of s set: the ladders read bits 254..0 only */
} cstark_sig_verdict;
/* verify_signature for `count` signatures (1 .. 2^20).  messages [count][28] (public key || 16 elements), sig_rx [count][6] (memory
 * form), sig_s [count][32] little-endian; verdicts [count] (cstark_sig_verdict); rx_out (optional) [count][6]: the affine x of
 * s*G + h*P as the SchnorrAir trace holds it in registers 0..5 of row 511, written for every signature whatever its verdict.  All
 * arrays are host memory.  Null messages, sig_rx, sig_s or verdicts, count == 0, count > 2^20, or a messages / sig_rx word >= p is
 * CSTARK_ERR_INVALID_ARG before anything is launched and with the outputs untouched; cstark_last_error names the first such word.
 * Synchronous, on the context's stream, in device scratch of its own that the context keeps and frees: the resident witness
 * (cstark_tx_witness_upload, cstark_schnorr_witness_upload, cstark_ledger_apply) is neither read nor written, so a proof after a check
 * is the proof without it. */
int cstark_schnorr_check_signatures(cstark_ctx *ctx, uint32_t count, const uint64_t *messages, const uint64_t *sig_rx,
                                    const uint8_t *sig_s, uint8_t *verdicts, uint64_t *rx_out);

/* ---- signing: schnorr::sign (src/schnorr/mod.rs:197-217) and generator() * skey (mod.rs:92) on the device -------------
 * The scheme is the one of cstark_tx_witness_generate (csrc/witness_gen.hip), callable with chosen inputs.  The order of the curve's
 * scalar field is stated nowhere in the reference tree, so signatures use integer arithmetic: R = r*G, h = hash_message(R.x, message)
 * read as a 4-limb integer, s = r - sk*h, accepted when 0 <= s < 2^255; then s*G + h*(sk*G) = R holds in the group whatever its order.
 * This forces rejection sampling: an attempt is accepted with probability about 2 / (sk + 2), so secret keys are small integers,
 * 1 .. CSTARK_SIG_MAX_SECRET.  With such keys this is a signer for building batches, tests and benchmarks.  It is not a wallet.
 * r*G and sk*G are sums of entries of a table of multiples of G (d * 16^w * G, built on the device by the context's first signing call
 * and kept by it): at most 66 complete mixed additions and no doubling.
 * Misuse of the three calls -- a null pointer (attempts_out may be null), count == 0, count > 2^20, a secret of 0 or above the
 * maximum, a nonce >= 2^264, a message word >= p, max_attempts outside 1 .. 4096 -- is CSTARK_ERR_INVALID_ARG before anything is
 * launched and with the outputs untouched; cstark_last_error names the first offender.  The calls are synchronous, on the context's
 * stream, in the device scratch of cstark_schnorr_check_signatures, which the context keeps and frees (nothing stays in it between
 * calls): the resident witness is neither read nor written, so a proof after a signing call is the proof without it.  All arrays are
 * host memory. */
#define CSTARK_SIG_MAX_SECRET 255u
/* the status of one signing attempt.  INFINITY is tested first, then NEGATIVE, then RANGE (the latter two exclude each other). */
typedef enum cstark_sign_status {
    CSTARK_SIGN_OK = 0,
    CSTARK_SIGN_NEGATIVE = 1,   /* r < sk*h */
    CSTARK_SIGN_RANGE = 2,      /* r - sk*h >= 2^255 */
    CSTARK_SIGN_INFINITY = 3,   /* r*G is the point at infinity (r = 0, or a multiple of the group order) */
    CSTARK_SIGN_EXHAUSTED = 4   /* cstark_schnorr_sign only: no accepted attempt among max_attempts */
} cstark_sign_status;
/* keys_out [count][12] = secrets[i] * G, affine (x, y) in memory form: what an account of cstark_ledger_set_accounts holds in words
 * 0..11 and a Schnorr message in words 0..11. */
int cstark_schnorr_public_keys(cstark_ctx *ctx, uint32_t count, const uint64_t *secrets, uint64_t *keys_out);
/* One attempt per entry with the caller's nonce: nonces [count][5] little-endian limbs, r < 2^264.  Every output is defined whatever
 * the status: sig_rx [count][6] = x(r*G), all zero on INFINITY; sig_s [count][32] = bits 0..255 of r - sk*h, little-endian; status
 * [count] (cstark_sign_status).  The key inside the message (words 0..11) is hashed as given and not compared with sk*G: a signature
 * over a message with someone else's key is simply one that cstark_schnorr_check_signatures calls MISMATCH. */
int cstark_schnorr_sign_nonces(cstark_ctx *ctx, uint32_t count, const uint64_t *messages, const uint64_t *secrets, const uint64_t *nonces,
                               uint64_t *sig_rx, uint8_t *sig_s, uint8_t *status);
/* The seeded signer.  Signature t has a SplitMix64 stream of its own, state seed ^ (0xD1B54A32D192ED03 * (t + 1)); attempt a = 0, 1, 2 ...
 * draws five outputs from it (r[0..3], then hi = next % (sk + 2); r[3] &= 2^62 - 1; hi << 62 is added into limbs 3 and 4: r uniform in
 * [0, (sk + 2) * 2^254)), exactly as the host signer of cstark_tx_witness_generate.  The result of signature t is that of its first
 * attempt whose status is OK, and attempts_out[t] (optional) = a + 1; how many attempts run together on the device does not show in it.
 * Without an OK attempt below max_attempts (1 .. 4096): status CSTARK_SIGN_EXHAUSTED, zero sig_rx and sig_s, attempts_out[t] =
 * max_attempts.  status [count]: CSTARK_SIGN_OK or CSTARK_SIGN_EXHAUSTED. */
int cstark_schnorr_sign(cstark_ctx *ctx, uint32_t count, const uint64_t *messages, const uint64_t *secrets, uint64_t seed,
                        uint32_t max_attempts, uint64_t *sig_rx, uint8_t *sig_s, uint32_t *attempts_out, uint8_t *status);

/* ---- account ledger: the witness from what an operator holds (replaces the sequential loop of TransactionMetadata::build_random,
 * src/lib.rs:341-422: record the root and the sender's path, apply the transfer, re-hash two leaf-to-root paths, record the receiver's
 * path) ------------------------------------------------------------------------------------------------------------------------------
 * A ledger is a sparse Rescue `merge` tree of accounts (leaf = merge(value[0..7], value[7..14]); empty leaves are the all-zero digest,
 * as in cstark_tx_witness_generate) whose digests live in device memory of its context: storage grows with the touched nodes, so depth 31
 * with indices above 2^24 works.  The host keeps which nodes exist and the account values (the balance checks need them).  A batch is
 * hashed as depth + 1 dependent launches of 2 n_tx independent merges, not as 2 n_tx (depth + 1) dependent merges.
 * Every call is synchronous and takes the ledger's own context.  Misuse (null pointers, count or n_tx == 0, a ledger of another
 * context, a word that is no reduced field element) is CSTARK_ERR_INVALID_ARG.  After a HIP failure inside a ledger call the ledger is
 * unusable: every later call on it returns CSTARK_ERR_HIP. */
typedef struct cstark_ledger cstark_ledger;
/* why cstark_ledger_apply refused a batch.  Transfers are examined in transfer order, each against the accounts as the transfers before
 * it in the same batch leave them; the batch is refused at the first transfer that matches a reason, with the first reason in this
 * order that this transfer matches: either index out of range, then sender equals receiver, then either account absent, then the
 * balance, then (cstark_ledger_apply_checked only) the signature. */
typedef enum cstark_ledger_reason {
    CSTARK_LEDGER_APPLIED = 0,
    CSTARK_LEDGER_INDEX_RANGE = 1,  /* an index >= 2^merkle_depth */
    CSTARK_LEDGER_SELF_TRANSFER = 2, /* sender equals receiver */
    CSTARK_LEDGER_ABSENT = 3,       /* sender or receiver has no account */
    CSTARK_LEDGER_BALANCE = 4,      /* delta above the sender's balance, both as canonical integers */
    CSTARK_LEDGER_SIGNATURE = 5,    /* cstark_ledger_apply_checked only: the transfer's signature has another verdict than CSTARK_SIG_VALID */
    CSTARK_LEDGER_UNKNOWN = 6,      /* a partial ledger only: sender or receiver is not among the accounts it knows; tested after the self
                                       transfer and before absence (index range, self transfer, unknown, absent, balance, signature) */
    CSTARK_LEDGER_KEY = 7,          /* cstark_ledger_sign only: the transfer's secret is not the secret of its sender's public key */
    CSTARK_LEDGER_HELD = 8,         /* cstark_ledger_select only: an earlier candidate of the call with the same sender index was refused */
    CSTARK_LEDGER_NOT_REACHED = 9   /* cstark_ledger_select only: `want` candidates were selected before this one */
} cstark_ledger_reason;
/* An empty tree of depth 1, 3, 7, 15 or 31 (the depths cstark_tx_witness_upload accepts).  Destroy it before its context. */
int cstark_ledger_create(cstark_ctx *ctx, uint32_t merkle_depth, cstark_ledger **out);
void cstark_ledger_destroy(cstark_ledger *ledger);
/* Bulk insert or overwrite: indices[count] distinct within the call, values[count][14] (pk.x pk.y balance nonce).  The leaves and then
 * the unique parents of every level are hashed in parallel, one launch per level. */
int cstark_ledger_set_accounts(cstark_ctx *ctx, cstark_ledger *ledger, uint32_t count, const uint64_t *indices, const uint64_t *values);
/* values_out[count][14] and present_out[count] (1 = the account exists; absent accounts read as zeros) */
int cstark_ledger_get_accounts(cstark_ctx *ctx, cstark_ledger *ledger, uint32_t count, const uint64_t *indices, uint64_t *values_out,
                               uint8_t *present_out);
int cstark_ledger_root(cstark_ctx *ctx, cstark_ledger *ledger, uint64_t root[7]);
/* The authentication paths of `count` (1 .. 2^20) leaves under the CURRENT root.  indices may repeat and may name absent accounts.
 * values_out [count][14] and present_out [count] are what cstark_ledger_get_accounts gives; paths_out [count][depth + 1][7] has the
 * witness's path form (s_paths / r_paths of cstark_tx_witness): [leaf digest, sibling at level depth, ..., sibling at level 1]; root_out
 * is the root every path folds to (cstark_account_check_paths states the fold).  The leaf entry of an absent account is the all-zero
 * digest and its siblings are what the tree holds, empty-subtree digests where nothing was touched: a proof of absence.  Null pointers,
 * count == 0, count > 2^20 or an index >= 2^depth is CSTARK_ERR_INVALID_ARG with the outputs untouched.  Synchronous and read-only: one
 * upload of a slot list, one gather on the device, no hashing; root, stored nodes, accounts and the resident witness are unchanged. */
int cstark_ledger_open_accounts(cstark_ctx *ctx, cstark_ledger *ledger, uint32_t count, const uint64_t *indices,
                                uint64_t *values_out /* [count][14] */, uint8_t *present_out /* [count] */,
                                uint64_t *paths_out /* [count][depth + 1][7] */, uint64_t root_out[7]);
/* ---- the verifier's side of an opening: needs no ledger --------------------------------------------------------------------------
 * The verdict of a path is the first that applies, in the order INDEX_RANGE, LEAF, ROOT. */
typedef enum cstark_path_verdict {
    CSTARK_PATH_VALID = 0,
    CSTARK_PATH_INDEX_RANGE = 1, /* index >= 2^depth */
    CSTARK_PATH_LEAF = 2,        /* paths[i][0] is not the leaf of the stated account: merge(value[0..7], value[7..14]) if present,
                                    all-zero if absent */
    CSTARK_PATH_ROOT = 3         /* the path does not fold to the stated root */
} cstark_path_verdict;
/* Folds `count` (1 .. 2^20) paths of a tree of any depth 1 .. 31 on the device, each in one chain of depth Rescue merges inside ONE
 * launch: cur = paths[i][0]; for k = 0 .. depth - 1: cur = bit k of indices[i] ? merge(paths[i][k + 1], cur) : merge(cur, paths[i][k + 1]).
 * The fold reads bits 0 .. depth - 1 of the index whatever the verdict, and roots_out (optional, [count][7]) receives its result for
 * every path whatever the verdict.  roots: n_roots = 1 (one root for all paths) or count (one each), [n_roots][7].
 * values [count][14] given: the LEAF test runs, against merge(value[0..7], value[7..14]) where present[i] != 0 (a NULL present: all
 * present) and against the all-zero digest where present[i] == 0.  values == NULL is digest mode: present must be NULL too, no LEAF
 * test runs and the path is taken as a path of digests.  verdicts [count]: one cstark_path_verdict each.  All arrays are host memory.
 * Null ctx, indices, paths, roots or verdicts, count == 0, count > 2^20, depth == 0, depth > 31, n_roots neither 1 nor count, present
 * without values, or a word >= p in values, paths or roots is CSTARK_ERR_INVALID_ARG before anything is launched and with the outputs
 * untouched; cstark_last_error names the first such word (values, then paths, then roots).  Synchronous, on the context's stream, in a
 * device block of its own that the context keeps and frees: the resident witness is neither read nor written, so a proof after a check
 * is the proof without it. */
int cstark_account_check_paths(cstark_ctx *ctx, uint32_t count, uint32_t depth, const uint64_t *indices,
                               const uint64_t *values /* [count][14] or NULL */, const uint8_t *present /* [count] or NULL */,
                               const uint64_t *paths /* [count][depth + 1][7] */, const uint64_t *roots, uint32_t n_roots /* 1 or count */,
                               uint8_t *verdicts /* [count] */, uint64_t *roots_out /* optional [count][7] */);
/* Applies n_tx transfers in order with the reference's arithmetic (sender balance - delta, sender nonce + 1, receiver balance + delta:
 * field operations, src/lib.rs:373-375), advances the ledger and leaves the batch's witness RESIDENT in the context exactly as
 * cstark_tx_witness_upload would: cstark_tx_build_trace / cstark_tx_prove / cstark_air_prove follow without an upload.  Roots, paths
 * and old values are written on the device; indices, deltas and signatures (sig_rx [n_tx][6], sig_s [n_tx][32]) are copied through.
 * Signatures are NOT checked here, and nothing later checks them either: TransactionAir asserts the four root values only
 * (src/air.rs:175-184) and a forged signature satisfies every transition constraint, so a batch with a wrong signature still proves and
 * the proof still verifies.  An operator who must enforce signatures calls cstark_ledger_apply_checked.  out (optional): a witness whose
 * arrays the caller allocated for (n_tx, merkle_depth), filled with all eleven fields.
 * Refusal is not a failure: the status is CSTARK_OK, *refused_at = the first offending transfer (-1: none) and *reason its
 * cstark_ledger_reason; a refused batch changes neither the ledger nor the resident witness (and `out` is not written). */
int cstark_ledger_apply(cstark_ctx *ctx, cstark_ledger *ledger, uint32_t n_tx, const uint64_t *s_indices, const uint64_t *r_indices,
                        const uint64_t *deltas, const uint64_t *sig_rx, const uint8_t *sig_s, cstark_tx_witness *out,
                        int32_t *refused_at, int32_t *reason);
/* The same call with the same arguments and contract, and every transfer's signature checked before anything is applied
 * (cstark_schnorr_check_signatures).  The message of transfer t is build_tx_message (src/lib.rs:467-481): the sender's key (12 words),
 * the receiver's key (12 words), delta, the sender's nonce, two zeros -- keys and nonce as the transfers before t in the same batch
 * leave the accounts.  Transfers are examined in transfer order; within a transfer the four reasons above come first, then
 * CSTARK_LEDGER_SIGNATURE (any verdict other than CSTARK_SIG_VALID).  So a batch whose first unappliable transfer is k is refused at
 * the first transfer below k with a bad signature, else at k with its own reason; an appliable batch is refused at its first bad
 * signature.  A sig_rx word >= p of an examined transfer is CSTARK_ERR_INVALID_ARG.  The check runs in scratch of the context, ahead of
 * every change: a refused batch changes neither the ledger nor the resident witness nor `out`; a batch whose signatures are all valid
 * is applied exactly as cstark_ledger_apply applies it. */
int cstark_ledger_apply_checked(cstark_ctx *ctx, cstark_ledger *ledger, uint32_t n_tx, const uint64_t *s_indices, const uint64_t *r_indices,
                                const uint64_t *deltas, const uint64_t *sig_rx, const uint8_t *sig_s, cstark_tx_witness *out,
                                int32_t *refused_at, int32_t *reason);
/* The message each transfer of a batch has to sign (build_tx_message, as above): messages_out [n_tx][28].  The walk is the one
 * cstark_ledger_apply makes, run read-only: the call refuses exactly where cstark_ledger_apply would, with the same reason
 * (CSTARK_LEDGER_UNKNOWN on a partial ledger included), and then messages_out is not written.  Root, pool, host index, checkpoints and
 * the resident witness are unchanged whatever the outcome; nothing is launched. */
int cstark_ledger_messages(cstark_ctx *ctx, cstark_ledger *ledger, uint32_t n_tx, const uint64_t *s_indices, const uint64_t *r_indices,
                           const uint64_t *deltas, uint64_t *messages_out, int32_t *refused_at, int32_t *reason);
/* Signs a batch for cstark_ledger_apply_checked: the messages of cstark_ledger_messages, then cstark_schnorr_sign with secrets [n_tx]
 * (the sender's secret key of every transfer, 1 .. CSTARK_SIG_MAX_SECRET), seed and max_attempts (its misuse rules apply).  Before
 * anything is signed every secret's public key is derived on the device and compared with the sender's key in the message: the first
 * transfer whose secret is not its sender's key refuses the batch with CSTARK_LEDGER_KEY.  Within a transfer that reason comes after
 * the plan's: a batch whose first unappliable transfer is k is refused at the first transfer below k with a wrong secret, else at k with
 * its own reason.  A refused batch writes none of the outputs.  sig_rx_out [n_tx][6], sig_s_out [n_tx][32], attempts_out (optional)
 * [n_tx].  A signature without an accepted attempt among max_attempts is CSTARK_ERR_UNSUPPORTED, and cstark_last_error names the
 * transfer.  The call is read-only: root, pool, host index, checkpoints and the resident witness are unchanged.  This signs with small
 * integer keys (see "signing" above): a signer for building batches, tests and benchmarks.  It is not a wallet. */
int cstark_ledger_sign(cstark_ctx *ctx, cstark_ledger *ledger, uint32_t n_tx, const uint64_t *s_indices, const uint64_t *r_indices,
                       const uint64_t *deltas, const uint64_t *secrets, uint64_t seed, uint32_t max_attempts, uint64_t *sig_rx_out,
                       uint8_t *sig_s_out, uint32_t *attempts_out, int32_t *refused_at, int32_t *reason);

/* Selects a provable batch from a pool of n candidate transfers in arrival order: every candidate gets a status (status_out [n], a
 * cstark_ledger_reason), up to `want` of them are selected, and nothing is refused as a whole.  Candidates are examined in list order,
 * each against the accounts as the candidates SELECTED before it leave them, and a candidate gets the first status that applies, in this
 * order: NOT_REACHED (`want` candidates are selected already), INDEX_RANGE, SELF_TRANSFER, UNKNOWN (a partial ledger only), ABSENT, HELD,
 * BALANCE (cstark_ledger_apply's arithmetic), SIGNATURE (only with CSTARK_SELECT_CHECK_SIGNATURES), else APPLIED: selected.
 * THE HOLD: a refused candidate (any status but NOT_REACHED) whose sender index is in range holds that sender for the rest of the call:
 * the sender's later candidates are HELD.  A held account still receives.  A wallet signs nonce n, n + 1, ... expecting all of them to
 * be accepted; after a refusal the sender's later candidates carry the wrong nonce anyway, so honest senders lose nothing.  The hold
 * makes the message of every candidate that reaches the signature test known before any verdict is: the sender's key, the receiver's
 * key, delta, the sender's STORED nonce + k (k = the earlier candidates in the list with the same sender index), two zeros.  So the
 * signatures are checked in passes of many candidates on the device, whatever the bad candidates do: a sender who submits 1,000
 * transfers for one nonce costs one pass, not 1,000 retries.
 * flags: CSTARK_SELECT_CHECK_SIGNATURES -- any verdict other than CSTARK_SIG_VALID is SIGNATURE; a candidate that reaches the
 *   signature test with a sig_rx word >= p is SIGNATURE without being sent to the device (it equals no canonical x).
 * CSTARK_SELECT_POW2 -- with A candidates selected under `want`, the result is that of the same call with want = the largest power of
 *   two <= A: everything after that many selected candidates is NOT_REACHED (cstark_tx_prove needs a power of two).
 * CSTARK_SELECT_APPLY -- the selected candidates, in order, are applied exactly as cstark_ledger_apply applies that batch (the witness
 *   resident, live checkpoints honoured, report->root_after the root they leave); `out` (optional, APPLY only): a witness the caller
 *   allocated for merkle_depth and at least min(want, n) transfers (out->n_tx states the capacity), whose first report->n_selected rows
 *   are filled.  With nothing selected nothing changes.  Without APPLY the call is read-only: root, pool, host index, checkpoints and the
 *   resident witness are unchanged and a proof after the call is the proof without it.
 * chunk: the checkable candidates (those that pass the tests before HELD) sent to the device per pass; 0: the number still missing from
 *   `want`, rounded up to a multiple of 1,024.  Statuses and selection never depend on it; report->n_sig_checked and n_chunks do, and
 *   so do the rows of messages_out of candidates whose verdict was not needed in the end.
 * selected_out (optional) [min(want, n)]: the selected candidate numbers, ascending, report->n_selected of them.  messages_out
 * (optional) [n][28]: the message of every candidate sent to the device, zeros elsewhere.
 * n and want are 1 .. 2^20 (want may exceed n); chunk <= 2^20; sig_rx and sig_s may be NULL only without CHECK_SIGNATURES and APPLY.
 * Unknown flag bits, null required pointers, a ledger of another context, `out` without APPLY or of another shape, or a delta word
 * >= p (cstark_last_error names it) are CSTARK_ERR_INVALID_ARG, raised before any launch with the outputs untouched.  Synchronous. */
#define CSTARK_SELECT_CHECK_SIGNATURES 1u
#define CSTARK_SELECT_POW2 2u
#define CSTARK_SELECT_APPLY 4u
typedef struct cstark_ledger_selection {
    uint32_t n_candidates;
    uint32_t n_selected;
    uint32_t n_sig_checked;     /* signatures sent to the device, all passes */
    uint32_t n_chunks;          /* passes of the signature check */
    uint32_t counts[10];        /* candidates per cstark_ledger_reason */
    uint64_t root_after[7];     /* with CSTARK_SELECT_APPLY: the root the selection leaves; zero otherwise */
} cstark_ledger_selection;
int cstark_ledger_select(cstark_ctx *ctx, cstark_ledger *ledger, uint32_t n, const uint64_t *s_indices, const uint64_t *r_indices,
                         const uint64_t *deltas, const uint64_t *sig_rx, const uint8_t *sig_s, uint32_t want, uint32_t flags,
                         uint32_t chunk, uint8_t *status_out, uint32_t *selected_out, uint64_t *messages_out,
                         cstark_ledger_selection *report, cstark_tx_witness *out);

/* ---- witness check: is a cstark_tx_witness consistent?  Needs no ledger ---------------------------------------------------------------
 * What cstark_tx_prove starts from, tested transfer by transfer before a trace is built: the indices, the sender's leaf and path under
 * initial_roots[t], the balance, the root between the two updates, the receiver's leaf and path under the next root and, when asked for,
 * the signature.  With s_new = (pk, balance - delta, nonce + 1) of s_old_values[t] and r_new = (pk, balance + delta, nonce) of
 * r_old_values[t] (field arithmetic, src/lib.rs:373-375, as cstark_ledger_apply), leaf(v) = merge(v[0..7], v[7..14]) and fold the one
 * cstark_account_check_paths states, "s siblings" = s_paths[t][1..], "r siblings" = r_paths[t][1..].  A transfer's verdict is the FIRST
 * that applies in the order of the values; every test of every transfer runs whatever the others give, so one bad transfer does not hide
 * the next.  A receiver balance that wraps past p is no verdict: cstark_ledger_apply does not refuse it either. */
typedef enum cstark_witness_verdict {
    CSTARK_WITNESS_VALID = 0,
    CSTARK_WITNESS_INDEX_RANGE = 1,   /* s_index or r_index >= 2^merkle_depth */
    CSTARK_WITNESS_SELF_TRANSFER = 2, /* s_index == r_index */
    CSTARK_WITNESS_SENDER_LEAF = 3,   /* s_paths[t][0] != leaf(s_old) */
    CSTARK_WITNESS_SENDER_PATH = 4,   /* fold(s_paths[t][0], s siblings, s_index) != initial_roots[t] */
    CSTARK_WITNESS_BALANCE = 5,       /* delta > sender balance, both as canonical integers (the ledger's rule) */
    CSTARK_WITNESS_MIDDLE_ROOT = 6,   /* fold(leaf(s_new), s siblings, s_index) != fold(leaf(r_old), r siblings, r_index) */
    CSTARK_WITNESS_RECEIVER_LEAF = 7, /* r_paths[t][0] != leaf(r_new) */
    CSTARK_WITNESS_NEXT_ROOT = 8,     /* fold(r_paths[t][0], r siblings, r_index) != initial_roots[t + 1], or the final root for the last transfer */
    CSTARK_WITNESS_SIGNATURE = 9      /* only with CSTARK_WITNESS_CHECK_SIGNATURES: verdict other than CSTARK_SIG_VALID */
} cstark_witness_verdict;
#define CSTARK_WITNESS_CHECK_SIGNATURES 1u
typedef struct cstark_witness_report {
    uint32_t n_tx, merkle_depth; /* of the witness that was checked */
    int32_t first_bad;           /* the first transfer whose verdict is not VALID; -1: none */
    uint32_t first_verdict;      /* its cstark_witness_verdict (VALID when first_bad == -1) */
    uint32_t n_bad;              /* transfers whose verdict is not VALID */
    uint32_t reserved;           /* 0 */
    uint64_t final_root[7];      /* the receiver-new fold of the last transfer, whatever the verdicts: the root the batch leaves */
} cstark_witness_report;
/* Checks a witness on the device in one launch, one workgroup per transfer.  Two forms:
 *  - w != NULL, the host form: w's arrays are host memory, n_tx 1 .. 2^20 and need not be a power of two, merkle_depth one that
 *    cstark_tx_witness_upload accepts; w->final_root is the stated final root and the final_root argument must be NULL.  A null field, or
 *    a word >= p in any field of field elements (in the order of the struct's fields; sig_rx included, whatever the flags), is
 *    CSTARK_ERR_INVALID_ARG before anything is launched and with the outputs untouched; cstark_last_error names the first such word.
 *    The witness goes into a device block of its own, which the context keeps and frees: the RESIDENT witness is not replaced.
 *  - w == NULL, the resident form: the witness that cstark_tx_witness_upload or cstark_ledger_apply left in the context is checked as it
 *    lies; nothing is uploaded but final_root ([7], reduced words), which is optional: without it the last transfer's NEXT_ROOT test does
 *    not run.  No resident transaction witness, or one of more than 2^20 transfers, is CSTARK_ERR_INVALID_ARG.  The resident words are
 *    not tested against p (cstark_tx_witness_upload does not test them either): a transfer with such a word gets the verdict its
 *    arithmetic happens to give, every read stays inside the witness, and a sig_rx word >= p can equal no x coordinate, so that
 *    transfer's signature verdict is CSTARK_WITNESS_SIGNATURE.
 * flags: 0 or CSTARK_WITNESS_CHECK_SIGNATURES.  With it the message of transfer t -- build_tx_message of s_old_values[t],
 * r_old_values[t], deltas[t] and the sender's old nonce, what cstark_ledger_apply_checked signs against -- is gathered on the device
 * and the device run of cstark_schnorr_check_signatures follows, in that call's scratch; a transfer whose verdict is VALID so far and
 * whose signature verdict is anything but CSTARK_SIG_VALID becomes CSTARK_WITNESS_SIGNATURE.
 * report (required) is described above; verdicts_out (optional) [n_tx]: one cstark_witness_verdict each; folds_out (optional)
 * [n_tx][4][7]: the four folds of every transfer, sender-old, sender-new, receiver-old, receiver-new, whatever the verdicts (the first
 * and last from the stated leaf digests).  An inconsistency is a finding, not a failure: the status is CSTARK_OK.  Synchronous and
 * read-only: the resident witness, the statement caches and every ledger are neither written nor moved, so a proof after a check is
 * the proof without it. */
int cstark_tx_witness_check(cstark_ctx *ctx, const cstark_tx_witness *w /* NULL: the RESIDENT witness */,
                            const uint64_t *final_root /* [7]; resident form only, may be NULL */, uint32_t flags,
                            cstark_witness_report *report, uint8_t *verdicts_out /* [n_tx] or NULL */,
                            uint64_t *folds_out /* [n_tx][4][7] or NULL: sender-old, sender-new, receiver-old, receiver-new */);

/* ---- ledger checkpoints: take a batch back, open accounts under a past root, audit the resident tree -----------------------------
 * A checkpoint names the ledger's state at the moment it is taken.  Old states are kept by not overwriting them: while a checkpoint is
 * live, the first change of a tree node since the newest checkpoint goes to a fresh slot of the device pool and the old slot stays as it
 * is.  cstark_ledger_apply and cstark_ledger_set_accounts run the same launches and copies with and without live
 * checkpoints and write the same witness; a ledger without a live checkpoint allocates what it always did.  Ids are 64-bit, count from
 * 1 and are never reused within a ledger; 0 means "the current state" wherever an id is read (revert and release refuse it).  At most
 * CSTARK_LEDGER_MAX_CHECKPOINTS are live at once: one more is CSTARK_ERR_UNSUPPORTED.  Misuse as for the other ledger calls: null
 * pointers, a ledger of another context, or an id that is unknown, released or dropped by a revert give CSTARK_ERR_INVALID_ARG with the
 * outputs untouched; a ledger broken by an earlier HIP failure gives CSTARK_ERR_HIP; every call is synchronous on the ledger's context. */
#define CSTARK_LEDGER_MAX_CHECKPOINTS 16
/* O(1), no device work. */
int cstark_ledger_checkpoint(cstark_ctx *ctx, cstark_ledger *ledger, uint64_t *id_out);
/* The ledger's state becomes the state at `id`: root, accounts and openings are those of that moment, the slots written since are free
 * again, the checkpoints taken after `id` are dropped (their ids are invalid from now on) and `id` itself stays live, so it can be
 * reverted to again.  Host bookkeeping only: nothing is launched or copied.  The RESIDENT WITNESS is left alone: it is still the last
 * applied batch's, and proving it stays legal although the ledger no longer holds its final root. */
int cstark_ledger_revert(cstark_ctx *ctx, cstark_ledger *ledger, uint64_t id);
/* The checkpoint ends; the current state and the other checkpoints are unchanged, the slots only it kept are free again.  No device work. */
int cstark_ledger_release(cstark_ctx *ctx, cstark_ledger *ledger, uint64_t id);
/* cstark_ledger_root for the state at `id` (0: the current state). */
int cstark_ledger_root_at(cstark_ctx *ctx, cstark_ledger *ledger, uint64_t id, uint64_t root[7]);
/* cstark_ledger_open_accounts for the state at `id`, with the same arguments, outputs and refusals: values, presence, paths and root
 * as they were at the checkpoint (an account created later is absent: an all-zero leaf under the old siblings).  One upload, one
 * gather, no hashing.  With id 0 it is cstark_ledger_open_accounts, byte for byte. */
int cstark_ledger_open_accounts_at(cstark_ctx *ctx, cstark_ledger *ledger, uint64_t id, uint32_t count, const uint64_t *indices,
                                   uint64_t *values_out /* [count][14] */, uint8_t *present_out /* [count] */,
                                   uint64_t *paths_out /* [count][depth + 1][7] */, uint64_t root_out[7]);
/* The audit: is the state at `id` (0: the current one) a Merkle tree?  Three kinds of test, every one on digests as they are STORED:
 *   EMPTY  empty-subtree digest l equals merge(digest l + 1, digest l + 1), and digest `depth` is all zero;
 *   LEAF   every stored leaf equals merge(value[0..7], value[7..14]) of its account;
 *   INNER  every stored inner node (level, x) equals merge of its children (level + 1, 2x) and (level + 1, 2x + 1), an untouched child
 *          reading the empty-subtree digest of its level.
 * The tests run in one launch in a fixed order: EMPTY from level depth down to 0, LEAF by ascending index, INNER from level depth - 1
 * down to 0 (the root) and by ascending x within a level.  A wrong node fails its own test and, unless it is the root, its parent's.
 * An inconsistency is a finding, not a failure of the call: the status is CSTARK_OK and the report says so.  Read-only: pool, index,
 * root and resident witness are unchanged.  A state too large to plan is CSTARK_ERR_UNSUPPORTED. */
typedef enum cstark_ledger_node_kind { CSTARK_LEDGER_NODE_EMPTY = 0, CSTARK_LEDGER_NODE_LEAF = 1, CSTARK_LEDGER_NODE_INNER = 2 } cstark_ledger_node_kind;
typedef struct cstark_ledger_audit_report {
    uint32_t consistent;        /* 1: every test passed */
    uint32_t n_bad;             /* failing tests */
    uint32_t first_kind;        /* cstark_ledger_node_kind of the first failing test in the order above (0 when consistent) */
    uint32_t first_level;       /* its level: 0 = the root, depth = the leaves; for EMPTY the level of the digest */
    uint64_t first_index;       /* its index within the level (0 for EMPTY) */
    uint64_t n_nodes;           /* nodes of the audited state, all levels */
    uint64_t slots_live, slots_held, slots_free; /* of the whole ledger: current nodes, slots only checkpoints keep, free list */
} cstark_ledger_audit_report;
int cstark_ledger_audit(cstark_ctx *ctx, cstark_ledger *ledger, uint64_t id, cstark_ledger_audit_report *report);

/* ---- multi-openings: one Merkle multiproof for many accounts -------------------------------------------------------
 * The multiproof of a tree of depth d and a STRICTLY ASCENDING list of leaf indices I:
 *     K_d = I;  for each level l = d .. 1, every x of K_l in ascending order contributes the proof node (l, x ^ 1) iff x ^ 1 is not in
 *     K_l;  K_{l-1} is the set of parents {x >> 1} of K_l.
 * nodes [n_nodes][7] holds those digests in that order: level d (the leaves' level) first, ascending x within a level.  The fold takes
 * n_merges = sum over l < d of |K_l| merges (the `count` leaf hashes are not among them).  The leaf of an opened index is
 * merge(value[0..7], value[7..14]) when the account is present and the all-zero digest when it is absent, and an untouched sibling is the
 * empty-subtree digest of its level, exactly as in cstark_ledger_open_accounts: absence is provable.  With all 2^d leaves opened,
 * n_nodes = 0.
 * Host only: n_nodes and n_merges of (depth, indices).  depth outside 1 .. 31, count outside 1 .. 2^20, null pointers, or indices that
 * are not strictly ascending below 2^depth are CSTARK_ERR_INVALID_ARG with the outputs untouched (cstark_last_error names the first
 * offending position). */
int cstark_account_multiproof_shape(uint32_t depth, uint32_t count, const uint64_t *indices, uint32_t *n_nodes, uint32_t *n_merges);
/* The multiproof of `count` (1 .. 2^20) leaves of the state at `id` (0: the current state; otherwise a live checkpoint, as in
 * cstark_ledger_open_accounts_at).  values_out [count][14] and present_out [count] are what cstark_ledger_get_accounts gives (of that
 * state); nodes_out receives the n_nodes proof nodes, *n_nodes their number, root_out the root they fold to.  Indices must be strictly
 * ascending below 2^depth: if not, the call is CSTARK_ERR_INVALID_ARG with the outputs untouched, as for null pointers (nodes_out may be
 * null only with nodes_capacity == 0), a bad count, an unknown id or a ledger of another context.  A nodes_capacity below the need is
 * CSTARK_ERR_INVALID_ARG with *n_nodes set to the need and nothing else written (cstark_account_multiproof_shape states the need
 * beforehand).  n_nodes == 0 is legal.  Synchronous and read-only: one upload of a slot list, one gather on the device, no hashing;
 * root, stored nodes, accounts and the resident witness are unchanged. */
int cstark_ledger_open_multi(cstark_ctx *ctx, cstark_ledger *ledger, uint64_t id, uint32_t count, const uint64_t *indices,
                             uint64_t *values_out /* [count][14] */, uint8_t *present_out /* [count] */,
                             uint64_t *nodes_out /* [nodes_capacity][7] */, uint32_t nodes_capacity, uint32_t *n_nodes, uint64_t root_out[7]);
/* The verifier's side: needs no ledger and takes any depth 1 .. 31.  The verdict is the first that applies. */
typedef enum cstark_multi_verdict {
    CSTARK_MULTI_VALID = 0,
    CSTARK_MULTI_INDEX = 1,      /* *at = the first position whose index is >= 2^depth or not above its predecessor */
    CSTARK_MULTI_NODE_COUNT = 2, /* n_nodes differs from the shape's count; *at = the needed count */
    CSTARK_MULTI_ROOT = 3        /* the fold differs from `root`; root_out holds the fold */
} cstark_multi_verdict;
/* Folds one multiproof on the device: the leaf hashes in one launch, then one launch per level.  Exactly one of `values` [count][14] and
 * `leaves` [count][7] is given: with values the leaf of position i is merge(values[i][0..7], values[i][7..14]) where present[i] != 0 (a
 * NULL present: all present) and the all-zero digest where present[i] == 0; with leaves (digest mode, present must be NULL) the stated
 * digests are the leaves.  nodes [n_nodes][7] may be NULL iff n_nodes == 0.  The shape of an untrusted proof is data, so INDEX and
 * NODE_COUNT are verdicts, not misuse: the status is CSTARK_OK, nothing is launched and root_out is untouched.  *at is 0 for VALID and
 * ROOT.  root_out (optional) receives the fold for VALID and ROOT; n_merges (optional) receives the shape's merge count unless the
 * verdict is INDEX.
 * Null ctx, indices, root, verdict or at, depth outside 1 .. 31, count outside 1 .. 2^20, both or neither of values and leaves, present
 * without values, nodes null with n_nodes != 0 or the reverse, or a word >= p in values, leaves, nodes or root is CSTARK_ERR_INVALID_ARG
 * before anything is launched and with the outputs untouched; cstark_last_error names the first such word, in that order of the arrays.
 * Synchronous, on the context's stream, in a device block of its own that the context keeps and frees: the resident witness and the
 * blocks of the other checks are neither read nor written, so a proof after a check is the proof without it. */
int cstark_account_check_multiproof(cstark_ctx *ctx, uint32_t depth, uint32_t count, const uint64_t *indices,
                                    const uint64_t *values /* [count][14] or NULL */, const uint8_t *present /* [count] or NULL */,
                                    const uint64_t *leaves /* [count][7] or NULL */, const uint64_t *nodes /* [n_nodes][7] */, uint32_t n_nodes,
                                    const uint64_t root[7], uint32_t *verdict /* cstark_multi_verdict */, uint32_t *at,
                                    uint64_t *root_out /* optional [7] */, uint32_t *n_merges /* optional */);

/* ---- a partial ledger from a multi-opening ----------------------------------------------------------------------------
 * A ledger of someone who does not hold the tree: built from a multi-opening (indices, values, present, nodes) under a stated root, it
 * stores the leaf of every opened PRESENT account, every proof node (opaque: taken on trust under the root, nothing stored beneath it)
 * and every node of the fold.  A leaf is KNOWN iff it has no opaque ancestor-or-self: exactly the opened indices, present or absent, for
 * the ledger's life.  For known accounts every ledger call behaves as on a full ledger: apply and apply_checked (the resident witness
 * follows), set_accounts (which may create an opened absent account), root, open, open_multi, checkpoint, revert, release, audit.  What
 * would touch an unknown account is refused: a transfer with an unknown sender or receiver with CSTARK_LEDGER_UNKNOWN (nothing changed),
 * and cstark_ledger_set_accounts, _get_accounts, _open_accounts(_at) and _open_multi with an unknown index with CSTARK_ERR_INVALID_ARG,
 * nothing changed, outputs untouched, cstark_last_error naming the first such position.  cstark_ledger_audit does not test an opaque
 * node itself (its parent's test reads it); n_nodes of the report still counts every stored node.
 * merkle_depth as for cstark_ledger_create; count 1 .. 2^20; indices strictly ascending below 2^depth; a NULL present: all present.  The
 * shape of an untrusted opening is data, as in cstark_account_check_multiproof: CSTARK_MULTI_INDEX and _NODE_COUNT are verdicts with
 * status CSTARK_OK, *at as there, nothing launched and *out = NULL.  A fold that differs from `root` is the verdict CSTARK_MULTI_ROOT with
 * *out = NULL and nothing left allocated; CSTARK_MULTI_VALID gives a ledger whose cstark_ledger_root is `root`.  Null ctx, indices,
 * values, root, out, verdict or at, a bad depth or count, nodes null with n_nodes != 0 or the reverse, or a word >= p in values, nodes or
 * root is CSTARK_ERR_INVALID_ARG before anything is launched, outputs untouched; cstark_last_error names the first such word, in that
 * order of the arrays.  Device work: one upload that puts the proof nodes into their final pool slots and the values into scratch, the
 * leaf hashes and one launch per level straight into the new ledger's pool, the root read back.  The resident witness is not touched.
 * One opening per ledger: several openings cannot be combined, and none can be added later. */
int cstark_ledger_create_partial(cstark_ctx *ctx, uint32_t merkle_depth, uint32_t count, const uint64_t *indices,
                                 const uint64_t *values /* [count][14] */, const uint8_t *present /* [count] or NULL */,
                                 const uint64_t *nodes /* [n_nodes][7], NULL iff n_nodes == 0 */, uint32_t n_nodes, const uint64_t root[7],
                                 cstark_ledger **out, uint32_t *verdict /* cstark_multi_verdict */, uint32_t *at);
/* known_out[i] = 1 iff the ledger knows leaf indices[i]; a full ledger knows every index below 2^depth. */
int cstark_ledger_known(cstark_ctx *ctx, cstark_ledger *ledger, uint32_t count, const uint64_t *indices, uint8_t *known_out);
/* Full ledger: is_partial = 0, n_opaque = 0, n_known = the number of accounts.  Partial: n_known opened indices, n_opaque proof nodes. */
int cstark_ledger_partial_info(cstark_ctx *ctx, cstark_ledger *ledger, uint32_t *is_partial, uint64_t *n_known, uint64_t *n_opaque);

/* ---- a root update checked without a ledger -------------------------------------------------------------------------
 * Whoever holds only roots checks "these accounts changed from old_values to new_values, and that takes old_root to new_root", or
 * computes the root the change leads to.  The opening (indices, old_values, old_present, nodes) is a multi-opening under old_root as
 * cstark_ledger_open_multi gives it; the new state of the SAME positions is (new_values, new_present), and the proof nodes, which no
 * opened leaf lies under, serve both states.  The verdict is the first that applies. */
typedef enum cstark_update_verdict {
    CSTARK_UPDATE_VALID = 0,
    CSTARK_UPDATE_INDEX = 1,      /* as CSTARK_MULTI_INDEX */
    CSTARK_UPDATE_NODE_COUNT = 2, /* as CSTARK_MULTI_NODE_COUNT */
    CSTARK_UPDATE_OLD_ROOT = 3,   /* the old values do not fold to old_root; nothing is said about the new side */
    CSTARK_UPDATE_NEW_ROOT = 4    /* the old side is valid, the new values fold to something other than new_root */
} cstark_update_verdict;
/* Folds both states on the device in ONE pass: the leaf hashes in one launch, then one launch per level, as many launches as one
 * cstark_account_check_multiproof takes.  A node of the new state is hashed only where a changed leaf lies below it and is the old
 * state's digest elsewhere, so one changed account among many costs `depth` more hashes than the check of the opening alone.  Any depth
 * 1 .. 31 and count 1 .. 2^20.  A NULL old_present or new_present means all present; where a flag is 0 the leaf is the all-zero digest
 * and the value words do not enter the fold.  new_root == NULL means "compute only": the verdict is then VALID or OLD_ROOT.  new_root_out
 * (optional) receives the fold of the new state for VALID and NEW_ROOT and is untouched otherwise; n_changed (optional) receives, for
 * VALID, OLD_ROOT and NEW_ROOT, the number of positions whose (value, presence) differ -- two absent positions are equal whatever their
 * value words.  INDEX and NODE_COUNT are verdicts with *at as in cstark_account_check_multiproof: the status is CSTARK_OK and nothing is
 * launched.  *at is 0 for the other verdicts.
 * Null ctx, indices, old_values, new_values, old_root, verdict or at, depth outside 1 .. 31, count outside 1 .. 2^20, nodes null with
 * n_nodes != 0 or the reverse, or a word >= p in old_values, new_values, nodes, old_root or new_root is CSTARK_ERR_INVALID_ARG before
 * anything is launched and with the outputs untouched; cstark_last_error names the first such word, in that order of the arrays.
 * Synchronous, on the context's stream, in the device block of cstark_account_check_multiproof, which neither call keeps anything in
 * between calls: the resident witness and the blocks of the path and signature checks are neither read nor written, so a proof after
 * a check is the proof without it. */
int cstark_account_check_update(cstark_ctx *ctx, uint32_t depth, uint32_t count, const uint64_t *indices,
                                const uint64_t *old_values /* [count][14] */, const uint8_t *old_present /* [count] or NULL */,
                                const uint64_t *new_values /* [count][14] */, const uint8_t *new_present /* [count] or NULL */,
                                const uint64_t *nodes /* [n_nodes][7] */, uint32_t n_nodes, const uint64_t old_root[7],
                                const uint64_t *new_root /* [7] or NULL */, uint32_t *verdict /* cstark_update_verdict */, uint32_t *at,
                                uint64_t *new_root_out /* optional [7] */, uint32_t *n_changed /* optional */);

/* ---- verification (TransactionExample::verify, src/lib.rs:144-150: winterfell::verify over this library's own proof layout) -------
 * The call's status (cstark_status) is kept apart from the proof's verdict.  A verdict names the FIRST check that fails, in this
 * order: layout (MALFORMED, then UNSUPPORTED) | OPTIONS_MISMATCH | OOD | REMAINDER_COMMITMENT | POW | per query q = 0..nq-1:
 * TRACE_OPENING(q), COMPOSITION_OPENING(q) (a compact proof: TRACE_OPENING, then COMPOSITION_OPENING, one multiproof each: a wrong
 * n_nodes, a wrong node or a wrong row of the tree) | per FRI layer l: LAYER_COUNT(l), LAYER_OPENING(l), LAYER_FOLDING(l) (layer 0: the DEEP
 * values against the layer-0 rows) | REMAINDER_FOLDING | REMAINDER_DEGREE.  A field element word >= p anywhere in the proof is
 * MALFORMED (the prover never writes one). */
typedef enum cstark_verdict {
    CSTARK_PROOF_OK = 0,                 /* verify: accepted;  inspect: well-formed */
    CSTARK_PROOF_MALFORMED = 1,          /* layout, counts, lengths, non-canonical field element, trailing bytes */
    CSTARK_PROOF_UNSUPPORTED = 2,        /* well-formed proof of another AIR than the call verifies or the caller states */
    CSTARK_PROOF_OPTIONS_MISMATCH = 3,   /* differs from `expected` */
    CSTARK_PROOF_OOD = 4,                /* out-of-domain constraint evaluations inconsistent (also: wrong public inputs) */
    CSTARK_PROOF_REMAINDER_COMMITMENT = 5,
    CSTARK_PROOF_POW = 6,
    CSTARK_PROOF_TRACE_OPENING = 7,
    CSTARK_PROOF_COMPOSITION_OPENING = 8,
    CSTARK_PROOF_LAYER_COUNT = 9,        /* a layer's number of openings differs from the derived positions */
    CSTARK_PROOF_LAYER_OPENING = 10,
    CSTARK_PROOF_LAYER_FOLDING = 11,
    CSTARK_PROOF_REMAINDER_FOLDING = 12,
    CSTARK_PROOF_REMAINDER_DEGREE = 13
} cstark_verdict;

typedef struct cstark_proof_info {
    uint32_t air, trace_width, log_n, header_word;   /* header_word: the Merkle depth for TransactionAir */
    cstark_options options;
} cstark_proof_info;

/* Host only: no context, no device.  Checks the complete layout of a proof of any of the five AIRs (see "Proof layout" at
 * cstark_tx_prove: every count against the stated options before anything is read, no trailing bytes, the header bounds the prover
 * enforces) and fills *info (zeroed when the header cannot be read).  *verdict = CSTARK_PROOF_OK or CSTARK_PROOF_MALFORMED; field
 * elements are not read (their canonical form is checked by cstark_tx_verify).  Returns CSTARK_ERR_INVALID_ARG only for null pointers. */
int cstark_proof_inspect(const uint8_t *proof, size_t len, cstark_proof_info *info, int32_t *verdict);
/* Host only: *form = CSTARK_FORM_PLAIN or CSTARK_FORM_COMPACT by the proof's magic; CSTARK_ERR_INVALID_ARG for null pointers, fewer than
 * four bytes or neither magic.  Says nothing about the rest of the layout (cstark_proof_inspect accepts both forms). */
int cstark_proof_form(const uint8_t *proof, size_t len, uint32_t *form);

/* TransactionExample::verify for `count` proofs in one call (count = 1 for a single proof).  initial_roots / final_roots: [count][7],
 * memory form.  expected: NULL = each proof's own options (the reference's semantics), else every proof must state exactly these.
 * Proofs of one call may differ in every header field (sizes, depths, hashes, extensions); a proof's verdict does not depend on the
 * others.  Synchronous: verdicts[count] are on the host when it returns CSTARK_OK.  Negative status only for misuse (null pointers with
 * count > 0, a root word >= p) or a HIP failure.  The verifier's buffers belong to the context; the prover's are not touched. */
int cstark_tx_verify(cstark_ctx *ctx, uint32_t count, const uint8_t *const *proofs, const size_t *proof_lens,
                     const uint64_t *initial_roots, const uint64_t *final_roots, const cstark_options *expected,
                     int32_t *verdicts);
/* The same for TransactionAir, MerkleAir, RangeProofAir and RescueAir proofs, `count` of them in one call; a batch may mix AIRs, sizes,
 * hashes and extensions (one pipeline, cstark_tx_verify is its all-TransactionAir call).  airs[i]: the AIR the caller expects proof i to be
 * (CSTARK_AIR_*).  public_inputs: [count][14] words, memory form -- TransactionAir / MerkleAir: initial root | final root; RescueAir: seed
 * | result; RangeProofAir: word 0 = number, words 1..13 ignored.  A well-formed proof whose header states another AIR than airs[i] is
 * UNSUPPORTED, and so is every proof with airs[i] == CSTARK_AIR_SCHNORR (its statement is O(n) public data, which the 14 words cannot
 * carry: cstark_schnorr_verify); header
 * values no prover of this library writes (a Merkle depth or a trace length the AIR does not have) are MALFORMED.  Negative status only
 * for null pointers, an airs[i] that is no CSTARK_AIR_* id, a used public word >= p, or a HIP failure. */
int cstark_air_verify(cstark_ctx *ctx, uint32_t count, const uint8_t *const *proofs, const size_t *proof_lens, const int32_t *airs,
                      const uint64_t *public_inputs, const cstark_options *expected, int32_t *verdicts);
/* SchnorrExample::verify (src/schnorr/mod.rs:175-186) for `count` SchnorrAir proofs in one call: the pipeline, the verdict order and the
 * chunking of cstark_air_verify; a batch may mix numbers of signatures, hashes, extensions and options, and a verdict does not depend on the
 * rest of the batch.  statements[i]: everything the proof is about -- the messages (public key || 16 elements), R.x and s of every
 * signature; its bytes are staged with the proof (and count towards a chunk), its channel seed is hashed on the host, and the values the
 * out-of-domain check needs of it (19 public-input columns, 12 sequence polynomials, at z) are formed on the device in one pass
 * (cstark_schnorr_public_at is that stage alone).  A well-formed proof of another AIR is UNSUPPORTED.  A statement whose n_sig differs from
 * the proof's header word -- any n_sig that is not a power of two among them -- gives CSTARK_PROOF_OOD, after MALFORMED, UNSUPPORTED and
 * OPTIONS_MISMATCH.  Negative status only for null pointers with count > 0, n_sig == 0, a messages / sig_rx word >= p, or a HIP failure. */
typedef struct cstark_schnorr_statement {
    uint32_t n_sig;
    const uint64_t *messages;   /* [n_sig][28], memory form */
    const uint64_t *sig_rx;     /* [n_sig][6],  memory form */
    const uint8_t  *sig_s;      /* [n_sig][32] */
} cstark_schnorr_statement;
int cstark_schnorr_verify(cstark_ctx *ctx, uint32_t count, const uint8_t *const *proofs, const size_t *proof_lens,
                          const cstark_schnorr_statement *statements, const cstark_options *expected, int32_t *verdicts);
/* ---- conversion between the proof forms: a proof of either form and its statement -> the same proof in the other form, byte for byte
 * what the prover would have written (a proof written before the compact form existed, a sharded proof -- the sharded phases write the
 * plain form only -- or a compact proof for a consumer that reads paths).
 * cstark_proof_convert_bound (host only): a capacity that holds `proof` converted to `form` whatever its positions.  To
 * CSTARK_FORM_PLAIN: the exact plain length (it follows from the header and each layer's stated n_positions).  To CSTARK_FORM_COMPACT:
 * the plain length plus 4 bytes per tree (a multiproof never holds more nodes than the paths it is selected from; each tree gains a count
 * word).  CSTARK_ERR_INVALID_ARG for a null pointer, another form, or a layout that does not parse (cstark_proof_inspect).
 * The three convert calls ARE their verify calls: the same arguments, misuse rules, chunking and verdicts -- verdicts[i] is what the
 * verify call returns for the same inputs, whatever the neighbours are and wherever the chunks divide -- and each also writes every proof
 * whose verdict is CSTARK_PROOF_OK to out[i] in `form`, out_lens[i] its length.  Plain to compact: every path section becomes the
 * canonical multiproof of its tree ("Proof layout"), selected on the device next to the replayed positions.  Compact to plain: one path
 * per opened row in proof order, from the inner nodes the multiproof's fold computes on the device.  Everything outside the path sections
 * is copied unchanged; a proof already in `form` is copied through unchanged.  A proof with any other verdict is not converted:
 * out_lens[i] = 0 and out[i] is not written.  form must be CSTARK_FORM_PLAIN or CSTARK_FORM_COMPACT.  Null out, capacities or out_lens
 * with count > 0 is CSTARK_ERR_INVALID_ARG.  Every capacities[i] is checked against cstark_proof_convert_bound before anything is
 * launched, for every proof whose layout parses: a short one (or a null out[i]) is CSTARK_ERR_INVALID_ARG, cstark_last_error names the
 * proof, and no output is written.  The verifier's buffers belong to the context; the prover's arena, the resident witness and the
 * context's proof form setting are neither read nor changed.  cstark_verify_stage_ms and cstark_verify_h2d_bytes describe a convert call
 * as they describe a verify call: the conversion's kernels count under the openings stage, its copy back under the last stage, the
 * host's writing of the proofs under the first. */
int cstark_proof_convert_bound(const uint8_t *proof, size_t len, uint32_t form, size_t *bound);
int cstark_tx_convert(cstark_ctx *ctx, uint32_t count, const uint8_t *const *proofs, const size_t *proof_lens,
                      const uint64_t *initial_roots, const uint64_t *final_roots, const cstark_options *expected,
                      uint32_t form, uint8_t *const *out, const size_t *capacities, size_t *out_lens, int32_t *verdicts);
int cstark_air_convert(cstark_ctx *ctx, uint32_t count, const uint8_t *const *proofs, const size_t *proof_lens, const int32_t *airs,
                       const uint64_t *public_inputs, const cstark_options *expected,
                       uint32_t form, uint8_t *const *out, const size_t *capacities, size_t *out_lens, int32_t *verdicts);
int cstark_schnorr_convert(cstark_ctx *ctx, uint32_t count, const uint8_t *const *proofs, const size_t *proof_lens,
                           const cstark_schnorr_statement *statements, const cstark_options *expected,
                           uint32_t form, uint8_t *const *out, const size_t *capacities, size_t *out_lens, int32_t *verdicts);
/* Stage entry point, like the other stages: the 19 public-input columns (12 public-key words, 7 hash-input words) and the 12
 * sequence-value polynomials (R.x at step 0, at step 511) of a statement at one point z of the degree-m extension, m in {1, 2, 3};
 * out [31][m], memory form, host memory.  CSTARK_ERR_INVALID_ARG if z^n = 1 (n = 512 n_sig) or n_sig is not a power of two (at most 4096). */
int cstark_schnorr_public_at(cstark_ctx *ctx, uint32_t n_sig, const uint64_t *messages, const uint64_t *sig_rx, const uint64_t *z,
                             uint32_t m, uint64_t *out);
/* Stage times of the last cstark_tx_verify / cstark_air_verify / cstark_schnorr_verify on this context, like cstark_prove_stage_ms (milliseconds, summed over its chunks):
 * host parse + staging, host-to-device copy, transcript replay (on the device), out-of-domain check, Merkle openings, DEEP + FRI,
 * remainder + reduction + device-to-host copy.  cstark_verify_h2d_bytes: the bytes the same call copied host -> device (proof bytes,
 * descriptors, opening records). */
#define CSTARK_VERIFY_NUM_STAGES 7
/* Batches of any size: the verify calls stage proofs (their bytes, descriptors and opening records) for the device in chunks of at
 * most this many bytes and verifies one chunk after the other, so a large count never sizes its buffers beyond one chunk (a single
 * larger proof is a chunk of its own).  Verdicts do not depend on where the chunks divide. */
#define CSTARK_VERIFY_CHUNK_BYTES 67108864 /* 64 MiB */
int cstark_verify_stage_ms(cstark_ctx *ctx, float *ms /* [CSTARK_VERIFY_NUM_STAGES] */);
int cstark_verify_h2d_bytes(cstark_ctx *ctx, uint64_t *bytes);

/* ---- trace validation: Trace::validate of the reference's debug builds, on the device ----
 * Evaluates every transition constraint of `air` on every frame (r, r + 1), r < n - 1, of the base trace d_trace ([width][n] device memory,
 * the layout of the cstark_*_build_trace entry points, n = 2^log_n) and, with public_inputs, every boundary entry, and names the first
 * violation.  A constraint is violated where the SUM of its contributions is non-zero.  Cycles: 1024 rows (one transfer) for TransactionAir,
 * 512 for MerkleAir and SchnorrAir, 8 for RescueAir, the whole trace for RangeProofAir.
 *   item           the Merkle depth for TransactionAir and MerkleAir (1, 3, 7, 15 or 31); ignored otherwise.
 *   public_inputs  host [14] as cstark_air_verify takes them (RangeProofAir: word 0); NULL: no boundary check (boundary = -1).  Boundary
 *                  lists, in the order of `boundary`: TransactionAir / MerkleAir registers 58..64 at step 0 against the initial root, then
 *                  at step n - 1 against the final root (for TransactionAir entries 0, 1, 7, 8 are the AIR's assertions, the others public
 *                  words the channel seed binds); RescueAir registers 0..6 at the first and last row against seed | result; RangeProofAir
 *                  register 1 = 0 at step 0, = number at step n - 1; SchnorrAir: any non-NULL pointer checks the 61 assertions of
 *                  get_assertions (every 512 rows) against the resident statement (cstark_schnorr_witness_upload), whose messages the
 *                  transitions always read: no resident statement of this trace length is CSTARK_ERR_INVALID_ARG.
 *   cycle_codes    optional host [n / cycle length]: per cycle CSTARK_TRACE_CLEAN or (first violated row in the cycle) * n_constraints +
 *                  its lowest violated constraint.
 *   frame_values   optional host [n_constraints]: all constraint values of the first violated frame, memory form, from the free-standing
 *                  frame evaluator; untouched when the transitions are clean.  The named constraint's value is checked to be non-zero
 *                  there on every call that finds a violation: CSTARK_ERR_HIP if the two evaluators disagree.
 * Synchronous, on the context's stream.  Violations are not failures: the status is CSTARK_OK.  Null ctx, d_trace or report, an unknown
 * air, a log_n the AIR cannot have (fewer rows than one cycle, more than 2^24), a bad depth or a public word >= p is
 * CSTARK_ERR_INVALID_ARG before anything is launched and with the outputs untouched.  Trace cells >= p are the caller's responsibility,
 * as for every other device-table entry point.  The resident witness, the prover's buffers and the scratch of the signature and path
 * checks are neither read nor written: a proof after a validation is the proof without it. */
#define CSTARK_TRACE_CLEAN 0xFFFFFFFFu
typedef struct cstark_trace_report {
    int64_t  step;               /* first row r whose frame (r, r+1) violates a transition constraint; -1: none */
    uint32_t constraint;         /* the lowest violated constraint index at that row (CSTARK_TRACE_CLEAN: none) */
    uint32_t bad_cycles;         /* cycles with at least one violated frame */
    int32_t  boundary;           /* index of the first failing boundary entry (list order above); -1: none, or not checked */
    uint32_t boundary_register;
    uint64_t boundary_step;
} cstark_trace_report;
/* The shape cstark_air_validate_trace works on (csrc/trace_check.h; host only): trace width, transition constraints and log2 of the
 * cycle length (RangeProofAir: log_n) of `air` at 2^log_n rows.  CSTARK_ERR_INVALID_ARG for an unknown air or a log_n the AIR cannot have. */
int cstark_air_trace_shape(int air, uint32_t log_n, uint32_t *width, uint32_t *n_constraints, uint32_t *log_cycle);
int cstark_air_validate_trace(cstark_ctx *ctx, int air, const uint64_t *d_trace, uint32_t log_n, uint32_t item,
                              const uint64_t *public_inputs, cstark_trace_report *report,
                              uint32_t *cycle_codes, uint64_t *frame_values);

/* ---- device memory helpers for callers without a HIP runtime of their own (the Rust shim) ---- */
int cstark_malloc(cstark_ctx *ctx, size_t bytes, void **d_ptr);
int cstark_free(cstark_ctx *ctx, void *d_ptr);
int cstark_memcpy_h2d(cstark_ctx *ctx, void *d_dst, const void *src, size_t bytes);
int cstark_memcpy_d2h(cstark_ctx *ctx, void *dst, const void *d_src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* CSTARK_H */
