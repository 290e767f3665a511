/* cstark_debug_commit.h -- TEST-ONLY, served by libcstark_debug.so like cstark_debug_channel.h: thin wrappers over internal host
 * functions of the product library, so that a test chooses the layouts and the positions of the commitment and opening kernels -- row
 * hashes of a table in block order (csrc/blake3.h), the batched tables and trees of the batched range prover (csrc/blake3.hip,
 * csrc/sha3.hip), the opening gathers of a proof (csrc/prove.hip, GatherList / k_gather_batch) and the opening kernel of the batched
 * range prover (csrc/range_batch.hip, k_rb_open).  `ctx` is a cstark_ctx; every call runs on the context's stream and synchronises it.
 *
 * Every argument is checked on the host BEFORE anything is launched or written: shapes against the limits of the wrapped function,
 * every position against its domain, and the reach of the kernels against the buffer sizes the caller states (`*_words`: 64-bit words,
 * `*_bytes`: bytes).  Return: 0 = success; 1 (hipErrorInvalidValue) = refused, nothing launched, nothing written; any other value is
 * the hipError_t of a failed runtime call.  hash_fn: 0 = Blake3_256, 1 = Sha3_256.  d_ pointers are device memory, all others host.
 */
#ifndef CSTARK_DEBUG_COMMIT_H
#define CSTARK_DEBUG_COMMIT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* cs::hash_rows / cs::hash_rows_sha3 with a block order: d_table = slots [k0, k0 + nk) of a table [2^log_b][width][2^log_n] whose slot
 * s holds LDE coset (s mod ce) 2^log_s + s / ce, ce = 2^(log_b - log_s); leaf 2^log_b j + k of d_leaves [2^(log_n + log_b)][32] = the
 * digest of row j of coset k, written for the cosets of the window only.  width 1..128, log_n <= 20, log_s <= log_b <= 4, nk >= 1,
 * k0 + nk <= 2^log_b. */
int cstark_debug_hash_rows_slots(void *ctx, uint32_t hash_fn, const uint64_t *d_table, size_t table_words, uint8_t *d_leaves, size_t leaves_bytes,
                                 uint32_t width, uint32_t log_n, uint32_t log_b, uint32_t log_s, uint32_t k0, uint32_t nk);
/* cs::hash_rows_batch(_sha3) then cs::merkle_build_batch(_sha3), as the batched range prover commits its tables: table t = columns
 * [t gw, (t + 1) gw) of d_table [2^log_b][gw batch][2^log_n]; its tree of L = 2^(log_n + log_b) leaves at d_nodes + t stride: 2 L
 * digests, node 0 zeroed, leaves in the upper half.  gw 1..8, batch 1..1024, 1 <= log_n + log_b <= 11, log_b <= 4, stride >= 64 L and a
 * multiple of 32. */
int cstark_debug_commit_batch(void *ctx, uint32_t hash_fn, const uint64_t *d_table, size_t table_words, uint8_t *d_nodes, size_t nodes_bytes, uint32_t gw,
                              uint32_t log_n, uint32_t log_b, uint32_t batch, size_t stride);
/* cs::merkle_build_batch(_sha3) alone, on leaves already in place: log_leaves 1..11, the rest as above */
int cstark_debug_merkle_batch(void *ctx, uint32_t hash_fn, uint8_t *d_nodes, size_t nodes_bytes, uint32_t log_leaves, uint32_t batch, size_t stride);
/* One job of the opening gather.  paths = 0: rows positions[q] = 2^log_b j + k of the table d_src [2^log_b][width][2^log_n] (slots in
 * block order log_s) -> d_out [count][width] words.  paths = 1: levels [lvl0, log_leaves) of the authentication paths of the leaves
 * positions[q] in the node array d_src [2 2^log_leaves][32] -> d_out [count][log_leaves][32] bytes (the levels below lvl0 are not
 * written).  dcount >= 0: that value is placed in device memory and the kernel reads the number of positions there (dcount <= count);
 * dcount < 0: the kernel takes `count`.  width 1..1024, log_n <= 24, log_s <= log_b <= 4, 1 <= log_leaves <= 28, lvl0 <= log_leaves,
 * count <= 4096, every position inside its domain (all `count` of them, whatever dcount). */
typedef struct cstark_debug_gather_job {
    uint32_t paths;
    const void *d_src;
    size_t src_bytes;
    uint32_t width, log_n, log_b, log_s; /* rows */
    uint32_t log_leaves, lvl0;           /* paths */
    const uint32_t *positions;           /* host [count] (may be null when count = 0) */
    uint32_t count;
    int64_t dcount;
    void *d_out;
    size_t out_bytes;
} cstark_debug_gather_job;
/* 1 .. 32 jobs in ONE launch of k_gather_batch, built by the prover's own GatherList::rows / paths / launch (gather_jobs_launch,
 * csrc/ctx.h); the positions are uploaded by the call */
int cstark_debug_gather(void *ctx, const cstark_debug_gather_job *jobs, uint32_t n_jobs);
/* cs::rb_open over a cs::RangeBatchOpen (csrc/range_batch.h) filled from these fields.  Tables of the batched range prover: d_lde,
 * d_clde [8][2 batch][64] words, d_layer [batch][512] words, d_tnodes, d_cnodes [batch][1024][32] bytes, d_lnodes [batch][256][32]
 * bytes (the layer buffers, lpos and lcount may be null when n_layers = 0).  pos, lpos [batch][nq] and lcount [batch] are HOST arrays:
 * pos < 512, lpos < 128, lcount[t] <= nq.  Proof t's slot = d_out + t slot; its sections at the byte offsets trows [nq][2] words,
 * tpaths [nq][9][32], crows [nq][2] words, cpaths [nq][9][32], lrows [nq][4] words, lpaths [nq][7][32] must lie inside the slot (rows
 * at multiples of 8, paths and `slot` at multiples of 16).  batch 1..1024, nq 1..128, n_layers 0..1. */
typedef struct cstark_debug_rb_open {
    const uint64_t *d_lde, *d_clde, *d_layer;
    size_t lde_words, clde_words, layer_words;
    const uint8_t *d_tnodes, *d_cnodes, *d_lnodes;
    size_t tnodes_bytes, cnodes_bytes, lnodes_bytes;
    const uint32_t *pos, *lpos, *lcount;
    uint8_t *d_out;
    size_t out_bytes;
    uint32_t nq, batch, n_layers;
    size_t slot, trows, tpaths, crows, cpaths, lrows, lpaths;
} cstark_debug_rb_open;
int cstark_debug_range_open(void *ctx, const cstark_debug_rb_open *o);
#ifdef __cplusplus
}
#endif
#endif
