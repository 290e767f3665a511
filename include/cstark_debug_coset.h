/* cstark_debug_coset.h -- TEST-ONLY, served by libcstark_debug.so like cstark_debug_commit.h: thin wrappers over internal host
 * functions of the product library, so that a test drives the kernels that carry polynomials between cosets as coefficient vectors
 * one at a time -- the extension from the even to the odd cosets, plain and merged, and the coset combination (csrc/ntt.h), the high
 * part of the final addition, its merged form and the data mover of the sharded path (csrc/constraints.h).  `ctx` is a cstark_ctx;
 * every call builds the power tables it needs (cs::ntt_power_table), runs on the context's stream and synchronises it.
 *
 * Every argument is checked on the host BEFORE anything is launched or written: shapes, windows, exponent and table indices, and the
 * reach of the kernels against the buffer sizes the caller states (`*_words`: 64-bit words).  Return: 0 = success; 1
 * (hipErrorInvalidValue) = refused, nothing launched, nothing written; any other value is the hipError_t of a failed runtime call.
 * Field elements: uint64_t in BaseElement memory form.  d_ pointers are device memory, all others host.  n = 2^log_n.
 */
#ifndef CSTARK_DEBUG_COSET_H
#define CSTARK_DEBUG_COSET_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define CSTARK_DEBUG_MERGE_FAMILIES 5 /* cs::COSET_MERGE_MAX_FAMILIES */
#define CSTARK_DEBUG_MERGE_TERMS 4    /* cs::COSET_MERGE_MAX_TERMS */
/* cs::coset_even_to_odd: d_in [tables][4 even cosets][n] -> d_out [4 odd cosets][tables][n], only the even cosets [kc0, kc0 + nkc)
 * counting (the words of the others are never read).  6 <= log_n <= NTT_MAX_LOG_N - 3, tables 1..64, nkc >= 1, kc0 + nkc <= 4,
 * in_words >= 4 tables n, out_words >= 4 tables n, d_in and d_out apart. */
int cstark_debug_even_to_odd(void *ctx, const uint64_t *d_in, size_t in_words, uint64_t *d_out, size_t out_words, uint32_t log_n, uint32_t tables,
                             uint32_t kc0, uint32_t nkc);
/* The families of cs::coset_even_to_odd_merged: family f = sum over t < terms[f] of x^exponent[f][t] S_table[f][t], every term built by
 * cs::coset_merge_term(table, exponent, log_n, base, k0).  families 1..5, terms 1..4, table < tables_per_set <= 64, raw_family in
 * [-1, families), base a canonical word, k0 1 or 2 (k0 = 2 only changes the constants: the kernel always writes the odd cosets). */
typedef struct cstark_debug_merge_desc {
    uint32_t families, tables_per_set;
    int32_t raw_family;
    uint32_t k0;
    uint64_t base;
    uint32_t terms[CSTARK_DEBUG_MERGE_FAMILIES];
    uint32_t table[CSTARK_DEBUG_MERGE_FAMILIES][CSTARK_DEBUG_MERGE_TERMS];
    uint64_t exponent[CSTARK_DEBUG_MERGE_FAMILIES][CSTARK_DEBUG_MERGE_TERMS];
} cstark_debug_merge_desc;
/* what cs::coset_merge_term built for one term: cs::CosetMergeTerm, field by field */
typedef struct cstark_debug_merge_term {
    uint64_t c[4][2];
    uint32_t table, r;
} cstark_debug_merge_term;
/* cs::coset_even_to_odd_merged: d_in [sets][tables_per_set][4][n] -> d_out [4 odd cosets][sets][families][n]; d_raw (may be null: then
 * nothing is written for raw_family) [sets][terms of raw_family][n].  terms_out (host, may be null): [5][4] terms, those of the
 * descriptor filled in -- written before the launch, after the checks.  6 <= log_n <= NTT_MAX_LOG_N - 3, sets 1..8, in_words >= 4 sets
 * tables_per_set n, out_words >= 4 sets families n, raw_words >= sets terms[raw_family] n where d_raw is given with raw_family >= 0. */
int cstark_debug_even_to_odd_merged(void *ctx, const uint64_t *d_in, size_t in_words, uint64_t *d_out, size_t out_words, uint64_t *d_raw, size_t raw_words,
                                    uint32_t log_n, uint32_t sets, const cstark_debug_merge_desc *desc, cstark_debug_merge_term *terms_out);
/* cs::coset_combine with the powers of w_N^-1, N = 2^(log_n + log_b), and 2^-log_b: d_b [tables][2^log_b][n] interpolants of the cosets
 * of a coset-major table -> d_h [tables][2^log_b n] coefficients.  log_b 1..3, 6 <= log_n, log_n + log_b <= NTT_MAX_LOG_N, tables 1..64,
 * `words` (of either buffer) >= tables 2^log_b n, d_b and d_h apart. */
int cstark_debug_coset_combine(void *ctx, const uint64_t *d_b, uint64_t *d_h, size_t words, uint32_t log_n, uint32_t log_b, uint32_t tables);
/* cs::launch_final_hi with half = 1/2: d_hi [rows][n], row r = (d_odd's table (r / per_set) tables_per_set + first + r mod per_set -
 * d_direct [rows][n]) / 2; d_odd = the first coset block [rows / per_set][tables_per_set][n].  8 <= log_n <= 20, rows 1..64 a multiple
 * of per_set, first + per_set <= tables_per_set <= 64, odd_words >= (rows / per_set) tables_per_set n, direct_words, hi_words >= rows n. */
int cstark_debug_final_hi(void *ctx, const uint64_t *d_odd, size_t odd_words, const uint64_t *d_direct, size_t direct_words, uint64_t *d_hi, size_t hi_words,
                          uint32_t log_n, uint32_t rows, uint32_t first, uint32_t per_set, uint32_t tables_per_set);
/* cs::launch_final_hi_merge with half = 1/2, a CeParams that carries log_n and m alone and the term cs::coset_merge_term(0, e, log_n,
 * base, k0): d_tco, d_qco [m][2][n] -> d_out [3][m][n].  8 <= log_n <= NTT_MAX_LOG_N - 3, m 1..3, base canonical, k0 1 or 2, in_words
 * (of d_tco and of d_qco) >= 2 m n, out_words >= 3 m n.  term_out (host, may be null): the term. */
int cstark_debug_final_hi_merge(void *ctx, const uint64_t *d_tco, const uint64_t *d_qco, size_t in_words, uint64_t *d_out, size_t out_words, uint32_t log_n,
                                uint32_t m, uint64_t e, uint64_t base, uint32_t k0, cstark_debug_merge_term *term_out);
/* cs::launch_shard_combine: d_parts [4 / nkc][nkc + 4][n] -> d_out [8][n].  nkc 1 or 2, 8 <= log_n <= 20, parts_words >= (4 / nkc)
 * (nkc + 4) n, out_words >= 8 n. */
int cstark_debug_shard_combine(void *ctx, const uint64_t *d_parts, size_t parts_words, uint64_t *d_out, size_t out_words, uint32_t log_n, uint32_t nkc);
#ifdef __cplusplus
}
#endif
#endif
