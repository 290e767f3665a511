// Host-visible declarations for the NTT kernels (ntt.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace cs {

constexpr unsigned NTT_MIN_LOG_N = 6, NTT_MAX_LOG_N = 24;

// One batched transform: `batch` x `width` independent length-2^log_n sequences, column stride n.
struct NttArgs {
    const uint64_t *in;    // natural order
    uint64_t *scratch;     // same shape as one batch of `in` times batch; may alias `in` (destroys it)
    uint64_t *out;         // natural order; must not alias scratch
    unsigned width, batch, log_n;
    const uint64_t *w;         // [n] powers of the root of unity to use (forward or inverse table)
    const uint64_t *prescale;  // optional [n] per batch: input element m is multiplied by prescale[m] (coset shift^m)
    size_t prescale_batch_stride;
    uint64_t post_scale;       // applied to every output when do_scale (n^-1 for the inverse transform)
    bool do_scale;
    bool inverse;              // w is the inverse table (selects the compile-time twiddles of the register kernels)
    size_t in_batch_stride, scratch_batch_stride, out_batch_stride; // in elements
    // dense tables (ntt_build_aux_*) of `w` and, per batch, of `prescale`: required at the sizes ntt_three_step_shape names -- ntt_columns
    // answers hipErrorInvalidValue without them -- and not read at any other size
    const uint64_t *aux = nullptr, *aux_ps = nullptr;
    size_t aux_ps_batch_stride = 0;
};

// The sizes that run on the three-step register kernels, and their shape there (false: every other size; it takes no dense tables):
// column pass over 2^log_r points, row pass over 2^log_c, output factors tabulated for 2^log_kb row classes.
struct NttThreeStepShape { unsigned log_r, log_c, log_kb; };
bool ntt_three_step_shape(unsigned log_n, NttThreeStepShape *s);
size_t ntt_aux_plan_words(const NttThreeStepShape &s);
size_t ntt_aux_coset_words(const NttThreeStepShape &s);
// d_w: the n-entry power table of the plan (forward or inverse); d_s: one coset's n-entry prescale table (powers of its shift)
hipError_t ntt_build_aux_plan(uint64_t *d_aux, const uint64_t *d_w, const NttThreeStepShape &s, hipStream_t stream);
hipError_t ntt_build_aux_coset(uint64_t *d_aux, const uint64_t *d_w, const uint64_t *d_s, const NttThreeStepShape &s, hipStream_t stream);

hipError_t ntt_columns(const NttArgs &a, hipStream_t stream);

// Step columns: constant over blocks of 2^log_block rows, f[i] = g[i >> log_block] (ntt.hip, "step columns").  Served at the three-step
// sizes whose row length holds a whole number of periods T = n >> log_block; every other (log_n, log_block) takes ntt_columns.
bool ntt_step_shape(unsigned log_n, unsigned log_block);
// The constants of one (log_n, log_block, coset set), everything in Montgomery form: d_d [n] = the fixed vector D, and the forward column pass
// of D under each coset of `a` -- a forward NttArgs with in = d_d, width = 1, its batch / prescale / aux fields as for ntt_columns --
// written to a.scratch [batch][n] (a.out is not used).  d_winv: the n powers of w_n^-1.
// split = R, 0 < R < 2^log_block: the same for D_R, the fixed vector of the first R rows of every block (two-level columns: one value
// on rows [0, R) of a block and another on [R, 2^log_block))
hipError_t ntt_step_build_tables(uint64_t *d_d, unsigned log_block, unsigned split, const uint64_t *d_winv, const NttArgs &a, hipStream_t stream);
// d_evals [ncols][n] (only the first row of every block is read) -> d_fac [ncols][T], the per-column factors A, and d_coeffs [ncols][n],
// the interpolants c_k = A[k mod T] D[k]
hipError_t ntt_step_coefficients(const uint64_t *d_evals, uint64_t *d_fac, uint64_t *d_coeffs, const uint64_t *d_d, unsigned ncols, unsigned log_n,
                                 unsigned log_block, const uint64_t *d_winv, uint64_t n_inv, hipStream_t stream);
// Two-level columns: rows 0 and `split` of every block are read -> d_fac [ncols][2][T], the factors A1 (of the value on rows >= split)
// and A2 (of the difference), and d_coeffs, the interpolants c_k = A1[k mod T] D[k] + A2[k mod T] D_R[k]
hipError_t ntt_step2_coefficients(const uint64_t *d_evals, uint64_t *d_fac, uint64_t *d_coeffs, const uint64_t *d_d, const uint64_t *d_dr, unsigned ncols,
                                  unsigned log_n, unsigned log_block, unsigned split, const uint64_t *d_winv, uint64_t n_inv, hipStream_t stream);
// The extension: the row pass alone, its input formed as d_wtab[batch][k1][c] * d_fac[column][c mod T] at the load.  Of `a`: out, width,
// batch, log_n, out_batch_stride, aux.  d_wtab_r (or null): the tables of D_R -- two-level columns, d_fac as ntt_step2_coefficients writes it.
hipError_t ntt_step_rows(const NttArgs &a, const uint64_t *d_wtab, const uint64_t *d_wtab_r, const uint64_t *d_fac, unsigned log_block, hipStream_t stream);
// table[e] = base^e, e < n
hipError_t ntt_power_table(uint64_t *d_table, size_t n, uint64_t base, hipStream_t stream);

// composition-polynomial helpers: coset-major -> natural order; split of H's coefficients into b columns (with the g^-m scaling)
hipError_t interleave_cosets(const uint64_t *d_in, uint64_t *d_out, unsigned log_n, unsigned log_b, hipStream_t stream);
// Second half of the interpolation over the whole b n-point domain from per-coset interpolants (B cosets = 2^log_b <= 8):
// d_b [B][n] = iNTT_n of every coset of a coset-major table; d_h [B n] = coefficients a_t in natural order.  With t = q + n i:
//   a_{q + n i} = (1 / B) sum_k w_B^(-k i) (w_N^(-k q) B_k[q]),   N = B n;  winv_N = powers of w_N^-1.
hipError_t coset_combine(const uint64_t *d_b, uint64_t *d_h, unsigned log_n, unsigned log_b, const uint64_t *d_winv_N, uint64_t b_inv,
                         hipStream_t stream, unsigned tables = 1);
// The way to the odd cosets for polynomials of degree < 4n given by the interpolants of the four even cosets (d_b [tables][4][n]):
// coset_combine with log_b = 2 (coefficients a_t of P(g y), t = q + n i) followed by b_k'[q] = sum_{i<4} w_8^((2k'+1) i) a_{q + n i}, the
// inputs of the n-point transforms over the odd cosets (whose prescale table supplies the twist w_8n^((2k'+1) q)), in one pass: the
// 4n coefficients are never written.  d_out [4 odd cosets][tables][n]; d_winv_4n = powers of w_4n^-1, d_w_8n = powers of w_8n, quarter = 1/4.
hipError_t coset_even_to_odd(const uint64_t *d_b, uint64_t *d_out, unsigned log_n, unsigned tables, const uint64_t *d_winv_4n, const uint64_t *d_w_8n,
                             uint64_t quarter, hipStream_t stream, unsigned kc0 = 0, unsigned nkc = 4); // (only even cosets [kc0, kc0 + nkc) present)
// coset_even_to_odd with the monomial recombination of a flag family done on the coefficient vectors, before any transform: a family
// sum_t x^(e_t) S_t(x) (x = g y) becomes ONE input vector per odd coset.  With e = n d + r (0 <= r < n) and y^n = w_8^k on coset k,
//   x^e S_t on coset k = sum_q' y^q' c_k[q' < r] s_k[(q' - r) mod n],   c_k[0] = base^e w_8^(k d),  c_k[1] = c_k[0] w_8^k
// (s_k = what coset_even_to_odd writes for the table; base = g): a rotation by r, the wrapped entries picking up y^n.
struct CosetMergeTerm {
    uint32_t table, r; // table within its set; rotation
    uint64_t c[4][2];  // per coset slot i (coset k0 + 2 i): the factor of the entries that did not / did wrap
};
constexpr int COSET_MERGE_MAX_FAMILIES = 5, COSET_MERGE_MAX_TERMS = 4;
struct CosetMergeDesc {
    uint32_t families, tables_per_set;
    uint32_t terms[COSET_MERGE_MAX_FAMILIES];
    CosetMergeTerm term[COSET_MERGE_MAX_FAMILIES][COSET_MERGE_MAX_TERMS];
    int32_t raw_family; // the family whose tables are also written unmerged for the first odd coset (d_raw), -1: none
};
// host: the term x^e S_table for the cosets k0, k0 + 2, k0 + 4, k0 + 6 of the 8n-point domain (base: see above)
CosetMergeTerm coset_merge_term(unsigned table, uint64_t e, unsigned log_n, uint64_t base, unsigned k0 = 1);
// d_b [sets][tables_per_set][4][n] -> d_out [4 odd cosets][sets][families][n].  d_raw (with raw_family >= 0) [sets][terms][n]:
// w_8n^q s_1[q] of the family's tables, the coefficients of S_t(g w_8n z) mod (z^n - 1): the table's interpolant over the first odd coset.
hipError_t coset_even_to_odd_merged(const uint64_t *d_b, uint64_t *d_out, unsigned log_n, unsigned sets, const CosetMergeDesc &desc,
                                    const uint64_t *d_winv_4n, const uint64_t *d_w_8n, uint64_t quarter, uint64_t *d_raw, hipStream_t stream);
hipError_t split_columns(const uint64_t *d_h, uint64_t *d_out, unsigned log_n, unsigned log_b, uint64_t ginv, hipStream_t stream);

} // namespace cs
