// Host-visible declarations for the constraint-evaluation kernels (constraints.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "ntt.h" // CosetMergeTerm
#include "trace_check.h" // ValidateEntry, VALIDATE_CLEAN

namespace cs {

// Degree group of transition constraint i of TransactionAir (src/air.rs:76-108): constraints are merged per
// evaluation degree; the AIR has exactly five (base degree; number of 1024-cycles) classes.
//   0: (5;2)  1: (4;2)  2: (3;1)  3: (2;1)  4: (1;1)
__host__ __device__ constexpr int tx_degree_group(int i) {
    return (i < 6 || (i >= 19 && i < 37)) ? 0 : (i >= 6 && i < 18) ? 1 : (i == 18 || (i >= 37 && i < 58)) ? 2 : (i == 92) ? 3 : 4;
}
constexpr unsigned TX_GROUP_BASE[5] = {5, 4, 3, 2, 1};
constexpr unsigned TX_GROUP_CYCLES[5] = {2, 2, 1, 1, 1};

constexpr int CE_RTAB_WORDS = 12288;
constexpr int CE_COEF_WORDS = 115 * 2 + 8; // one coefficient set: alpha[115] | beta[115] | b_alpha[4] | b_beta[4]
constexpr int CE_MAX_SETS = 3;             // coefficient sets merged in one pass (the components of an extension proof)
constexpr int CE_COSET_CONSTS = 10; // per coset: shift, 1/(shift^n - 1), shift^adj[0..5), shift^badj, shift^(n-1), unused
// The generator addition as a functional on the doubling's six products (generator_fold.h): 36 monomial components; per coefficient
// set three functionals (alpha | beta of x | beta of y, z); the constant matrix J[18][36] they are folded from
constexpr int CE_GFOLD_COMPONENTS = 36, CE_GFOLD_WORDS = 3 * CE_GFOLD_COMPONENTS, CE_GFOLD_J_WORDS = 18 * CE_GFOLD_COMPONENTS;

struct CeParams {
    const uint64_t *lde;   // cosets [k0, k0+nk), coset-major [kk][94][n]
    const uint64_t *ptab;  // periodic table [b][48][1024]
    const uint64_t *w;     // [n] powers of w_n
    const uint64_t *coset; // [b][CE_COSET_CONSTS]
    const uint64_t *coef;  // m sets of CE_COEF_WORDS: alpha[115] | beta[115] | b_alpha[4] | b_beta[4]   (device)
    const uint64_t *binv;  // [b][2][n]: 1/(x-1), 1/(x-w^(n-1)) over the evaluation domain
    uint64_t *rtab;        // [m][CE_RTAB_WORDS] scratch: per-proof folded coefficients of the Rescue windows (k_rounds_setup)
    const uint64_t *gfold_j; // [CE_GFOLD_J_WORDS] the matrix of the generator addition (device; constant, uploaded once per context)
    uint64_t *out;         // merged evaluations of coefficient set 0
    uint64_t *out_ext[CE_MAX_SETS - 1]; // ... of sets 1, 2 (m > 1)
    uint32_t m;            // number of coefficient sets (0 reads as 1)
    uint64_t pub[4];       // initial_root[0..2], final_root[0..2]
    const uint64_t *pubd;  // non-null: the 14 public inputs on the device (first / last row of registers 58..64) -- [0], [1], [7], [8] replace pub[]
    uint64_t w_last;       // w_n^(n-1)
    uint32_t adj_mod_n[5]; // degree adjustments reduced mod n (x^adj = shift^adj * w^(j*adj mod n))
    uint32_t badj_mod_n;
    uint32_t log_n, log_b, k0;
    uint32_t nkc;          // split evaluation of a coset window (one rank of a sharded proof): even cosets in p.lde, 1 or 2; 0 = all four
};

constexpr int AIR_MAX_GROUPS = 8;
// generic merge of materialised constraint evaluations (standalone sub-AIRs); all pointers are device memory
struct AirCombineParams {
    const uint64_t *lde, *evals, *w, *shifts; // shifts[k] = g * w_{bn}^k for every LDE coset
    const uint64_t *t_alpha, *t_beta;         // [n_constraints]
    const uint64_t *b_alpha, *b_beta, *a_value;
    const uint32_t *a_reg;                    // [n_assertions]
    const int32_t *a_seq;                     // column of `avals` holding the asserted values, or -1 for the constant a_value
    const uint64_t *avals;                    // [nk][n_avals][n] LDE of the sequence-value polynomials (may be null)
    const uint64_t *tsum;                     // [nk][n] merged transition sum of a fused evaluator (then `evals` is not read), or null
    uint64_t *out;
    uint64_t w_last;
    uint32_t width, n_constraints, n_assertions, n_avals, stride, log_n, k0;
    // grouping (host-built): constraint i uses x^tgrp_adj[t_grp[i]]; assertion a uses divisor / adjustment group a_grp[a]
    const uint32_t *t_grp, *a_grp; // device
    uint32_t n_tgrp, n_agrp;
    uint64_t tgrp_adj[AIR_MAX_GROUPS], agrp_m[AIR_MAX_GROUPS], agrp_zc[AIR_MAX_GROUPS], agrp_badj[AIR_MAX_GROUPS];
    // powers of a point x = shift_k w_n^j without a square-and-multiply per point: x^e = shift_k^e * w_n^((j e) mod n).  Per LDE coset
    // k (host-built): shift_k^adj of every transition group, shift_k^badj and shift_k^m of every assertion group, 1 / (shift_k^n - 1)
    uint64_t tgrp_shift[8][AIR_MAX_GROUPS], agrp_bshift[8][AIR_MAX_GROUPS], agrp_mshift[8][AIR_MAX_GROUPS], zinv_coset[8];
    // optional (all groups or none): cached 1 / (x^m - zc), agrp_inv[g][k (n / m_g) + (j mod n / m_g)] for LDE coset k; null = one
    // inversion per point (Montgomery's trick over the groups)
    const uint64_t *agrp_inv[AIR_MAX_GROUPS];
};
// tab[k][i] = 1 / (shift_m[k] w_n^(i m) - zc), i < n / m, for the b cosets (shift_m[k] = shift_k^m)
hipError_t launch_assert_inverses(uint64_t *d_tab, const uint64_t *d_w, const uint64_t shift_m[8], unsigned b, uint64_t m, uint64_t zc, unsigned log_n,
                                  hipStream_t stream);
hipError_t launch_air_combine(const AirCombineParams &p, unsigned nk, hipStream_t stream);
hipError_t launch_eval_transitions_merkle(const uint64_t *lde, const uint64_t *ptab, uint64_t *out, unsigned log_n, unsigned k0, unsigned nk,
                                          hipStream_t stream);
hipError_t launch_eval_transitions_schnorr(const uint64_t *lde, const uint64_t *aux, const uint64_t *ptab, uint64_t *out, unsigned log_n, unsigned k0,
                                           unsigned nk, hipStream_t stream);
// SchnorrAir, fused: writes sum_i (alpha_i + beta_i x^adj_i) C_i(x) of the nk cosets into p.out (six launches); aux / ptab as for
// launch_eval_transitions_schnorr.  Follow with launch_air_combine on the same parameters with p.tsum = p.out.
// MerkleAir likewise (one launch; ptab as for launch_eval_transitions_merkle)
// d_rtab != null (MERKLE_RTAB_WORDS device words, scratch): the four Rescue round gadgets through their folded form (k_merkle_rounds; blowup
// at most 8), round_group = p.t_grp of the round slots; null: every constraint through the generic frame evaluator
constexpr int MERKLE_RTAB_WORDS = 2048;
constexpr int MERKLE_RTAB_LAMBDA = MERKLE_RTAB_WORDS - CE_GFOLD_WORDS; // its last words: d_lambda of launch_schnorr_ec_split
hipError_t launch_merkle_fused(const AirCombineParams &p, const uint64_t *ptab, unsigned nk, hipStream_t stream, uint64_t *d_rtab = nullptr,
                               unsigned round_group = 0);
hipError_t launch_schnorr_fused(const AirCombineParams &p, const uint64_t *aux, const uint64_t *ptab, unsigned nk, hipStream_t stream);
// SchnorrAir's doubling / addition gadgets in the degree-split form (all cosets, k0 = 0; constraints.hip): eight polynomials on the even
// cosets, d_even = [8][4][n] (d_coefs_tx_layout: alpha[i] at word i, beta[i] at word 115 + i, device); after their extension to the odd
// cosets (d_odd = [4][8][n]) the recombination into p.out, to which the final addition and the remaining constraints are then added
constexpr int SCHNORR_SPLIT_EC_TABLES = 8, SCHNORR_SPLIT_TABLES = 11; // without / with the final addition's three sums (tables 8..10)
// d_gfold_j = the matrix of the generator addition, d_lambda = CE_GFOLD_WORDS words of per-proof scratch: the addition of G is folded into
// the doubling of the same point (k_generator_fold, then three launches)
hipError_t launch_schnorr_ec_split(const AirCombineParams &p, const uint64_t *aux, const uint64_t *d_coefs_tx_layout, uint64_t *d_even, const uint64_t *d_gfold_j,
                                   uint64_t *d_lambda, hipStream_t stream);
hipError_t launch_schnorr_split_finish(const AirCombineParams &p, const uint64_t *aux, const uint64_t *ptab, const uint64_t *d_even, const uint64_t *d_odd,
                                       unsigned g0, unsigned g1, hipStream_t stream, uint64_t *d_rtab = nullptr, unsigned round_group = 0,
                                       const uint64_t *d_hi = nullptr);
// The final addition on five cosets: its three sums on the even cosets (coset < 0: d_out = tables 8..10 of d_even, [3][4][n]) or directly
// on LDE coset 1 (coset = 1: d_out = [3][n]); launch_final_hi(rows 3, first 8, per_set 3): d_hi[q] = (d_odd's table 8 + q on coset 1 - d_direct[q]) / 2.
// With d_hi = [4 odd cosets][3][n] (coset 1 from launch_final_hi, cosets 3, 5, 7 its extension) launch_schnorr_split_finish
// recombines the final addition too (tables of SCHNORR_SPLIT_TABLES); without it the tables are SCHNORR_SPLIT_EC_TABLES wide.
hipError_t launch_schnorr_final_split(const AirCombineParams &p, const uint64_t *d_coefs_tx_layout, uint64_t *d_out, int coset, hipStream_t stream);
hipError_t launch_eval_transitions_range(const uint64_t *lde, uint64_t *out, unsigned log_n, unsigned nk, hipStream_t stream);
// RescueAir (benches/rescue.rs): ptab [b][29][8]
hipError_t launch_eval_transitions_rescue(const uint64_t *lde, const uint64_t *ptab, uint64_t *out, unsigned log_n, unsigned k0, unsigned nk,
                                          hipStream_t stream);

hipError_t launch_eval_transitions(const CeParams &p, unsigned nk, hipStream_t stream);
// All 115 transition-constraint values of TransactionAir on nf free-standing frames (the verifier's out-of-domain check): frame j is
// cur[c * nf + j] (c < 94), next[c * nf + j] and the periodic values per[c * nf + j] (c < 48); out[i * nf + j], i < 115 (device memory)
hipError_t launch_eval_frames(const uint64_t *cur, const uint64_t *next, const uint64_t *per, uint64_t *out, unsigned nf, hipStream_t stream);
// The same for any AIR the verifier knows (CSTARK_AIR_STATE_TRANSITION: launch_eval_frames; MerkleAir 65 / 33 periodic / 106 slots,
// RangeProofAir 2 / 0 / 2, RescueAir 14 / 29 / 14, SchnorrAir 56 / 36 + the 19 public-input values of the frame's point / 56, in the four
// parts of its table kernel), through the bodies the table kernels run
hipError_t launch_eval_frames_air(int air, const uint64_t *cur, const uint64_t *next, const uint64_t *per, uint64_t *out, unsigned nf, hipStream_t stream);
// Trace validation (cstark_air_validate_trace): every transition constraint of AIR `air` on the frames (r, r + 1) of the trace itself.
struct ValidateParams {
    const uint64_t *trace;    // [width][n], the layout of the build-trace entry points
    const uint64_t *per;      // raw periodic columns [n_per][cycle_len] (null for RangeProofAir)
    const uint64_t *messages; // SchnorrAir: the statement's messages [n / 512][28]; null otherwise
    uint32_t *codes;          // [n / cycle_len], pre-filled with VALIDATE_CLEAN: min over the cycle's violated frames of row * NC + slot
    uint32_t *summary;        // [0] first violated cycle, [1] boundary verdict (entry << 24 | step), both pre-filled with VALIDATE_CLEAN; [2] violated cycles, pre-filled 0
    uint32_t log_n, log_cycle;
};
// the frame kernel of the AIR (one wave per 64 frames, slot sums in LDS), then the summary over the cycles
hipError_t launch_validate_frames(int air, const ValidateParams &p, hipStream_t stream);
// the boundary list (trace_check.h) against the trace: max_occ = the largest number of occurrences of an entry; d_seq may be null
hipError_t launch_validate_boundary(const ValidateParams &p, const ValidateEntry *d_entries, unsigned n_entries, const uint64_t *d_seq, unsigned max_occ,
                                    hipStream_t stream);
// frame r as the input of launch_eval_frames_air with nf = 1: d_dst = cur[width] | next[width] | per[n_per] (| the 19 public-input values)
hipError_t launch_validate_gather_frame(const ValidateParams &p, uint64_t *d_dst, size_t r, unsigned width, unsigned n_per, hipStream_t stream);
constexpr int CE_NUM_PARTS = 9; // launches of the fused evaluation: rounds, dbl0, add0, dbl1, add1, final, lin_a, lin_b, lin_c (split form: the one
                                // linear pass is timed as lin_a, lin_b = 0, lin_c = the extension and the recombination)
hipError_t launch_eval_constraints(const CeParams &p, unsigned nk, hipStream_t stream, hipEvent_t *part_events = nullptr);
// Split evaluation of the Rescue windows (m = 1, all 8 cosets, k0 = 0; constraints.hip): setup of the per-proof tables; the four
// low-degree polynomials on the even cosets, d_even = [4][4][n]; recombination over all cosets from d_even and their extension to
// the odd cosets d_odd = [4 cosets][4][n] (writes p.out, like the first part of launch_eval_constraints).
hipError_t launch_rounds_setup(const CeParams &p, hipStream_t stream);
hipError_t launch_rounds_split(const CeParams &p, uint64_t *d_even, hipStream_t stream);
// split evaluation of a curve gadget (part 1 = doubling of s*G AND addition of G to the same point, 3 = doubling of h*P; 1 writes the
// doubling family's three polynomials into d_even_family and the addition family's two into d_even_linear -- the addition of the
// constant G is a functional on the doubling's six products, folded per proof by launch_rounds_setup, which must precede it; 3 adds
// to the doubling family): d_even_family = [3][4][n]
// part 4 = addition of the public key: its quartic half is a family of its own (d_even_family), its linear half is ADDED to the
// addition family d_even_linear (after part 1 wrote it)
hipError_t launch_ec_split(const CeParams &p, int part, uint64_t *d_even_family, uint64_t *d_even_linear, hipStream_t stream);
constexpr int CE_SPLIT_TABLES = 13, CE_SPLIT_FAM0 = 4, CE_SPLIT_FINAL = 11; // first family (Rescue windows + linear groups): four polynomials; doubling 3 | addition 2 | addition x bit 2 | final addition 2
// split evaluation of the three linear groups in one pass over the frame (k_lin_all): adds to the first family, d_even_family0 = [4][4][n]
hipError_t launch_lin_all(const CeParams &p, uint64_t *d_even_family0, hipStream_t stream);
// one rank of a proof sharded by LDE coset (p.k0 even, p.nkc = 1 or 2 even cosets, m = 1): rows [p.nkc + 4][n] = its even cosets'
// complete values, then its share of the four odd cosets (constraints.hip, k_split_finish_shard); d_bit37_all = register 37 on all cosets
hipError_t launch_split_finish_shard(const CeParams &p, const uint64_t *d_even, const uint64_t *d_odd, const uint64_t *d_hi, const uint64_t *d_bit37_all,
                                     uint64_t *d_out, hipStream_t stream);
// the ranks' rows [4 / nkc][nkc + 4][n] -> merged evaluations of all cosets [8][n]
hipError_t launch_shard_combine(const uint64_t *d_parts, uint64_t *d_out, unsigned log_n, unsigned nkc, hipStream_t stream);
// d_hi = [4 odd cosets][2 m][n]: the high parts of the final-addition polynomials on the odd cosets (launch_final_hi + their extension)
// merged: the family sums of the odd cosets were formed before their transforms (ntt.h: coset_even_to_odd_merged with the families
// table 0..3 | 4..6 | 7, 8 | 9, 10 | 11, 12, terms 1 + x^adj_0 + x^adj_1 + x^adj_2): d_odd = [4][m][CE_SPLIT_FAMILIES][n], d_hi = [4][m][n]
constexpr int CE_SPLIT_FAMILIES = 5;
hipError_t launch_split_finish(const CeParams &p, const uint64_t *d_even, const uint64_t *d_odd, const uint64_t *d_hi, hipStream_t stream,
                               bool merged = false);
// Final addition (degree 5 (n - 1): one n-coefficient block above the 4n the even cosets determine).  coset < 0: the two sums
// (alpha; beta of groups 0, 1 merged) on the four even cosets into the family's tables d_out = [2][4][n] (per set: stride of the
// table block); coset >= 0: on that one coset, d_out = [m][2][n].
hipError_t launch_final_split(const CeParams &p, int coset, uint64_t *d_out, hipStream_t stream);
// Values of the high-part polynomials on LDE coset 1, for either AIR: d_hi[r][j] = (T_r(coset 1)[j] - d_direct[r][j]) / 2, r < rows, where
// T_r is table first + r % per_set of set r / per_set in d_odd = [4 odd cosets][sets][tables_per_set][n] (coset 1 first) and d_direct the
// direct evaluation on coset 1.  TransactionAir: rows = 2 m, (first, per_set, tables_per_set) = (11, 2, CE_SPLIT_TABLES); SchnorrAir:
// rows = 3, (SCHNORR_SPLIT_EC_TABLES, 3, SCHNORR_SPLIT_TABLES).
hipError_t launch_final_hi(const uint64_t *d_odd, const uint64_t *d_direct, uint64_t *d_hi, uint64_t half /* 1/2, memory form */, unsigned log_n,
                           unsigned rows, unsigned first, unsigned per_set, unsigned tables_per_set, hipStream_t stream);
// The same for the merged tables: d_hi[c][j] = (family 4 of d_odd on coset 1 - (direct[c][0] + x^adj_0 direct[c][1])) / 2, d_hi = [m][n]
hipError_t launch_final_hi_merged(const CeParams &p, const uint64_t *d_odd, const uint64_t *d_direct, uint64_t *d_hi, uint64_t half, hipStream_t stream);
// inputs of the high part's transforms over cosets 3, 5, 7, d_out = [3][m][n]: with h = (d_tco - d_qco) / 2 ([m][2][n] each: the
// interpolants over LDE coset 1 of the family's two tables -- the raw output of coset_even_to_odd_merged -- and of the direct sums),
// h[c][0] + x^adj_0 h[c][1] merged on the coefficients; tm = coset_merge_term(0, adj_0, log_n, g w_8n, 2)
hipError_t launch_final_hi_merge(const CeParams &p, const uint64_t *d_tco, const uint64_t *d_qco, uint64_t *d_out, const CosetMergeTerm &tm, uint64_t half,
                                 hipStream_t stream);
hipError_t build_boundary_inverses(uint64_t *d_table, const uint64_t *d_w, const uint64_t *d_coset, uint64_t w_last, unsigned log_n, unsigned log_b,
                                   hipStream_t stream);

} // namespace cs
